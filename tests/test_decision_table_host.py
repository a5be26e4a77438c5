"""CPU: the decision table (tests/decision_table.py) reaches its edges, and its two
references — the literal oracle on each case's objects, the C oracle on the packed table —
and the host build of the decision arithmetic agree on every case, bit for bit, before any
GPU sees them."""
import ctypes as C
import struct

import numpy as np
import pytest

import decision_table as DT
from oracle import oracle as O
from oracle import soa

soa.build()


def _bits(x):
    return struct.pack("<d", float(x))


@pytest.fixture(scope="module")
def table():
    return DT.build()


@pytest.fixture(scope="module")
def packed(table):
    from escalator_amd.context import Context
    asm = DT.assemble(table)
    P, N = Context(asm["groups"], device=-1).pack(asm["pods"], asm["nodes"], asm["trackers"])
    return asm, P, N


def test_table_size(table):
    """Roughly 1 500 groups, 6 000 nodes, 4 000 pods at the most, 300 nodes in a case; the
    full table takes the word-array totals path (G > 1 024) and the core subset the pinned
    totals record (G <= 1 024)."""
    n_nodes, n_pods = sum(len(c["nodes"]) for c in table), sum(len(c["pods"]) for c in table)
    print("decision table: %d groups, %d nodes, %d pods, core %d groups" % (len(table), n_nodes, n_pods,
                                                                            len(DT.core(table))))
    assert 1024 < len(table) <= 1500 and n_nodes <= 6000 and n_pods <= 4000
    assert max(len(c["nodes"]) for c in table) <= 300
    core = DT.core(table)
    assert len(core) <= 1024
    assert {c["family"] for c in core} == set(DT.FAMILIES)
    assert sum(c["group"]["name"] == "default" for c in table) == 1
    assert len({c["group"]["label_value"] for c in table}) == len(table)


@pytest.mark.parametrize("subset", ["full", "core"])
def test_coverage(table, subset):
    cov = DT.coverage(table if subset == "full" else DT.core(table))
    print(cov)
    assert set(cov["families"]) == set(DT.FAMILIES)
    assert set(cov["branches"]) == set(DT.BRANCHES)
    # ERR_TAINT_MIN needs n_untainted < min_nodes at the clamp, which the below_min return
    # (controller.go:281) has taken before; NOT_OWNED is no decision
    assert set(cov["statuses"]) == {0, 1, 2, 3, 4, 5}
    assert cov["ceil_k"] >= 10 and cov["ceil_k1"] >= 10 and cov["ceil_other"] == 0
    assert cov["division"] >= (64 if subset == "full" else 8)
    assert cov["delta_gt_2_31"] >= 1 and cov["delta_int64_min"] >= 1
    assert cov["negative_pct"] >= 1 and cov["total_ge_2_53"] >= 1 and cov["taint_clamped"] >= 1
    for probe in ("lower", "upper", "up"):
        for side in (True, False):
            assert cov["sides"].get((probe, side), 0) >= 1, (probe, side)


def test_division_pairs_all_qualify(table):
    """Every division case is one the seeded search accepted, on both sides."""
    div = [c for c in table if c["family"] == "division"]
    assert DT.coverage(div)["division"] == len(div) >= 128
    assert {c["tags"]["side"] for c in div} == {"cpu", "mem"}


def test_oracles_agree(table, packed):
    """The C oracle over the packed table (soa.totals, soa.decide, soa.metrics) equals the
    literal oracle over each case's objects: totals, percentages as bits, integers,
    statuses, gauges."""
    asm, P, N = packed
    otot = soa.totals(P, N, asm["groups"])
    odf, odi = soa.decide(asm["groups"], asm["states"], otot)
    rtot, known, rdf, rdi, mets = DT.oracle_arrays(table, asm["node_base"])
    DT.compare(table, "C oracle against the literal oracle", otot, odf, odi, rtot, known, rdf, rdi)
    for g, (a, b) in enumerate(zip(soa.metrics(otot, odf, odi), mets)):
        assert a.keys() == b.keys() and all(_bits(a[k]) == _bits(b[k]) for k in a), DT.describe(table[g])
    flipped = DT.flipped_states(table)
    odf, odi = soa.decide(asm["groups"], flipped, otot)
    rtot, known, rdf, rdi, _ = DT.oracle_arrays(table, asm["node_base"], flipped)
    DT.compare(table, "C oracle against the literal oracle, flipped states", otot, odf, odi, rtot, known, rdf, rdi)


def test_conversion_sums_on_both_sides(table):
    """Pod and node sums of 2^53 + 1, 2^53 + 3, 2^62 + 2^9 + 1, 2^63 - 1 and a negative one
    occur, for cpu and for memory, without the overflow gate."""
    want = {(1 << 53) + 1, (1 << 53) + 3, (1 << 62) + (1 << 9) + 1, (1 << 63) - 1, -((1 << 53) + 1)}
    conv = [c["want"] for c in table if c["family"] == "conversions"]
    assert all(w["err"] != O.ERR_OVERFLOW for w in conv)
    for key in ("pod_cpu_m", "pod_mem_b", "node_cpu_m", "node_mem_b"):
        assert want <= {w[key] for w in conv}, key


def test_gauge_mismatch_names_the_group(table):
    """The report behind a failing gauge comparison: the group, the gauge, both values."""
    from escalator_amd._lib import METRIC_NAMES
    from escalator_amd.context import METRICS_DTYPE
    mets = [c["want_metrics"] for c in table]
    met = np.zeros(len(table), METRICS_DTYPE)
    for g, e in enumerate(mets):
        met["set_mask"][g] = sum(1 << k for k, n in enumerate(METRIC_NAMES) if n in e)
        for n, v in e.items():
            met[n][g] = v
    assert DT.gauge_mismatch(met, mets, METRIC_NAMES) is None
    g = next(g for g, e in enumerate(mets) if "mem_request" in e and e["mem_request"] < 0)
    met["mem_request"][g] = np.nextafter(met["mem_request"][g], 0.0)
    got = DT.gauge_mismatch(met, mets, METRIC_NAMES)
    assert got[0] == g and got[1].startswith("mem_request: got ") and "case %d" % table[g]["id"] in DT.describe(table[g])
    met["set_mask"][3] ^= 1
    assert DT.gauge_mismatch(met, mets, METRIC_NAMES)[0] == 3


def test_host_build_matches_oracle(table, packed):
    """esc_calc_percent_usage / esc_calc_scale_up_delta (the host build of esc_common.h) on
    every case's totals that reach them: percentages as bits, delta and status equal."""
    from escalator_amd import _lib as L
    lib = L.load()
    asm, P, N = packed
    otot = soa.totals(P, N, asm["groups"])
    a, b, d = C.c_double(), C.c_double(), C.c_int64()
    n_pct = n_up = 0
    for g, c in enumerate(table):
        w = c["want"]
        if w["branch"] in ("empty", "gate", "below_min"):
            continue
        t = [int(x) for x in otot[g]]
        assert (t[0], t[1], t[3], t[4], t[6]) == (w["pod_cpu_m"], w["pod_mem_b"], w["node_cpu_m"], w["node_mem_b"],
                                                  w["n_untainted"]), DT.describe(c)
        st = lib.esc_calc_percent_usage(t[0], t[1], t[3], t[4], t[6], C.byref(a), C.byref(b))
        assert _bits(a.value) == _bits(w["cpu_pct"]) and _bits(b.value) == _bits(w["mem_pct"]), DT.describe(c)
        assert st == (3 if w["branch"] == "pct_err" else 0), DT.describe(c)
        n_pct += 1
        if w["branch"] != "scale_up":
            continue
        st = lib.esc_calc_scale_up_delta(t[6], a.value, b.value, t[0], t[1], w["cached_cpu_m"], w["cached_mem_b"],
                                         c["group"]["scale_up_pct"], C.byref(d))
        assert d.value == w["delta"] and st == DT.STATUS[w["err"]], (d.value, st, DT.describe(c))
        n_up += 1
    assert n_pct > 1000 and n_up > 500
