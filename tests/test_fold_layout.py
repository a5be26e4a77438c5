"""CPU: ``layout.pod_bytes`` at every edge of the fold rule, against bytes written out by hand
(tests/fold_cases.py): for each edge one pod just inside and one just outside."""
import numpy as np
import pytest

import fold_cases as FC
from escalator_amd import layout

INT64_MIN = -(1 << 63)
FEW, MANY = 5, (1 << 14) - 1                       # group pairs of the context: small blocks or none


def soa(pods, xpairs=None):
    """The packed arrays of hand-built pods, restated from the pod record's definition
    (include/escalator_hip.h): the first regular container inline when its cpu fits u32, then
    the other regular containers, the init containers (an absent key INT64_MIN) and the
    overhead (when it has a key) as records."""
    out = {k: [] for k in ("flags", "cpu0", "mem0", "pair0", "xc_cpu", "xc_mem", "xp_pair")}
    for i, p in enumerate(pods):
        reg = [(c["cpu"] or 0, c["mem"] or 0) for c in p["containers"]]
        cpu0 = mem0 = 0
        if reg and 0 <= reg[0][0] <= 0xFFFFFFFF:
            (cpu0, mem0), reg = reg[0], reg[1:]
        init = [(INT64_MIN if c["cpu"] is None else c["cpu"], INT64_MIN if c["mem"] is None else c["mem"])
                for c in p["init_containers"]]
        o = p["overhead"]
        ovh = [(o["cpu"] or 0, o["mem"] or 0)] if o and (o["cpu"] is not None or o["mem"] is not None) else []
        xp = list(xpairs[i]) if xpairs else []
        out["flags"].append(len(ovh) << 4 | len(reg) << 8 | len(init) << 16 | len(xp) << 24 | (1 << 2))   # HAS_SEL
        out["cpu0"].append(cpu0)
        out["mem0"].append(mem0)
        out["pair0"].append(0)
        for c, m in reg + init + ovh:
            out["xc_cpu"].append(c)
            out["xc_mem"].append(m)
        out["xp_pair"] += xp
    dt = {"flags": np.uint32, "cpu0": np.uint32, "mem0": np.int64, "pair0": np.uint32, "xc_cpu": np.int64,
          "xc_mem": np.int64, "xp_pair": np.uint32}
    return {k: np.array(v, dtype=dt[k]) for k, v in out.items()}


@pytest.mark.parametrize("name", [c[0] for c in FC.CASES])
def test_case_bytes(name):
    P = soa(FC.pods_of({name}))
    assert layout.pod_bytes(P, FEW) == FC.bytes_of({name})
    assert layout.pod_bytes(P, MANY - 1) == FC.bytes_of({name})            # still fewer than 2^14 - 1 pairs
    assert layout.pod_bytes(P, MANY) == FC.bytes_of({name}, many_pairs=True)


def test_all_cases_together_and_in_ranges():
    P = soa(FC.pods_of())
    n = len(FC.CASES)
    assert layout.pod_bytes(P, FEW) == FC.bytes_of()
    assert layout.pod_bytes(P, MANY) == FC.bytes_of(many_pairs=True)
    # a shard's range prices its own pods (the C tile's offsets with the C pod's range)
    for lo, hi in ((0, 7), (7, n - 1), (n - 1, n), (3, 3)):
        names = {c[0] for c in FC.CASES[lo:hi]}
        assert layout.pod_bytes(P, FEW, lo, hi) == (FC.bytes_of(names) if names else 0), (lo, hi)


def test_folded_request_values():
    by = {c[0]: i for i, c in enumerate(FC.CASES)}
    cpu, mem = layout.folded_request(soa(FC.pods_of()))
    want = {"sum_cpu_in8": (FC.C14 - 1, 10), "sum_cpu_out8": (FC.C14, 10), "sum_mem_in8": (10, FC.M34 - 1),
            "sum_mem_out12": (10, FC.M44 - 1), "init_wins": (FC.C14, 100), "init_loses": (100, 100),
            "init_cpu_absent": (100, FC.M34), "init_mem_absent": (FC.C14 - 1, 100), "init_both_absent": (100, 100),
            "init_vs_sum": (120, 120), "ovh_in8": (FC.C14 - 1, FC.M34 - 1), "ovh_out12_cpu": (FC.C20 - 1, 6),
            "all_three_kinds": (FC.C14, 201), "sum3_12": (3000, 18 << 30)}
    for name, (c, m) in want.items():
        assert (int(cpu[by[name]]), int(mem[by[name]])) == (c, m), name


def test_extra_pairs_priced_by_block():
    """Extra pairs: 2 B each in the 8-B block, 4 B each in the 12-B and plain blocks; a pod
    with records keeps its pairs when it folds."""
    names = ["sum_cpu_in8", "sum_cpu_out8", "sum_cpu_out12"]
    base = [FC.bytes_of({n}) for n in names]
    for k in (1, 2, 3):
        xp = [list(range(1, k + 1))] * 3
        for j, n in enumerate(names):
            P = soa(FC.pods_of({n}), [xp[j]])
            assert layout.pod_bytes(P, FEW) == base[j] + k * (2 if j == 0 else 4), (n, k)
    # 4 extra pairs: the C section, records unfolded (20 + 16 + 4 * 4 + the tile's 8)
    P = soa(FC.pods_of({"sum_cpu_in8"}), [[1, 2, 3, 4]])
    assert layout.pod_bytes(P, FEW) == 20 + 16 + 16 + 8
