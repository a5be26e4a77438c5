"""A table of scale decisions at the edges of the float64 decision arithmetic.

The decision (``decide_one``, ``percent_usage``, ``scale_up_delta``, ``go_ceil``, ``go_int``,
``go_max``, ``milli_mem``, ``metrics_one`` in ``esc_common.h``) is compiled twice: into the
host library and into K4 on the device.  Random clusters reach its edges only by luck, so
this module builds them on purpose: usages on and beside a threshold, quotients where a
division by reciprocal would differ, ``ceil`` arguments that are mathematically integers,
sums beyond 2^53, the wrapped ``MilliValue``, Inf / NaN / -0 needs, every gate and clamp.

Every case is one group with its own label pair (``"t"``, ``"c<i>"``), pods selecting that
pair and nodes carrying it, so a case's expectation is the literal oracle over that case's
objects alone (no other case can contribute) and the whole table loads into one context.

``build`` gives the cases with their expectations, ``coverage`` counts from the oracle's
outputs what the table reaches (the tests assert the counts, so the table cannot silently
stop reaching its edges), ``assemble`` concatenates cases into one cluster,
``oracle_arrays`` gives the literal oracle's expectation in the layout of the results (the
C oracle's ``soa.totals`` / ``soa.decide`` already have it) and ``compare`` names the case
that differs.
"""
from __future__ import annotations

import random

import numpy as np

from oracle import oracle as O

KEY = "t"
TAINT = O.TO_BE_REMOVED_KEY
Gi = 1 << 30
INT64_MIN = -(1 << 63)
STATUS = {None: 0, O.ERR_MIN_NODES: 1, O.ERR_MAX_NODES: 2, O.ERR_DIV_ZERO: 3, O.ERR_NEG_DELTA: 4, O.ERR_OVERFLOW: 5}
# ERR_TAINT_MIN (scaleDownTaint's n_untainted < min_nodes) cannot occur in a decision: the
# below_min return (controller.go:281) takes every such group first.  No case has it.
ST_TAINT_MIN = 6
BRANCHES = ["empty", "gate", "below_min", "pct_err", "locked", "fast_down", "slow_down", "scale_up", "none"]
TOT_FIELDS = ["pod_cpu_m", "pod_mem_b", "n_pods", "node_cpu_m", "node_mem_b", "n_nodes", "n_untainted",
              "n_tainted", "n_cordoned", "first_node", "first_cpu_m", "first_mem_b", "flags"]
DEC_FIELDS = ["delta", "n_to_taint", "cached_cpu_m", "cached_mem_b", "status", "branch", "taint_status"]
FAMILIES = ["thresholds", "division", "ceil", "conversions", "millivalue", "zero", "gates"]


class _Table:
    def __init__(self):
        self.cases = []

    def add(self, family, desc, pods=(), nodes=(), spec=None, state=None, tracker=(), default=False, **tags):
        """pods: (cpu, mem) of one container each; nodes: (cpu, mem[, kind]) with kind in
        "taint", "cordon", "both"; tracker: node positions of the case (dry mode) or names."""
        i = len(self.cases)
        value = "c%d" % i
        group = {"name": "default" if default else "g%d" % i, "label_key": KEY, "label_value": value,
                 "min_nodes": 0, "max_nodes": 1000, "taint_lower_pct": 30, "taint_upper_pct": 45,
                 "scale_up_pct": 70, "slow_removal_rate": 1, "fast_removal_rate": 2, "dry_mode": False}
        group.update(spec or {})
        st = {"locked": False, "requested_nodes": i % 7 - 2, "cached_cpu_m": 0, "cached_mem_b": 0}
        st.update(state or {})
        P = [{"name": "c%d-p%d" % (i, k), "owner_kinds": [], "annotations": {},
              "node_selector": None if default else {KEY: value}, "affinity": None,
              "containers": [{"cpu": p[0], "mem": p[1]}], "init_containers": [], "overhead": None, "node_name": ""}
             for k, p in enumerate(pods)]
        N = []
        for k, n in enumerate(nodes):
            kind = n[2] if len(n) > 2 else ""
            N.append({"name": "c%d-n%d" % (i, k), "labels": {KEY: value}, "unschedulable": kind in ("cordon", "both"),
                      "taints": [TAINT] if kind in ("taint", "both") else [], "cpu": n[0], "mem": n[1],
                      "created_ns": 1_700_000_000_000_000_000 + 1000 * k})
        trk = [N[t]["name"] if isinstance(t, int) else t for t in tracker]
        self.cases.append({"id": i, "family": family, "desc": desc, "tags": tags, "group": group, "state": st,
                           "pods": P, "nodes": N, "tracker": trk})


def _split(total: int, n: int) -> list[int]:
    """n parts summing to total (every partial sum stays between 0 and total)."""
    part = total // n
    return [part] * (n - 1) + [total - part * (n - 1)]


def _big_parts(s: int) -> list[int]:
    """|s| >= 2^53 as a 2^53 part, the rest, and a 1 — the sign on every part, so no order of
    addition leaves [min(s, 0), max(s, 0)]."""
    sign, a = (-1 if s < 0 else 1), abs(s)
    rest = a - (1 << 53)
    parts = [1 << 53] + ([rest - 1, 1] if rest > 1 else [rest])
    assert sum(parts) == a and all(p > 0 for p in parts)
    return [sign * p for p in parts]


def division_pairs(rng: random.Random, n: int, scale: int) -> list[tuple[int, int]]:
    """Seeded search for (a, c) < 2^40 whose quotient (of a*scale, c*scale: scale 1000 is the
    memory side's MilliValue) differs between a true division and a multiplication by the
    reciprocal, and still differs after the * 100."""
    out = []
    while len(out) < n:
        c = rng.randrange(1000, 1 << 40)
        a = rng.randrange(c // 2 + 1, min(8 * c, 1 << 40))
        if divides_differently(a * scale, c * scale):
            out.append((a, c))
    return out


def divides_differently(a: int, c: int) -> bool:
    fa, fc = float(a), float(c)
    q, r = fa / fc, fa * (1.0 / fc)
    return q != r and q * 100.0 != r * 100.0


# ------------------------------------------------------------------ families
def _thresholds(t: _Table):
    """Usage on, and one unit of request either side of, each comparison of the decision
    (mx < taint_lower, mx < taint_upper, mx > scale_up); the other resource stays at 0 % so
    go_max picks the probed side.  Where T * capacity / 100 is no integer the three requests
    are the nearest integer and its neighbours.  7 / 100 * 100 = 7.000000000000001 and
    29 / 100 * 100 = 28.999999999999996 are the point: "on the threshold" is decided by the
    rounding of one division and one multiplication."""
    for T in (1, 7, 29, 33, 57, 70, 99):
        for cap in (1000, 3000, 4096, 7000):
            for probe in ("lower", "upper", "up"):
                if probe == "lower":
                    spec = {"taint_lower_pct": T, "taint_upper_pct": T + 10, "scale_up_pct": T + 20}
                elif probe == "upper":
                    spec = {"taint_lower_pct": T - 1, "taint_upper_pct": T, "scale_up_pct": T + 15}
                else:
                    spec = {"taint_lower_pct": 0, "taint_upper_pct": T - 1, "scale_up_pct": T}
                for side in ("cpu", "mem"):
                    unit = cap if side == "cpu" else cap * 1024
                    r0 = (T * unit + 50) // 100
                    for dr in (-1, 0, 1):
                        req = r0 + dr
                        pods = [(req, 0)] if side == "cpu" else [(0, req)]
                        nodes = [(cap, Gi)] if side == "cpu" else [(1000, unit)]
                        t.add("thresholds", "%s %s T=%d cap=%d req=%d" % (probe, side, T, unit, req), pods, nodes,
                              spec, probe=probe, side=side)


def _division(t: _Table, rng: random.Random, n_each: int):
    for side, scale in (("cpu", 1), ("mem", 1000)):
        for k, (a, c) in enumerate(division_pairs(rng, n_each, scale)):
            reqs, caps = _split(a, 1 + k % 2), _split(c, 1 + k % 3)
            usage = a * 100 // c
            spec = {"taint_lower_pct": 0, "taint_upper_pct": 0, "scale_up_pct": max(1, usage // 2)}
            if side == "cpu":
                pods, nodes = [(r, 0) for r in reqs], [(x, Gi) for x in caps]
            else:
                pods, nodes = [(0, r) for r in reqs], [(1000, x) for x in caps]
            t.add("division", "%s a=%d c=%d" % (side, a, c), pods, nodes, spec, side=side)


def _ceil(t: _Table):
    """n nodes of 1000 m, threshold T, request 10 T (n + k): the need n (pct - T) / T is
    mathematically k, and float noise makes its ceil k or k + 1.  The neighbouring requests
    are the plain k and k + 1.  Then the scale-from-zero form ceil(req / cached / T * 100)
    with quotients that are mathematically integers, and their neighbours.

    Two budgets cut the family: about 6 000 nodes in the table (so k stops at 4 for n = 100
    and at 1 for n = 300: 125 on-integer cases) and 1 024 groups in the core subset, which
    holds this whole family (so the neighbours of k = 4, 5 exist only at n <= 3, T <= 70)."""
    up = {"taint_lower_pct": 0, "taint_upper_pct": 0}
    for n in (1, 3, 7, 10, 100, 300):
        for T in (1, 3, 50, 70, 99):
            for k in (range(1, 6) if n <= 10 else range(1, 5) if n == 100 else (1,)):
                for dr in ((-1, 0, 1) if n <= 10 and (k <= 3 or (n <= 3 and T <= 70)) else (0,)):
                    t.add("ceil", "n=%d T=%d k=%d req%+d" % (n, T, k, dr), [(10 * T * (n + k) + dr, 0)],
                          [(1000, Gi)] * n, dict(up, scale_up_pct=T), form="nodes", k=k, dr=dr)
    for cached in (1000, 3000, 4096, 7000):
        for T in (1, 3, 50, 70, 99):
            if cached * T % 100:
                continue
            for q in (1, 3):
                for dr in ((-1, 0, 1) if q == 1 else (0,)):
                    t.add("ceil", "from zero cached=%d T=%d q=%d req%+d" % (cached, T, q, dr),
                          [(q * cached * T // 100 + dr, 0)], [], dict(up, scale_up_pct=T),
                          {"cached_cpu_m": cached, "cached_mem_b": Gi}, form="zero", k=q, dr=dr)
    for T in (1, 3, 50, 70, 99):                       # the memory side: both operands through * 1000
        cached = 1000 * 1024
        for dr in (-1, 0, 1):
            t.add("ceil", "from zero mem cached=%d T=%d q=2 req%+d" % (cached, T, dr),
                  [(0, 2 * cached * T // 100 + dr)], [], dict(up, scale_up_pct=T),
                  {"cached_cpu_m": 1000, "cached_mem_b": cached}, form="zero", k=2, dr=dr)


def _conversions(t: _Table):
    """int64 -> float64 of sums that are no float64 (2^53 + 1 rounds to even), up to
    2^63 - 1, and negatives; every sum holds one container / node at 2^53, so the pods take
    K1's exact wide path and the nodes K2's split sums.  The memory side wraps in * 1000."""
    sums = [(1 << 53) + 1, (1 << 53) + 3, (1 << 62) + (1 << 9) + 1, (1 << 63) - 1,
            -((1 << 53) + 1), -((1 << 62) + (1 << 9) + 1), -(1 << 63)]
    for sp in sums:
        # 2^63 - 1 is the largest node sum K2 delivers without the overflow flag (the gates
        # family has 2 x 2^62 beside it) and converts to 2^63 in the divisor
        for sn in ((1 << 53) + 1, (1 << 53) + 3, (1 << 62) + (1 << 9) + 1, (1 << 63) - 1, -((1 << 53) + 1)):
            t.add("conversions", "cpu pods=%d nodes=%d" % (sp, sn), [(x, 0) for x in _big_parts(sp)],
                  [(x, Gi) for x in _big_parts(sn)])
            t.add("conversions", "mem pods=%d nodes=%d" % (sp, sn), [(0, x) for x in _big_parts(sp)],
                  [(1000, x) for x in _big_parts(sn)])


def _millivalue(t: _Table):
    """Quantity.MilliValue of bytes: * 1000 with int64 wrap."""
    W = (1 << 63) // 1000 + 1                          # the smallest amount whose product wraps (negative)
    wp = [(-5, x) for x in _split(W, 2)]
    t.add("millivalue", "request wraps negative, cpu negative: fast_down", wp, [(1000, 8 * Gi)])
    t.add("millivalue", "request wraps negative, cpu 50 %", [(250, x) for x in _split(W, 2)], [(1000, 8 * Gi)])
    t.add("millivalue", "request wraps negative, far", [(0, W + 12345678901), (0, 7)], [(1000, 8 * Gi)])
    t.add("millivalue", "request product wraps to 0", [(500, 1 << 60), (0, 1 << 60)], [(1000, 8 * Gi)])
    t.add("millivalue", "request product wraps to 1000", [(500, 1 << 60), (0, (1 << 60) + 1)], [(1000, 8 * Gi)])
    t.add("millivalue", "capacity product wraps to 0: divide by zero", [(500, Gi)], [(1000, 1 << 60)] * 2)
    t.add("millivalue", "capacity wraps negative", [(500, Gi)], [(1000, x) for x in _split(W, 2)])
    t.add("millivalue", "both wrap negative: positive percentage", [(500, W + 5000)], [(1000, W + 900)])
    t.add("millivalue", "both wrap, scale up", [(500, W + 5000), (0, 1 << 40)], [(1000, W + 900)])
    t.add("millivalue", "request wraps twice", [(500, (1 << 62) // 250 + 3)], [(1000, 8 * Gi)])
    # (a product that is no multiple of 1000, whose gauge truncates, needs a wrap: the cases above)
    t.add("millivalue", "negative request, no wrap: exact negative gauge", [(500, -1), (0, -(1 << 33))], [(1000, 8 * Gi)])
    t.add("millivalue", "from zero: wrapped request over wrapped cached", [(500, W + 5000)], [],
          state={"cached_cpu_m": 1000, "cached_mem_b": W + 900})


def _zero(t: _Table):
    """Scale from zero, thresholds the validation would refuse, zero capacity."""
    for cached in ((0, 0), (0, 8 * Gi), (4000, 0)):
        t.add("zero", "no untainted node, cached %r: delta 1" % (cached,), [(500, Gi)], [],
              state={"cached_cpu_m": cached[0], "cached_mem_b": cached[1]})
    t.add("zero", "cached (1, 1): delta beyond int32", [(1 << 30, 1 << 20)] * 20, [],
          state={"cached_cpu_m": 1, "cached_mem_b": 1}, wide=True)
    t.add("zero", "delta beyond int64", [(1 << 62, 1)], [], {"scale_up_pct": 1},
          {"cached_cpu_m": 1, "cached_mem_b": 1})
    t.add("zero", "negative cached cpu, memory decides", [(5000, Gi)], [],
          state={"cached_cpu_m": -1000, "cached_mem_b": 8 * Gi})
    t.add("zero", "negative cached, needs -7 and -0", [(5000, Gi)], [],
          state={"cached_cpu_m": -1000, "cached_mem_b": -8 * Gi})
    t.add("zero", "negative cached, negative delta", [(5000, 64 * Gi)], [],
          state={"cached_cpu_m": -1000, "cached_mem_b": -8 * Gi})
    t.add("zero", "needs in (-1, 0): ceil -> -0, max(-0, -0), int(-0)", [(1, 1)], [],
          state={"cached_cpu_m": -1000, "cached_mem_b": -1000})
    t.add("zero", "needs -0 and +0", [(1, 0)], [], state={"cached_cpu_m": -1000, "cached_mem_b": 1000})
    z = {"taint_lower_pct": 0, "taint_upper_pct": 0, "scale_up_pct": 0}
    two = [(1000, 8 * Gi)] * 2
    t.add("zero", "scale_up 0, two nodes: Inf, Inf", [(1000, Gi)], two, z)
    t.add("zero", "scale_up 0, memory 0 %: max(Inf, NaN)", [(1000, 0)], two, z)
    t.add("zero", "scale_up 0, cpu 0 %: max(NaN, Inf)", [(0, Gi)], two, z)
    t.add("zero", "scale_up 0, cpu negative: max(-Inf, Inf)", [(-5, Gi)], two, z)
    t.add("zero", "scale_up 0, both 0 %: no scale up", [(0, 0)], two, z)
    c48 = {"cached_cpu_m": 4000, "cached_mem_b": 8 * Gi}
    t.add("zero", "scale_up 0 from zero: Inf", [(500, Gi)], [], z, c48)
    t.add("zero", "scale_up 0 from zero, cpu request 0: max(NaN, Inf)", [(0, Gi)], [], z, c48)
    t.add("zero", "scale_up 0 from zero, memory request 0: max(Inf, NaN)", [(500, 0)], [], z, c48)
    neg = {"taint_lower_pct": -20, "taint_upper_pct": -10, "scale_up_pct": -5}
    t.add("zero", "scale_up -5, nothing requested, no node: 0 * -1 = -0", [(0, 0)], [], neg)
    t.add("zero", "scale_up -5, two nodes: negative delta", [(100, 0)], two, neg)
    # (0 * Inf and max(NaN, NaN) cannot be reached: n_untainted = 0 with finite percentages
    # means all four totals are 0, so both percentages are 0 and nothing exceeds scale_up 0.)
    stale = {"cached_cpu_m": 999, "cached_mem_b": 999}
    t.add("zero", "every node tainted or cordoned: cached from the first node",
          [(3000, Gi)], [(2000, 8 * Gi, "taint"), (4000, 16 * Gi, "cordon"), (1000, Gi, "both")], state=stale)
    t.add("zero", "first node cordoned, odd capacity", [(3000, 7 * Gi)], [(1234, 5 * Gi + 1, "cordon"), (64000, Gi, "taint")],
          state=stale)
    t.add("zero", "first node without allocatable cpu: delta 1", [(3000, Gi)], [(None, 8 * Gi, "taint")], state=stale)
    for what, node in (("cpu", (0, 8 * Gi)), ("mem", (1000, 0)), ("both", (0, 0)), ("absent", (None, None))):
        t.add("zero", "capacity zero (%s) with an untainted node: divide by zero" % what, [(100, Gi)], [node])
    t.add("zero", "nothing requested of zero capacity, one node: divide by zero", [(0, 0)], [(0, 0)])


def _gates(t: _Table):
    node = (1000, 8 * Gi)
    t.add("gates", "empty")
    for n in (1, 2, 4, 5):
        t.add("gates", "min 2, max 4, %d nodes" % n, [(500, Gi)], [node] * n, {"min_nodes": 2, "max_nodes": 4})
    t.add("gates", "pods and no node under min 1", [(500, Gi)], [], {"min_nodes": 1})
    t.add("gates", "pod memory beyond int64", [(1, 1 << 62)] * 3, [node])
    t.add("gates", "pod cpu beyond int64", [(1 << 62, 1)] * 2, [node])
    t.add("gates", "pod cpu below int64", [(-(1 << 62), 1)] * 3, [node])
    t.add("gates", "node cpu beyond int64", [(500, Gi)], [(1 << 62, 8 * Gi)] * 2)
    t.add("gates", "node memory beyond int64", [(500, Gi)], [(1000, 1 << 62)] * 2 + [node])
    t.add("gates", "beyond int64 behind the max gate", [(1, 1 << 62)] * 3, [node] * 3, {"max_nodes": 2})
    t.add("gates", "only tainted capacity beyond int64: no overflow", [(500, Gi)],
          [(1 << 62, 1 << 62, "taint")] * 2 + [node])
    t.add("gates", "below min: 3 nodes, 1 untainted, min 2", [(500, Gi)], [node, node + ("taint",), node + ("cordon",)],
          {"min_nodes": 2})
    for req in (0, 5, -3):
        t.add("gates", "locked, requested %d" % req, [(900, Gi)], [node] * 2, state={"locked": True, "requested_nodes": req})
    for kind in ("fast", "slow"):
        for min_nodes, n in ((2, 4), (2, 5), (2, 6), (2, 2), (0, 2), (0, 3), (0, 4)):
            spec = {"min_nodes": min_nodes, "slow_removal_rate": 3 if kind == "slow" else 1,
                    "fast_removal_rate": 3 if kind == "fast" else 5}
            pods = [] if kind == "fast" else [(400 * n, Gi)]
            t.add("gates", "%s rate 3, %d untainted, min %d" % (kind, n, min_nodes), pods, [node] * n + [node + ("taint",)],
                  spec)
    t.add("gates", "fast rate 0", [], [node] * 3, {"fast_removal_rate": 0})
    t.add("gates", "dry mode with tracker entries", [(800, Gi)],
          [node, node + ("taint",), node + ("cordon",), node, node], {"dry_mode": True, "min_nodes": 1},
          tracker=[3, 4, "ghost-node"])
    t.add("gates", "dry mode, every node tracked", [(800, Gi)], [node, node], {"dry_mode": True}, tracker=[0, 1])
    t.add("gates", "the default group", [(2500, Gi), (300, 2 * Gi)], [node] * 3, default=True)


def expect(case: dict, state: dict | None = None) -> tuple[dict, dict]:
    """The literal oracle's run of one case over that case's objects, and its gauges."""
    out = O.scale_node_group(case["group"], case["state"] if state is None else state, case["pods"], case["nodes"],
                             tracker=case["tracker"])
    return out, O.node_group_metrics(out)


def build(seed: int = 0, n_division: int = 88) -> list[dict]:
    t = _Table()
    _thresholds(t)
    _ceil(t)
    _conversions(t)
    _millivalue(t)
    _zero(t)
    _gates(t)
    _division(t, random.Random(0xD1F + seed), n_division)      # last: the core subset is a prefix
    for c in t.cases:
        c["want"], c["want_metrics"] = expect(c)
    return t.cases


def core(cases: list[dict], n_division: int = 8) -> list[dict]:
    """Every family, with the first n_division cases of each side of the division family."""
    out, seen = [], {"cpu": 0, "mem": 0}
    for c in cases:
        if c["family"] == "division":
            seen[c["tags"]["side"]] += 1
            if seen[c["tags"]["side"]] > n_division:
                continue
        out.append(c)
    return out


def coverage(cases: list[dict]) -> dict:
    """What the table reaches, from the oracle's outputs (case["want"]) alone."""
    cov = {"branches": {}, "statuses": {}, "families": {}, "ceil_k": 0, "ceil_k1": 0, "ceil_other": 0, "division": 0,
           "delta_gt_2_31": 0, "delta_int64_min": 0, "negative_pct": 0, "total_ge_2_53": 0, "taint_clamped": 0,
           "sides": {}}
    for c in cases:
        w, tags = c["want"], c["tags"]
        cov["families"][c["family"]] = cov["families"].get(c["family"], 0) + 1
        cov["branches"][w["branch"]] = cov["branches"].get(w["branch"], 0) + 1
        st = STATUS[w["err"]]
        cov["statuses"][st] = cov["statuses"].get(st, 0) + 1
        if w["taint_err"] is not None:
            cov["statuses"][ST_TAINT_MIN] = cov["statuses"].get(ST_TAINT_MIN, 0) + 1
        if c["family"] == "ceil" and tags["dr"] == 0 and tags["form"] == "nodes":
            key = "ceil_k" if w["delta"] == tags["k"] else "ceil_k1" if w["delta"] == tags["k"] + 1 else "ceil_other"
            cov[key] += 1
        if c["family"] == "division" and w["pod_cpu_m"] is not None:
            if tags["side"] == "cpu":
                ok = divides_differently(w["pod_cpu_m"], w["node_cpu_m"])
            else:
                ok = divides_differently(O.milli_value_mem(w["pod_mem_b"]), O.milli_value_mem(w["node_mem_b"]))
            cov["division"] += bool(ok)
        if c["family"] == "thresholds":
            hit = {"lower": "fast_down", "upper": "slow_down", "up": "scale_up"}[tags["probe"]]
            key = (tags["probe"], w["branch"] == hit)
            cov["sides"][key] = cov["sides"].get(key, 0) + 1
        cov["delta_gt_2_31"] += w["delta"] > (1 << 31)
        cov["delta_int64_min"] += w["delta"] == INT64_MIN
        cov["negative_pct"] += w["cpu_pct"] < 0 or w["mem_pct"] < 0
        cov["total_ge_2_53"] += any(w[k] is not None and abs(w[k]) >= (1 << 53)
                                    for k in ("pod_cpu_m", "pod_mem_b", "node_cpu_m", "node_mem_b"))
        cov["taint_clamped"] += w["delta"] < 0 and w["err"] is None and w["n_to_taint"] != -w["delta"]
    return cov


# ------------------------------------------------------------------ one cluster
def assemble(cases: list[dict]) -> dict:
    """The cases as one cluster, in the given order: groups, states, pods, nodes, trackers
    ({group: names}) and each case's first node index."""
    out = {"groups": [], "states": [], "pods": [], "nodes": [], "trackers": {}, "node_base": []}
    for g, c in enumerate(cases):
        out["groups"].append(c["group"])
        out["states"].append(c["state"])
        out["node_base"].append(len(out["nodes"]))
        out["pods"] += c["pods"]
        out["nodes"] += c["nodes"]
        if c["tracker"]:
            out["trackers"][g] = c["tracker"]
    return out


def flipped_states(cases: list[dict]) -> list[dict]:
    """Every case's lock flipped and its cached capacities swapped."""
    return [{"locked": not c["state"]["locked"], "requested_nodes": c["state"]["requested_nodes"],
             "cached_cpu_m": c["state"]["cached_mem_b"], "cached_mem_b": c["state"]["cached_cpu_m"]} for c in cases]


def oracle_arrays(cases: list[dict], node_base: list[int], states: list[dict] | None = None):
    """The literal oracle's expectation in the layout of the results: totals int64 [G, 13]
    with a mask of the fields the oracle gives (the four sums are unknown where a Quantity
    left int64; `flags` holds 1 there, to be compared as non-zero), percentages float64
    [G, 2], the seven integer decision fields int64 [G, 7], and the gauges."""
    G = len(cases)
    tot, known = np.zeros((G, 13), np.int64), np.ones((G, 13), bool)
    df, di, mets = np.zeros((G, 2), np.float64), np.zeros((G, 7), np.int64), []
    for g, c in enumerate(cases):
        w, m = (c["want"], c["want_metrics"]) if states is None else expect(c, states[g])
        mets.append(m)
        first = c["nodes"][0] if c["nodes"] else None
        fc, fm = O.node_alloc(first) if first else (0, 0)
        sums = [w["pod_cpu_m"], w["pod_mem_b"], w["node_cpu_m"], w["node_mem_b"]]
        over = sums[0] is None
        if over:
            known[g, [0, 1, 3, 4]] = False
            sums = [0, 0, 0, 0]
        tot[g] = [sums[0], sums[1], w["n_pods"], sums[2], sums[3], w["n_nodes"], w["n_untainted"], w["n_tainted"],
                  w["n_cordoned"], node_base[g] + w["first_node"] if w["first_node"] >= 0 else -1, fc, fm, int(over)]
        df[g] = [w["cpu_pct"], w["mem_pct"]]
        di[g] = [w["delta"], w["n_to_taint"], w["cached_cpu_m"], w["cached_mem_b"], STATUS[w["err"]],
                 BRANCHES.index(w["branch"]), 0 if w["taint_err"] is None else ST_TAINT_MIN]
    return tot, known, df, di, mets


def describe(case: dict) -> str:
    def short(xs, f):
        return "[%s%s]" % (", ".join(f(x) for x in xs[:4]), ", ... %d in all" % len(xs) if len(xs) > 4 else "")
    return "case %d, family %s: %s\n  spec %r\n  state %r\n  pods %s\n  nodes %s\n  tracker %r" % (
        case["id"], case["family"], case["desc"], {k: v for k, v in case["group"].items() if k != "label_key"},
        case["state"], short(case["pods"], lambda p: "(%r, %r)" % (p["containers"][0]["cpu"], p["containers"][0]["mem"])),
        short(case["nodes"], lambda n: "(%r, %r%s%s)" % (n["cpu"], n["mem"], ", cordoned" if n["unschedulable"] else "",
                                                         ", tainted" if n["taints"] else "")), case["tracker"])


def compare(cases, what, tot, df, di, rtot, rknown, rdf, rdi):
    """Results (totals int64 [G, 13], percentages [G, 2], integers [G, 7]) against a
    reference in the same layout: integers equal, percentages equal as bits, flags equal as
    non-zero where the reference only knows that; a mismatch names the case."""
    bad = np.zeros(len(cases), bool)
    why = [""] * len(cases)

    def note(mask, text):
        for g in np.nonzero(mask & ~bad)[0]:
            why[g] = text(g)
        bad[:] |= mask

    for k, name in enumerate(TOT_FIELDS):
        a, b = tot[:, k], rtot[:, k]
        if name == "flags" and rknown is not None:
            a, b = (a != 0), (b != 0)
        m = (a != b) & (rknown[:, k] if rknown is not None else True)
        note(m, lambda g, k=k, name=name: "%s: got %d, want %d" % (name, tot[g, k], rtot[g, k]))
    for k, name in enumerate(("cpu_pct", "mem_pct")):
        a, b = np.ascontiguousarray(df[:, k]).view(np.uint64), np.ascontiguousarray(rdf[:, k]).view(np.uint64)
        note(a != b, lambda g, k=k, name=name: "%s: got %r (%#018x), want %r (%#018x)" % (
            name, float(df[g, k]), int(a[g]), float(rdf[g, k]), int(b[g])))
    for k, name in enumerate(DEC_FIELDS):
        note(di[:, k] != rdi[:, k], lambda g, k=k, name=name: "%s: got %d, want %d" % (name, di[g, k], rdi[g, k]))
    if bad.any():
        idx = np.nonzero(bad)[0]
        raise AssertionError("%s: %d of %d cases differ; the first:\n%s\n%s" % (
            what, len(idx), len(cases), "\n".join("group %d: %s\n%s" % (g, why[g], describe(cases[g])) for g in idx[:3]),
            "families: %r" % sorted({cases[g]["family"] for g in idx})))


def gauge_mismatch(met, expected, names):
    """The first group whose gauges (esc_metrics_results) differ from the expected ones by
    check_metrics' rule — the same set mask, every set gauge equal as bits — and what
    differs; None when all agree.  names: _lib.METRIC_NAMES."""
    for g, e in enumerate(expected):
        mask = sum(1 << k for k, n in enumerate(names) if n in e)
        if int(met["set_mask"][g]) != mask:
            return g, "set_mask: got %#x, want %#x" % (int(met["set_mask"][g]), mask)
        for n, v in e.items():
            a, b = np.float64(met[n][g]).view(np.uint64), np.float64(v).view(np.uint64)
            if a != b:
                return g, "%s: got %r (%#018x), want %r (%#018x)" % (n, float(met[n][g]), int(a), float(v), int(b))
    return None


def result_arrays(tot, dec):
    """esc_results' structured arrays in the layout above."""
    t = np.stack([tot[n].astype(np.int64) for n in TOT_FIELDS], axis=1)
    df = np.stack([dec["cpu_pct"], dec["mem_pct"]], axis=1)
    di = np.stack([dec[n].astype(np.int64) for n in DEC_FIELDS], axis=1)
    return t, df, di
