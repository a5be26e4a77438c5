"""calculateNewNodeMetrics (pkg/controller/controller.go:157-189) restated literally, with
the Prometheus histogram it feeds (pkg/metrics/metrics.go:185-193), as the checker of the
device pass (esc_new_nodes_eval).  Node records are the plain dicts of tests/randobj.py;
`inst` maps a node name to its instance's instantiation time in Unix ns — a name that is
missing (or maps to None) is GetInstance's error.

The bucket is picked with floats exactly as Prometheus does (the first upper bound >=
lag.Seconds(), else +Inf); `bucket_of_int` is the integer rule of the ABI, and the tests
check the two against each other."""
from __future__ import annotations

from oracle import oracle as O

I64_MIN, I64_MAX = -(1 << 63), (1 << 63) - 1
# metrics.go:190
BUCKETS = [60.0, 120.0, 180.0, 240.0, 300.0, 360.0, 420.0, 480.0, 540.0, 600.0, 660.0, 720.0, 780.0, 840.0, 900.0,
           960.0, 1020.0, 1080.0, 1140.0, 1200.0, 1260.0, 1320.0, 1380.0, 1440.0, 1500.0, 1560.0, 1620.0, 1680.0,
           1740.0]
N_BUCKETS = len(BUCKETS) + 1                        # and +Inf
LAG_OVERFLOW = 1


def time_sub(t_ns: int, u_ns: int) -> int:
    """time.Time.Sub: t - u as a Duration, saturated to the int64 range."""
    return max(I64_MIN, min(I64_MAX, t_ns - u_ns))


def duration_seconds(d_ns: int) -> float:
    """time.Duration.Seconds: float64(d / Second) + float64(d % Second) / 1e9 (Go's / and %
    truncate toward zero)."""
    sec = abs(d_ns) // 1_000_000_000 * (1 if d_ns >= 0 else -1)
    nsec = d_ns - sec * 1_000_000_000
    return float(sec) + float(nsec) / 1e9


def bucket_of_float(seconds: float) -> int:
    """prometheus histogram.findBucket: the first upper bound >= v, else the +Inf bucket."""
    for k, bound in enumerate(BUCKETS):
        if seconds <= bound:
            return k
    return len(BUCKETS)


def bucket_of_int(lag_ns: int) -> int:
    """The ABI's rule: the first k with lag_ns <= 60e9 * (k + 1), else 29."""
    for k in range(len(BUCKETS)):
        if lag_ns <= 60_000_000_000 * (k + 1):
            return k
    return len(BUCKETS)


def group_nodes(group: dict, nodes: list[dict]) -> list[int]:
    """Indices of the group's allNodes (controller.go:201, :259: the NodeInfoMap is built
    from allNodes — untainted, tainted and cordoned alike)."""
    f = O.new_node_label_filter_func(group.get("label_key", ""), group.get("label_value", ""))
    keep = set(id(n) for n in O.filtered_list(nodes, f))
    return [i for i, n in enumerate(nodes) if id(n) in keep]


def calculate_new_node_metrics(group: dict, nodes: list[dict], since_ns: int, inst: dict) -> dict:
    """controller.go:165-188 for one group whose scaleDelta > 0.  since_ns = lastScaleOut
    (I64_MIN: the zero time.Time; I64_MAX: the function is not reached: the zero record).
    Returns the record's fields, and the new nodes as (index, known) pairs."""
    out = {"n_new": 0, "n_observed": 0, "lag_sum_ns": 0, "flags": 0, "bucket": [0] * N_BUCKETS, "list": []}
    if since_ns == I64_MAX:
        return out
    total = 0
    for i in group_nodes(group, nodes):                         # :168 (map order: any)
        node_reg_time = int(nodes[i].get("created_ns", 0))     # :169
        # :171 nodeRegTime.Sub(lastScaleOut) > 0; against the zero time every node is newer
        if not (since_ns == I64_MIN or time_sub(node_reg_time, since_ns) > 0):
            continue
        out["n_new"] += 1
        t = inst.get(nodes[i].get("name", ""))                  # :173 GetInstance
        out["list"].append((i, 0 if t is None else 1))
        if t is None:                                           # :174-175 skipped, not counted
            continue
        lag = time_sub(node_reg_time, int(t))                   # :177
        out["bucket"][bucket_of_float(duration_seconds(lag))] += 1   # :179 Observe(lag.Seconds())
        total += lag
        out["n_observed"] += 1                                  # :180 countNewNodes++
    if not I64_MIN <= total <= I64_MAX:
        out["flags"] |= LAG_OVERFLOW
    out["lag_sum_ns"] = (total + (1 << 63)) % (1 << 64) - (1 << 63)   # the low 64 bits
    return out
