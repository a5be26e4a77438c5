"""GPU: ResidentController (events -> resident snapshot -> decision) in lock-step with the
unchanged Controller (re-list, re-pack, reload every scan) on one seeded history.

``FakeCluster`` is the API server of the test: it holds the objects in insertion order, serves
as the actuator of its controller and turns its own writes (taint, untaint, delete, the cloud
add that creates nodes a scan later) and a seeded churn script into informer events.  Two
copies get the same churn; one feeds ``ResidentController.events``, the other serves the
listers of ``Controller``.  Equal results on every scan keep the two copies equal."""
import copy
import random
import struct

import pytest

from oracle import oracle as O
from randobj import make_groups, make_nodes, make_pods

pytestmark = pytest.mark.gpu

TAINT = "atlassian.com/escalator"
NO_DELETE = "atlassian.com/no-delete"
T0 = 1_700_000_000 * 10**9
SCAN_NS = 60 * 10**9
SCANS = 6
BURST_SCAN, BURST_NODES = 3, 20


def _bits(x):
    return struct.pack("<d", float(x))


def _engineered():
    """Five groups whose first scans are known: a cloud add, an untaint walk (then a reap of
    what stays tainted), taint walks followed by reaps, dry-mode taints, and a steady group
    that takes the burst of node adds."""
    common = dict(label_key="pool", taint_lower_pct=20, taint_upper_pct=40, scale_up_pct=70, slow_removal_rate=1,
                  fast_removal_rate=2, scale_up_cool_down_ns=2 * SCAN_NS, dry_mode=False)
    shapes = [("up", 4, 0, 10, 1500, 1, 40), ("untaint", 3, 3, 9, 1200, 1, 40), ("down", 10, 0, 2, 500, 2, 40),
              ("drydown", 8, 0, 2, 500, 2, 40), ("hold", 12, 0, 12, 2200, 1, 200)]
    groups, pods, nodes = [], [], []
    for name, n_unt, n_tnt, n_pods, cpu, mn, mx in shapes:
        groups.append(dict(common, name=name, label_value=name, min_nodes=mn, max_nodes=mx, dry_mode=name == "drydown"))
        for i in range(n_unt + n_tnt):
            x = {"name": "%s-%d" % (name, i), "labels": {"pool": name}, "unschedulable": False, "taints": [],
                 "cpu": 4000, "mem": 8 << 30, "created_ns": T0 - (10**6 - len(nodes)) * 1000}
            if i >= n_unt:
                x["taints"], x["taint_value"] = [TAINT], str(T0 // 10**9 - 30)
            nodes.append(x)
        for i in range(n_pods):
            bound = "%s-%d" % (name, n_unt - 1 - i % 2) if i < 4 else ""       # on the two newest untainted nodes
            pods.append({"name": "%s-pod-%d" % (name, i), "owner_kinds": [], "annotations": {},
                         "node_selector": {"pool": name}, "affinity": None, "containers": [{"cpu": cpu, "mem": 1 << 28}],
                         "init_containers": [], "overhead": None, "node_name": bound})
    return groups, pods, nodes


def make_cluster(seed):
    rng = random.Random(seed)
    rnd_groups = make_groups(rng, rng.choice([3, 5, 7]), with_default=True)
    for g in rnd_groups:
        g["scale_up_cool_down_ns"] = rng.choice([0, SCAN_NS, 3 * SCAN_NS])
    eg, ep, en = _engineered()
    groups = rnd_groups + eg
    for g in groups:
        g["soft_delete_grace_ns"], g["hard_delete_grace_ns"] = SCAN_NS, 3 * SCAN_NS + 1
    nodes = make_nodes(rng, 30, rnd_groups, big_frac=0.0)
    for x in nodes:
        x["taint_value"] = str(T0 // 10**9 - rng.randrange(0, 300))
    for g in rnd_groups:                                       # the cloud adds stay small: a few nodes per group
        f = O.new_node_label_filter_func(g["label_key"], g["label_value"])
        if g["max_nodes"]:
            g["max_nodes"] = sum(1 for x in nodes if f(x)) + rng.choice([0, 2, 4])
    pods = make_pods(rng, 300, rnd_groups, big_frac=0.0)
    for p in pods:
        r = rng.random()
        p["node_name"] = "" if r < 0.2 else ("ghost" if r < 0.25 else rng.choice(nodes)["name"])
    return groups, pods + ep, nodes + en, rnd_groups


class FakeCluster:
    def __init__(self, seed, groups, rnd_groups, clock, burst):
        self.seed, self.groups, self.rnd_groups, self.clock, self.burst = seed, groups, rnd_groups, clock, burst
        self.nodes, self.pods = {}, {}            # insertion order = the listers' order
        self.sink = None                          # an EventQueue, or None (listers only)
        self.resolve = None                       # node index of this copy's controller -> name
        self.pending = []                         # cloud adds: nodes that register a scan later
        self.returning = {}                       # scan -> node records that come back under their name
        self.serial = 0
        self.fail = {"down-0"}                    # taint writes that fail (the walk moves on)

    # -- the object store; every change is an informer event
    def put_node(self, x):
        self.nodes[x["name"]] = x
        if self.sink is not None:
            self.sink.node_add(x)

    def del_node(self, name):
        if self.nodes.pop(name, None) is not None and self.sink is not None:
            self.sink.node_delete(name)

    def put_pod(self, p):
        self.pods[p["name"]] = p
        if self.sink is not None:
            self.sink.pod_add(p)

    def del_pod(self, name):
        if self.pods.pop(name, None) is not None and self.sink is not None:
            self.sink.pod_delete(name)

    def list_pods(self):
        return list(self.pods.values())

    def list_nodes(self):
        self.listed = list(self.nodes)
        return list(self.nodes.values())

    # -- the actuator (controller.ACTUATOR_METHODS)
    def taint(self, g, j):
        x = self.nodes[self.resolve(j)]
        if x["name"] in self.fail:
            return False
        self.put_node(dict(x, taints=x["taints"] + [TAINT], taint_value=str(self.clock() // 10**9)))
        return True

    def untaint(self, g, j):
        x = self.nodes[self.resolve(j)]
        self.put_node(dict(x, taints=[t for t in x["taints"] if t != TAINT], taint_value=None))
        return True

    def _members(self, g):
        f = O.new_node_label_filter_func(self.groups[g].get("label_key", ""), self.groups[g].get("label_value", ""))
        return [x for x in self.nodes.values() if f(x)]

    def target_size(self, g):
        return len(self._members(g)) + sum(n for h, n in self.pending if h == g)

    def max_size(self, g):
        return int(self.groups[g].get("max_nodes", 0))

    def increase_size(self, g, n):
        self.pending.append((g, n))

    def delete_nodes(self, g, nodes):
        for name in [self.resolve(j) for j in nodes]:
            self.del_node(name)

    # -- the seeded churn of one scan (identical on both copies while their stores are equal)
    def churn(self, scan, tracked):
        rng = random.Random(self.seed * 1000 + scan)
        now = self.clock()
        for g, n in self.pending:                              # the cloud's nodes register
            grp = self.groups[g]
            for _ in range(n):
                self.serial += 1
                self.put_node({"name": "cloud-%d" % self.serial, "labels": {grp["label_key"]: grp["label_value"]},
                               "unschedulable": False, "taints": [], "cpu": 4000, "mem": 8 << 30, "created_ns": now})
        self.pending = []
        for x in self.returning.pop(scan, []):                 # back under the old name: a new node
            self.put_node(dict(x, created_ns=now))
        rnd_nodes = [m for m in self.nodes if m.startswith(("node-", "add"))]
        rnd_pods = [k for k in self.pods if k.startswith(("p", "c"))]
        # pods: deletes, spec changes, adds (bound, unbound, naming a node that comes a scan later)
        for k in rng.sample(rnd_pods, 6):
            self.del_pod(k)
            rnd_pods.remove(k)
        for k in rng.sample(rnd_pods, 6):
            q = make_pods(rng, 1, self.rnd_groups, big_frac=0.0)[0]
            self.put_pod(dict(q, name=k, node_name=self.pods[k]["node_name"]))
        fresh = make_pods(rng, 6, self.rnd_groups, big_frac=0.0)
        for i, q in enumerate(fresh):
            to = ["", rng.choice(rnd_nodes), rng.choice(rnd_nodes), "add%d-0" % (scan + 1), "add%d-0" % scan][i % 5]
            self.put_pod(dict(q, name="c%d-%d" % (scan, i), node_name=to))
        for k in rng.sample(rnd_pods, 6):                      # scheduled, moved, unbound
            to = rng.choice([rng.choice(rnd_nodes), rng.choice(rnd_nodes), ""])
            self.put_pod(dict(self.pods[k], node_name=to))
        # nodes: deletes (one tracked by a dry group, one that returns two scans later)
        gone = rng.sample(rnd_nodes, 2)
        if scan == 2 and tracked:
            gone.append(sorted(tracked)[0])
        for m in gone:
            if m not in self.nodes:
                continue
            if m != gone[0]:                                   # the first one stays away
                self.returning.setdefault(scan + 2, []).append(self.nodes[m])
            self.del_node(m)
            if m in rnd_nodes:
                rnd_nodes.remove(m)
        new = make_nodes(rng, 3, self.rnd_groups, big_frac=0.0)          # older, newer, equal creation times
        some = self.nodes[rng.choice(rnd_nodes)]["created_ns"]
        for i, x in enumerate(new):
            x["name"] = "add%d-%d" % (scan, i)
            x["created_ns"] = [T0 - 10**15, now, some][i]
            x["taint_value"] = str(now // 10**9 - 200)
            self.put_node(x)
        if scan == BURST_SCAN and self.burst:                  # the marked burst: one label pair
            for i in range(BURST_NODES):
                self.put_node({"name": "burst-%d" % i, "labels": {"pool": "hold"}, "unschedulable": False, "taints": [],
                               "cpu": 4000, "mem": 8 << 30, "created_ns": now + i})
        for m in rng.sample(rnd_nodes, 3):                     # relabels between groups
            x = make_nodes(rng, 1, self.rnd_groups, big_frac=0.0)[0]
            self.put_node(dict(self.nodes[m], labels=x["labels"]))
        for m in rng.sample(rnd_nodes, 3):                     # cordons
            self.put_node(dict(self.nodes[m], unschedulable=not self.nodes[m]["unschedulable"]))
        for m in rng.sample(rnd_nodes, 2):                     # allocatable
            self.put_node(dict(self.nodes[m], cpu=rng.choice([2000, 16000]), mem=rng.choice([8 << 30, 64 << 30])))
        for m in rng.sample(rnd_nodes, 4):                     # taint value / no-delete only
            x = self.nodes[m]
            if rng.random() < 0.6:
                self.put_node(dict(x, taint_value=str(now // 10**9 - rng.choice([100, 500]))))
            else:
                self.put_node(dict(x, annotations={} if (x.get("annotations") or {}).get(NO_DELETE) else {NO_DELETE: "true"}))
        for m in rng.sample(rnd_nodes, 2):                     # an annotation nothing reads
            self.put_node(dict(self.nodes[m], annotations=dict(self.nodes[m].get("annotations") or {}, note=str(scan))))


def _record(r, name_of):
    out = {k: r.get(k) for k in ("delta", "err", "branch", "n_to_taint", "added", "pods_evicted", "action_err",
                                 "walk_fallback", "reap_err")}
    out["pct"] = (_bits(r["cpu_pct"]), _bits(r["mem_pct"])) if "cpu_pct" in r else None
    for k in ("tainted_now", "untainted_now", "removed"):
        out[k] = [name_of(j) for j in r.get(k, [])]
    t = dict(r.get("totals", {}))
    if "first_node" in t:
        t["first_node"] = name_of(t["first_node"]) if t["first_node"] >= 0 else None
    out["totals"] = t
    return out


def _check_literal(groups, states, trackers, pods, nodes, out, scan):
    from escalator_amd.controller import ERRORS  # noqa: F401
    for g, grp in enumerate(groups):
        L = O.scale_node_group(grp, states[g], pods, nodes, tracker=trackers[g])
        r, t = out[g], out[g]["totals"]
        assert (t["n_pods"], t["n_nodes"], t["n_untainted"], t["n_tainted"], t["n_cordoned"]) == \
            (L["n_pods"], L["n_nodes"], L["n_untainted"], L["n_tainted"], L["n_cordoned"]), (scan, g)
        assert t["first_node"] == (nodes[L["first_node"]]["name"] if L["first_node"] >= 0 else None), (scan, g)
        if L["pod_cpu_m"] is not None:
            assert (t["pod_cpu_m"], t["pod_mem_b"], t["node_cpu_m"], t["node_mem_b"]) == \
                (L["pod_cpu_m"], L["pod_mem_b"], L["node_cpu_m"], L["node_mem_b"]), (scan, g)
        assert r["branch"] == L["branch"], (scan, g)
        assert r["pct"] == (_bits(L["cpu_pct"]), _bits(L["mem_pct"])), (scan, g)
        assert r["n_to_taint"] == L["n_to_taint"], (scan, g)
        if L["branch"] != "below_min":                         # there the record holds ScaleUp's result
            assert r["delta"] == L["delta"], (scan, g)


def drive(seed, spare, make_resident, make_reload, burst):
    """Runs SCANS scans of both controllers on the seeded history; returns what the
    assertions of the tests need."""
    groups, pods, nodes, rnd_groups = make_cluster(seed)
    clock = [T0]
    A = FakeCluster(seed, groups, rnd_groups, lambda: clock[0], burst)
    B = FakeCluster(seed, groups, rnd_groups, lambda: clock[0], burst)
    ra = make_resident(groups, lambda: clock[0], A, spare)
    rb = make_reload(groups, lambda: clock[0], B)
    A.sink, A.resolve = ra.events, ra.events.node_name
    B.resolve = lambda j: B.listed[j]
    for c in (A, B):
        for x in nodes:
            c.put_node(x)
        for p in pods:
            c.put_pod(p)
    seen = {"taint": False, "untaint": False, "added": False, "reaped": False, "dry_seen": False}
    dry_tainted = {}
    reloads = []
    for scan in range(SCANS):
        tracked = sorted({m for g, t in rb.taint_tracker.items() for m in t if m in B.nodes})
        A.churn(scan, tracked)
        B.churn(scan, tracked)
        assert list(A.nodes) == list(B.nodes) and A.pods == B.pods and A.nodes == B.nodes, scan
        rb._lock_states(clock[0])                              # what run_once does first (idempotent)
        states, trackers = copy.deepcopy(rb.state), {g: list(t) for g, t in rb.taint_tracker.items()}
        cur_pods, cur_nodes = B.list_pods(), B.list_nodes()
        out_a = [_record(r, A.resolve) for r in ra.run_once()]
        out_b = [_record(r, B.resolve) for r in rb.run_once(B.list_pods, B.list_nodes)]
        reloads.append(ra.events.reloads)
        assert [x["name"] for x in ra.events.live_nodes()] == [x["name"] for x in cur_nodes], scan
        for g in range(len(groups)):
            assert out_a[g] == out_b[g], (scan, g, out_a[g], out_b[g])
        assert ra.state == rb.state and ra.taint_tracker == rb.taint_tracker and ra.lock_time == rb.lock_time, scan
        _check_literal(groups, states, trackers, cur_pods, cur_nodes, out_a, scan)
        for g, r in enumerate(out_a):
            dry = groups[g]["dry_mode"]
            seen["taint"] |= bool(r["tainted_now"]) and not dry
            seen["untaint"] |= bool(r["untainted_now"]) and not dry
            seen["added"] |= r["added"] > 0
            seen["reaped"] |= bool(r["removed"])
            if dry and dry_tainted.get(g) and r["totals"]["n_tainted"] > 0:
                seen["dry_seen"] = True                        # filterNodes saw an earlier scan's dry taint
            if dry and r["tainted_now"]:
                dry_tainted[g] = True
        clock[0] += SCAN_NS
    return ra, rb, seen, reloads


def _resident(groups, clock, actuator, spare):
    from escalator_amd.controller import ResidentController
    return ResidentController(groups, clock=clock, actuator=actuator, spare=spare)


def _reload(groups, clock, actuator):
    from escalator_amd.controller import Controller
    return Controller(groups, clock=clock, actuator=actuator)


@pytest.mark.parametrize("seed", [1, 10])       # 8 and 12 groups, 2 and 3 of them dry
def test_resident_parity_generous_spare(seed):
    """Spare 2.0 (what the event tests use): every scan's records are equal between the two
    controllers and equal the literal oracle; the walks, the cloud add, a reap and a dry-mode
    taint read back by filterNodes all happened; no reload beyond the initial load, and every
    kind of event was applied in place."""
    ra, rb, seen, reloads = drive(seed, 2.0, _resident, _reload, burst=True)
    assert all(seen.values()), seen
    assert reloads == [1] * SCANS, (reloads, ra.events.reload_causes)
    assert all(n > 0 for n in ra.events.applied.values()), ra.events.applied
    assert ra.events.flushes == SCANS


def test_resident_one_reload_when_the_burst_does_not_fit():
    """Spare 0.5: the burst of BURST_NODES nodes into one label pair of 12 does not fit its
    ceil(12 * 0.5) + 4 spare entries — exactly one further reload, at that scan; parity holds on
    that scan and after it (drive asserts it on every scan)."""
    ra, rb, seen, reloads = drive(1, 0.5, _resident, _reload, burst=True)
    assert reloads == [1] * BURST_SCAN + [2] * (SCANS - BURST_SCAN), (reloads, ra.events.reload_causes)
    assert ra.events.reload_causes == ["first", "nodes_add"]
    assert all(seen.values()), seen
