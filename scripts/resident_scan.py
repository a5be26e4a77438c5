"""What a controller loop pays per scan: ResidentController (events into the resident
snapshot) against Controller (re-list, re-pack, reload) on identical histories.

    python scripts/resident_scan.py [--pods 100000] [--nodes 1000] [--groups 100] [--scans 20]

Builds one synthetic object-level cluster, then per scan applies 1 % pod churn (a third
each deleted, added, spec-changed; some of the added ones bound) and a few node events (a
taint with its time, a no-delete annotation, a cordon, an add, a delete) to both, runs both
controllers, checks that every group's decision is the same, and prints one JSON line with
the median wall time of ``run_once`` of each (the resident one also split into the queue's
ingest, outside run_once, and the scan itself)."""
import argparse
import json
import os
import random
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

TAINT = "atlassian.com/escalator"
T0 = 1_700_000_000 * 10**9


def make_cluster(rng, n_pods, n_nodes, n_groups):
    groups = [{"name": "g%d" % g, "label_key": "pool", "label_value": "g%d" % g, "min_nodes": 1, "max_nodes": 10 * n_nodes,
               "taint_lower_pct": 30, "taint_upper_pct": 45, "scale_up_pct": 70, "slow_removal_rate": 1,
               "fast_removal_rate": 2, "soft_delete_grace_ns": 300 * 10**9, "hard_delete_grace_ns": 900 * 10**9,
               "scale_up_cool_down_ns": 120 * 10**9} for g in range(n_groups)]
    nodes = [new_node(rng, "node-%d" % j, j % n_groups, T0 - rng.randrange(10**12)) for j in range(n_nodes)]
    members = [[x["name"] for x in nodes if x["labels"]["pool"] == "g%d" % g] for g in range(n_groups)]
    pods = [new_pod(rng, "pod-%d" % i, i % n_groups, members) for i in range(n_pods)]
    return groups, pods, nodes, members


def new_node(rng, name, g, created_ns):
    return {"name": name, "labels": {"pool": "g%d" % g}, "unschedulable": False, "taints": [],
            "cpu": rng.choice([16000, 32000, 64000]), "mem": rng.choice([64, 128, 256]) << 30, "created_ns": created_ns}


def new_pod(rng, name, g, members):
    return {"name": name, "owner_kinds": [], "annotations": {}, "node_selector": {"pool": "g%d" % g}, "affinity": None,
            "containers": [{"cpu": rng.randrange(50, 600), "mem": rng.randrange(1 << 26, 1 << 31)}
                           for _ in range(rng.choice([1, 1, 2]))],
            "init_containers": [], "overhead": None,
            "node_name": rng.choice(members[g]) if members[g] and rng.random() < 0.8 else ""}


class Store:
    """The objects of one controller's cluster; every change is also an event when a queue listens."""

    def __init__(self, sink=None):
        self.pods, self.nodes, self.sink = {}, {}, sink

    def put_pod(self, p):
        self.pods[p["name"]] = p
        if self.sink is not None:
            self.sink.pod_add(p)

    def del_pod(self, k):
        del self.pods[k]
        if self.sink is not None:
            self.sink.pod_delete(k)

    def put_node(self, x):
        self.nodes[x["name"]] = x
        if self.sink is not None:
            self.sink.node_add(x)

    def del_node(self, m):
        del self.nodes[m]
        if self.sink is not None:
            self.sink.node_delete(m)


def churn(store, seed, scan, n_groups, members, now_ns):
    rng = random.Random(seed * 7919 + scan)
    keys = list(store.pods)
    k = max(3, len(keys) // 100) // 3
    picked = rng.sample(keys, 2 * k)
    for key in picked[:k]:
        store.del_pod(key)
    for key in picked[k:]:
        g = int(store.pods[key]["node_selector"]["pool"][1:])
        store.put_pod(dict(new_pod(rng, key, g, members), node_name=store.pods[key]["node_name"]))
    for i in range(k):
        store.put_pod(new_pod(rng, "pod-s%d-%d" % (scan, i), rng.randrange(n_groups), members))
    names = [m for m in store.nodes if m.startswith("node-")]
    a, b, c, d = rng.sample(names, 4)
    x = store.nodes[a]
    store.put_node(dict(x, taints=[TAINT], taint_value=str(now_ns // 10**9 - 1000)))
    store.put_node(dict(store.nodes[b], annotations={"atlassian.com/no-delete": "true"}))
    store.put_node(dict(store.nodes[c], unschedulable=not store.nodes[c]["unschedulable"]))
    store.del_node(d)
    store.put_node(new_node(rng, "node-s%d" % scan, rng.randrange(n_groups), now_ns))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pods", type=int, default=100_000)
    ap.add_argument("--nodes", type=int, default=1_000)
    ap.add_argument("--groups", type=int, default=100)
    ap.add_argument("--scans", type=int, default=20)
    ap.add_argument("--spare", type=float, default=0.5)
    ap.add_argument("--seed", type=int, default=7)
    args = ap.parse_args()
    from escalator_amd.controller import Controller, ResidentController
    rng = random.Random(args.seed)
    groups, pods, nodes, members = make_cluster(rng, args.pods, args.nodes, args.groups)
    clock = [T0]
    res = ResidentController(groups, clock=lambda: clock[0], spare=args.spare)
    rel = Controller(groups, clock=lambda: clock[0])
    a, b = Store(res.events), Store()
    for s in (a, b):
        for x in nodes:
            s.put_node(x)
        for p in pods:
            s.put_pod(p)
    t = time.perf_counter()
    first = res.run_once()                               # the initial load
    first_s = time.perf_counter() - t
    assert [r["delta"] for r in first] == [r["delta"] for r in rel.run_once(lambda: list(b.pods.values()),
                                                                            lambda: list(b.nodes.values()))]
    t_res, t_ing, t_rel = [], [], []
    for scan in range(args.scans):
        clock[0] += 60 * 10**9
        t = time.perf_counter()
        churn(a, args.seed, scan, args.groups, members, clock[0])
        with_queue = time.perf_counter() - t
        t = time.perf_counter()
        churn(b, args.seed, scan, args.groups, members, clock[0])
        t_ing.append(max(0.0, with_queue - (time.perf_counter() - t)))    # the queue's share of the churn
        t = time.perf_counter()
        ra = res.run_once()
        t_res.append(time.perf_counter() - t)
        t = time.perf_counter()
        rb = rel.run_once(lambda: list(b.pods.values()), lambda: list(b.nodes.values()))
        t_rel.append(time.perf_counter() - t)
        for g, (x, y) in enumerate(zip(ra, rb)):
            assert (x["delta"], x["err"], x["branch"], x["cpu_pct"], x["mem_pct"], x["n_to_taint"]) == \
                (y["delta"], y["err"], y["branch"], y["cpu_pct"], y["mem_pct"], y["n_to_taint"]), (scan, g, x, y)
    ms = lambda v: round(statistics.median(v) * 1e3, 3)  # noqa: E731
    print(json.dumps({"pods": args.pods, "nodes": args.nodes, "groups": args.groups, "scans": args.scans,
                      "spare": args.spare, "pod_churn_per_scan": 3 * (max(3, args.pods // 100) // 3), "node_events_per_scan": 5,
                      "resident_run_once_ms": ms(t_res), "reload_run_once_ms": ms(t_rel),
                      "resident_ingest_ms": ms(t_ing), "resident_ingest_plus_run_once_ms": ms([x + y for x, y in zip(t_res, t_ing)]),
                      "resident_first_load_s": round(first_s, 3), "reloads": res.events.reloads,
                      "events_applied": res.events.applied,
                      "speedup": round(statistics.median(t_rel) / statistics.median(t_res), 2)}))


if __name__ == "__main__":
    main()
