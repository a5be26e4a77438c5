"""The new-node pass (calculateNewNodeMetrics, controller.go:157-189: esc_new_nodes_eval)
beside the reaping pass (esc_try_remove, K7) on one context, at BASELINE config #4's node
side: 1M nodes / 10k groups (the 100M pods are not needed: neither pass reads a pod; a
small pod snapshot is loaded so that a placement exists for esc_try_remove).

    python scripts/new_nodes_probe.py [--nodes 1000000] [--groups 10000] [--config 4]
                                      [--steps 20] [--warmup 3] [--out probe.json]

Per group `since` is the creation time below which 99 % of the group's nodes lie, so about
1 % of each group's nodes are new; a random half of all nodes have their instantiation time
known.  Reports ms per esc_new_nodes_eval call and, in the same run on the same context, ms
per esc_try_remove call — both through the Python wrapper and through the C ABI with the
argument and result arrays made once (what a cgo caller does) — the same call with no group
evaluated (the call's floor: upload, launch, record copy), and checks four groups' records
against a numpy restatement.  Prints one JSON line (and writes it to --out)."""
import argparse
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

NONE = 0xFFFFFFFF
INT64_MIN = np.iinfo(np.int64).min
S = 10**9


def timed(fn, warmup, steps):
    for _ in range(warmup):
        fn()
    t0 = time.perf_counter()
    for _ in range(steps):
        fn()
    return (time.perf_counter() - t0) / steps * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pods", type=int, default=1_000_000)
    ap.add_argument("--nodes", type=int, default=1_000_000)
    ap.add_argument("--groups", type=int, default=10_000)
    ap.add_argument("--config", type=int, default=4)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    import escalator_amd as esc
    from escalator_amd import _lib as L
    from oracle import soa
    P, N, G = args.pods, args.nodes, args.groups
    s = esc.Synth(P, N, G, config=args.config, seed=0xE5CA1A7E00000000 + args.config, threads=16)
    nodes = s.nodes()
    ctx = esc.Context(s)
    ctx.load_synth(s)
    rng = np.random.default_rng(23)

    # the groups' members: one entry per (label pair, node), as esc_load_nodes builds them
    t = soa.group_tables(s.groups)
    n_gp, gpair = t["n_gp"], np.asarray(t["gpair"])
    xl_n = (nodes["flags"] >> 8) & 0xFF
    has0 = nodes["label0"] != NONE
    ent_node = np.concatenate([np.flatnonzero(has0), np.repeat(np.arange(N), xl_n)])
    ent_pair = np.concatenate([nodes["label0"][has0], nodes["xl_pair"]]).astype(np.int64)
    keep = ent_pair < n_gp
    ent_node, ent_pair = ent_node[keep], ent_pair[keep]
    created = nodes["created_ns"]
    order = np.lexsort((created[ent_node], ent_pair))
    ent_node, ent_pair = ent_node[order], ent_pair[order]
    cnt = np.bincount(ent_pair, minlength=n_gp)
    start = np.concatenate([[0], np.cumsum(cnt)])
    # since = the creation time of the member at the 99th percentile of its pair (older: not new)
    pair_since = np.full(n_gp, INT64_MIN, np.int64)
    nz = cnt > 0
    pos = start[:-1][nz] + np.maximum((cnt[nz] * 99) // 100 - 1, 0)
    pair_since[nz] = created[ent_node[pos]]
    since = pair_since[gpair]

    known = rng.random(N) < 0.5
    ids = np.flatnonzero(known).astype(np.int64)
    inst = np.full(N, INT64_MIN, np.int64)
    inst[ids] = created[ids] - rng.integers(30, 1800, size=len(ids)) * S
    t0 = time.perf_counter()
    ctx.nodes_instantiated(ids, inst[ids])
    upload_s = time.perf_counter() - t0

    # a placement for esc_try_remove: every pod on a random node, taints up to 20 minutes old
    pod_node = rng.integers(0, N, size=P, dtype=np.uint32)
    now_s = 1_800_000_000
    tainted = (nodes["flags"] & 2) != 0
    taint_s = np.where(tainted, now_s - rng.integers(0, 1200, size=N), INT64_MIN).astype(np.int64)
    no_delete = (rng.random(N) < 0.01).astype(np.uint8)
    ctx.load_placement(pod_node, taint_s, no_delete)
    now_ns, soft, hard = now_s * S, 300 * S, 900 * S

    nn_ms = timed(lambda: ctx.new_nodes(since), args.warmup, args.steps)
    rm_ms = timed(lambda: ctx.try_remove(now_ns, soft, hard), args.warmup, args.steps)
    rec = ctx.new_nodes(since)
    # the same two calls through the C ABI with the arrays made once
    p64 = C.POINTER(C.c_int64)
    s_arr, h_arr = np.full(G, soft, np.int64), np.full(G, hard, np.int64)
    o_rm = np.empty(G, esc.context.REMOVAL_DTYPE)
    o_nn = np.empty(G, esc.context.NEW_NODES_DTYPE)
    since_c = np.ascontiguousarray(since)
    nn_abi = timed(lambda: L.check(ctx.lib.esc_new_nodes_eval(ctx.handle, since_c.ctypes.data_as(p64),
                                                              o_nn.ctypes.data_as(C.POINTER(L.NewNodes)))),
                   args.warmup, args.steps)
    rm_abi = timed(lambda: L.check(ctx.lib.esc_try_remove(ctx.handle, int(now_ns), s_arr.ctypes.data_as(p64),
                                                          h_arr.ctypes.data_as(p64),
                                                          o_rm.ctypes.data_as(C.POINTER(L.Removal)))),
                   args.warmup, args.steps)
    assert o_nn.tobytes() == rec.tobytes()               # deterministic: call after call
    # the call's floor: no group evaluated (every wave writes the zero record and walks
    # nothing), so what is left is the since upload, the launch, the record copy and the wait
    off_c = np.full(G, np.iinfo(np.int64).max, np.int64)
    o_off = np.empty(G, esc.context.NEW_NODES_DTYPE)
    nn_floor = timed(lambda: L.check(ctx.lib.esc_new_nodes_eval(ctx.handle, off_c.ctypes.data_as(p64),
                                                                o_off.ctypes.data_as(C.POINTER(L.NewNodes)))),
                     args.warmup, args.steps)
    assert not o_off.tobytes().strip(b"\0")
    ctx.new_nodes(since)                                 # (the lists checked below are this eval's)

    # parity on four groups: counts, sum, buckets and the list
    parity = True
    for g in sorted({0, min(37, G - 1), G // 2, G - 1}):
        q = gpair[g]
        members = ent_node[start[q]:start[q + 1]]
        new = np.sort(members[created[members] > since[g]])
        obs = new[known[new]]
        lag = created[obs] - inst[obs]
        bucket = np.bincount(np.minimum(np.maximum(lag - 1, 0) // (60 * S), 29), minlength=30)
        r = rec[g]
        parity &= (int(r["n_new"]), int(r["n_observed"]), int(r["lag_sum_ns"]), int(r["flags"])) == \
            (len(new), len(obs), int(lag.sum()), 0)
        parity &= np.array_equal(r["bucket"], bucket)
        idx, kn = ctx.new_nodes_list(g)
        parity &= np.array_equal(idx, new) and np.array_equal(kn != 0, known[new])

    per_group = cnt[gpair]
    out = {
        "metric": "new-node pass (esc_new_nodes_eval) beside the reaping pass (esc_try_remove) on one context",
        "ms_per_new_nodes_eval": nn_ms, "ms_per_try_remove": rm_ms,
        "ms_per_new_nodes_eval_abi": nn_abi, "ms_per_try_remove_abi": rm_abi,
        "new_over_try_remove": nn_ms / rm_ms, "new_over_try_remove_abi": nn_abi / rm_abi,
        "ms_per_new_nodes_eval_abi_no_group_evaluated": nn_floor,
        "steps": args.steps, "warmup": args.warmup,
        "data": "synthetic (esc_synth.cpp config %d node side; since = each group's 99th creation percentile; "
                "a random half of the instantiation times known)" % args.config,
        "config": {"pods": P, "nodes": N, "node_groups": G, "group_pair_entries": int(len(ent_node)),
                   "largest_group": int(per_group.max()), "median_group": int(np.median(per_group))},
        "new_nodes": int(rec["n_new"].sum()), "observed": int(rec["n_observed"].sum()),
        "new_fraction": float(rec["n_new"].sum()) / max(int(per_group.sum()), 1),
        "candidates": int(ctx.try_remove(now_ns, soft, hard)["n_candidates"].sum()),
        "record_bytes_per_call": {"new_nodes": int(G * 152), "try_remove": int(G * 16)},
        "nodes_instantiated_upload_s": upload_s, "nodes_instantiated_ids": int(len(ids)),
        "parity": "exact vs numpy on four groups" if parity else "MISMATCH",
    }
    ctx.close()
    s.close()
    line = json.dumps(out)
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")
    return 0 if parity else 1


if __name__ == "__main__":
    sys.exit(main())
