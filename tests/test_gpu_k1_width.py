"""GPU: K1 (k_pod_reduce) at both workgroup widths, against the C oracle, bit-exact.

The product runs K1 at 512 threads at every window.  The 1024-thread kernel (16 waves per CU)
measured slower and is instantiated in the measurement library only, where
ESC_K1_THREADS forces a width.  Where it could matter is a window whose partials take more than
half the LDS, which leaves a CU one workgroup: above SWITCH_S = 5 120 slots (81 920 B; two
workgroups per CU) a 512-thread K1 runs 2 waves per SIMD and a 1024-thread one 4.  The slot
counts here lie on each side of that edge (tests/test_k1_width_source.py, CPU, recomputes it
from the sources), at a full window, and at 10 241: a full window and a tail window of the
default filter's slot alone, with the 8 LDS copies.

The pod mix is packed from objects over the generator's groups (synth_groups_for_slots): packed
small pods with 0..3 extra pairs, 12-B packed pods, plain pods of three record shapes, random
pods of every other kind (tests/randobj.py), C tiles and one C tile past 128 records
(k_pod_bigtiles).  The packed small class without extra pairs holds 42 tiles (more than the 16
waves of the wide workgroup), every other class fewer than 16 (idle waves).

The in-process tests run the product library (512 threads).  A child process on the measurement
library (tests/k1_width_child.py) forces each width on each side of the edge and compares them
byte for byte, runs the same paths at 1024 threads, and the no-plan walk at 1024 threads."""
import json
import os
import random
import subprocess
import sys

import numpy as np
import pytest

from oracle import soa
from test_gpu import _packed_subset, check_against_c_oracle
from test_gpu_slots import WINDOW, _big_tiles, _n_extra_records, slots_of, synth_groups_for_slots, windows

pytestmark = pytest.mark.gpu
soa.build()

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
MEASURE = os.path.join(ROOT, "escalator_amd", "libescalator_hip_measure.so")

SWITCH_S = WINDOW // 2          # the largest window of which two workgroups fit a CU's LDS
MIX_S = [SWITCH_S, SWITCH_S + 1, WINDOW, WINDOW + 1]
PATH_S = [SWITCH_S + 1, WINDOW + 1]      # one workgroup per CU: one window; a full one and a tail with copies
GI = 1 << 30
# class id = signature | packed << 7, signature = regular * 32 + init * 8 + overhead * 4 + extra pairs
CLASS_ID = {"s0": 256, "s1": 257, "s2": 258, "s3": 259, "p12": 128, "k00": 0, "k11": 1 * 32 + 1, "k33": 3 * 32 + 3}
# pods per kind: 255 / 256 / 257 around a tile's 256 (the random pods add to some classes)
COUNTS = [("s0", 300), ("s1", 255), ("s2", 257), ("s3", 300), ("p12", 300), ("k00", 300), ("k11", 255), ("k33", 257)]
N_UPSERT = 300                  # more than a tile: the batch crosses a tile edge wherever the class stands
S0_COPIES = 34                  # the 300 s0 pods again, packed: 10 500 pods, 42 tiles


@pytest.fixture(scope="module")
def esc():
    import escalator_amd
    return escalator_amd


def _in(key, values):
    return {"node_affinity": {"required": [[{"key": key, "op": "In", "values": list(values)}]]},
            "pod_affinity": False, "pod_anti_affinity": False}


def kind_pod(kind, i, own, extra):
    """Pod i of a class kind under the pair (customer, own), its extra pairs (customer, extra[k])."""
    np_, containers = {
        "s0": (0, [(100 + i % 900, (1 << 20) + i)]), "s1": (1, [(100 + i % 900, (1 << 20) + i)]),
        "s2": (2, [(100 + i % 900, (1 << 20) + i)]), "s3": (3, [(100 + i % 900, (1 << 20) + i)]),
        "p12": (0, [(200 + i % 900, 17 * GI + i)]),                      # a request past 16 GiB
        "k00": (0, [((1 << 20) + i, 5)]),                                # outside the packed ranges
        "k11": (1, [((1 << 20) + i, 5), (3, 7 + i)]),
        "k33": (3, [((1 << 20) + i, 5), (3, 7 + i), (5, 11), (7, 13 + i)]),
        "c5": (1, [(10 + i % 90, 1000 + i)] * (5 + i % 3)),              # > 3 extra records: a C tile
        "c9": (0, [(10 + i % 90, 1000 + i)] * 9),                        # 64 of them: 512 records in a tile
    }[kind]
    return {"name": "%s-%d" % (kind, i), "owner_kinds": [], "annotations": {}, "node_selector": {"customer": own},
            "affinity": _in("customer", extra[:np_]) if np_ else None,
            "containers": [{"cpu": c, "mem": m} for c, m in containers], "init_containers": [], "overhead": None,
            "node_name": ""}


_WORLDS = {}


def world(esc, S):
    """Groups, states, packed pods and nodes and the oracle's answer for S slots, built once."""
    if S in _WORLDS:
        return _WORLDS[S]
    from randobj import make_nodes, make_pods
    s = esc.Synth(1000, 100, synth_groups_for_slots(S), config=4, seed=0xE5CA1A7E00000004)   # groups and states only
    groups, states = s.groups, s.states
    t = soa.group_tables(groups)
    assert t["n_gp"] + 1 == S and t["default"] >= 0
    rng = random.Random(S)
    vals = [g["label_value"] for g in groups if g["label_key"] == "customer" and g["name"] != "default"]
    slot_of = {g["label_value"]: int(t["gpair"][i]) for i, g in enumerate(groups) if g["label_key"] == "customer"}
    by_slot = sorted(vals, key=lambda v: slot_of[v])
    # the window's first and last columns, the slots beside the switch, and anywhere
    edge = by_slot[:3] + by_slot[-3:] + [v for v in by_slot if SWITCH_S - 34 <= slot_of[v] <= SWITCH_S + 2][:6]
    pick = lambda: rng.choice(edge) if rng.random() < 0.2 else rng.choice(vals)      # noqa: E731
    pods, first = [], {}
    for kind, n in COUNTS + [("c5", 200), ("c9", 64)]:
        first[kind] = len(pods)
        pods += [kind_pod(kind, len(pods) + k, pick(), [pick() for _ in range(3)]) for k in range(n)]
    n_kinds = len(pods)
    pods += [kind_pod("s0", n_kinds + k, "", []) | {"node_selector": None} for k in range(150)]   # the default filter's slot
    pods += make_pods(rng, 1500, groups, big_frac=0.02)
    nodes = make_nodes(rng, 300, groups)
    host = esc.Context(groups, device=-1)
    P, N = host.pack(pods, nodes)
    extra_s1 = host.pack([kind_pod("s1", 90_000 + k, pick(), [pick() for _ in range(3)]) for k in range(N_UPSERT)], [])[0]
    host.close()
    # the s0 pods S0_COPIES times more, behind every pod with extra records or pairs
    a, b = first["s0"], first["s0"] + 300
    assert np.all(_n_extra_records(P)[a:b] == 0) and np.all((P["flags"][a:b].astype(np.uint64) >> 24) & 0x3F == 0)
    for f in ("flags", "cpu0", "mem0", "pair0"):
        P[f] = np.concatenate([P[f], np.tile(P[f][a:b], S0_COPIES)])
    # ---- what the input holds
    f = P["flags"].astype(np.uint64)
    rec, nxp = _n_extra_records(P), ((f >> 24) & 0x3F).astype(np.int64)
    in_c = (rec > 3) | (nxp > 3)
    assert in_c.sum() >= 264 and _big_tiles(P), int(in_c.sum())
    otot = soa.totals(P, N, groups)
    odf, odi = soa.decide(groups, states, otot)
    slot = t["gpair"].astype(np.int64)
    for g0, gw in windows(S):                                   # pods in every window's first and last column
        sel = (np.arange(t["G"]) != t["default"]) & (slot >= g0) & (slot < g0 + gw)
        if sel.any():
            assert otot[sel & (slot < g0 + 32), 2].sum() > 0 and otot[sel & (slot >= g0 + gw - 34), 2].sum() > 0, (S, g0)
    assert otot[t["default"], 2] >= 150
    w = {"groups": groups, "states": states, "P": P, "N": N, "otot": otot, "odf": odf, "odi": odi, "extra_s1": extra_s1,
         "n": len(P["flags"])}
    _WORLDS[S] = w
    return w


def check_mix(ctx):
    """Every class kind of the mix has a class; packed small without pairs has more tiles than a
    workgroup has waves at either width, the others fewer (loaded at spare 0: whole tiles)."""
    r = ctx.pods_room()
    for kind, n in COUNTS:
        assert r["per_class"][CLASS_ID[kind]] >= 0, kind
    # tiles by construction: s0 holds its 300 pods S0_COPIES + 1 times; no other class can reach 16
    # tiles (its own pods, and at most every random and every C pod)
    assert (300 * (S0_COPIES + 1)) // 256 >= 40 and max(n for _, n in COUNTS[1:]) + 1500 + 264 < 16 * 256
    assert int((r["per_class"] >= 0).sum()) >= 12               # the random pods' kinds beside the eight


def run_exact(ctx, w, times=2):
    for _ in range(times):
        ctx.run()
        check_against_c_oracle(*ctx.results(), w["otot"], w["odf"], w["odi"])


@pytest.mark.parametrize("S", MIX_S)
def test_pod_mix_each_side_of_the_switch(esc, S):
    """The pod mix at 5 120 slots (two workgroups per CU), 5 121 and 10 240 (one) and 10 241 (a
    full window, then the tail window with its copies); the exact wide path as the cross-check."""
    w = world(esc, S)
    assert [gw for _, gw in windows(S)] == {SWITCH_S: [S], SWITCH_S + 1: [S], WINDOW: [S], WINDOW + 1: [WINDOW, 1]}[S]
    ctx = esc.Context(w["groups"])
    assert slots_of(ctx) == S
    ctx.load(w["P"], w["N"])
    check_mix(ctx)
    ctx.set_state(w["states"])
    run_exact(ctx, w)
    ctx.force_wide(True)
    run_exact(ctx, w, 1)


# ---- the paths: plain functions, run here on the product library and by the child at 1024 threads
def path_flush_rounds(esc, S):
    """A generator snapshot of 300 000 pods: the workgroups' shares touch more than 32 columns
    each on average (asserted; pods lie in column order, so a share's columns are few), so the
    compact flush takes a second round of 32 entries at 16 waves and a third of 16 at 8."""
    s = esc.Synth(300_000, 30_000, synth_groups_for_slots(S), config=4, seed=0xE5CA1A7E00000004)
    otot = soa.totals(s.pods(), s.nodes(), s.groups)
    odf, odi = soa.decide(s.groups, s.states, otot)
    ctx = esc.Context(s)
    assert slots_of(ctx) == S
    ctx.load_synth(s)
    ctx.set_state(s.states)
    ctx.run()
    check_against_c_oracle(*ctx.results(), otot, odf, odi)
    entries, full = ctx.k1_flush_entries()
    nblk = int(ctx.k1_trace().shape[0])
    assert nblk > 1 and 32 * nblk < entries <= full, (entries, full, nblk)
    ctx.run()
    check_against_c_oracle(*ctx.results(), otot, odf, odi)


def path_graph_replay_two_replicas(esc, S):
    w = world(esc, S)
    ctx = esc.Context(w["groups"])
    ctx.load(w["P"], w["N"], replicas=2)
    ctx.use_graph(True)
    ctx.set_state(w["states"])
    run_exact(ctx, w, 4)


def path_after_calibrate(esc, S):
    """esc_k1_calibrate times and re-plans the shares with launch_k1's own launches."""
    w = world(esc, S)
    ctx = esc.Context(w["groups"])
    ctx.load(w["P"], w["N"])
    ctx.set_state(w["states"])
    run_exact(ctx, w, 1)
    ctx.k1_calibrate(2)
    run_exact(ctx, w)


def path_upsert_across_a_tile_edge(esc, S):
    """300 new pods with one extra pair into their class's spare room: more than a tile's 256, so
    the batch crosses a tile edge, and the next decision counts them."""
    w = world(esc, S)
    ctx = esc.Context(w["groups"])
    ctx.set_spare(1.5)                                   # room for the batch: 1.5 x the class's >= 255 pods
    ctx.load(w["P"], w["N"])
    ctx.set_state(w["states"])
    run_exact(ctx, w, 1)
    before = int(ctx.pods_room()["per_class"][CLASS_ID["s1"]])
    assert before >= N_UPSERT > 256
    ids = list(range(w["n"], w["n"] + N_UPSERT))
    assert ctx.pods_upsert(ids, w["extra_s1"]) == 0
    assert int(ctx.pods_room()["per_class"][CLASS_ID["s1"]]) == before - N_UPSERT
    P = {k: np.concatenate([w["P"][k], w["extra_s1"][k]]) for k in w["P"]}
    otot = soa.totals(P, w["N"], w["groups"])
    assert not np.array_equal(otot, w["otot"])
    odf, odi = soa.decide(w["groups"], w["states"], otot)
    for _ in range(2):
        ctx.run()
        check_against_c_oracle(*ctx.results(), otot, odf, odi)


def path_two_sharded_contexts(esc, S):
    """Two ranks' halves of the pod mix, exchanged through the host."""
    from escalator_amd.dist import merge_owned
    w = world(esc, S)
    half = w["n"] // 2
    ctxs, words, firsts = [], [], []
    for r in range(2):
        c = esc.Context(w["groups"], rank=r, world=2)
        assert slots_of(c) == S
        lo, hi = (0, half) if r == 0 else (half, w["n"])
        c.load(_packed_subset(w["P"], list(range(lo, hi))), w["N"], pod_offset=lo)
        c.set_state(w["states"])
        for _ in range(2):
            c.reduce()
        a, b = c.exchange_download()
        words.append(a)
        firsts.append(b)
        ctxs.append(c)
    W, F = np.sum(words, axis=0), np.min(firsts, axis=0)
    parts = []
    for c in ctxs:
        c.exchange_upload(W, F)
        c.decide()
        parts.append(c.results())
    check_against_c_oracle(*merge_owned(parts), w["otot"], w["odf"], w["odi"])


PATHS = {"flush_rounds": path_flush_rounds, "graph_replicas": path_graph_replay_two_replicas,
         "calibrated": path_after_calibrate, "upsert": path_upsert_across_a_tile_edge, "sharded": path_two_sharded_contexts}


@pytest.mark.parametrize("S", PATH_S)
@pytest.mark.parametrize("path", sorted(PATHS))
def test_path(esc, path, S):
    """Each path above at 5 121 and at 10 241 slots (the child process runs them at 1024 threads)."""
    PATHS[path](esc, S)


# ------------------------------------------------------- forced widths (measurement library)
def test_forced_widths_agree_and_1024_thread_paths():
    """ESC_K1_THREADS = 512 and 1024 at 5 120 and at 5 121 slots: totals and decisions equal the
    oracle's and each other's, byte for byte.  At 1024 threads, at 5 121 and 10 241 slots: the
    graph replay over two replicas, a decision after k1_calibrate, an upsert across a tile edge
    and two sharded contexts; the pod mix at 10 240; ESC_K1_VARIANT=7 (no plan: the weight-range
    walk, the full-row flush) over 10 241 slots."""
    assert os.path.exists(MEASURE), "build the measurement library: make -C escalator_amd/csrc ABLATIONS=1"
    env = dict(os.environ, ESC_LIB_PATH=MEASURE)
    r = subprocess.run([sys.executable, "-u", os.path.join(HERE, "k1_width_child.py")],
                       capture_output=True, text=True, timeout=240, env=env, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-3000:]
    out = json.loads([x for x in r.stdout.splitlines() if x.startswith("{")][-1])
    assert sorted(out["widths"]) == sorted("%d@%d" % (s, t) for s in (SWITCH_S, SWITCH_S + 1) for t in (512, 1024)), out
    for key, c in out["widths"].items():
        assert c["slots"] == int(key.split("@")[0]) and c["exact"] and c["same_as_first"] and c["workgroups"] > 1, out
    assert out["mix_full_window"] == {"slots": WINDOW, "exact": True}, out
    assert sorted(int(k) for k in out["paths"]) == PATH_S
    for c in out["paths"].values():
        assert c == {"graph_replicas": True, "calibrated": True, "upsert": True, "sharded": True, "flush_rounds": True}, out
    n = out["noplan"]
    assert n["slots"] == WINDOW + 1 and n["exact"] and n["entries"] == n["full"] > 0 and n["plan_words_zero"], out
