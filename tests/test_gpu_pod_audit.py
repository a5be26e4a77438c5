"""GPU: esc_audit_pods — the resident pod side checked against itself and the host mirrors.

Clean snapshots report zero mismatches after the load, after event rounds through the event
queue, after esc_pods_grow, esc_pods_compact and esc_nodes_compact, at the tile edges of every
class format, on both sides of the packed small format's pair limit and through the C
section's paths.  MAP's, KSLOT's, CSLOT's and PODREF's n_checked are counted by the threads that
read the words and equal counts computed on the CPU (live pods, K capacity, bound pods), which
proves those checks looked; REPLICA's is counted by the compare kernel per element it loaded, and
doubles from 2 replicas to 3.  Of REPLICA's arrays only replica 1's K blocks are shown to be
compared by a poke (target 8): the injection table the audit was specified with has no other
replica target.
That every check detects a wrong word is shown in child processes on the measurement library
(tests/pod_audit_child.py), the only build that can make one wrong."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import test_gpu_pods_compact as TC
import test_gpu_pods_grow as TG
from oracle import soa
from pod_audit_child import OWNER, POKES, REPLICAS, bound, is_clean, load_pods_small, pod_cluster
from audit_child import SPARE
from test_gpu_pods_compact import drain  # noqa: F401  (the 22 classes at their tile edges: a fixture)
from test_gpu_pods_grow import four_pools, small_pods

pytestmark = pytest.mark.gpu
soa.build()

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
MEASURE = os.path.join(ROOT, "escalator_amd", "libescalator_hip_measure.so")
CHECKS = ["MAP", "KSLOT", "CSLOT", "COUNT", "PODREF", "REPLICA"]
E_STATE = -5


@pytest.fixture(scope="module")
def esc():
    import escalator_amd
    assert escalator_amd._lib.ESC_E_STATE == E_STATE
    return escalator_amd


def assert_clean(ctx, want=None, tag="", skipped=()):
    """No mismatch, first_bad unset, exactly `skipped` skipped; n_checked as computed on the CPU."""
    rep = ctx.audit_pods()
    print(tag, json.dumps(rep))
    assert sorted(rep["skipped"]) == sorted(skipped), (tag, rep)
    assert sorted(k for k in rep if k != "skipped") == sorted(set(CHECKS) - set(skipped)), (tag, rep)
    assert is_clean(rep), (tag, rep)
    r = ctx.pods_room()
    assert rep["KSLOT"]["n_checked"] == r["k_capacity"], (tag, rep["KSLOT"], r["k_capacity"])
    assert rep["COUNT"]["n_checked"] == (want or {}).get("COUNT", 9)          # (9 per device)
    assert rep["CSLOT"]["n_checked"] % 64 == 0 and rep["CSLOT"]["n_checked"] >= r["c_free"]
    for k, n in (want or {}).items():
        assert rep[k]["n_checked"] == n, (tag, k, rep[k], n)
    return rep


# ------------------------------------------------------------------ clean snapshots
def test_clean_after_load_events_grow_and_compactions(esc):
    """The small cluster through the event queue with 3 replicas and a placement: clean after the
    load, after two mixed rounds (pod delete / update / add / bind, node add / delete), after
    pods_grow, pods_compact and nodes_compact; live and bound pods counted on the CPU."""
    from escalator_amd.events import EventQueue
    from randobj import make_nodes, make_pods
    rng, groups, states, pods, nodes, first = pod_cluster()
    ctx = esc.Context(groups)
    load = ctx.load
    ctx.load = lambda P, N, **kw: load(P, N, replicas=REPLICAS)
    q = EventQueue(spare=SPARE, pod_grow=True)             # a full class grows on the device: no reload
    for x in nodes:
        q.node_add(x)
    for p in pods:
        q.pod_add(p)

    def check(tag):
        live_p, live_n = q.live_pods(), q.live_nodes()
        rep = assert_clean(ctx, {"MAP": len(live_p), "PODREF": bound(live_p, live_n)}, tag)
        assert ctx.audit_pods() == rep                          # two calls on one snapshot: equal reports
        return rep

    q.flush(ctx)
    check("load")
    for rnd in range(2):
        live = [x["name"] for x in q.live_nodes()]
        # deletes of nodes without pods (a deleted node's pods keep their run positions until a
        # pod event unbinds them, so the CPU's count of bound pods would need the event history)
        for m in (["node-1"] if rnd == 0 else ["r0-1", "r0-2", "r0-3"]):
            q.node_delete(m)
            live.remove(m)
        for k, x in enumerate(make_nodes(rng, 4, groups, big_frac=0.0)):
            q.node_add(dict(x, name="r%d-%d" % (rnd, k)))
        keys = sorted(q.pods)
        for k in rng.sample(keys, 40):
            q.pod_delete(k)
            keys.remove(k)
        for k in rng.sample(keys, 40):                          # spec changes in place, other classes
            q.pod_update(dict(make_pods(rng, 1, groups, big_frac=0.0)[0], name=k, node_name=q.pods[k]["node_name"]))
        for k, p in enumerate(make_pods(rng, 30, groups, big_frac=0.0)):
            q.pod_add(dict(p, name="r%d-p%d" % (rnd, k), node_name=rng.choice(live + ["", "r%d-0" % rnd])))
        for k in rng.sample(keys, 25):                          # moved, unbound
            q.pod_update(dict(q.pods[k], node_name=rng.choice(live + [""])))
        q.flush(ctx)
        check("round %d" % rnd)
    print(q.reload_causes, q.applied)
    # (a round whose upserts fit neither the classes nor a growth reloads; at least one round's
    # events of every pod kind were applied in place)
    assert q.reloads <= 2 and min(q.applied[k] for k in ("pods_upsert", "pods_delete", "pods_bind")) > 0, (q.reload_causes, q.applied)
    ctx.decide_all(states)
    check("after a decision")
    ctx.pods_grow(None, None)
    check("pods_grow")
    ctx.pods_compact()
    check("pods_compact")
    ctx.nodes_compact()
    check("nodes_compact")
    ctx.close()


def test_replica_elements_double_from_two_to_three_replicas(esc):
    n = {}
    for reps in (1, 2, 3):
        ctx, groups, states, pods, nodes, first, P, N = load_pods_small(esc, replicas=reps)
        rep = assert_clean(ctx, {"MAP": len(pods), "PODREF": bound(pods, nodes)}, "replicas %d" % reps,
                           skipped=["REPLICA"] if reps == 1 else [])
        n[reps] = rep.get("REPLICA", {}).get("n_checked")
        ctx.close()
    assert n[2] > 0 and n[3] == 2 * n[2], n


# ------------------------------------------------------------------ tile edges, every format
def test_tile_edges_of_every_class_format(esc, drain):  # noqa: F811
    """The 22 classes (packed small x 0-3 pairs, 12-B x 0-3, plain with 1-3 records x 0-3 pairs
    and without records, an inert class) drained to 255 / 256 / 257 / 513 live pods with holes
    at a tile's start, middle and end and whole free first and last tiles: clean before and after
    the compaction, on 3 replicas."""
    D = drain
    assert len(TC.DRAIN) == 22
    ctx = esc.Context(D["groups"])
    ctx.set_spare(0.0)
    ctx.load(D["P0"], D["N"], replicas=3)
    assert_clean(ctx, {"MAP": len(D["pods"])}, "loaded", skipped=["PODREF"])
    ctx.pods_delete(D["gone"])
    live = len(D["pods"]) - len(D["gone"])
    assert live == sum(TC.LIVE.values())
    assert_clean(ctx, {"MAP": live}, "drained", skipped=["PODREF"])
    ctx.pods_compact()
    rep = assert_clean(ctx, {"MAP": live}, "compacted", skipped=["PODREF"])
    assert rep["KSLOT"]["n_checked"] == 256 * sum(TG.tiles(v) for v in TC.LIVE.values())
    ctx.close()


def test_a_class_without_a_tile_and_grown_again(esc, drain):  # noqa: F811
    D = drain
    ctx = esc.Context(D["groups"])
    ctx.set_spare(0.0)
    ctx.load(D["P0"], D["N"])
    lo = D["first"]["s2"]
    ctx.pods_delete(list(range(lo, lo + 300)))                 # every pod of the 2-pair packed small class
    ctx.pods_compact()
    assert ctx.pods_room()["per_class"][TC.CLS["s2"]] == 0     # a class, no position
    assert_clean(ctx, {"MAP": len(D["pods"]) - 300}, "no tile", skipped=["PODREF", "REPLICA"])
    B, _ = ctx.pack([D["pods"][lo]], [])
    assert ctx.pods_upsert([lo], B) == TG.E_LIMIT
    ctx.pods_grow([lo], B)
    assert ctx.pods_upsert([lo], B) == 0 and ctx.pod_where(lo) == (TC.CLS["s2"], 0)
    assert_clean(ctx, {"MAP": len(D["pods"]) - 299}, "grown again", skipped=["PODREF", "REPLICA"])
    ctx.close()


# ------------------------------------------------------------------ group-pair edges
@pytest.mark.parametrize("n_groups", [16382, 20480])
def test_both_sides_of_the_packed_small_pair_limit(esc, n_groups):
    """16 382 group pairs: the last context with packed small classes; 20 480: none (the same pods
    sit in 12-B classes, two K1 windows).  Filled by upserts and compacted (order_case)."""
    ctx, groups, P1, N = TC.order_case(esc, n_groups, 320, 0)
    cid = ctx.pod_where(5)[0]
    assert (256 <= cid < 260) == (n_groups == 16382) and (128 <= cid < 132) == (n_groups == 20480), cid
    assert_clean(ctx, {"MAP": 322}, "n_gp %d" % n_groups, skipped=["PODREF", "REPLICA"])
    ctx.close()


# ------------------------------------------------------------------ the C section
class AuditedWorld(TG.PodWorld):
    """PodWorld whose every check() also runs the pod audit (a placement is loaded)."""
    stages = []

    def check(self, tag, *a, **kw):
        super().check(tag, *a, **kw)
        live = [p for p in self.pods if p is not None]
        names = set(self.idx)
        rep = self.ctx.audit_pods()
        print(tag, json.dumps(rep))
        assert is_clean(rep) and set(rep["skipped"]) <= {"REPLICA"}, (tag, rep)
        assert rep["MAP"]["n_checked"] == len(live), (tag, rep["MAP"])
        assert rep["PODREF"]["n_checked"] == sum(1 for p in live if p["node_name"] in names), (tag, rep["PODREF"])
        AuditedWorld.stages.append(tag)


def test_c_section_big_tiles_indirect_refs_spare_slots(esc, monkeypatch):
    """test_gpu_pods_grow's C-section history with the pod audit at every stage: a tile of 256
    extra records, pods of 6 pairs (indirect PodRefs), the spare slots filled, the C section grown
    by spare tiles, binds and deletes after (freed slots)."""
    monkeypatch.setattr(TG, "PodWorld", AuditedWorld)
    AuditedWorld.stages = []
    TG.test_c_section_grows_by_spare_tiles(esc)
    assert AuditedWorld.stages == ["load", "spare slots full", "grown", "burst in", "bind and delete after"]


@pytest.mark.parametrize("devices", [None, [0, 0]])
def test_parked_pods_rehomed_and_slots_reused(esc, monkeypatch, devices):
    """test_gpu_pods_compact's parked history (pods parked in spare C slots by a full class, re-homed
    by pods_compact, events after) with the pod audit at every stage, on one device and as a
    two-shard multi-device context; then a freed spare slot re-used by a smaller pod."""
    monkeypatch.setattr(TC, "PodWorld", AuditedWorld)
    AuditedWorld.stages = []
    w = TC.run_parked(esc, devices=devices)
    assert AuditedWorld.stages == ["parked", "compacted", "compacted twice", "events after"]
    n = len(w.pods)
    pools = ["one", "some", "dry"]
    assert w.upsert([n], [TG.c_pod("again", 1, pools, "n2", containers=5, pairs=2)]) == 0      # a freed spare slot
    assert w.ctx.pod_where(n)[0] == -1
    w.check("spare slot re-used", fresh=False)
    assert w.upsert([n], [TG.c_pod("again", 1, pools, "n2", containers=5, pairs=1)]) == 0      # smaller, in place
    w.check("neutral remainder", fresh=False)
    w.ctx.close()


def test_three_shards_in_one_multi_device_context(esc):
    """devices=[0, 0, 0]: every shard audits its own pods; the merged report is clean and its
    counts are the shards' summed — the live pods, the K positions of all three, the bound pods,
    9 counters per shard; REPLICA skipped with one replica and run on every shard with two."""
    from escalator_amd.objects import placement
    rng, groups, states, pods, nodes, first = pod_cluster()
    ctx = esc.Context(groups, devices=[0, 0, 0])
    ctx.set_spare(SPARE)
    P, N = ctx.pack(pods, nodes)
    ctx.load(P, N)
    ctx.load_placement(*placement(pods, nodes))
    ctx.decide_all(states)
    rep = assert_clean(ctx, {"MAP": len(pods), "PODREF": bound(pods, nodes), "COUNT": 27}, "three shards", skipped=["REPLICA"])
    # (assert_clean: KSLOT's count is esc_pods_room's k_capacity, the three shards' summed)
    assert rep["KSLOT"]["n_checked"] % 256 == 0
    one = ctx.audit_pods(["MAP"])
    assert set(one) == {"MAP", "skipped"} and one["MAP"] == rep["MAP"]
    ctx.load(P, N, replicas=2)
    ctx.load_placement(*placement(pods, nodes))
    two = assert_clean(ctx, {"MAP": len(pods), "PODREF": bound(pods, nodes), "COUNT": 27}, "three shards, two replicas")
    assert two["KSLOT"] == rep["KSLOT"] and two["REPLICA"]["n_checked"] > two["KSLOT"]["n_checked"]
    ctx.close()


def test_two_sharded_ranks_of_which_one_had_events(esc):
    from test_gpu import _packed_subset
    groups, nodes = four_pools()
    base = small_pods(1200)
    ctxs = []
    for r in range(2):
        c = esc.Context(groups, rank=r, world=2)
        c.set_spare(0.25)
        P, N = c.pack(base, nodes)
        c.load(_packed_subset(P, list(range(600 * r, 600 * r + 600))), N, pod_offset=600 * r)
        ctxs.append(c)
    c0, c1 = ctxs
    gone = list(range(0, 600, 2)) + list(range(301, 400, 2))   # 350 of rank 1's 600 pods (shard-local ids)
    c1.pods_delete(gone)
    c1.pods_compact()
    a = assert_clean(c0, {"MAP": 600}, "rank 0", skipped=["PODREF", "REPLICA"])
    b = assert_clean(c1, {"MAP": 250}, "rank 1", skipped=["PODREF", "REPLICA"])
    assert a["MAP"]["n_checked"] + b["MAP"]["n_checked"] == 1200 - len(gone)
    for c in ctxs:
        c.close()


# ------------------------------------------------------------------ skips, single checks, read-only
def test_skips_single_checks_and_read_only(esc):
    from escalator_amd.objects import placement
    rng, groups, states, pods, nodes, first = pod_cluster()
    ctx = esc.Context(groups)
    ctx.set_spare(SPARE)
    P, N = ctx.pack(pods, nodes)
    with pytest.raises(esc._lib.EscError) as e:
        ctx.audit_pods()
    assert e.value.code == E_STATE                             # before esc_load_pods
    ctx.load(P, N)
    assert sorted(ctx.audit_pods()["skipped"]) == ["PODREF", "REPLICA"]
    ctx.load(P, N, replicas=2)
    assert ctx.audit_pods()["skipped"] == ["PODREF"]
    ctx.load_placement(*placement(pods, nodes))
    assert ctx.audit_pods()["skipped"] == []
    for k in CHECKS:                                           # a single named check reports only itself
        rep = ctx.audit_pods([k])
        assert set(rep) == {k, "skipped"} and rep[k]["n_bad"] == 0 and rep[k]["n_checked"] > 0, rep
    # read-only: a captured decision replays to the same bytes; selections and reaping still answer
    ctx.use_graph(True)
    ctx.set_order_in_step(True)
    ctx.set_selections(4)
    a = ctx.decide_all(states)
    def sel():
        try:
            return [np.asarray(x).tobytes() for x in ctx.selections()]
        except esc._lib.EscError as err:                        # (a look-back that gave up: the same answer after)
            return err.code
    s0 = sel()
    assert not isinstance(s0, int), s0                         # selections answered before the audit
    rm = ctx.try_remove(1_700_000_000 * 10**9, [0] * len(groups), [0] * len(groups))
    assert is_clean(ctx.audit_pods())
    assert sel() == s0                                         # sel_valid stayed
    b = ctx.decide_all(states)
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()
    assert is_clean(ctx.audit_pods())
    rm2 = ctx.try_remove(1_700_000_000 * 10**9, [0] * len(groups), [0] * len(groups))
    assert np.asarray(rm).tobytes() == np.asarray(rm2).tobytes()
    ctx.close()


# ------------------------------------------------------------------ detection (child processes)
def run_child(*args):
    assert os.path.exists(MEASURE), "build the measurement library: make -C escalator_amd/csrc ABLATIONS=1"
    env = dict(os.environ, ESC_LIB_PATH=MEASURE)
    try:
        r = subprocess.run([sys.executable, "-u", os.path.join(HERE, "pod_audit_child.py"), *args], capture_output=True,
                           text=True, timeout=240, env=env, cwd=ROOT)
    except subprocess.TimeoutExpired:
        pytest.exit("pod_audit_child.py %s hung: nothing more is started on this GPU" % " ".join(args), 1)
    if r.returncode in (134, 139, -6, -11):                    # an abort or a fault: the session ends here
        pytest.exit("pod_audit_child.py %s died (%d): %s" % (" ".join(args), r.returncode, r.stderr[-2000:]), 1)
    assert r.returncode == 0, r.stderr[-3000:]
    return json.loads([x for x in r.stdout.splitlines() if x.startswith("{")][-1])


# What a poke changes besides the check that owns the word: {target: {check: (n_bad, why)}}.
# Every target here is a pod that is not bound, or a word no other check reads, so one wrong word
# is one mismatch in one check:
#   free_k / ds_bits / inert_pair write every replica (REPLICA stays equal) and a slot whose pod, if
#     any, is unbound (no PodRef names it); MAP and COUNT read host tables only;
#   map orphans one slot: COUNT derives its numbers from the free lists, which did not change;
#   cflags flips a bit of the host's flags that is no count, so no offset moves; PodRefs come from
#     the device's flags;
#   parked_pair changes a pair past the pod's count in every replica; the slot has room for more
#     than 3 pairs, so a PodRef of it is indirect (an offset and the room) and names no pair;
#   podref changes the PodRef buffer alone; replica changes replica 1 alone, which only REPLICA reads.
#   free_k12 is free_k in a class of the 12-byte format (the poke's other branch).
ALSO = {t: {} for t in POKES}


@pytest.mark.parametrize("target", sorted(POKES, key=lambda t: (POKES[t], t)))
def test_every_poke_is_found_once_by_its_check(target):
    r = run_child("poke", target)
    print(json.dumps(r))
    rep = r["report"]
    assert rep["skipped"] == [] and sorted(k for k in rep if k != "skipped") == sorted(CHECKS), rep
    own = OWNER[target]
    assert rep[own]["n_bad"] == 1 and rep[own]["first_bad"] == r["id"], (own, rep[own], r["id"])
    for k in CHECKS:
        if k != own:
            n, _why = ALSO[target].get(k, (0, ""))
            assert rep[k]["n_bad"] == n and (n or rep[k]["first_bad"] == -1), (k, rep[k])
    assert r["refused"] == [-1] * len(r["refused"]), r["refused"]         # ESC_E_INVAL


def test_state_before_the_load_and_on_a_stale_context():
    r = run_child("state")
    print(json.dumps(r))
    assert r["unloaded_rc"] == E_STATE and r["stale_rc"] == E_STATE and r["delete_code"] != 0, r
    assert r["loaded_clean"] and r["reloaded_clean"], r


def test_controller_heals_after_a_poked_free_position():
    """ResidentController(pod_audit_every=1): the scan whose pod audit finds the poked position
    reloads once (cause "pod_audit:KSLOT"); that scan's records and every later scan's equal the
    reloading Controller's and the literal oracle's (asserted scan by scan inside the child)."""
    r = run_child("heal")
    print(json.dumps(r))
    assert r["reload_causes"] == ["first", "pod_audit:KSLOT"], r
    assert r["reloads"] == [1, 1] + [2] * (r["scans"] - 2), r
    assert r["pod_audit_failures"] == 1 and r["pod_audits"] == r["scans"] and r["last_clean"], r
