"""GPU: esc_audit — the resident snapshot's derived state recomputed from its primary tables.

Clean snapshots report zero mismatches, after the load and after rounds of every kind of
informer event applied in place, and n_checked equals counts computed on the CPU from the SoA
arrays, which proves the checks looked.  Shapes at which the kernels can go wrong each get a
small context.  That every check detects a wrong word is shown in child processes on the
measurement library (tests/audit_child.py), the only build that can make one wrong.

"Loaded" below means resident: loaded, placed, and one decision taken — the K1 work plan, and
with it the compact-flush tables TOUCH checks, is made by the first step."""
import json
import os
import random
import subprocess
import sys

import numpy as np
import pytest

from audit_child import POKES, SPARE, expected_counts, load_small, node_cap, pair_counts, small_cluster
from oracle import oracle as O
from oracle import soa
from test_gpu_slots import synth_groups_for_slots

pytestmark = pytest.mark.gpu
soa.build()

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
MEASURE = os.path.join(ROOT, "escalator_amd", "libescalator_hip_measure.so")
CHECKS = ["ENTRY", "FIRST", "REGION", "OCC", "TOUCH", "TRACKER", "MIRROR"]
TAINT = "atlassian.com/escalator"


@pytest.fixture(scope="module")
def esc():
    import escalator_amd
    return escalator_amd


def assert_clean(rep, want=None, tag=""):
    """Nothing skipped, no mismatch, first_bad unset; n_checked as computed on the CPU."""
    print(tag, json.dumps(rep))
    assert rep["skipped"] == [], (tag, rep)
    assert sorted(k for k in rep if k != "skipped") == sorted(CHECKS), (tag, rep)
    for k in CHECKS:
        assert rep[k]["n_bad"] == 0 and rep[k]["first_bad"] == -1, (tag, k, rep[k])
    for k, n in (want or {}).items():
        assert rep[k]["n_checked"] == n, (tag, k, rep[k], n)
    assert rep["TOUCH"]["n_checked"] > 0, (tag, rep["TOUCH"])          # (its count depends on the K1 plan)


def assert_decision(ctx, states, P, N, groups, name_of=None, names=None):
    """Totals and decisions equal the C oracle's (first_node through the nodes' names when the
    device's indices are not the list's)."""
    otot = soa.totals(P, N, groups)
    odf, odi = soa.decide(groups, states, otot)
    tot, dec = ctx.decide_all(states)
    diff = {}
    for k, name in enumerate(soa.TOT_FIELDS):
        if name == "flags":
            bad = np.nonzero((tot[name] != 0) != (otot[:, k] != 0))[0]
        elif name == "first_node" and name_of is not None:
            got = [name_of(int(j)) if j >= 0 else None for j in tot[name]]
            want = [names[int(j)] if j >= 0 else None for j in otot[:, k]]
            bad = np.array([g for g in range(len(got)) if got[g] != want[g]])
        else:
            bad = np.nonzero(tot[name] != otot[:, k])[0]
        if len(bad):
            diff[name] = [(int(g), int(tot[name][g]), int(otot[g, k])) for g in bad[:4]]
    assert not diff, diff                                      # {field: [(group, device, oracle), ...]}
    assert np.array_equal(dec["cpu_pct"].view(np.uint64), odf[:, 0].view(np.uint64))
    assert np.array_equal(dec["mem_pct"].view(np.uint64), odf[:, 1].view(np.uint64))
    for k, name in enumerate(["delta", "n_to_taint", "cached_cpu_m", "cached_mem_b", "status", "branch", "taint_status"]):
        assert np.array_equal(dec[name].astype(np.int64), odi[:, k]), name


# ------------------------------------------------------------------ clean snapshots
def test_clean_after_load_and_event_rounds(esc):
    """The small context through the event queue: after the load and after each of two mixed
    rounds (node add / delete / relabel / update / facts, a dry group's tracker, pod upsert /
    delete / bind with the placement loaded) every check is clean, nothing is skipped, the counts
    are the CPU's, the decision equals the C oracle and the captured step still replays."""
    from escalator_amd.events import EventQueue
    from randobj import make_nodes, make_pods
    rng, groups, states, pods, nodes = small_cluster()
    ctx = esc.Context(groups)
    ctx.use_graph(True)
    q = EventQueue(spare=SPARE)
    for x in nodes:
        q.node_add(x)
    for p in pods:
        q.pod_add(p)
    dry = next(g for g, s in enumerate(groups) if s["dry_mode"] and s["label_key"])
    member = O.new_node_label_filter_func(groups[dry]["label_key"], groups[dry]["label_value"])
    tracked = []
    loaded = [0, 0]                                            # [reloads seen, nodes at the last load]

    def check(tag):
        if q.reloads != loaded[0]:
            loaded[:] = [q.reloads, len(q.live_nodes())]
        live_n, live_p = q.live_nodes(), q.live_pods()
        trk = {dry: [m for m in tracked if q.node_index(m) is not None]}
        P, N = ctx.pack(live_p, live_n, trk)
        names = [x["name"] for x in live_n]
        assert_decision(ctx, states, P, N, groups, q.node_name, names)    # (the first one makes the plan)
        want = expected_counts(N, groups, node_cap(loaded[1]))
        assert_clean(ctx.audit(), want, tag)
        assert_decision(ctx, states, P, N, groups, q.node_name, names)    # after the audit: a graph replay
        assert ctx.audit(["OCC", "FIRST"]).keys() == {"OCC", "FIRST", "skipped"}

    q.flush(ctx)
    check("load")
    for rnd in range(2):
        live = [x["name"] for x in q.live_nodes()]
        for m in rng.sample(live[2:], 3):                       # deletes (node-0 and node-1 stay)
            q.node_delete(m)
            live.remove(m)
        some = q.nodes[rng.choice(live)]["created_ns"]
        for k, x in enumerate(make_nodes(rng, 5, groups, big_frac=0.0)):   # adds: old, new, an equal creation time
            q.node_add(dict(x, name="r%d-%d" % (rnd, k), created_ns=[some, some + 10**9, 10**18][k % 3], taints=[TAINT],
                            taint_value=str(1_700_000_000 - 100 * k)))
        q.node_add({"name": "r%d-dry" % rnd, "labels": {groups[dry]["label_key"]: groups[dry]["label_value"]},
                    "unschedulable": False, "taints": [], "cpu": 4000, "mem": 8 << 30, "created_ns": some})
        for m in rng.sample(live[2:], 4):                       # relabels between groups
            q.node_update(dict(q.nodes[m], labels=make_nodes(rng, 1, groups, big_frac=0.0)[0]["labels"]))
        for m in rng.sample(live[2:], 4):                       # cordons, allocatable
            q.node_update(dict(q.nodes[m], unschedulable=not q.nodes[m]["unschedulable"], cpu=rng.choice([2000, 32000])))
        for m in rng.sample(live[2:], 3):                       # the taint time alone
            q.node_update(dict(q.nodes[m], taints=[TAINT], taint_value=str(1_700_000_500 + rnd)))
        keys = sorted(q.pods)
        for k in rng.sample(keys, 20):
            q.pod_delete(k)
            keys.remove(k)
        for k in rng.sample(keys, 20):                          # spec changes in place
            q.pod_update(dict(make_pods(rng, 1, groups, big_frac=0.0)[0], name=k, node_name=q.pods[k]["node_name"]))
        for k, p in enumerate(make_pods(rng, 15, groups, big_frac=0.0)):
            q.pod_add(dict(p, name="r%d-p%d" % (rnd, k), node_name=rng.choice(live + ["", "r%d-0" % rnd])))
        for k in rng.sample(keys, 15):                          # moved, unbound
            q.pod_update(dict(q.pods[k], node_name=rng.choice(live + [""])))
        q.flush(ctx)
        free = [x["name"] for x in q.live_nodes() if member(x) and x["name"] not in tracked][:3]
        assert free, "the dry group has no untracked member"
        tracked = tracked[1 if rnd else 0:] + free              # round 1 also drops the oldest name
        # the device's tracker against the names (a reload drops it, as ResidentController knows)
        have = {int(j) for j in ctx.tracker_list(dry)}
        want_idx = {q.node_index(m) for m in tracked} - {None}
        ctx.tracker_update(dry, add=sorted(want_idx - have), remove=sorted(have - want_idx))
        check("round %d" % rnd)
    print(q.reload_causes, q.applied)
    assert all(n > 0 for n in q.applied.values()), q.applied     # every kind of event was applied in place


# ------------------------------------------------------------------ shapes
def _node(name, labels, i, **kw):
    return dict({"name": name, "labels": labels, "unschedulable": False, "taints": [], "cpu": 4000, "mem": 8 << 30,
                 "created_ns": 1_700_000_000 * 10**9 + i * 1000}, **kw)


def _pod(name, pool, node_name=""):
    return {"name": name, "owner_kinds": [], "annotations": {}, "node_selector": {"pool": pool}, "affinity": None,
            "containers": [{"cpu": 100, "mem": 1 << 20}], "init_containers": [], "overhead": None, "node_name": node_name}


def _group(name, **kw):
    return dict({"name": name, "label_key": "pool", "label_value": name, "min_nodes": 0, "max_nodes": 5000,
                 "taint_lower_pct": 20, "taint_upper_pct": 40, "scale_up_pct": 70, "slow_removal_rate": 1,
                 "fast_removal_rate": 2, "dry_mode": False}, **kw)


def _resident(esc, groups, pods, nodes, spare, states=None):
    from escalator_amd.objects import placement
    ctx = esc.Context(groups)
    ctx.set_spare(spare)
    P, N = ctx.pack(pods, nodes)
    ctx.load(P, N)
    ctx.load_placement(*placement(pods, nodes))
    ctx.decide_all(states)
    return ctx, P, N


def test_pair_of_one_node_and_group_without_members(esc):
    groups = [_group("one"), _group("none"), _group("some"), _group("dry", dry_mode=True)]
    nodes = [_node("a", {"pool": "one"}, 0)] + [_node("s%d" % i, {"pool": "some"}, i + 1) for i in range(5)]
    pods = [_pod("p%d" % i, ["one", "none", "some", "dry"][i % 4], ["a", "", "s0"][i % 3]) for i in range(12)]
    ctx, P, N = _resident(esc, groups, pods, nodes, 1.0)
    assert pair_counts(N, 4).tolist() == [1, 0, 5, 0]
    want = expected_counts(N, groups, node_cap(6, 1.0))
    assert (want["ENTRY"], want["REGION"], want["FIRST"]) == (6, 6, 4)
    assert_clean(ctx.audit(), want, "one / none")
    ctx.nodes_delete([0])                                      # the pair of one node loses it
    want = dict(want, ENTRY=5, OCC=5, REGION=5)
    assert_clean(ctx.audit(), want, "deleted")
    assert_decision(ctx, None, *ctx.pack(pods, nodes[1:]), groups, lambda j: nodes[j]["name"], [x["name"] for x in nodes[1:]])


def test_two_piece_pair_with_relabelled_in_nodes(esc):
    """A pair of more than NODE_PIECE (1 024) entries — two pieces — that then takes relabelled
    nodes of lower indices: their entries sit behind the others, so the pair's entries are not
    node-sorted and its lowest member is found at its end."""
    groups = [_group("big"), _group("other")]
    nodes = [_node("o%d" % i, {"pool": "other"}, 5000 - i) for i in range(20)] + \
            [_node("b%d" % i, {"pool": "big"}, i) for i in range(1100)]
    pods = [_pod("p%d" % i, "big", "b%d" % (i % 7)) for i in range(300)]
    ctx, P, N = _resident(esc, groups, pods, nodes, 0.1)
    want = expected_counts(N, groups, node_cap(1120, 0.1))
    assert want["ENTRY"] == 1120
    assert_clean(ctx.audit(), want, "two pieces")
    moved = [dict(nodes[j], labels={"pool": "big"}) for j in (3, 4, 11)]
    ctx.nodes_relabel([3, 4, 11], ctx.pack([], moved)[1])
    now = [moved[[3, 4, 11].index(j)] if j in (3, 4, 11) else x for j, x in enumerate(nodes)]
    P2, N2 = ctx.pack(pods, now)
    assert pair_counts(N2, 2).tolist() == [1103, 17]
    assert_clean(ctx.audit(), expected_counts(N2, groups, node_cap(1120, 0.1)), "relabelled in")
    assert_decision(ctx, None, P2, N2, groups)
    tot, _ = ctx.results()
    assert int(tot["first_node"][0]) == 3                      # the pair's lowest member: a relabelled node


def test_split_region_with_equal_creation_times(esc):
    """A group of more than ORD_CHUNK (4 096) memberships — a split region — holding runs of
    equal creation times (ordered by node index), beside a dry group with a tracker."""
    s = esc.Synth(20_000, 40_000, 6, config=5, seed=0xE5CA1A7E00000005)
    P, N = s.pods(), {k: v.copy() for k, v in s.nodes().items()}
    t = soa.group_tables(s.groups)
    cnt = pair_counts(N, t["n_gp"])
    big = int(np.argmax(cnt))
    members = np.nonzero(N["label0"] == big)[0]
    N["created_ns"][members[100:160]] = N["created_ns"][members[0:60]]
    N["created_ns"][members[200:204]] = N["created_ns"][members[0]]
    assert cnt[big] > 4096 and t["dry"].any() and len(N["trk_node"]) > 0
    ctx = esc.Context(s)
    ctx.set_spare(0.05)
    ctx.load(P, N)
    rng = np.random.default_rng(5)
    pod_node = rng.integers(0, len(N["flags"]), len(P["flags"])).astype(np.uint32)
    ctx.load_placement(pod_node, np.full(len(N["flags"]), -(1 << 63), np.int64), np.zeros(len(N["flags"]), np.uint8))
    ctx.set_order_in_step(True)
    assert_decision(ctx, s.states, P, N, s.groups)
    assert_clean(ctx.audit(), expected_counts(N, s.groups, node_cap(40_000, 0.05)), "split region")
    g = int(np.nonzero(t["gpair"] == big)[0][0])
    assert np.array_equal(ctx.group_order(g, 0), soa.order(N, s.groups, g, 0))


@pytest.mark.parametrize("S", [129, 10_241])
def test_pod_slots_across_lds_windows(esc, S):
    """S pod slots: one LDS window at 129, two at 10 241 (the default filter's slot alone in the
    second) — the touch bitmap's columns span the windows."""
    s = esc.Synth(40_000, 12_000, synth_groups_for_slots(S), config=4, seed=0xE5CA1A7E00000004)
    P, N = s.pods(), s.nodes()
    t = soa.group_tables(s.groups)
    assert t["n_gp"] + 1 == S and t["default"] >= 0
    ctx = esc.Context(s)
    ctx.load_synth(s)
    rng = np.random.default_rng(S)
    pod_node = rng.integers(0, len(N["flags"]), len(P["flags"])).astype(np.uint32)
    ctx.load_placement(pod_node, np.full(len(N["flags"]), -(1 << 63), np.int64), np.zeros(len(N["flags"]), np.uint8))
    assert_decision(ctx, s.states, P, N, s.groups)
    rep = ctx.audit()
    assert_clean(rep, expected_counts(N, s.groups, node_cap(12_000, 0.0)), "S=%d" % S)
    assert rep["TOUCH"]["n_checked"] >= S // 32                # every column with a pod, in some workgroup


def test_three_pod_shards_in_one_context(esc):
    """Three shards on one device (the peer exchange): every shard audits what it holds; the
    report is clean and its counts are the shards' summed — each holds the whole node table and
    its own pods' occupancy words over all entries, and the regions of the groups it owns."""
    from escalator_amd.objects import placement
    from randobj import make_trackers
    rng, groups, states, pods, nodes = small_cluster()
    trk = make_trackers(rng, groups, nodes)
    ctx = esc.Context(groups, devices=[0, 0, 0])
    ctx.set_spare(SPARE)
    P, N = ctx.pack(pods, nodes, trk)
    ctx.load(P, N)
    ctx.load_placement(*placement(pods, nodes))
    assert_decision(ctx, states, P, N, groups)
    one = expected_counts(N, groups, node_cap(300))
    want = expected_counts(N, groups, node_cap(300), ranks=3)
    assert want["OCC"] == 3 * one["OCC"] and want["REGION"] == one["REGION"] and want["FIRST"] == one["FIRST"]
    assert_clean(ctx.audit(), want, "three shards")
    assert_decision(ctx, states, P, N, groups)


# ------------------------------------------------------------------ detection (child processes)
def run_child(*args):
    assert os.path.exists(MEASURE), "build the measurement library: make -C escalator_amd/csrc ABLATIONS=1"
    env = dict(os.environ, ESC_LIB_PATH=MEASURE)
    try:
        r = subprocess.run([sys.executable, "-u", os.path.join(HERE, "audit_child.py"), *args], capture_output=True,
                           text=True, timeout=240, env=env, cwd=ROOT)
    except subprocess.TimeoutExpired:
        pytest.exit("audit_child.py %s hung: nothing more is started on this GPU" % " ".join(args), 1)
    if r.returncode in (134, 139, -6, -11):                    # an abort or a fault: the session ends here
        pytest.exit("audit_child.py %s died (%d): %s" % (" ".join(args), r.returncode, r.stderr[-2000:]), 1)
    assert r.returncode == 0, r.stderr[-3000:]
    return json.loads([x for x in r.stdout.splitlines() if x.startswith("{")][-1])


# poke target -> the check that owns the poked word.  One wrong word is reported once: n_bad == 1
# and first_bad == the poked id (the reverse half of ENTRY is not reachable by a poke: no target
# changes an entry's node or the node -> entries map, which kernels index with).
OWNER = {"entry_flags": "ENTRY", "entry_cpu": "ENTRY", "region_flags": "REGION", "region_swap": "REGION", "occ": "OCC",
         "touch": "TOUCH", "node_tracked": "TRACKER", "first_cpu": "FIRST", "host_ncpu": "MIRROR"}
# words that legitimately feed more than one check: a node's tracker bit in the node table is
# copied into each of its entries (ENTRY, one mismatch per group pair of the node), into its
# membership word of each wet group (REGION) and into the host mirror (MIRROR)
ALSO = {"node_tracked": {"ENTRY": "incidences", "REGION": "wet_memberships", "MIRROR": 1}}


@pytest.mark.parametrize("target", sorted(POKES))
def test_every_check_detects_its_corruption(target):
    r = run_child("poke", target)
    rep, own = r["report"], OWNER[target]
    print(target, json.dumps(r))
    assert rep["skipped"] == [], rep
    assert rep[own]["n_bad"] == 1 and rep[own]["first_bad"] == r["id"], (target, rep[own], r["id"])
    also = ALSO.get(target, {})
    for k in CHECKS:
        if k == own:
            continue
        n = also.get(k, 0)
        n = r["aux"][n] if isinstance(n, str) else n
        assert rep[k]["n_bad"] == n, (target, k, rep[k], n)
        if n:
            assert rep[k]["first_bad"] >= 0
            if k == "MIRROR":
                assert rep[k]["first_bad"] == r["id"]
        else:
            assert rep[k]["first_bad"] == -1
    assert r["refused"] == [-1] * len(r["refused"]), r["refused"]          # ESC_E_INVAL outside the table
    if target == "node_tracked":
        assert r["aux"]["incidences"] >= 1


def test_controller_heals_after_a_poked_occupancy_word():
    """ResidentController(audit_every=1): the scan whose audit finds the poked word reloads once
    (cause "audit:OCC"); that scan's records and every later scan's equal the reloading
    Controller's (asserted scan by scan inside the child's drive)."""
    r = run_child("heal")
    print(json.dumps(r))
    assert r["reload_causes"] == ["first", "audit:OCC"], r
    assert r["reloads"] == [1, 1] + [2] * (r["scans"] - 2), r
    assert r["audit_failures"] == 1 and r["audits"] == r["scans"] and r["last_clean"], r


def test_checks_without_resident_state_are_skipped():
    r = run_child("skips")
    print(json.dumps(r))
    assert r["unloaded_rc"] == -5                              # ESC_E_STATE before esc_load_nodes
    assert r["loaded"] == ["OCC", "TOUCH"], r
    assert set(r["asked_tracker_only"]) == {"TRACKER", "skipped"} and r["asked_tracker_only"]["skipped"] == [], r
    assert r["build_rc"] == -2 and r["no_index"] == ["REGION", "OCC", "TOUCH"], r      # ESC_E_HIP: the build failed
    assert r["index_again"] == ["OCC", "TOUCH"], r
    assert r["placed"] == ["TOUCH"], r
    assert r["resident"] == [] and r["resident_clean"], r
