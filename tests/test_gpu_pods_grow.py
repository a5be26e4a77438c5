"""GPU: esc_pods_grow — the pod classes of the resident snapshot grown on the device.

``PodWorld`` is tests/test_gpu_rebuild.py's ``World`` with pod events: it holds the live pods by
id and, after every step a test names, compares everything the context answers with the oracles
on the live objects and with a fresh context loaded with the same objects, and asserts a clean
esc_audit with every check (TOUCH, OCC and MIRROR among them).  The capacities a grow leaves are
compared with the rule of include/escalator_hip.h, computed here.

The injected failure before the swap runs in a child process on the measurement library
(tests/pods_grow_child.py)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from oracle import soa
from test_gpu_audit import assert_decision
from test_gpu_rebuild import E_LIMIT, MEASURE, World, group, node, pod, tainted

pytestmark = pytest.mark.gpu
soa.build()

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SMALL0 = 256                                      # class id of packed small pods without extra pairs
NONE = 0xFFFFFFFF


@pytest.fixture(scope="module")
def esc():
    import escalator_amd
    assert escalator_amd._lib.ESC_E_LIMIT == E_LIMIT
    return escalator_amd


def tiles(n):
    return (n + 255) // 256


def want(live, arr, f):
    x = live + arr
    return x + (max(1, int(x * f)) if f > 0 else 0)


def room(ctx):
    r = ctx.pods_room()
    return [r["k_capacity"], r["k_free"], r["c_free"], r["per_class"].tolist()]


def code_of(esc, fn, *a):
    with pytest.raises(esc._lib.EscError) as e:
        fn(*a)
    return e.value.code


class PodWorld(World):
    """World + pod events by id (a new id appends; ids of deleted pods are None)."""

    def _targets(self, pods):
        return np.array([self.idx.get(p["node_name"], NONE) if p["node_name"] else NONE for p in pods], np.uint32)

    def upsert(self, ids, pods):
        rc = self.ctx.pods_upsert(ids, self.ctx.pack(pods, [])[0])
        if rc:
            return rc
        for i, p in zip(ids, pods):
            self.pods.extend([None] * (i + 1 - len(self.pods)))
            self.pods[i] = p
        self.ctx.pods_bind(ids, self._targets(pods))
        return 0

    def grow(self, ids=None, pods=None):
        self.ctx.pods_grow(ids, self.ctx.pack(pods, [])[0] if pods else None)

    def delete(self, ids):
        self.ctx.pods_delete(ids)
        for i in ids:
            self.pods[i] = None

    def bind(self, ids, names):
        for i, m in zip(ids, names):
            self.pods[i] = dict(self.pods[i], node_name=m)
        self.ctx.pods_bind(ids, self._targets([self.pods[i] for i in ids]))


def four_pools(n_nodes=12):
    groups = [group("one"), group("some"), group("dry", dry_mode=True), group("default", key="", value="")]
    nodes = [(tainted if i % 4 == 3 else node)("n%d" % i, {"pool": ["one", "some", "dry"][i % 3]}, i)
             for i in range(n_nodes)]
    return groups, nodes


def small_pods(n, start=0, n_nodes=12, bound=lambda i: i % 5 != 0):
    return [pod("p%d" % i, ["one", "some", "dry", ""][i % 4], "n%d" % (i % n_nodes) if bound(i) else "", cpu=100 + i % 50)
            for i in range(start, start + n)]


def burst_pods(n, start):
    """A burst as the scheduler has seen little of it yet: few of its pods are bound (the runs'
    spare room is the placement's matter, not the classes')."""
    return small_pods(n, start, bound=lambda i: i % 61 == 7)         # (61: the bound ones spread over the 12 nodes)


# ------------------------------------------------------------------ a full class
def run_full_class(esc, devices=None):
    """300 packed-small pods at spare 0.25: want 375, two tiles, 212 free; 16 spare C slots."""
    groups, nodes = four_pools()
    w = PodWorld(esc, groups, small_pods(300), nodes, 0.25, devices=devices)
    w.check("load")
    k = len(devices) if devices else 1
    if k == 1:
        r = w.ctx.pods_room()
        assert r["per_class"][SMALL0] == 212 and r["c_free"] == 16
        assert sorted(set(r["per_class"].tolist())) == [-1, 212, 256]
        # with spare room every signature the K layout holds has a class: 64 plain (at most 3
        # records, 0..3 extra pairs), 4 packed, 4 packed small; the 71 without pods one tile each
        assert int((r["per_class"] >= 0).sum()) == 72
        assert r["k_capacity"] == (71 + 2) * 256 and r["k_free"] == 71 * 256 + 212
    burst = burst_pods(400, 300)
    ids = list(range(300, 700))
    before, r0 = w.ctx.audit(), room(w.ctx)
    assert w.upsert(ids, burst) == E_LIMIT                     # more than 212 + 16
    assert w.ctx.audit() == before and room(w.ctx) == r0       # refused: nothing changed
    w.grow(ids, burst)
    r = w.ctx.pods_room()
    if k == 1:
        # the rule: 300 live + 400 arrivals + floor(700 * 0.25) = 875 -> 4 tiles; the classes
        # without pods keep their one tile; the 16 free C slots are the spare the rule asks for
        assert tiles(want(300, 400, 0.25)) == 4
        assert r["per_class"][SMALL0] == 4 * 256 - 300 and r["c_free"] == 16
        assert r["k_capacity"] == (71 + 4) * 256
    w.check("grown")                                           # nothing moved for the answers
    assert w.upsert(ids, burst) == 0
    if k == 1:
        assert w.ctx.pods_room()["per_class"][SMALL0] == 4 * 256 - 700
    w.check("burst in")
    w.grow()                                                   # room enough: nothing to do
    assert room(w.ctx)[0] == r["k_capacity"]
    return w


def test_full_class_grows_and_the_burst_fits(esc):
    w = run_full_class(esc)
    # pod events go on in the grown layout
    w.delete(list(range(0, 700, 7)))
    assert w.upsert([0, 7, 700], small_pods(3, 900)) == 0
    w.bind([1, 2], ["n5", ""])
    w.check("events after")


def test_multi_device_context(esc):
    """devices=[0, 0]: the burst's new ids belong to the last device's shard; every device's share
    is checked before any device grows."""
    run_full_class(esc, devices=[0, 0])


def test_two_shards_only_one_grows(esc):
    """Two sharded contexts (world 2) with the host exchange: the burst lands on rank 1, whose
    class is full; rank 0 takes a few pods in place and does not grow.  No collective: rank 1's
    grow is its own.  The merged decision equals the C oracle over every pod."""
    from escalator_amd.dist import merge_owned
    from test_gpu import _packed_subset, check_against_c_oracle
    groups, nodes = four_pools()
    base, few, burst = small_pods(600), small_pods(5, 2000), burst_pods(400, 3000)
    ctxs, rooms = [], []
    for r in range(2):
        c = esc.Context(groups, rank=r, world=2)
        c.set_spare(0.25)
        P, N = c.pack(base, nodes)
        c.load(_packed_subset(P, list(range(300 * r, 300 * r + 300))), N, pod_offset=300 * r)
        ctxs.append(c)
        rooms.append(room(c))
    c0, c1 = ctxs
    assert c0.pods_upsert(list(range(300, 305)), c0.pack(few, [])[0]) == 0          # ids are the shard's own
    B = c1.pack(burst, [])[0]
    ids = list(range(300, 700))
    assert c1.pods_upsert(ids, B) == E_LIMIT and room(c1) == rooms[1]
    c1.pods_grow(ids, B)
    assert c1.pods_room()["per_class"][SMALL0] == tiles(want(300, 400, 0.25)) * 256 - 300
    assert c1.pods_upsert(ids, B) == 0
    assert c0.pods_room()["k_capacity"] == rooms[0][0]                               # rank 0 did not grow
    words, firsts = [], []
    for c in ctxs:
        c.set_state(None)
        c.reduce()
        w, f = c.exchange_download()
        words.append(w)
        firsts.append(f)
    W, F = np.sum(words, axis=0), np.min(firsts, axis=0)
    parts = []
    for c in ctxs:
        c.exchange_upload(W, F)
        c.decide()
        parts.append(c.results())
    tot, dec = merge_owned(parts)
    P, N = c0.pack(base + few + burst, nodes)
    otot = soa.totals(P, N, groups)
    odf, odi = soa.decide(groups, None, otot)
    check_against_c_oracle(tot, dec, otot, odf, odi)
    for c in ctxs:
        rep = c.audit(["ENTRY", "FIRST", "REGION", "TOUCH", "TRACKER", "MIRROR"])
        assert rep["skipped"] == [] and all(rep[k]["n_bad"] == 0 for k in rep if k != "skipped"), rep
        c.close()


# ------------------------------------------------------------------ every format
KEY = "t"
GI = 1 << 30


def _in(key, values):
    return {"node_affinity": {"required": [[{"key": key, "op": "In", "values": list(values)}]]},
            "pod_affinity": False, "pod_anti_affinity": False}


def fmt_pod(kind, i, n_groups):
    """Pod i under its own group pair (t, c<i>), its extra pairs the next groups' (as
    tests/decision_table.py gives every case its own pair): one misplaced byte changes one group."""
    np_, containers = {
        "s0": (0, [(100 + i % 900, (1 << 20) + i)]), "s1": (1, [(100 + i % 900, (1 << 20) + i)]),
        "s2": (2, [(100 + i % 900, (1 << 20) + i)]), "s3": (3, [(100 + i % 900, (1 << 20) + i)]),
        "p12": (0, [(200 + i % 900, 17 * GI + i)]),                      # a request past 16 GiB
        "k00": (0, [((1 << 20) + i, 5)]),                                # outside the packed ranges
        "k11": (1, [((1 << 20) + i, 5), (3, 7 + i)]),
        "k33": (3, [((1 << 20) + i, 5), (3, 7 + i), (5, 11), (7, 13 + i)]),
    }[kind]
    extra = ["c%d" % ((i + 1 + k) % n_groups) for k in range(np_)]
    return {"name": "f%d" % i, "owner_kinds": [], "annotations": {}, "node_selector": {KEY: "c%d" % i},
            "affinity": _in(KEY, extra) if extra else None,
            "containers": [{"cpu": c, "mem": m} for c, m in containers], "init_containers": [], "overhead": None,
            "node_name": ""}


LOADED = [("s0", 255), ("s1", 256), ("s2", 257), ("s3", 255), ("p12", 256), ("k00", 257), ("k11", 255)]
BURST = [("s1", 1), ("p12", 600), ("k33", 257)]                 # one tile, several, a class created; s0 gets nothing
# class id = signature | packed << 7, signature = regular * 32 + init * 8 + overhead * 4 + extra pairs
CLASS_ID = {"s0": 256, "s1": 257, "s2": 258, "s3": 259, "p12": 128, "k00": 0, "k11": 1 * 32 + 1, "k33": 3 * 32 + 3}


@pytest.fixture(scope="module")
def formats(esc):
    """The objects and the oracle's expectation, computed once for every variant."""
    n_total = sum(n for _, n in LOADED + BURST)
    groups = [dict(group("g%d" % i, key=KEY, value="c%d" % i)) for i in range(n_total)]
    pods, i = [], 0
    for kind, n in LOADED + BURST:
        pods += [fmt_pod(kind, i + k, n_total) for k in range(n)]
        i += n
    nodes = [node("n%d" % j, {KEY: "c%d" % (j * 37 % n_total)}, j) for j in range(64)]
    n_loaded = sum(n for _, n in LOADED)
    ctx = esc.Context(groups, device=-1)
    P0, N = ctx.pack(pods[:n_loaded], nodes)
    P1, _ = ctx.pack(pods, nodes)
    ctx.close()
    return {"groups": groups, "pods": pods, "nodes": nodes, "n_loaded": n_loaded, "P0": P0, "P1": P1, "N": N}


@pytest.mark.parametrize("variant", ["plain", "force_wide", "graph", "replicas", "calibrated"])
def test_every_format_in_one_context(esc, formats, variant):
    """Loaded at spare 0 (classes only for the formats present, every class full to its last
    tile): packed small with 0..3 extra pairs, 12-B packed, plain with (R, NXP) = (0, 0), (1, 1);
    255 / 256 / 257 pods.  The grow gives packed small nothing, the 1-pair class one tile, the
    12-B class several and creates the plain (3, 3) class."""
    F = formats
    groups, pods, n0 = F["groups"], F["pods"], F["n_loaded"]
    reps = 3 if variant == "replicas" else 1
    ctx = esc.Context(groups)
    ctx.set_spare(0.0)
    ctx.load(F["P0"], F["N"], replicas=reps)
    if variant == "force_wide":
        ctx.force_wide(True)
    if variant == "graph":
        ctx.use_graph(True)
    assert_decision(ctx, None, F["P0"], F["N"], groups)
    if variant == "calibrated":
        ctx.k1_calibrate(2)
    r = ctx.pods_room()
    for kind, n in LOADED:
        assert r["per_class"][CLASS_ID[kind]] == tiles(n) * 256 - n, kind
    assert r["per_class"][CLASS_ID["k33"]] == -1 and r["c_free"] == 0
    assert r["k_capacity"] == sum(tiles(n) for _, n in LOADED) * 256
    ids = list(range(n0, len(pods)))
    B, _ = ctx.pack(pods[n0:], [])
    before = ctx.audit()
    assert ctx.pods_upsert(ids, B) == E_LIMIT
    assert ctx.audit() == before
    ctx.pods_grow(ids, B)
    r = ctx.pods_room()
    arr = dict(BURST)
    for kind, n in LOADED + [("k33", 0)]:
        assert r["per_class"][CLASS_ID[kind]] == tiles(n + arr.get(kind, 0)) * 256 - n, kind
    assert r["c_free"] == 0
    for _ in range(reps):                                      # every replica, before the batch
        assert_decision(ctx, None, F["P0"], F["N"], groups)
    assert ctx.pods_upsert(ids, B) == 0
    for _ in range(reps):                                      # and with it
        assert_decision(ctx, None, F["P1"], F["N"], groups)
    rep = ctx.audit(["TOUCH", "MIRROR", "ENTRY", "FIRST", "REGION", "TRACKER"])
    assert rep["skipped"] == [] and all(rep[k]["n_bad"] == 0 for k in rep if k != "skipped"), rep
    # a fresh context loaded with the same pods: the same capacity and the same words
    fresh = esc.Context(groups)
    fresh.set_spare(0.0)
    fresh.load(F["P1"], F["N"])
    a, b = ctx.decide_all(None), fresh.decide_all(None)
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()
    assert fresh.pods_room()["k_capacity"] == r["k_capacity"]
    assert ctx.stream_bytes() == fresh.stream_bytes()
    fresh.close()
    ctx.close()


# ------------------------------------------------------------------ the C section
def c_pod(name, i, pools, node_name, containers=5, pairs=1):
    """A C-section pod: `containers` containers, `pairs` group pairs (the selector's + In values)."""
    own = pools[i % len(pools)]
    more = [pools[(i + 1 + k) % len(pools)] for k in range(pairs - 1)]
    return {"name": name, "owner_kinds": [], "annotations": {}, "node_selector": {"pool": own},
            "affinity": _in("pool", more) if more else None,
            "containers": [{"cpu": 10 + (i + k) % 90, "mem": (1 << 20) + k} for k in range(containers)],
            "init_containers": [], "overhead": None, "node_name": node_name}


def test_c_section_grows_by_spare_tiles(esc):
    pools = ["q%d" % k for k in range(9)]
    groups = [group(m) for m in pools]
    nodes = [(tainted if i % 4 == 3 else node)("n%d" % i, {"pool": pools[i % 9]}, i) for i in range(18)]
    # 64 pods of 5 containers in a row: one C tile of 256 extra records (the big-tile path);
    # then pods with 6 pairs (5 extra: indirect PodRefs once bound) and a few K pods
    pods = [c_pod("big%d" % i, i, pools, "n%d" % (i % 18)) for i in range(64)]
    pods += [c_pod("wide%d" % i, i, pools, "n%d" % (i % 18), containers=1, pairs=6) for i in range(10)]
    pods += [pod("k%d" % i, pools[i % 9], "n%d" % (i % 18)) for i in range(40)]
    w = PodWorld(esc, groups, pods, nodes, 0.25)
    w.check("load")
    n0 = len(pods)
    free = w.ctx.pods_room()["c_free"]
    assert free == 32                                          # max(16, ceil(74 * 0.25)) = 19 -> two tiles of 16
    fill = [c_pod("fill%d" % i, i, pools, "n%d" % (i % 18), containers=5, pairs=1 + 5 * (i % 2)) for i in range(free)]
    assert w.upsert(list(range(n0, n0 + free)), fill) == 0     # the spare C slots used up
    assert w.ctx.pods_room()["c_free"] == 0
    w.check("spare slots full")
    more = [c_pod("more%d" % i, i, pools, "n%d" % (i % 18), containers=3 + 2 * (i % 2), pairs=6) for i in range(5)]
    ids = list(range(n0 + free, n0 + free + 5))
    before, r0 = w.ctx.audit(), room(w.ctx)
    assert w.upsert(ids, more) == E_LIMIT
    assert w.ctx.audit() == before and room(w.ctx) == r0
    # a pod with 7 extra pairs fits no spare slot: refused whole, nothing changed
    odd = more[:2] + [c_pod("odd", 0, pools, "", containers=1, pairs=8)]
    assert code_of(esc, w.grow, ids[:2] + [ids[-1] + 1], odd) == E_LIMIT
    assert w.ctx.audit() == before and room(w.ctx) == r0
    w.grow(ids, more)
    # the rule: 5 arrivals + max(16, ceil((74 + 32 + 5) * 0.25)) = 33 wanted, none free: 3 tiles
    assert w.ctx.pods_room()["c_free"] == 48
    w.check("grown")
    assert w.upsert(ids, more) == 0
    assert w.ctx.pods_room()["c_free"] == 43
    w.check("burst in")
    w.bind([ids[0], n0], ["n3", ""])
    w.delete([ids[1], 2, 65])
    w.check("bind and delete after")


# ------------------------------------------------------------------ three bursts in a row
def test_three_bursts_with_deletes_between(esc):
    groups, nodes = four_pools()
    w = PodWorld(esc, groups, small_pods(1000), nodes, 0.25)
    w.check("load", fresh=False)
    n, grows = 1000, 0
    for k, add in enumerate([1000, 1300, 1700]):
        gone = [i for i in range(k, n, 11 + k) if w.pods[i] is not None]
        w.delete(gone)
        burst = burst_pods(add, 10_000 * (k + 1))
        ids = gone[:50] + list(range(n, n + add - 50))         # freed ids and new ones
        before = room(w.ctx)
        if w.upsert(ids, burst) == E_LIMIT:
            assert room(w.ctx) == before
            w.grow(ids, burst)
            grows += 1
            # every pod here is in the packed small class without extra pairs, none parked in a C
            # slot (a refused batch parks none): the class holds the live pods, capacity = free + live
            live = sum(p is not None for p in w.pods)
            cap0 = before[3][SMALL0] + live
            assert cap0 % 256 == 0
            assert w.ctx.pods_room()["per_class"][SMALL0] == max(cap0, tiles(want(live, add, 0.25)) * 256) - live, k
            assert w.upsert(ids, burst) == 0
        n += add - 50
        w.check("burst %d" % k)
    assert grows == 3 and sum(p is not None for p in w.pods) > 4500


# ------------------------------------------------------------------ refusals
def test_refusals(esc):
    L = esc._lib
    groups, nodes = four_pools()
    ctx = esc.Context(groups)
    assert code_of(esc, ctx.pods_grow) == L.ESC_E_STATE        # before a load
    assert code_of(esc, ctx.pods_room) == L.ESC_E_STATE
    ctx.set_spare(0.25)
    pods = small_pods(20)
    P, N = ctx.pack(pods, nodes)
    ctx.load(P, N)
    B, _ = ctx.pack(small_pods(3, 50), [])
    r0 = room(ctx)
    assert code_of(esc, ctx.pods_grow, [20, 21, 20], B) == L.ESC_E_INVAL     # a repeated id
    assert code_of(esc, ctx.pods_grow, [20, -1, 22], B) == L.ESC_E_INVAL
    assert room(ctx) == r0
    ctx.pods_grow([20, 21, 22], B)                             # fits already: nothing to do
    assert room(ctx) == r0
    ctx.close()
    nodev = esc.Context(groups, device=-1)
    assert code_of(esc, nodev.pods_grow) == L.ESC_E_NODEV
    nodev.close()


def test_a_failure_before_the_swap_changes_nothing():
    assert os.path.exists(MEASURE), "build the measurement library: make -C escalator_amd/csrc ABLATIONS=1"
    env = dict(os.environ, ESC_LIB_PATH=MEASURE)
    try:
        r = subprocess.run([sys.executable, "-u", os.path.join(HERE, "pods_grow_child.py"), "refuse"], capture_output=True,
                           text=True, timeout=240, env=env, cwd=ROOT)
    except subprocess.TimeoutExpired:
        pytest.exit("pods_grow_child.py hung: nothing more is started on this GPU", 1)
    if r.returncode in (134, 139, -6, -11):                    # an abort or a fault: the session ends here
        pytest.exit("pods_grow_child.py died (%d): %s" % (r.returncode, r.stderr[-2000:]), 1)
    assert r.returncode == 0, r.stderr[-3000:]
    out = json.loads([x for x in r.stdout.splitlines() if x.startswith("{")][-1])
    print(json.dumps(out))
    assert out["limit"] == out["e_limit"] and out["code"] == out["hip"], out
    assert out["audit_equal"] and out["room_equal"] and out["answers_equal"], out
    assert out["still_limit"] == out["e_limit"], out
    assert out["upsert"] == 0 and out["bad_after"] == [] and out["skipped_after"] == [], out
    assert out["n_pods"] > 0


# ------------------------------------------------------------------ the controller
def _pod_burst_cluster(base, scan_at, n):
    """tests/test_gpu_resident.py's FakeCluster whose history has a burst of n pods at one scan."""
    class Bursty(base):
        def churn(self, scan, tracked):
            super().churn(scan, tracked)
            if scan == scan_at:
                grp = self.rnd_groups[0]
                for i in range(n):
                    self.put_pod({"name": "pb%d" % i, "owner_kinds": [], "annotations": {},
                                  "node_selector": {grp["label_key"]: grp["label_value"]}, "affinity": None,
                                  "containers": [{"cpu": 50 + i % 20, "mem": 1 << 20}], "init_containers": [],
                                  "overhead": None, "node_name": ""})
    return Bursty


@pytest.mark.parametrize("pod_grow", [True, False])
def test_resident_controller_over_a_burst_history(monkeypatch, pod_grow):
    """Spare 2.0 holds every node event of the history; 1 500 pods at scan 3 fit no class.  With
    the switch on: one pods_grow, no reload after the first load, every scan's records equal to
    the reloading Controller's (drive asserts it scan by scan).  Off: one reload, as before."""
    import test_gpu_resident as R
    from escalator_amd.controller import ResidentController
    monkeypatch.setattr(R, "FakeCluster", _pod_burst_cluster(R.FakeCluster, 3, 1500))

    def resident(groups, clock, actuator, spare):
        return ResidentController(groups, clock=clock, actuator=actuator, spare=spare, pod_grow=pod_grow)
    ra, rb, seen, reloads = R.drive(1, 2.0, resident, R._reload, burst=False)
    ev = ra.events
    if pod_grow:
        assert reloads == [1] * R.SCANS, (reloads, ev.reload_causes)
        assert (ev.pod_grows, ev.pod_grow_causes) == (1, ["pods_upsert"])
    else:
        assert reloads == [1] * 3 + [2] * (R.SCANS - 3), (reloads, ev.reload_causes)
        assert ev.reload_causes == ["first", "pods_upsert"] and ev.pod_grows == 0
