"""GPU: esc_pods_verify — the resident pods compared with a batch of pods as the caller holds them —
and esc_pods_live_ids.

Every expected status comes from tests/pod_verify_literal.py, a restatement of a pod's stored form
that never calls the library; the cases the issue names are asserted by their code as well, so
that the literal and the device cannot agree on a wrong answer unnoticed.  The snapshot is 6
groups (5 pools and the default group) and 1 510 pods hand-packed into every kind of class: packed
small without and with an extra pair (3 and 2 tiles), the 12-byte packed class (one tile, 6 free
positions at spare 0.02, so that a later upsert parks pods in spare C slots), plain classes with
no record, two regular records and an init record, an inert class and C-section pods of 5 records
and 5 extra pairs.

Pair ids that no group selects are stored exactly while they fit a class's field: in a packed
small class "none" is what pair0 >= 2^14 - 1 and an extra pair >= 0xFFFF are stored as, so the
non-group pairs of the lossy cases are 20 000 and 30 000 (pair0) here."""
import copy

import numpy as np
import pytest

import pod_verify_literal as PL
from oracle import soa
from pod_verify_literal import ABSENT, BIND, CLASS, NONE, VALUE, pod
from test_gpu_audit import assert_decision
from test_gpu_rebuild import group, node
from test_gpu_rebuild import pod as obj_pod

pytestmark = pytest.mark.gpu
soa.build()

E_STATE = -5
POOLS = ["q%d" % k for k in range(5)]
N_NODES = 12
SPARE = 0.02
I64_MIN = -(1 << 63)
SMALL, SMALL1, PACKED, PLAIN, PLAIN2, PLAIN_INIT, INERT = 256, 257, 128, 0, 64, 8, 384


@pytest.fixture(scope="module")
def esc():
    import escalator_amd
    assert escalator_amd._lib.ESC_E_STATE == E_STATE
    assert (escalator_amd._lib.PV_ABSENT, escalator_amd._lib.PV_CLASS, escalator_amd._lib.PV_VALUE,
            escalator_amd._lib.PV_BIND) == (ABSENT, CLASS, VALUE, BIND)
    return escalator_amd


def cluster():
    groups = [group(m) for m in POOLS] + [group("default", key="", value="")]
    nodes = [node("n%d" % i, {"pool": POOLS[i % 5]}, i) for i in range(N_NODES)]
    return groups, nodes


def base_pods():
    """The 1 510 pods by id, and each kind's first id."""
    SEL = 4                                                     # has-selector: blocks the default filter
    kinds = {}
    out = []

    def add(name, pods):
        kinds[name] = len(out)
        out.extend(pods)
    add("small", [pod(100 + i % 50, (1 << 20) + i, i % 5, SEL) for i in range(580)] +
        [pod(100 + i, 1 << 20, 20000 + i) for i in range(20)])            # a pair no group selects, stored as none
    add("small1", [pod(200 + i % 50, (2 << 20) + i, i % 3, SEL, xp=[3 + i % 2]) for i in range(300)])
    add("packed", [pod(20000 + i, (1 << 20) + i, i % 5, SEL) for i in range(240)] +
        [pod(21000 + i, 1 << 20, 20000 + i) for i in range(10)])
    add("plain", [pod((1 << 20) + i, (1 << 20) + i) for i in range(100)])
    add("plain2", [pod(1 << 20, 1 << 20, i % 5, SEL, reg=[(100 + i, 1 << 20), (200, 2 << 20)]) for i in range(100)])
    add("init", [pod(1 << 20, 1 << 20, i % 5, SEL, init=[(50 + i, 1 << 20)]) for i in range(60)])
    add("inert", [pod(100 + i, 1 << 20, NONE, 1) for i in range(60)])
    add("c", [pod(10 + i, (1 << 20) + i, 0, SEL, reg=[(10 + i, 1 << 10), (20, 2 << 10), (30, 3 << 10)], init=[(500, 1 << 12)],
                  ovh=(5, 1 << 8), xp=[1, 2, 3, 4, 7]) for i in range(40)])
    return out, kinds


def load(esc, replicas=1, devices=None, placed=False):
    groups, nodes = cluster()
    ctx = esc.Context(groups, **({"devices": devices} if devices else {}))
    ctx.set_spare(SPARE)
    pods, kinds = base_pods()
    _, N = ctx.pack([], nodes)
    ctx.load(PL.soa(pods), N, replicas=replicas)
    n_gp = 6                                                    # the pools' pairs, ids 0..4 in group order, and the default group's
    if not devices:
        assert ctx.lib.esc_ctx_num_group_pairs(ctx.handle) == n_gp and ctx.lib.esc_ctx_pair_id(ctx.handle, b"pool", b"q3") == 3
    pod_node = np.array([i % 11 if i % 4 else NONE for i in range(len(pods))], np.uint32)   # (node 11 holds no pod)
    if placed:
        ctx.load_placement(pod_node, np.full(N_NODES, I64_MIN, np.int64), np.zeros(N_NODES, np.uint8))
    return ctx, pods, kinds, n_gp, pod_node


def where_of(ctx, pods, n_gp):
    """(resident, where) of PL.expect from the context's own map: None for a K pod, else the
    room of its C slot (its own counts for a pod the load put there, a spare slot's for a parked one)."""
    cids = PL.class_ids([p for p in pods if p is not None], n_gp)
    res, where, k = [], [], 0
    for i, p in enumerate(pods):
        cid = ctx.pod_where(i)[0]
        if p is None or cid == -2:
            assert p is None and cid == -2, i
            res.append(None)
            where.append(None)
            continue
        res.append(p)
        where.append(None if cid >= 0 else (PL.room_of(p) if cids[k] < 0 else PL.SPARE_ROOM))
        k += 1
    return res, where


def verify(ctx, ids, offered, pod_node=None):
    st, rep = ctx.pods_verify(ids, PL.soa(offered), pod_node)
    print("verify", len(ids), rep)
    assert rep["n_checked"] == len(ids)
    for name, bit in (("n_absent", ABSENT), ("n_class", CLASS), ("n_value", VALUE), ("n_bind", BIND)):
        assert rep[name] == int(np.count_nonzero(st & bit)), (name, rep)
    bad = np.flatnonzero(st)
    assert rep["first_bad"] == (int(bad[0]) if len(bad) else -1), rep
    assert not np.any((st & CLASS != 0) & (st & VALUE != 0))                    # exclusive
    return st, rep


def assert_all_clean(ctx, pods, tag, pod_node=None):
    ids = [i for i, p in enumerate(pods) if p is not None]
    st, rep = verify(ctx, ids, [pods[i] for i in ids], None if pod_node is None else pod_node[ids])
    assert not st.any() and rep["first_bad"] == -1, (tag, np.flatnonzero(st)[:8], st[st != 0][:8])


# ------------------------------------------------------------------ 1. clean
@pytest.mark.parametrize("replicas", [1, 2])
def test_clean_after_load_upserts_grow_and_compact(esc, replicas):
    ctx, pods, kinds, n_gp, _ = load(esc, replicas)
    assert_all_clean(ctx, pods, "load")
    # 190 changed in place and 10 new pods of the full 12-byte class: 6 take its free positions, 4 are parked
    ids = list(range(190)) + list(range(len(pods), len(pods) + 10))
    new = [dict(pods[i], cpu0=pods[i]["cpu0"] + 7) for i in range(190)] + [pod(30000 + i, 1 << 21, i % 5, 4) for i in range(10)]
    assert ctx.pods_upsert(ids, PL.soa(new)) == 0
    pods = pods + [None] * 10
    for i, p in zip(ids, new):
        pods[i] = p
    parked = [i for i in ids[190:] if ctx.pod_where(i)[0] == -1]
    assert len(parked) == 4, parked
    assert_all_clean(ctx, pods, "upserts")
    ctx.pods_grow(None, None)
    assert_all_clean(ctx, pods, "grow")
    ctx.pods_compact()
    assert all(ctx.pod_where(i)[0] == PACKED for i in parked)                  # positions moved: the locators follow
    assert_all_clean(ctx, pods, "compact")
    assert np.array_equal(ctx.pods_live_ids(), np.arange(len(pods)))
    ctx.close()


# ------------------------------------------------------------------ 2. one change per kind
def pos_map(ctx, first, n):
    """position -> id of the n pods from id `first` (one class)."""
    m = {}
    cid = None
    for i in range(first, first + n):
        c, q = ctx.pod_where(i)
        assert cid is None or c == cid
        cid = c
        m[q] = i
    return cid, m


def case_two(ctx, pods, kinds):
    """The offered batch (every pod of the store, in id order) with one change on each of the
    chosen pods, and the code each named change must give: {id: code}."""
    off = copy.deepcopy(pods)
    want = {}

    def ch(i, code, **kw):
        assert i not in want
        off[i] = dict(off[i], **kw)
        want[i] = code

    def own(p, bits):
        return (p["f"] & ~0xF) | bits
    # --- packed small, no extra pair: 3 tiles, the pods of a pair no group selects last
    cid, at = pos_map(ctx, kinds["small"], 600)
    assert cid == SMALL and sorted(at) == list(range(600))
    assert all(pods[at[q]]["pair0"] >= 20000 for q in range(580, 600))
    p = lambda q: pods[at[q]]                                   # noqa: E731
    ch(at[0], VALUE, cpu0=p(0)["cpu0"] + 1)
    ch(at[1], VALUE, cpu0=p(1)["cpu0"] - 1)
    ch(at[2], VALUE, mem0=p(2)["mem0"] + 1)
    ch(at[3], VALUE, mem0=p(3)["mem0"] - 1)
    ch(at[255], VALUE, pair0=(p(255)["pair0"] + 1) % 5)
    ch(at[256], CLASS, f=own(p(256), 1 | 4))                    # daemonset on: the inert class
    ch(at[599], 0, pair0=30000)                                 # a non-group pair for another: both none
    ch(at[5], CLASS, cpu0=1 << 14)                              # across 2^14 m: the 12-byte class
    ch(at[6], CLASS, mem0=1 << 34)                              # across 2^34 B
    ch(at[7], 0, f=own(p(7), 2))                                # has-selector -> static: the one blocks-default bit
    ch(at[8], 0, f=PL.flags(4, reg=1), cpu0=p(8)["cpu0"] - 10, xc=[(10, 0)])         # a split with the same total
    ch(at[9], VALUE, f=PL.flags(4, reg=1), xc=[(10, 0)])        # a record added: the same class, another request
    ch(at[257], VALUE, f=own(p(257), 0))                        # blocks-default cleared
    # --- packed small, one extra pair: 2 tiles
    cid, at = pos_map(ctx, kinds["small1"], 300)
    assert cid == SMALL1
    p = lambda q: pods[at[q]]                                   # noqa: E731
    ch(at[0], VALUE, xp=[7 - p(0)["xp"][0]])                    # 3 <-> 4
    ch(at[1], VALUE, cpu0=p(1)["cpu0"] + 1)
    ch(at[2], CLASS, f=PL.flags(4), xp=[])                      # the extra pair dropped
    ch(at[3], VALUE, mem0=p(3)["mem0"] + 1)
    ch(at[255], VALUE, mem0=p(255)["mem0"] - 1)
    ch(at[256], VALUE, pair0=(p(256)["pair0"] + 1) % 3)
    ch(at[299], CLASS, f=own(p(299), 1 | 4))
    # --- the 12-byte packed class: one tile
    cid, at = pos_map(ctx, kinds["packed"], 250)
    assert cid == PACKED
    p = lambda q: pods[at[q]]                                   # noqa: E731
    ch(at[0], VALUE, cpu0=p(0)["cpu0"] + 1)
    ch(at[1], VALUE, mem0=p(1)["mem0"] + 1)
    ch(at[2], CLASS, cpu0=1 << 20)                              # across 2^20 m: a plain class
    ch(at[3], CLASS, mem0=1 << 44)                              # across 2^44 B
    ch(at[4], 0, f=PL.flags(4, reg=1), cpu0=p(4)["cpu0"] - 10, xc=[(10, 0)])
    ch(at[5], VALUE, f=own(p(5), 2))                            # the 12-byte class keeps the pod's four bits
    ch(at[6], CLASS, cpu0=100)                                  # small enough for the packed small class
    ch(at[249], VALUE, pair0=30000)                             # 28 bits of pair: kept exactly
    # --- plain, no record
    cid, at = pos_map(ctx, kinds["plain"], 100)
    assert cid == PLAIN
    p = lambda q: pods[at[q]]                                   # noqa: E731
    ch(at[0], VALUE, cpu0=p(0)["cpu0"] + 1)
    ch(at[1], VALUE, mem0=p(1)["mem0"] - 1)
    ch(at[2], VALUE, pair0=2)
    ch(at[3], CLASS, f=PL.flags(0, reg=1), xc=[(1, 1)])         # a record added
    ch(at[99], VALUE, f=own(p(99), 1))
    # --- plain, two regular records
    cid, at = pos_map(ctx, kinds["plain2"], 100)
    assert cid == PLAIN2
    p = lambda q: pods[at[q]]                                   # noqa: E731
    (c0, m0), (c1, m1) = p(0)["xc"]
    ch(at[0], VALUE, xc=[(c0 + 1, m0), (c1 - 1, m1)])           # the split, the same total: a plain class keeps it
    ch(at[1], VALUE, xc=[p(1)["xc"][0], (200, (2 << 20) + 1)])
    ch(at[2], CLASS, f=PL.flags(4, reg=1), xc=[p(2)["xc"][0]])
    ch(at[99], VALUE, cpu0=(1 << 20) - 1)
    # --- plain, one init record
    cid, at = pos_map(ctx, kinds["init"], 60)
    assert cid == PLAIN_INIT
    p = lambda q: pods[at[q]]                                   # noqa: E731
    ch(at[0], VALUE, xc=[(I64_MIN, 1 << 20)])                   # the key absent
    ch(at[1], VALUE, xc=[(p(1)["xc"][0][0] + 1, 1 << 20)])
    ch(at[59], VALUE, mem0=(1 << 20) + 1)
    # --- the inert class
    cid, at = pos_map(ctx, kinds["inert"], 60)
    assert cid == INERT
    p = lambda q: pods[at[q]]                                   # noqa: E731
    ch(at[0], CLASS, f=own(p(0), 0))                            # daemonset off
    ch(at[1], VALUE, cpu0=p(1)["cpu0"] + 1)
    ch(at[2], 0, pair0=3)                                       # a daemonset pod is stored without pairs
    return off, want


def test_one_change_per_kind(esc):
    ctx, pods, kinds, n_gp, _ = load(esc)
    off, want = case_two(ctx, pods, kinds)
    ids = list(range(len(pods)))
    st, rep = verify(ctx, ids, off)
    res, where = where_of(ctx, pods, n_gp)
    lit = PL.expect(res, off, n_gp, where)
    assert np.array_equal(st, lit), [(i, int(st[i]), int(lit[i])) for i in np.flatnonzero(st != lit)[:10]]
    for i, code in want.items():
        assert st[i] == code, (i, int(st[i]), code)
    assert set(np.flatnonzero(st).tolist()) == {i for i, c in want.items() if c}           # their neighbours stay 0
    assert rep["first_bad"] == min(i for i, c in want.items() if c)
    # an invalid batch is refused with nothing reported
    with pytest.raises(esc._lib.EscError) as e:
        ctx.pods_verify([3, 3], PL.soa([pods[3], pods[3]]))
    assert e.value.code == -1
    with pytest.raises(esc._lib.EscError) as e:
        ctx.pods_verify([1 << 31], PL.soa([pods[3]]))
    assert e.value.code == -1
    with pytest.raises(esc._lib.EscError) as e:
        ctx.pods_verify([4], PL.soa([dict(pods[kinds["c"]], xp=[1, 3, 2, 4, 7])]))            # pairs not ascending
    assert e.value.code == -1
    st0, rep0 = ctx.pods_verify([], PL.soa([]))
    assert len(st0) == 0 and rep0 == {"n_checked": 0, "n_absent": 0, "n_class": 0, "n_value": 0, "n_bind": 0, "first_bad": -1}
    ctx.close()


# ------------------------------------------------------------------ 3. the C section
def test_c_section(esc):
    ctx, pods, kinds, n_gp, _ = load(esc)
    c0 = kinds["c"]
    assert all(ctx.pod_where(i)[0] == -1 for i in range(c0, c0 + 40))
    # pods parked in spare slots: the 12-byte class has 6 free positions
    ids_new = list(range(len(pods), len(pods) + 10))
    new = [pod(30000 + i, 1 << 21, i % 5, 4, xp=[]) for i in range(10)]
    assert ctx.pods_upsert(ids_new, PL.soa(new)) == 0
    pods = pods + new
    parked = [i for i in ids_new if ctx.pod_where(i)[0] == -1]
    assert len(parked) == 4
    off = copy.deepcopy(pods)
    want = {}

    def ch(i, code, **kw):
        off[i] = dict(off[i], **kw)
        want[i] = code
    r = pods[c0]["xc"]
    ch(c0 + 0, VALUE, xc=[r[0], (r[1][0] + 1, r[1][1])] + r[2:])               # a regular record
    ch(c0 + 1, VALUE, xc=pods[c0 + 1]["xc"][:3] + [(500, (1 << 12) + 1)] + pods[c0 + 1]["xc"][4:])     # the init record
    ch(c0 + 2, VALUE, xc=pods[c0 + 2]["xc"][:4] + [(6, 1 << 8)])               # the overhead
    ch(c0 + 3, VALUE, xp=[1, 2, 3, 4, 8])                                      # the fifth pair
    ch(c0 + 4, VALUE, xp=[1, 2, 3, 5, 7])                                      # a pair past the third
    ch(c0 + 5, CLASS, f=PL.flags(4, reg=4, init=1, ovh=1, pairs=5), xc=pods[c0 + 5]["xc"][:3] + [(1, 1)] + pods[c0 + 5]["xc"][3:])
    ch(c0 + 6, VALUE, f=PL.flags(4, reg=2, init=1, ovh=1, pairs=5), xc=pods[c0 + 6]["xc"][:2] + pods[c0 + 6]["xc"][3:])
    ch(c0 + 7, VALUE, xc=pods[c0 + 7]["xc"][:3] + [(I64_MIN, 1 << 12)] + pods[c0 + 7]["xc"][4:])       # the init key absent
    a, b, c, d = parked
    ch(a, 0)                                                                    # its words and the neutral remainder
    ch(b, VALUE, cpu0=pods[b]["cpu0"] + 1)
    ch(c, CLASS, f=PL.flags(4, reg=5), xc=[(1, 1)] * 5)                         # more records than a spare slot's room
    ch(d, VALUE, f=PL.flags(4, reg=1), cpu0=pods[d]["cpu0"] - 10, xc=[(10, 0)])  # a C slot keeps the split
    ids = list(range(len(pods)))
    st, rep = verify(ctx, ids, off)
    res, where = where_of(ctx, pods, n_gp)
    lit = PL.expect(res, off, n_gp, where)
    assert np.array_equal(st, lit), [(i, int(st[i]), int(lit[i])) for i in np.flatnonzero(st != lit)[:10]]
    for i, code in want.items():
        assert st[i] == code, (i, int(st[i]), code)
    assert set(np.flatnonzero(st).tolist()) == {i for i, c in want.items() if c}
    # a smaller pod upserted over a bigger one in a parked slot (their class is full: the slot is
    # kept): the remainder it leaves is neutral, and compared
    big = pod(31000, 1 << 21, 1, 4, reg=[(5, 5), (6, 6)])
    small = pod(31000, 1 << 21, 1, 4, reg=[(5, 5)])
    for x in (big, small):
        assert ctx.pods_upsert([b], PL.soa([x])) == 0 and ctx.pod_where(b)[0] == -1
    st2, _ = verify(ctx, [b, a], [small, pods[a]])
    assert st2.tolist() == [0, 0]
    st3, _ = verify(ctx, [b], [big])
    assert st3.tolist() == [VALUE]
    st4, _ = verify(ctx, [b], [dict(small, xc=[(5, 6)])])
    assert st4.tolist() == [VALUE]
    ctx.close()


# ------------------------------------------------------------------ 4. absent and bind
def test_absent_bind_and_live_ids(esc):
    ctx, pods, kinds, n_gp, pod_node = load(esc, placed=True)
    n = len(pods)
    assert_all_clean(ctx, pods, "placed", pod_node)
    ctx.pods_delete([5, 7])
    assert ctx.pods_upsert([n + 90], PL.soa([pods[0]])) == 0                    # the map now reaches n + 90
    ids = [5, n + 50, n + 5000, 6, n + 90]
    st, _ = verify(ctx, ids, [pods[5], pods[0], pods[0], pods[6], pods[0]])
    assert st.tolist() == [ABSENT, ABSENT, ABSENT, 0, 0]                        # deleted, never loaded, past the map
    # bindings: a changed node is BIND alone; unbound is unbound however it is written
    ctx.nodes_delete([11])                                                      # (no pod was bound to it)
    bound = [i for i in range(20, 40) if pod_node[i] != NONE]
    free = [i for i in range(20, 40) if pod_node[i] == NONE]
    ids = bound[:3] + free[:3] + bound[3:5]
    offered = [pods[i] for i in ids]
    pn = pod_node[ids].copy()
    pn[0] = (pn[0] + 1) % 11                                                    # another node
    pn[1] = NONE                                                                # unbound in the store
    pn[2] = 11                                                                  # an absent slot: unbound
    pn[3] = 3                                                                   # bound in the store
    pn[4] = 11                                                                  # ESC_NONE <-> an absent node's index
    pn[5] = 10_000                                                              # ESC_NONE <-> outside the table
    st, rep = verify(ctx, ids, offered, pn)
    assert st.tolist() == [BIND, BIND, BIND, BIND, 0, 0, 0, 0] and rep["n_bind"] == 4
    offered[6] = dict(offered[6], cpu0=offered[6]["cpu0"] + 1)
    pn[6] = NONE
    st, _ = verify(ctx, ids, offered, pn)
    assert st[6] == VALUE | BIND                                                # or-ed
    st, _ = verify(ctx, [n + 50], [pods[0]], np.array([2], np.uint32))
    assert st.tolist() == [ABSENT | BIND]                                       # an absent pod is bound nowhere
    # the live ids after deletes and an id's reuse
    assert ctx.pods_upsert([5], PL.soa([pods[5]])) == 0
    assert ctx.pods_live_ids().tolist() == [i for i in range(n) if i != 7] + [n + 90]
    ctx.close()
    # bindings offered to a context without a placement
    ctx, pods, kinds, n_gp, pod_node = load(esc)
    with pytest.raises(esc._lib.EscError) as e:
        ctx.pods_verify([0], PL.soa([pods[0]]), pod_node[:1])
    assert e.value.code == E_STATE
    ctx.close()
    groups, _ = cluster()
    ctx = esc.Context(groups)
    for call in (lambda: ctx.pods_verify([0], PL.soa([pods[0]])), ctx.pods_live_ids):
        with pytest.raises(esc._lib.EscError) as e:
            call()
        assert e.value.code == E_STATE                                          # before esc_load_pods
    ctx.close()


# ------------------------------------------------------------------ 5. chunks
def test_one_call_over_several_staging_halves(esc):
    """70 000 pods of three records are 97 B each in the staging buffer: two 4 MiB halves."""
    groups, nodes = cluster()
    ctx = esc.Context(groups)
    ctx.set_spare(0.0)
    n = 70_000
    cpu0 = (1 << 20) + np.arange(n)
    P = {"flags": np.full(n, PL.flags(4, reg=3), np.uint32), "cpu0": cpu0.astype(np.uint32),
         "mem0": (1 << 20) + np.arange(n, dtype=np.int64), "pair0": (np.arange(n) % 5).astype(np.uint32),
         "xc_cpu": (np.arange(3 * n, dtype=np.int64) % 1000) + 1, "xc_mem": (np.arange(3 * n, dtype=np.int64) % 4096) + 1,
         "xp_pair": np.zeros(0, np.uint32)}
    ctx.load(P, ctx.pack([], nodes)[1])
    rng = np.random.RandomState(7)
    changed = np.unique(np.r_[0, n - 1, rng.choice(n, n // 100, replace=False)])
    Q = {k: v.copy() for k, v in P.items()}
    for j, i in enumerate(changed):
        if j % 3 == 0:
            Q["cpu0"][i] += 1
        elif j % 3 == 1:
            Q["xc_mem"][3 * i + 2] += 1
        else:
            Q["xc_cpu"][3 * i] -= 1
    # the literal over the changed pods and a sample of the others (a plain class keeps every word)
    def lit_pod(S, i):
        return {"f": int(S["flags"][i]), "cpu0": int(S["cpu0"][i]), "mem0": int(S["mem0"][i]), "pair0": int(S["pair0"][i]),
                "xc": [(int(S["xc_cpu"][3 * i + k]), int(S["xc_mem"][3 * i + k])) for k in range(3)], "xp": []}
    sample = np.unique(np.r_[changed, rng.choice(n, 500, replace=False)])
    lit = PL.expect([lit_pod(P, i) for i in sample], [lit_pod(Q, i) for i in sample], 6, [None] * len(sample))
    want = np.zeros(n, np.uint8)
    want[sample] = lit
    assert np.array_equal(np.flatnonzero(want), changed) and set(lit[np.isin(sample, changed)].tolist()) == {VALUE}
    st, rep = ctx.pods_verify(np.arange(n), Q)
    assert np.array_equal(st, want), np.flatnonzero(st != want)[:10]
    assert rep == {"n_checked": n, "n_absent": 0, "n_class": 0, "n_value": len(changed), "n_bind": 0, "first_bad": 0}
    st, rep = ctx.pods_verify(np.arange(n), P)
    assert not st.any() and rep["first_bad"] == -1
    ctx.close()


# ------------------------------------------------------------------ 6. read-only
def test_read_only(esc):
    ctx, pods, kinds, n_gp, pod_node = load(esc, replicas=2, placed=True)
    G = 6
    ctx.use_graph(True)
    ctx.set_order_in_step(True)
    ctx.set_selections(4)

    def snapshot():
        tot, dec = ctx.decide_all(None)
        sel = [np.asarray(x).tobytes() for x in ctx.selections()]
        rm = np.asarray(ctx.try_remove(1_700_000_000 * 10**9, [0] * G, [0] * G)).tobytes()
        return tot.tobytes(), dec.tobytes(), sel, ctx.stream_bytes(), ctx.audit(), ctx.audit_pods(), rm
    a = snapshot()
    off, want = case_two(ctx, pods, kinds)
    st, rep = verify(ctx, list(range(len(pods))), off, pod_node)
    assert rep["n_value"] > 0 and rep["n_class"] > 0 and rep["n_bind"] == 0
    sel_after = [np.asarray(x).tobytes() for x in ctx.selections()]               # the last decision's, still readable
    assert sel_after == a[2]
    b = snapshot()
    assert a == b
    assert all(v["n_bad"] == 0 for k, v in b[5].items() if k != "skipped")
    ctx.close()


# ------------------------------------------------------------------ 7. repair through the queue
def test_lost_events_are_repaired_by_a_resync(esc):
    """Three updates (two of a value, one into another class), a delete and a bind change reach the
    store and not the queue's dirty sets.  Before the resync the device's decision differs from the
    C oracle's over the store; the resync reports exactly those five; a second one reports
    nothing; then the decision equals the C oracle's (test_gpu_audit.assert_decision) and the
    selections and try_remove equal a context freshly loaded from the store."""
    from escalator_amd.events import EventQueue
    from escalator_amd.objects import placement
    groups, nodes = cluster()
    ctx = esc.Context(groups)
    ctx.set_order_in_step(True)
    ctx.set_selections(4)
    q = EventQueue(spare=0.5)
    for x in nodes:
        q.node_add(x)
    for i in range(300):
        q.pod_add(obj_pod("p%d" % i, POOLS[i % 5] if i % 6 else "", "n%d" % (i % N_NODES) if i % 3 else "", cpu=100 + i % 40))
    q.flush(ctx)
    assert q.resync(ctx) == {"checked": 300, "absent": 0, "class": 0, "value": 0, "bind": 0, "orphans": 0, "reloaded": False}
    # five events the queue never hears of: the store changes, the dirty sets do not
    q.pod_update(dict(q.pods["p10"], containers=[{"cpu": 777, "mem": 1 << 20}]))
    q.pod_update(dict(q.pods["p11"], containers=[{"cpu": 150, "mem": 2 << 20}]))
    q.pod_update(dict(q.pods["p12"], containers=[{"cpu": 40000, "mem": 1 << 20}]))          # another class
    q.pod_delete("p13")
    q.pod_update(dict(q.pods["p14"], node_name="n5" if q.pods["p14"]["node_name"] != "n5" else "n6"))
    q._dirty_pods.clear()
    gone = q.pod_id("p13")

    def decision_matches():
        live_n = q.live_nodes()
        store = [q.pods[k] for k in q.pods]
        P, N = ctx.pack(store, live_n)
        assert_decision(ctx, None, P, N, groups)
        return store, live_n
    with pytest.raises(AssertionError):
        decision_matches()                                                      # the device counts stale pods
    out = q.resync(ctx)
    assert out == {"checked": 299, "absent": 0, "class": 1, "value": 2, "bind": 1, "orphans": 1, "reloaded": False}
    assert q.resync_repairs == {"absent": 0, "class": 1, "value": 2, "bind": 1, "orphans": 1} and q.reloads == 1
    assert gone not in ctx.pods_live_ids().tolist()
    again = q.resync(ctx)
    assert again == {"checked": 299, "absent": 0, "class": 0, "value": 0, "bind": 0, "orphans": 0, "reloaded": False}
    store, live_n = decision_matches()
    # selections and reaping against a context loaded from the store
    fresh = esc.Context(groups)
    fresh.set_order_in_step(True)
    fresh.set_selections(4)
    order = sorted(q._pod_id, key=q._pod_id.get)
    P, N = fresh.pack([q.pods[k] for k in order], live_n)
    fresh.load(P, N)
    fresh.load_placement(*placement([q.pods[k] for k in order], live_n))
    for c in (ctx, fresh):
        c.decide_all(None)
    assert [np.asarray(x).tobytes() for x in ctx.selections()] == [np.asarray(x).tobytes() for x in fresh.selections()]
    now = 1_700_000_000 * 10**9
    assert np.asarray(ctx.try_remove(now, [0] * 6, [0] * 6)).tobytes() == np.asarray(fresh.try_remove(now, [0] * 6, [0] * 6)).tobytes()
    fresh.close()
    ctx.close()


# ------------------------------------------------------------------ 8. multi-device
def test_two_shards_answer_in_batch_order(esc):
    one, pods, kinds, n_gp, pod_node = load(esc, placed=True)
    off, want = case_two(one, pods, kinds)
    n = len(pods)
    order = np.ravel(np.column_stack([np.arange(n // 2), np.arange(n // 2, n)]))   # interleaved over the two shards
    assert sorted(order.tolist()) == list(range(n))
    batch = [off[i] for i in order]
    st1, rep1 = verify(one, order, batch, pod_node[order])
    one.close()
    two, _, _, _, _ = load(esc, devices=[0, 0], placed=True)
    st2, rep2 = verify(two, order, batch, pod_node[order])
    assert np.array_equal(st1, st2) and rep1 == rep2
    for i, code in want.items():
        assert st2[np.flatnonzero(order == i)[0]] == code
    assert np.array_equal(two.pods_live_ids(), np.arange(n))
    two.pods_delete([3, n - 1])
    assert two.pods_live_ids().tolist() == [i for i in range(n) if i not in (3, n - 1)]
    st, _ = verify(two, [3, 4, n - 1], [pods[3], pods[4], pods[n - 1]])
    assert st.tolist() == [ABSENT, 0, ABSENT]
    two.close()
