"""GPU: esc_nodes_verify — the resident node table compared with a batch of nodes as the caller
holds them — esc_nodes_live_ids, EventQueue.resync_nodes and ResidentController(node_resync_every).

Every expected status comes from tests/node_verify_literal.py: its Mirror is told of every load and
node event the test makes and restates the compare rule in Python without calling the library.  The
cluster is tests/node_verify_child.py's: 40 groups over 3 label keys, 600 nodes carrying 0 to 2 extra
label pairs (some with no label of a group's key at all), 400 pods, spare 0.5, a placement."""
import copy
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import node_verify_literal as NL
from node_verify_child import KEYS, N_GROUPS, N_NODES, T0, TAINT, cluster, node
from node_verify_literal import ABSENT, FACTS, INST, SHAPE, STATUS
from oracle import soa
from test_gpu_audit import assert_decision

pytestmark = pytest.mark.gpu
soa.build()

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
MEASURE = os.path.join(ROOT, "escalator_amd", "libescalator_hip_measure.so")
E_INVAL, E_LIMIT, E_STATE = -1, -4, -5
I64_MIN = -(1 << 63)
NOW = T0 + 10**12
POS = [0, 63, 64, 255, 256, N_NODES - 1]          # a wave's and a block's first and last lane, the batch's ends


@pytest.fixture(scope="module")
def esc():
    import escalator_amd
    L = escalator_amd._lib
    assert (L.ESC_E_INVAL, L.ESC_E_LIMIT, L.ESC_E_STATE) == (E_INVAL, E_LIMIT, E_STATE)
    assert (L.NV_ABSENT, L.NV_SHAPE, L.NV_STATUS, L.NV_FACTS, L.NV_INST) == (ABSENT, SHAPE, STATUS, FACTS, INST)
    return escalator_amd


class Dev:
    """A context, the store (slot -> node object, the instantiation times by slot) and the
    literal's mirror of what the device was sent.  The send_* methods reach the device and the
    mirror; store=True also makes the change the store's."""

    def __init__(self, esc, devices=None, placed=True, graph=False):
        from escalator_amd.objects import placement
        self.esc = esc
        self.groups, nodes, self.pods = cluster()
        self.ctx = esc.Context(self.groups, **({"devices": devices} if devices else {}))
        self.ctx.set_spare(0.5)
        if graph:
            self.ctx.use_graph(True)
            self.ctx.set_order_in_step(True)
            self.ctx.set_selections(4)
        P, N = self.ctx.pack(self.pods, nodes)
        self.ctx.load(P, N)
        self.m = NL.Mirror()
        self.m.load(N)
        self.store = dict(enumerate(nodes))
        self.inst = {}
        if placed:
            pn, t, d = placement(self.pods, nodes)
            self.ctx.load_placement(pn, t, d)
            self.m.placement(t, d)

    def pack(self, objs):
        return self.ctx.pack([], objs)[1]

    def facts_of(self, objs):
        from escalator_amd.events import _facts
        f = [_facts(x) for x in objs]
        return np.array([t for t, _ in f], np.int64), np.array([d for _, d in f], np.uint8)

    def verify(self, ids=None, objs=None, facts=True, inst=True):
        """The store's nodes `ids` (all the live ones, ascending) — or `objs` in their place —
        verified; the statuses and the report are the literal's."""
        ids = sorted(self.store) if ids is None else [int(j) for j in ids]
        objs = [self.store[j] for j in ids] if objs is None else objs
        N = self.pack(objs)
        t, d = self.facts_of(objs) if facts else (None, None)
        s = np.array([self.inst.get(j, I64_MIN) for j in ids], np.int64) if inst else None
        st, rep = self.ctx.nodes_verify(ids, N, t, d, s)
        lit = self.m.expect(ids, N, t, d, s)
        print("verify", len(ids), rep)
        assert np.array_equal(st, lit), [(ids[i], int(st[i]), int(lit[i])) for i in np.flatnonzero(st != lit)[:10]]
        assert rep == NL.report(st), (rep, NL.report(st))
        return st, rep

    def clean(self, tag):
        st, rep = self.verify()
        assert not st.any() and rep["first_bad"] == -1 and rep["n_checked"] == len(self.store), (tag, rep)
        assert self.ctx.nodes_live_ids().tolist() == self.m.live_ids() == sorted(self.store), tag

    # ---- the event calls, to the device and the mirror (and the store)
    def send_add(self, objs):
        N = self.pack(objs)
        ids = [int(j) for j in self.ctx.nodes_add(N)]
        assert ids == self.m.add(N)
        self.store.update(zip(ids, objs))
        return ids

    def send_delete(self, ids, store=True):
        self.ctx.nodes_delete(ids)
        self.m.delete(ids)
        for j in ids:
            self.inst.pop(j, None)
            if store:
                del self.store[j]

    def send_relabel(self, ids, objs, store=False):
        N = self.pack(objs)
        self.ctx.nodes_relabel(ids, N)
        self.m.relabel(ids, N)
        if store:
            self.store.update(zip(ids, objs))

    def send_update(self, ids, objs, store=False):
        N = self.pack(objs)
        self.ctx.nodes_update(ids, N["flags"], N["cpu"], N["mem"])
        self.m.update(ids, N["flags"], N["cpu"], N["mem"])
        if store:
            self.store.update(zip(ids, objs))

    def send_facts(self, ids, objs, store=False):
        t, d = self.facts_of(objs)
        self.ctx.nodes_facts(ids, t, d)
        self.m.facts(ids, t, d)
        if store:
            self.store.update(zip(ids, objs))

    def send_inst(self, ids, times, store=False):
        self.ctx.nodes_instantiated(ids, times)
        self.m.instantiated(ids, times)
        if store:
            self.inst.update(zip(ids, times))


# the changes of one kind, by turn: each leaves every other kind's fields as they are
def other_value(x, key):
    v = (x["labels"].get(key) or "v0")
    return "v%d" % ((int(v[1:]) + 1) % 13)


def shape_change(x, turn):
    y = copy.deepcopy(x)
    have = [k for k in KEYS if k in y["labels"]]
    if turn % 3 == 0 and have:                                  # a label's value (label0 or an extra pair)
        k = have[(turn // 3) % len(have)]
        y["labels"][k] = other_value(y, k)
    elif turn % 3 == 1 or not have:                             # the label count, up where it can go up
        if len(have) < 3:
            y["labels"][[k for k in KEYS if k not in have][0]] = "v1"
        else:
            del y["labels"][have[-1]]
    else:
        y["created_ns"] += 1
    return y


def status_change(x, turn):
    y = copy.deepcopy(x)
    if turn % 4 == 0:
        y["unschedulable"] = not y["unschedulable"]
    elif turn % 4 == 1:                                         # the taint's presence (its time stays a fact)
        y["taints"] = [] if TAINT in y["taints"] else [TAINT]
    elif turn % 4 == 2:
        y["cpu"] += 1
    else:
        y["mem"] -= 1
    return y


def facts_change(x, turn):
    y = copy.deepcopy(x)
    if turn % 2 == 0:                                           # the taint's time, present or not
        tainted = TAINT in y["taints"] and "taint_value" in y
        y["taints"], y["taint_value"] = [TAINT], str(int(y["taint_value"]) + 1) if tainted else "12345"
    else:
        y["annotations"] = {} if y["annotations"] else {"atlassian.com/no-delete": "x"}
    return y


# ------------------------------------------------------------------ 1. clean
def test_clean_after_load_every_event_rebuild_and_compact(esc):
    d = Dev(esc)
    d.clean("load")
    ids = sorted(d.store)
    # a round of every node event, each the store's too
    new = d.send_add([node(1000 + i, "new%d" % i) for i in range(20)])
    d.send_facts(new, [d.store[j] for j in new], store=True)
    d.send_delete(ids[5:15])
    rel = ids[20:35]
    d.send_relabel(rel, [shape_change(d.store[j], t) for t, j in enumerate(rel)], store=True)
    upd = ids[40:55]
    objs = [status_change(d.store[j], t) for t, j in enumerate(upd)]      # (a taint that goes takes its time along)
    d.send_update(upd, objs, store=True)
    d.send_facts(upd, objs, store=True)
    fct = ids[60:75]
    objs = [facts_change(d.store[j], t) for t, j in enumerate(fct)]        # (a new taint is a status change too)
    d.send_update(fct, objs, store=True)
    d.send_facts(fct, objs, store=True)
    ins = ids[80:110] + new[:5]
    d.send_inst(ins, [T0 - 90 * 10**9 - j for j in ins], store=True)
    d.clean("events")
    d.ctx.nodes_rebuild()
    d.clean("rebuild")
    new_index = d.ctx.nodes_compact()
    d.m.compact(new_index)
    d.store = {int(new_index[j]): x for j, x in d.store.items()}
    d.inst = {int(new_index[j]): t for j, t in d.inst.items()}
    assert sorted(d.store) == list(range(len(d.store)))
    d.clean("compact")
    assert all(v["n_bad"] == 0 for k, v in d.ctx.audit().items() if k != "skipped")
    d.ctx.close()


# ------------------------------------------------------------------ 2. one change per kind
def test_one_change_per_kind_at_the_lane_edges(esc):
    d = Dev(esc)
    ids = sorted(d.store)
    assert ids == list(range(N_NODES))
    at = [ids[p] for p in POS]
    cases = ((SHAPE, shape_change, d.send_relabel), (STATUS, status_change, d.send_update), (FACTS, facts_change, d.send_facts))
    for bit, change, send in cases:
        for shift in (0, 1, 2):                                 # every turn of the change reaches every position
            orig = [d.store[j] for j in at]
            send(at, [change(x, t + shift) for t, x in enumerate(orig)])      # the device alone
            st, rep = d.verify()
            assert np.flatnonzero(st).tolist() == POS and set(st[POS].tolist()) == {bit}, (bit, shift, st[POS])
            assert rep["first_bad"] == 0 and rep[{SHAPE: "n_shape", STATUS: "n_status", FACTS: "n_facts"}[bit]] == len(POS)
            send(at, orig)                                      # the event arrives after all
            d.clean((bit, shift))
    d.send_inst(at, [T0 - 1 - p for p in POS])
    st, rep = d.verify()
    assert np.flatnonzero(st).tolist() == POS and set(st[POS].tolist()) == {INST} and rep["n_inst"] == len(POS)
    d.send_inst(at[:3], [I64_MIN] * 3)
    st, rep = d.verify()
    assert np.flatnonzero(st).tolist() == POS[3:] and rep["first_bad"] == POS[3]
    d.send_inst(at[3:], [I64_MIN] * 3)
    d.clean("inst")
    # several kinds on one node are or-ed; SHAPE | STATUS is one node in both counts
    a, b, c = 100, 101, 599
    d.send_relabel([a], [status_change(shape_change(d.store[a], 0), 2)])
    d.send_facts([a, b], [facts_change(d.store[a], 0), facts_change(d.store[b], 1)])
    d.send_inst([a, c], [5, 6])
    d.send_update([c], [status_change(d.store[c], 0)])
    st, rep = d.verify()
    assert {int(i): int(st[i]) for i in np.flatnonzero(st)} == {a: SHAPE | STATUS | FACTS | INST, b: FACTS, c: STATUS | INST}
    assert (rep["n_shape"], rep["n_status"], rep["n_facts"], rep["n_inst"], rep["first_bad"]) == (1, 2, 2, 2, a)
    # the same batch backwards: the statuses follow the batch, first_bad is a batch index
    st, rep = d.verify(ids[::-1])
    assert np.flatnonzero(st).tolist() == [0, N_NODES - 1 - b, N_NODES - 1 - a] and rep["first_bad"] == 0
    d.ctx.close()


# ------------------------------------------------------------------ 3. ABSENT and the live ids
def test_absent_slots_batch_order_and_live_ids(esc):
    d = Dev(esc)
    lib, h = d.ctx.lib, d.ctx.handle
    assert d.ctx.nodes_live_ids().tolist() == list(range(N_NODES))
    d.send_delete([5, 77, N_NODES - 1], store=False)            # the store still holds them
    free = d.ctx.nodes_room()[0]
    assert free >= 2                                            # the spare slots behind the loaded ones
    x = d.store[0]
    odd = {N_NODES: "a free spare slot", N_NODES + free - 1: "the last slot of the table", N_NODES + free: "the first id past it",
           10_000_000: "far past it", (1 << 31) - 2: "the largest id"}
    ids = [3, 5, 4] + list(odd) + [77, 78, N_NODES - 1, 0]
    objs = [d.store.get(j, x) for j in ids]
    st, rep = d.verify(ids, objs)
    assert st.tolist() == [0, ABSENT, 0] + [ABSENT] * 5 + [ABSENT, 0, ABSENT, 0]
    assert (rep["n_absent"], rep["first_bad"]) == (8, 1)
    # an absent slot is ABSENT alone, whatever else is offered for it
    st, _ = d.verify([5, 6], [shape_change(d.store[5], 0), shape_change(d.store[6], 0)])
    assert st.tolist() == [ABSENT, SHAPE]
    # the whole store in descending and in shuffled order: the statuses return in batch order
    gone = {5, 77, N_NODES - 1}
    for order in (sorted(d.store, reverse=True), np.random.RandomState(3).permutation(sorted(d.store)).tolist()):
        st, rep = d.verify(order)
        assert [order[i] for i in np.flatnonzero(st)] == [j for j in order if j in gone] and rep["n_absent"] == 3
    # the live ids: the sizing call, a short array, the full one
    live = [j for j in range(N_NODES) if j not in gone]
    n = C.c_int64(-1)
    assert lib.esc_nodes_live_ids(h, None, 0, C.byref(n)) == 0 and n.value == len(live)
    short = np.full(len(live) - 1, -7, np.int64)
    n.value = -1
    assert lib.esc_nodes_live_ids(h, short.ctypes.data_as(C.POINTER(C.c_int64)), len(short), C.byref(n)) == E_LIMIT
    assert n.value == len(live) and short.tolist() == live[:-1]
    assert d.ctx.nodes_live_ids().tolist() == live
    new = d.send_add([node(2000, "late")])
    assert new == [N_NODES] and d.ctx.nodes_live_ids().tolist() == live + [N_NODES]
    d.ctx.close()


# ------------------------------------------------------------------ 4. NULL facts and errors
def test_null_fact_arrays_and_refusals(esc):
    d = Dev(esc)
    L = esc._lib
    at = [10, 11, 12]
    d.send_facts(at, [facts_change(d.store[j], t) for t, j in enumerate(at)])
    d.send_inst(at, [7, 8, 9])
    st, rep = d.verify(facts=False, inst=False)                 # the device differs; nothing of it is compared
    assert not st.any()
    st, rep = d.verify(facts=False)
    assert np.flatnonzero(st).tolist() == at and set(st[at].tolist()) == {INST}
    st, rep = d.verify(inst=False)
    assert np.flatnonzero(st).tolist() == at and set(st[at].tolist()) == {FACTS}
    ids = np.array(at, np.int64)
    N = d.pack([d.store[j] for j in at])
    t, nd = d.facts_of([d.store[j] for j in at])
    st, _ = d.ctx.nodes_verify(ids, N, taint_s=t)               # the taint times alone: node 11's change is its no-delete flag
    assert st.tolist() == [FACTS, 0, FACTS]
    st, _ = d.ctx.nodes_verify(ids, N, no_delete=nd)
    assert st.tolist() == [0, FACTS, 0]
    # refusals: nothing is reported
    ns, keep = esc.context.node_soa(N)
    rep = L.NodesVerifyReport()
    rep.n_checked, rep.first_bad = 77, 78
    stat = np.full(3, 9, np.uint8)

    def raw(id_list, soa_=ns):
        a = np.array(id_list, np.int64)
        return d.ctx.lib.esc_nodes_verify(d.ctx.handle, a.ctypes.data_as(C.POINTER(C.c_int64)), C.byref(soa_), None, None, None,
                                          stat.ctypes.data_as(C.POINTER(C.c_uint8)), C.byref(rep))
    assert raw([10, 11, 10]) == E_INVAL                         # a repeated id
    assert raw([10, (1 << 31) - 5, (1 << 31) - 5]) == E_INVAL   # repeated past the table
    assert raw([10, 11, 1 << 31]) == E_INVAL and raw([10, -1, 12]) == E_INVAL
    short, keep2 = esc.context.node_soa(N)
    short.n_xl = max(0, ns.n_xl - 1)
    if ns.n_xl:
        assert raw(at, short) == E_INVAL                        # label counts past n_xl
    assert (rep.n_checked, rep.first_bad) == (77, 78) and stat.tolist() == [9, 9, 9]
    assert raw(at) == 0 and rep.n_checked == 3 and rep.reserved == 0 and stat.tolist() == [0, 0, 0]
    st0, rep0 = d.ctx.nodes_verify([], d.pack([]), [], [], [])
    assert len(st0) == 0 and rep0 == NL.report(st0)
    del keep, keep2
    d.ctx.close()
    # without a placement the facts cannot be compared; the rest can
    d = Dev(esc, placed=False)
    N = d.pack([d.store[j] for j in at])
    for kw in ({"taint_s": t}, {"no_delete": nd}, {"taint_s": t, "no_delete": nd, "inst_ns": [I64_MIN] * 3}):
        with pytest.raises(L.EscError) as e:
            d.ctx.nodes_verify(at, N, **kw)
        assert e.value.code == E_STATE
    st, rep = d.ctx.nodes_verify(at, N, inst_ns=[I64_MIN, 5, I64_MIN])
    assert st.tolist() == [0, INST, 0] and rep["n_inst"] == 1
    d.ctx.close()
    ctx = esc.Context(d.groups)
    for call in (lambda: ctx.nodes_verify(at, N), ctx.nodes_live_ids):
        with pytest.raises(L.EscError) as e:
            call()
        assert e.value.code == E_STATE                          # before esc_load_nodes
    ctx.close()


# ------------------------------------------------------------------ 5. chunks
def test_one_call_over_several_staging_halves(esc):
    """200 000 nodes of one extra label are 64 + 4 + 1 staged bytes each, 13.8 MB: four chunks of
    at most (4 MiB - 64) // 69 nodes through the two 4 MiB halves."""
    groups, _, pods = cluster()
    ctx = esc.Context(groups)
    ctx.set_spare(0.0)
    n = 200_000
    i = np.arange(n, dtype=np.int64)
    a = i % 13
    # pair ids are the groups' in order: (k0, v_a) is 3a, (k1, v_b) is 3b + 1; b >= a keeps the pairs ascending
    D = {"flags": np.full(n, 1 << 8, np.uint32) | (i % 5 == 0).astype(np.uint32), "label0": (3 * a).astype(np.uint32),
         "cpu": 4000 + i % 9, "mem": (8 << 30) + i, "created_ns": T0 + i, "xl_pair": (3 * (a + (i // 13) % (13 - a)) + 1).astype(np.uint32),
         "trk_node": np.zeros(0, np.int32), "trk_group": np.zeros(0, np.int32)}
    assert ctx.lib.esc_ctx_pair_id(ctx.handle, b"k0", b"v2") == 6 and ctx.lib.esc_ctx_pair_id(ctx.handle, b"k1", b"v12") == 37
    assert np.all(D["xl_pair"] > D["label0"]) and D["xl_pair"].max() <= 37
    P, _ = ctx.pack(pods[:8], [])
    ctx.load(P, D)
    m = ((4 << 20) - 64) // 69
    edges = sorted({c * m + k for c in range(4) for k in (-1, 0) if 0 <= c * m + k < n} | {n - 1, 1, 12345})
    assert len(edges) == 10 and edges[0] == 0
    Q = {k: v.copy() for k, v in D.items()}
    want = np.zeros(n, np.uint8)
    for turn, e in enumerate(edges):
        if turn % 4 == 0:
            Q["xl_pair"][e] = 38 + e % 100; want[e] = SHAPE      # the node's one label word
        elif turn % 4 == 1:
            Q["cpu"][e] += 1; want[e] = STATUS
        elif turn % 4 == 2:
            Q["created_ns"][e] -= 1; want[e] = SHAPE
        else:
            Q["flags"][e] ^= 2; Q["label0"][e] = 39; want[e] = SHAPE | STATUS
    # the literal, vectorised for this one shape of node: what was sent against what is offered
    lit = np.where((D["label0"] != Q["label0"]) | (D["xl_pair"] != Q["xl_pair"]) | (D["created_ns"] != Q["created_ns"]), SHAPE, 0) | \
        np.where(((D["flags"] ^ Q["flags"]) & 3 != 0) | (D["cpu"] != Q["cpu"]) | (D["mem"] != Q["mem"]), STATUS, 0)
    assert np.array_equal(lit, want)
    inst = np.full(n, I64_MIN, np.int64)
    st, rep = ctx.nodes_verify(i, Q, inst_ns=inst)
    assert np.array_equal(st, want), np.flatnonzero(st != want)[:10]
    assert rep == NL.report(want) and rep["first_bad"] == 0 and rep["n_checked"] == n
    st, rep = ctx.nodes_verify(i, D, inst_ns=inst)
    assert not st.any() and rep == NL.report(st)
    ctx.close()


# ------------------------------------------------------------------ 6. read-only
def test_read_only(esc):
    d = Dev(esc, graph=True)
    ctx, G = d.ctx, N_GROUPS
    ctx.k1_calibrate(2)
    soft, hard = [60 * 10**9] * G, [600 * 10**9] * G

    def results():
        sel = [np.asarray(x).tobytes() for x in ctx.selections()]
        rm = [ctx.removal_nodes(g).tolist() for g in range(G)]
        nn = [[a.tolist() for a in ctx.new_nodes_list(g)] for g in range(G)]
        return sel, rm, nn
    tot, dec = ctx.decide_all(None)                              # captured
    tot, dec = ctx.decide_all(None)                              # replayed
    removal = np.asarray(ctx.try_remove(NOW, soft, hard)).tobytes()
    assert any(ctx.removal_nodes(g).size for g in range(G))
    new = np.asarray(ctx.new_nodes([T0 + 300_000] * G)).tobytes()
    before = results()
    plan = (ctx.stream_bytes(), ctx.k1_flush_entries(), ctx.order_info())
    order = [ctx.group_order(g, w).tolist() for g in range(0, G, 7) for w in (0, 1)]
    # a verify with mismatches of every kind
    ids = sorted(d.store)
    objs = [d.store[j] for j in ids]
    objs[3], objs[200], objs[599] = shape_change(objs[3], 1), status_change(objs[200], 2), facts_change(objs[599], 1)
    st, rep = d.verify(ids + [N_NODES + 1], objs + [objs[0]])
    assert (rep["n_shape"], rep["n_status"], rep["n_facts"], rep["n_absent"]) == (1, 1, 1, 1)
    # everything the last decision, reaping and new-node pass left still answers, unchanged
    assert results() == before
    assert plan == (ctx.stream_bytes(), ctx.k1_flush_entries(), ctx.order_info())
    assert order == [ctx.group_order(g, w).tolist() for g in range(0, G, 7) for w in (0, 1)]
    tot2, dec2 = ctx.decide_all(None)                            # the captured step replays
    assert tot2.tobytes() == tot.tobytes() and dec2.tobytes() == dec.tobytes()
    assert np.asarray(ctx.try_remove(NOW, soft, hard)).tobytes() == removal
    assert np.asarray(ctx.new_nodes([T0 + 300_000] * G)).tobytes() == new
    assert results() == before
    audit = ctx.audit()
    assert audit["skipped"] == [] and all(v["n_bad"] == 0 for k, v in audit.items() if k != "skipped"), audit
    ctx.close()


# ------------------------------------------------------------------ 7. repair through the controller
def test_lost_node_events_are_repaired_by_the_controllers_resync(esc):
    """Five node events reach the device and not the queue: a taint, a cordon with another
    allocatable, a relabel, a taint time and a delete.  The scan's resync_nodes reports and repairs
    exactly those with no reload; the decision then equals the C oracle's over the store's objects
    and the reaping a context's freshly loaded from them; the next resync is clean."""
    from escalator_amd.controller import ResidentController
    from escalator_amd.objects import placement
    groups, nodes, pods = cluster()
    now = [NOW]
    c = ResidentController(groups, clock=lambda: now[0], actuator=None, node_resync_every=1)
    q, ctx = c.events, c.ctx
    for x in nodes:
        q.node_add(x)
    for p in pods:
        q.pod_add(p)
    c.run_once()
    zero = {"checked": N_NODES, "absent": 0, "shape": 0, "status": 0, "facts": 0, "inst": 0, "orphans": 0, "reloaded": False}
    assert c.last_node_resync == zero and c.node_resyncs == 1
    # behind the queue's back: the device changes, the store and the dirty sets do not
    j = {m: q.node_index("n%d" % m) for m in (1, 2, 4, 7, 8)}
    _, N = ctx.pack([], [status_change(nodes[1], 1), status_change(status_change(nodes[2], 0), 2)])
    ctx.nodes_update([j[1], j[2]], N["flags"], N["cpu"], N["mem"])
    ctx.nodes_relabel([j[4]], ctx.pack([], [shape_change(nodes[4], 0)])[1])
    ctx.nodes_facts([j[7]], [int(nodes[7]["taint_value"]) - 100_000], [0])
    ctx.nodes_delete([j[8]])
    assert not q._dirty_nodes and not q._dirty_pods

    def decision_matches():
        live_n = q.live_nodes()
        P, N = ctx.pack(list(q.pods.values()), live_n)
        assert_decision(ctx, None, P, N, groups, name_of=q.node_name, names=[x["name"] for x in live_n])
        return live_n
    with pytest.raises(AssertionError):
        decision_matches()                                       # the device decides on stale nodes
    reloads = q.reloads
    now[0] += 10**9
    c.run_once()
    assert c.last_node_resync == dict(zero, absent=1, shape=1, status=2, facts=1)
    assert q.node_resync_repairs == {"absent": 1, "shape": 1, "status": 2, "facts": 1, "inst": 0, "orphans": 0}
    assert q.reloads == reloads and q.node_index("n8") not in (None, j[8])
    live_n = decision_matches()
    # the reaping against a context loaded from the store (records are counts: no index in them)
    fresh = esc.Context(groups)
    order = sorted(q._pod_id, key=q._pod_id.get)
    P, N = fresh.pack([q.pods[k] for k in order], live_n)
    fresh.load(P, N)
    fresh.load_placement(*placement([q.pods[k] for k in order], live_n))
    G = len(groups)
    soft, hard = [g["soft_delete_grace_ns"] for g in groups], [g["hard_delete_grace_ns"] for g in groups]
    a, b = ctx.try_remove(now[0], soft, hard), fresh.try_remove(now[0], soft, hard)
    assert np.asarray(a).tobytes() == np.asarray(b).tobytes() and int(np.asarray(a)["n_delete"].sum()) > 0
    for g in range(G):
        assert [q.node_name(i) for i in ctx.removal_nodes(g)] == [live_n[i]["name"] for i in fresh.removal_nodes(g)], g
    fresh.close()
    assert all(v["n_bad"] == 0 for k, v in ctx.audit().items() if k != "skipped")
    now[0] += 10**9
    c.run_once()
    assert c.last_node_resync == zero and c.node_resyncs == 3 and q.reloads == reloads
    ctx.close()


# ------------------------------------------------------------------ 8. two shards
def test_two_shards_answer_in_batch_order(esc):
    one, two = Dev(esc), Dev(esc, devices=[0, 0])
    order = np.random.RandomState(11).permutation(N_NODES).tolist()
    objs = [one.store[j] for j in order]
    for k, p in enumerate((0, 63, 64, 300, 599)):
        objs[p] = (shape_change, status_change, facts_change)[k % 3](objs[p], k)
    for d in (one, two):
        d.send_delete([order[10]], store=False)
        d.send_inst([order[20]], [5])
    st1, rep1 = one.verify(order, objs)
    st2, rep2 = two.verify(order, objs)
    assert np.array_equal(st1, st2) and rep1 == rep2 and rep2["n_checked"] == N_NODES
    assert np.flatnonzero(st2).tolist() == [0, 10, 20, 63, 64, 300, 599]
    assert two.ctx.nodes_live_ids().tolist() == [j for j in range(N_NODES) if j != order[10]]
    one.ctx.close()
    two.ctx.close()


def test_a_change_on_one_shards_copy_alone_is_reported():
    assert os.path.exists(MEASURE), "build the measurement library: make -C escalator_amd/csrc ABLATIONS=1"
    env = dict(os.environ, ESC_LIB_PATH=MEASURE)
    try:
        r = subprocess.run([sys.executable, "-u", os.path.join(HERE, "node_verify_child.py")], capture_output=True, text=True,
                           timeout=240, env=env, cwd=ROOT)
    except subprocess.TimeoutExpired:
        pytest.exit("node_verify_child.py hung: nothing more is started on this GPU", 1)
    if r.returncode in (134, 139, -6, -11):                     # an abort or a fault: the session ends here
        pytest.exit("node_verify_child.py died (%d): %s" % (r.returncode, r.stderr[-2000:]), 1)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    out = json.loads(r.stdout.strip().splitlines()[-1])
    print(out)
    assert out["clean"] == 0 and out["clean_rep"]["first_bad"] == -1 and out["bad_shard"] == E_INVAL
    assert out["found"] == {"40": STATUS, "300": STATUS, "500": STATUS}
    # counted from the or-ed bytes: node 500 differs on both shards and counts once
    assert out["rep"] == {"n_checked": N_NODES, "n_absent": 0, "n_shape": 0, "n_status": 3, "n_facts": 0, "n_inst": 0,
                          "first_bad": 40}
