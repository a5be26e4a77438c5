"""GPU: esc_nodes_facts — the per-node reaping facts (escalator-taint time, no-delete flag) of
a handful of nodes patched in place — against the literal oracle and, byte for byte, against
a context that got the same state through the whole-table refresh
(esc_load_placement with pod_node NULL)."""
import random

import numpy as np
import pytest

from oracle import oracle as O
from randobj import make_nodes, make_reaping_cluster, make_trackers

pytestmark = pytest.mark.gpu

NO_DELETE = "atlassian.com/no-delete"
TAINT = "atlassian.com/escalator"
I64_MIN = -(1 << 63)


@pytest.fixture(scope="module")
def esc():
    import escalator_amd
    return escalator_amd


def _table_facts(live, hw):
    from escalator_amd.objects import taint_time
    ts = np.full(hw, I64_MIN, np.int64)
    nd = np.zeros(hw, np.uint8)
    for j, x in live.items():
        ts[j] = taint_time(x)
        nd[j] = 1 if (x.get("annotations") or {}).get(NO_DELETE, "") else 0
    return ts, nd


def _build(esc, groups, pods, nodes, trackers, new, devices=None):
    """A context with `nodes` loaded and placed, `new` appended in place (no facts yet)."""
    from escalator_amd.objects import placement
    ctx = esc.Context(groups, devices=devices) if devices else esc.Context(groups)
    ctx.set_spare(2.0)
    P, N = ctx.pack(pods, nodes, trackers)
    ctx.load(P, N)
    ctx.load_placement(*placement(pods, nodes))
    _, packed = ctx.pack([], new)
    ids = [int(j) for j in ctx.nodes_add(packed)]
    assert ids == list(range(len(nodes), len(nodes) + len(new)))
    return ctx


def _removal(ctx, G, now_ns, soft, hard):
    res = ctx.try_remove(now_ns, soft, hard)
    return res.tobytes(), [list(ctx.removal_nodes(g)) for g in range(G)], res


def _check_literal(res, lists, groups, pods, live, trackers, now_ns, soft, hard, tag):
    idx = sorted(live)
    lst = [live[j] for j in idx]
    for g, grp in enumerate(groups):
        L = O.scale_node_group(grp, {}, pods, lst, tracker=trackers.get(g, []))
        pods_g = O.filtered_list(pods, O.group_pod_filter(grp))
        all_nodes = [x for x in lst if O.new_node_label_filter_func(grp.get("label_key", ""),
                                                                    grp.get("label_value", ""))(x)]
        tainted = L["tainted"]
        neg, remaining, ks = O.try_remove_tainted_nodes(grp, [lst[i] for i in tainted], pods_g, all_nodes, now_ns,
                                                        int(soft[g]), int(hard[g]), bool(grp.get("dry_mode")))
        r = res[g]
        assert int(r["n_candidates"]) == len(tainted), (tag, g)
        assert (-int(r["n_delete"]), int(r["pods_remaining"])) == (neg, remaining), (tag, g)
        assert lists[g] == [idx[tainted[k]] for k in ks], (tag, g)


def _scenario(seed, n_nodes=None):
    rng = random.Random(4200 + seed)
    G = rng.choice([3, 6, 12])
    groups, pods, nodes, now_ns = make_reaping_cluster(rng, G, rng.choice([300, 500]),
                                                       n_nodes or rng.choice([40, 90, 120]))
    trackers = make_trackers(rng, groups, nodes)
    new = make_nodes(rng, 7, groups, big_frac=0.0)
    for k, x in enumerate(new):
        x["name"] = "late-%d" % k
        x["taints"] = [TAINT]                     # tainted (the packed flag) with no taint time yet
    soft = np.array([rng.choice([0, 60, 300]) * 10**9 for _ in range(G)], np.int64)
    hard = soft + np.array([rng.choice([0, 600]) * 10**9 for _ in range(G)], np.int64)
    return rng, groups, pods, nodes, now_ns, trackers, new, soft, hard


def _batches(rng, live, n_loaded, hw, now_s, big):
    """Three rounds of fact changes as (ids, new records): slots 0 and N - 1, two adjacent
    slots, the nodes just added, a random rest; sizes that are no multiple of the 256-thread
    launch block (with `big`, more than one block)."""
    out = []
    for rnd in range(3):
        ids = {0, n_loaded - 1, hw - 1}
        a = rng.randrange(1, n_loaded - 2)
        ids |= {a, a + 1}
        if rnd == 0:
            ids |= set(range(n_loaded, hw))
        want = (300 if big else rng.choice([9, 17, 33])) + rnd
        rest = [j for j in range(hw) if j not in ids]
        ids |= set(rng.sample(rest, min(len(rest), max(0, want - len(ids)))))
        ids = sorted(ids)
        rng.shuffle(ids)
        recs = []
        for j in ids:
            x = dict(live[j])
            x["taint_value"] = rng.choice([str(now_s - rng.randrange(0, 900)), str(now_s - 5000), "bad", None,
                                           "+%d" % (now_s - 400)])
            x["annotations"] = rng.choice([{}, {}, {NO_DELETE: "true"}, {NO_DELETE: ""}])
            recs.append(x)
        assert len(ids) % 256 != 0
        out.append((ids, recs))
    return out


@pytest.mark.parametrize("seed, n_nodes", [(0, None), (1, None), (2, None), (3, None), (4, 700)])
def test_nodes_facts_vs_literal_and_full_refresh(esc, seed, n_nodes):
    """After every batch, TryRemoveTaintedNodes for every group equals the literal oracle on
    the live lists and equals, byte for byte, a second context refreshed over its whole table."""
    from escalator_amd.objects import taint_time
    rng, groups, pods, nodes, now_ns, trackers, new, soft, hard = _scenario(seed, n_nodes)
    G = len(groups)
    ctx = _build(esc, groups, pods, nodes, trackers, new)
    ref = _build(esc, groups, pods, nodes, trackers, new)
    live = dict(enumerate(nodes + new))
    hw = len(live)
    # the added nodes carry the taint flag but no time: nothing of theirs is deleted yet
    got = _removal(ctx, G, now_ns, soft, hard)
    assert all(j < len(nodes) for lst in got[1] for j in lst)
    changed = False
    for rnd, (ids, recs) in enumerate(_batches(rng, live, len(nodes), hw, now_ns // 10**9, n_nodes is not None)):
        for j, x in zip(ids, recs):
            live[j] = x
        ctx.nodes_facts(ids, [taint_time(x) for x in recs],
                        [1 if x["annotations"].get(NO_DELETE, "") else 0 for x in recs])
        ref.load_placement(None, *_table_facts(live, hw))
        last, got, want = got, _removal(ctx, G, now_ns, soft, hard), _removal(ref, G, now_ns, soft, hard)
        assert got[0] == want[0] and got[1] == want[1], rnd
        _check_literal(got[2], got[1], groups, pods, live, trackers, now_ns, soft, hard, rnd)
        changed |= got[1] != last[1]
    assert changed                                        # the facts took effect: some result moved


def test_nodes_facts_errors_apply_nothing(esc):
    from escalator_amd._lib import ESC_E_INVAL, ESC_E_STATE, EscError
    rng, groups, pods, nodes, now_ns, trackers, new, soft, hard = _scenario(11)
    G = len(groups)
    bare = esc.Context(groups)
    P, N = bare.pack(pods, nodes, trackers)
    bare.load(P, N)
    with pytest.raises(EscError) as e:                  # before any placement
        bare.nodes_facts([0], [5], [0])
    assert e.value.code == ESC_E_STATE
    ctx = _build(esc, groups, pods, nodes, trackers, new)
    hw = len(nodes) + len(new)
    ctx.nodes_delete([3])
    before = _removal(ctx, G, now_ns, soft, hard)
    old = now_ns // 10**9 - 5000
    late = list(range(len(nodes), hw))                  # tainted, no time yet: a time makes them reapable
    for bad in ([hw], [-1], [3], [late[0]], [hw + 1000]):               # out of range, absent, duplicate
        ids = late + bad
        with pytest.raises(EscError) as e:
            ctx.nodes_facts(ids, [old] * len(ids), [0] * len(ids))
        assert e.value.code == ESC_E_INVAL, ids
        got = _removal(ctx, G, now_ns, soft, hard)
        assert got[0] == before[0] and got[1] == before[1], ids
    import ctypes as C
    one = (C.c_int64 * 1)(1)
    assert ctx.lib.esc_nodes_facts(ctx.handle, None, 1, one, (C.c_uint8 * 1)(0)) == ESC_E_INVAL
    assert ctx.lib.esc_nodes_facts(ctx.handle, one, 1, None, (C.c_uint8 * 1)(0)) == ESC_E_INVAL
    assert ctx.lib.esc_nodes_facts(ctx.handle, one, 1, one, None) == ESC_E_INVAL
    assert ctx.lib.esc_nodes_facts(ctx.handle, None, 0, None, None) == 0           # n == 0
    ctx.nodes_facts([], [], [])
    got = _removal(ctx, G, now_ns, soft, hard)
    assert got[0] == before[0] and got[1] == before[1]
    # the same values in a valid batch: a result is no longer current after the call, and the
    # new one differs (so a refused batch that had written anything would have shown above)
    ctx.nodes_facts(late, [old] * len(late), [0] * len(late))
    with pytest.raises(EscError) as e:
        ctx.removal_nodes(0)
    assert e.value.code == ESC_E_STATE
    got = _removal(ctx, G, now_ns, soft, hard)
    assert got[1] != before[1] and any(j in late for lst in got[1] for j in lst)


def test_nodes_facts_multi_device_equals_single(esc):
    """The same batches through a multi-device context (two shards on device 0): every
    device's table gets them, the result is the single context's."""
    from escalator_amd.objects import taint_time
    rng, groups, pods, nodes, now_ns, trackers, new, soft, hard = _scenario(21)
    G = len(groups)
    one = _build(esc, groups, pods, nodes, trackers, new)
    multi = _build(esc, groups, pods, nodes, trackers, new, devices=[0, 0])
    live = dict(enumerate(nodes + new))
    for rnd, (ids, recs) in enumerate(_batches(rng, live, len(nodes), len(live), now_ns // 10**9, False)):
        for j, x in zip(ids, recs):
            live[j] = x
        args = (ids, [taint_time(x) for x in recs], [1 if x["annotations"].get(NO_DELETE, "") else 0 for x in recs])
        one.nodes_facts(*args)
        multi.nodes_facts(*args)
        got, want = _removal(multi, G, now_ns, soft, hard), _removal(one, G, now_ns, soft, hard)
        assert got[0] == want[0] and got[1] == want[1], rnd
        _check_literal(got[2], got[1], groups, pods, live, trackers, now_ns, soft, hard, rnd)
