"""GPU: pods whose container records are folded into one request at load.

The hand-built pods of tests/fold_cases.py (every edge of the rule, one pod just inside and
one just outside) and about 300 random pods with out-of-range values, one case at a time
and all together: every group's totals and decisions equal the literal oracle and the C
oracle, and the library's stream bytes equal ``layout.pod_bytes``.  Run without and with
spare room, through the captured graph and sharded over two contexts; then one pod id taken
through every layout by upserts on a resident context with a placement loaded."""
import random

import numpy as np
import pytest

import fold_cases as FC
from oracle import oracle as O
from oracle import soa
from randobj import make_groups, make_nodes, make_pods, make_states

pytestmark = pytest.mark.gpu
soa.build()

TAINT = "atlassian.com/escalator"


@pytest.fixture(scope="module")
def esc():
    import escalator_amd
    return escalator_amd


def make_cluster(seed, G, default):
    """G groups, the last one selecting ("k", "v0") — the pair of every hand-built pod — with
    gates that let its decision through; 300 random pods; nodes, some in that group."""
    rng = random.Random(seed)
    groups = make_groups(rng, G, with_default=default)
    groups[-1].update(label_key="k", label_value="v0", min_nodes=0, max_nodes=1000, dry_mode=False)
    rand = make_pods(rng, 300, groups, big_frac=0.1)
    nodes = make_nodes(rng, 30, groups, big_frac=0.0)
    for j in range(3):
        nodes[j]["labels"] = {"k": "v0"}
        nodes[j]["unschedulable"], nodes[j]["taints"] = False, []
    return groups, rand, nodes, make_states(rng, G)


CLUSTERS = {(G, d): make_cluster(4100 + G, G, d) for G, d in ((3, True), (5, False), (8, True))}
CLUSTER_IDS = sorted(CLUSTERS)


def check(esc, tot, dec, groups, states, pods, nodes, P, N, tag=""):
    """Every group against the literal oracle (objects) and the C oracle (packed arrays)."""
    from test_gpu import _bits, check_against_c_oracle
    for g in range(len(groups)):
        L = O.scale_node_group(groups[g], states[g], pods, nodes)
        t, d = tot[g], dec[g]
        assert (t["n_pods"], t["n_nodes"], t["n_untainted"], t["n_tainted"], t["n_cordoned"]) == \
            (L["n_pods"], L["n_nodes"], L["n_untainted"], L["n_tainted"], L["n_cordoned"]), (tag, g)
        if L["pod_cpu_m"] is not None:
            assert (t["pod_cpu_m"], t["pod_mem_b"], t["node_cpu_m"], t["node_mem_b"]) == \
                (L["pod_cpu_m"], L["pod_mem_b"], L["node_cpu_m"], L["node_mem_b"]), (tag, g)
        assert esc._lib.BRANCHES[d["branch"]] == L["branch"], (tag, g, L)
        assert int(d["delta"]) == L["delta"] and int(d["n_to_taint"]) == L["n_to_taint"], (tag, g, L)
        assert _bits(d["cpu_pct"]) == _bits(L["cpu_pct"]) and _bits(d["mem_pct"]) == _bits(L["mem_pct"]), (tag, g)
        assert soa.STATUS_ERR[int(d["status"])] == L["err"], (tag, g, L)
    otot = soa.totals(P, N, groups)
    odf, odi = soa.decide(groups, states, otot)
    check_against_c_oracle(tot, dec, otot, odf, odi)


def n_gp_of(ctx):
    return ctx.lib.esc_ctx_num_group_pairs(ctx.handle)


@pytest.mark.parametrize("spare", [0.0, 1.0])
@pytest.mark.parametrize("key", CLUSTER_IDS[:2])
def test_each_case_alone(esc, key, spare):
    from escalator_amd import layout
    groups, _, nodes, states = CLUSTERS[key]
    ctx = esc.Context(groups)
    ctx.set_spare(spare)
    for name, pod, want, _ in FC.CASES:
        P, N = ctx.pack([pod], nodes)
        ctx.load(P, N)
        tot, dec = ctx.decide_all(states)
        check(esc, tot, dec, groups, states, [pod], nodes, P, N, name)
        assert tot["n_pods"][-1] == 1, name
        got = ctx.stream_bytes()[0]
        assert got == layout.pod_bytes(P, n_gp_of(ctx)) == FC.bytes_of({name}), (name, got)


@pytest.mark.parametrize("spare", [0.0, 1.0])
@pytest.mark.parametrize("key", CLUSTER_IDS)
def test_all_together(esc, key, spare):
    from escalator_amd import layout
    groups, rand, nodes, states = CLUSTERS[key]
    pods = FC.pods_of() + rand
    ctx = esc.Context(groups)
    ctx.set_spare(spare)
    P, N = ctx.pack(pods, nodes)
    ctx.load(P, N)
    for wide in (False, True):
        ctx.force_wide(wide)
        tot, dec = ctx.decide_all(states)
        check(esc, tot, dec, groups, states, pods, nodes, P, N, "wide=%s" % wide)
        # the two plain pods whose requests together leave int64, beside the folded ones
        assert tot["flags"][-1] != 0 and int(dec["status"][-1]) == esc._lib.ESC_ST_ERR_OVERFLOW
    n = len(FC.CASES)
    assert ctx.stream_bytes()[0] == layout.pod_bytes(P, n_gp_of(ctx))
    assert layout.pod_bytes(P, n_gp_of(ctx), 0, n) == FC.bytes_of()
    # without the overflowing pair the group's sums are exact again
    keep = [c[0] for c in FC.CASES if c[0] not in FC.WRAPPING]
    pods2 = FC.pods_of(set(keep)) + rand
    P2, N2 = ctx.pack(pods2, nodes)
    ctx.load(P2, N2)
    ctx.force_wide(False)
    tot, dec = ctx.decide_all(states)
    check(esc, tot, dec, groups, states, pods2, nodes, P2, N2, "exact")
    assert tot["flags"][-1] == 0
    assert ctx.stream_bytes()[0] == layout.pod_bytes(P2, n_gp_of(ctx))


@pytest.mark.parametrize("key", CLUSTER_IDS[1:])
def test_all_together_through_the_graph(esc, key):
    groups, rand, nodes, states = CLUSTERS[key]
    pods = FC.pods_of() + rand
    ctx = esc.Context(groups)
    P, N = ctx.pack(pods, nodes)
    ctx.load(P, N)
    ctx.use_graph(True)
    for rep in range(3):                              # captured, then replayed twice
        tot, dec = ctx.decide_all(states)
        check(esc, tot, dec, groups, states, pods, nodes, P, N, "rep %d" % rep)
        assert int(dec["status"][-1]) == esc._lib.ESC_ST_ERR_OVERFLOW


@pytest.mark.parametrize("graph", [False, True])
def test_sharded_two_contexts_host_exchange(esc, graph):
    """Two ranks' pod shards, the words exchanged through the host (the pattern of
    tests/test_gpu.py::test_sharded_two_contexts_host_exchange): == the whole snapshot, each
    shard's stream bytes its own range's."""
    from escalator_amd import layout
    from escalator_amd.dist import merge_owned, shard_range
    from test_gpu import _packed_subset, check_against_c_oracle
    groups, rand, nodes, states = CLUSTERS[(8, True)]
    pods = FC.pods_of() + rand
    rng = random.Random(77)
    rng.shuffle(pods)                                  # both shards get hand-built pods
    ctxs, words, firsts = [], [], []
    for r in range(2):
        c = esc.Context(groups, rank=r, world=2)
        P, N = c.pack(pods, nodes)
        lo, hi = shard_range(len(pods), r, 2)
        c.load(_packed_subset(P, list(range(lo, hi))), N, pod_offset=lo)
        assert c.stream_bytes()[0] == layout.pod_bytes(P, n_gp_of(c), lo, hi), r
        c.set_state(states)
        c.use_graph(graph)
        for _ in range(2 if graph else 1):
            c.reduce()
        w, f = c.exchange_download()
        words.append(w)
        firsts.append(f)
        ctxs.append(c)
    W, F = np.sum(words, axis=0), np.min(firsts, axis=0)
    parts = []
    for c in ctxs:
        c.exchange_upload(W, F)
        c.decide()
        parts.append(c.results())
    tot, dec = merge_owned(parts)
    otot = soa.totals(P, N, groups)
    odf, odi = soa.decide(groups, states, otot)
    check_against_c_oracle(tot, dec, otot, odf, odi)
    check(esc, tot, dec, groups, states, pods, nodes, P, N, "sharded")
    assert int(dec["status"][-1]) == esc._lib.ESC_ST_ERR_OVERFLOW


# ------------------------------------------------------------------ upsert transitions
def _reaping_nodes(nodes, now_s):
    out = []
    for j, nd in enumerate(nodes):
        nd = dict(nd)
        if j < 3:                                     # the ("k", "v0") group's nodes: tainted long ago
            nd["taints"] = [TAINT]
            nd["taint_value"] = str(now_s - 900)
        out.append(nd)
    return out


def test_one_pod_through_every_layout(esc):
    """One pod id, bound to a tainted node of its group, upserted from layout to layout: no
    records, two containers folding to 8 B, three folding to 12 B, a sum past 2^44 (plain,
    records kept), 5 containers (a C slot), no records again; then deleted.  After every step:
    totals and decisions against the literal oracle, the stream bytes against ``layout`` and
    against the bytes written here by hand, TryRemoveTaintedNodes against the oracle's."""
    from escalator_amd import layout
    from escalator_amd.objects import placement
    from test_gpu import _check_reaping
    groups, rand, nodes, states = CLUSTERS[(5, False)]
    now_s = 1_700_000_000
    nodes = _reaping_nodes(nodes, now_s)
    rand = [dict(p, node_name=nodes[3 + i % 20]["name"]) for i, p in enumerate(rand[:120])]
    bound = nodes[1]["name"]
    steps = [("r0", FC.pod([(100, 1 << 20)]), 8),
             ("fold8", FC.pod([(100, 1 << 20), (200, 1 << 20)]), 8),
             ("fold12", FC.pod([(1000, 6 << 30), (1000, 6 << 30), (1000, 6 << 30)]), 12),
             ("plain", FC.pod([(100, (1 << 44) - 2), (100, 2)]), 20 + 16),
             ("c_slot", FC.pod([(100, 100)] * 5), 20 + 4 * 16),
             ("r0_again", FC.pod([(300, 1 << 21)]), 8)]
    me = len(rand)
    pods = rand + [dict(steps[0][1], node_name=bound)]
    ctx = esc.Context(groups)
    ctx.set_spare(1.0)
    P, N = ctx.pack(pods, nodes)
    ctx.load(P, N)
    pn, ts, nd = placement(pods, nodes)
    ctx.load_placement(pn, ts, nd)
    n_gp = n_gp_of(ctx)
    G = len(groups)
    soft, hard = np.full(G, 60 * 10**9, np.int64), np.full(G, 4000 * 10**9, np.int64)
    base = layout.pod_bytes(ctx.pack(rand, [])[0], n_gp)
    assert layout.pod_bytes(P, n_gp) == base + 8

    def verify(tag, want_bytes):
        tot, dec = ctx.decide_all(states)
        check(esc, tot, dec, groups, states, pods, nodes, *ctx.pack(pods, nodes), tag)
        assert ctx.stream_bytes()[0] == want_bytes, (tag, ctx.stream_bytes()[0], want_bytes)
        _check_reaping(ctx, groups, pods, nodes, {}, now_s * 10**9, soft, hard)

    verify("loaded", base + 8)
    for name, obj, nbytes in steps[1:]:
        obj = dict(obj, node_name=bound)
        Pe, _ = ctx.pack([obj], [])
        assert ctx.pods_upsert([me], Pe) == 0, name
        pods[me] = obj
        if name != "c_slot":                          # (a spare C slot adds no tile offsets of its own)
            assert layout.pod_bytes(ctx.pack(pods, nodes)[0], n_gp) == base + nbytes, name
        verify(name, base + nbytes)
    ctx.pods_delete([me])
    pods = pods[:me]
    verify("deleted", base)


def test_full_packed_class_takes_pods_with_records_like_any(esc):
    """A batch of pods that carry records and fold into one packed class: those the class's
    spare room holds land in place, the next take C slots, and a batch past every room is
    refused whole (ESC_E_LIMIT) with nothing applied — as for pods without records."""
    from escalator_amd._lib import ESC_E_LIMIT
    from escalator_amd import layout
    groups, rand, nodes, states = CLUSTERS[(3, True)]
    pods = list(rand[:100])
    seen = []
    for with_records in (False, True):
        ctx = esc.Context(groups)
        ctx.set_spare(0.25)
        P, N = ctx.pack(pods, nodes)
        ctx.load(P, N)
        n_gp = n_gp_of(ctx)

        def new(i):
            extra = [(10 + i, 1 << 20)] if with_records else []
            return FC.pod([(100 + i, 1 << 20)] + extra)

        before = ctx.decide_all(states)[0].tobytes()
        many = [new(i) for i in range(400)]           # past the class's spare room and the C slots'
        assert ctx.pods_upsert(list(range(1000, 1400)), ctx.pack(many, [])[0]) == ESC_E_LIMIT
        assert ctx.decide_all(states)[0].tobytes() == before
        # fill what there is, one pod at a time: in place first, then C slots, then refused
        live, i = list(pods), 0
        while i < 400:
            obj = new(i)
            rc = ctx.pods_upsert([1000 + i], ctx.pack([obj], [])[0])
            if rc == ESC_E_LIMIT:
                break
            assert rc == 0
            live.append(obj)
            i += 1
        assert 16 < i < 400, i                        # some in place, some in C slots, then full
        tot, dec = ctx.decide_all(states)
        check(esc, tot, dec, groups, states, live, nodes, *ctx.pack(live, nodes), "filled")
        # in place a pod costs 8 B with or without records; in a C slot it keeps its records
        c = 20 + (16 if with_records else 0)
        delta = ctx.stream_bytes()[0] - layout.pod_bytes(P, n_gp)
        assert (c * i - delta) % (c - 8) == 0, (i, delta)
        n_k = (c * i - delta) // (c - 8)               # delta = 8 n_k + c (i - n_k)
        assert 0 < n_k < i, (i, n_k)
        seen.append((i, n_k))
    assert seen[0] == seen[1], seen                   # the same room, records or not
