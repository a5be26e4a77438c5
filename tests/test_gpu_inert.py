"""GPU: pods that no group can ever count sit in inert classes that K1 never streams
(DESIGN.md §3, §8o).

The cluster of tests/inert_cases.py: five groups, each under its own pair, without and with a
sixth named "default"; pods at every edge of the definition times 0 .. 3 extra pairs, 255 / 256 /
257 in each inert class and in the matching packed small class.  Every group's totals and
decisions equal the literal oracle and the C oracle; the library's stream bytes equal
``layout.pod_bytes`` and are those of the same pods with nothing left out less the inert small
pods' 8 B + 2 B per extra pair — plain, with the exact wide path forced, through the captured
graph over three replicas, after ``k1_calibrate``, without a work plan (a child process on the
measurement library) and sharded over two contexts.  Then pod events: one pod id from a counted
class to an inert one and back with a placement loaded, an inert class filled and grown, and a
context whose every pod is inert."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import inert_cases as IC
from oracle import soa
from test_gpu_fold import check, n_gp_of
from test_gpu_pods_grow import E_LIMIT, MEASURE, PodWorld, tiles, want

pytestmark = pytest.mark.gpu
soa.build()

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
INERT0, SMALL0 = 384, 256                         # class ids: inert / packed small, no extra pairs


@pytest.fixture(scope="module")
def esc():
    import escalator_amd
    return escalator_amd


class Cluster:
    def __init__(self, with_default):
        self.groups = IC.groups(with_default)
        self.pods, self.kinds, self.inert = IC.pods()
        self.nodes = IC.nodes()
        self.states = IC.states(len(self.groups))


CLUSTERS = {d: Cluster(d) for d in (False, True)}


def small_inert_bytes(P, n_gp):
    """What K1 no longer streams: the inert pods of the packed small block, 8 B + 2 B per pair."""
    from escalator_amd import layout
    nxp = ((P["flags"].astype(np.uint64) >> 24) & 0x3F).astype(np.int64)
    return int((8 + 2 * nxp)[layout.inert_mask(P, n_gp) & layout.small_mask(P, n_gp)].sum())


def check_bytes(ctx, P, tag=""):
    from escalator_amd import layout
    n_gp = n_gp_of(ctx)
    got = ctx.stream_bytes()[0]
    assert got == layout.pod_bytes(P, n_gp), (tag, got)
    cut = small_inert_bytes(P, n_gp)
    by_hand = sum(8 + 2 * x for x, n in IC.N_INERT.items() for _ in range(n))
    assert cut == by_hand > 0, (tag, cut, by_hand)
    return got, cut


@pytest.mark.parametrize("with_default", [False, True])
def test_the_packer_gives_the_pods_the_table_describes(esc, with_default):
    """The hand-built pods land where the cases say: the mask row by row, group 4's pair the last
    group pair, the class counts at the tile edges (read back through esc_pods_room)."""
    from escalator_amd import layout
    c = CLUSTERS[with_default]
    ctx = esc.Context(c.groups)
    ctx.set_spare(0.25)
    P, N = ctx.pack(c.pods, c.nodes)
    n_gp = n_gp_of(ctx)
    assert n_gp == IC.N_GROUPS + with_default               # (the default group's empty pair is one too)
    assert layout.inert_mask(P, n_gp).tolist() == c.inert
    last = IC.N_GROUPS - 1                                   # the last group pair without "default"
    for kind, lo, hi in (("sel_last_group_pair", last, last), ("sel_first_other_pair", n_gp, 1 << 30)):
        got = {int(P["pair0"][i]) for i, k in enumerate(c.kinds) if k == kind}
        assert got and all(lo <= q <= hi for q in got), (kind, got)
    ctx.load(P, N)
    r = ctx.pods_room()["per_class"]
    for x in range(4):
        for base, n in ((INERT0, IC.N_INERT[x]), (SMALL0, IC.N_LIVE[x])):
            assert r[base + x] == tiles(want(n, 0, 0.25)) * 256 - n, (base, x)
    # the inert pods outside the packed small block: the packed and plain classes, as before
    assert r[128] == 256 - 7 and r[129] == r[130] == r[131] == 255 and r[0] == 255


@pytest.mark.parametrize("with_default", [False, True])
def test_totals_and_bytes_plain_wide_graph_replicas_calibrated(esc, with_default):
    c = CLUSTERS[with_default]
    ctx = esc.Context(c.groups)
    ctx.set_spare(0.25)
    P, N = ctx.pack(c.pods, c.nodes)
    ctx.load(P, N, replicas=3)

    def verify(tag):
        tot, dec = ctx.decide_all(c.states)
        check(esc, tot, dec, c.groups, c.states, c.pods, c.nodes, P, N, tag)
        return tot

    tot = verify("plain")
    # every counted pod is counted once per group pair it has, the default slot's besides
    assert int(tot["n_pods"][:IC.N_GROUPS].sum()) == sum(IC.N_LIVE.values()) - c.kinds.count("no_filter_bit")
    if with_default:
        assert int(tot["n_pods"][-1]) == c.kinds.count("no_filter_bit") > 0
    got, cut = check_bytes(ctx, P, "plain")
    # the same context's bytes with no pod left out: these plus the inert small pods'
    from escalator_amd import layout
    everyone = dict(P, flags=P["flags"] & ~np.uint32(0xF) | np.uint32(4), pair0=np.zeros_like(P["pair0"]))
    assert got + cut == layout.pod_bytes(everyone, n_gp_of(ctx)) and got < got + cut
    ctx.force_wide(True)
    verify("wide")
    ctx.force_wide(False)
    ctx.use_graph(True)
    for rep in range(4):                               # captured, then replayed: every replica
        verify("graph %d" % rep)
    ctx.k1_calibrate(2)
    for rep in range(3):
        verify("calibrated %d" % rep)
    check_bytes(ctx, P, "calibrated")


def test_flush_entries_are_those_of_the_snapshot_without_its_inert_pods(esc):
    """The inert tiles are in no workgroup's share and ask for no workgroup: K1's grid, its plan
    and the pod-slot columns its workgroups flush are those of the counted pods alone."""
    c = CLUSTERS[True]
    seen = []
    for keep in (None, [i for i, x in enumerate(c.inert) if not x or "12_bytes" in c.kinds[i] or c.kinds[i] == "ds_plain"]):
        pods = c.pods if keep is None else [c.pods[i] for i in keep]
        for spare in (0.0, 0.25):
            ctx = esc.Context(c.groups)
            ctx.set_spare(spare)
            P, N = ctx.pack(pods, c.nodes)
            ctx.load(P, N)
            tot, dec = ctx.decide_all(c.states)
            check(esc, tot, dec, c.groups, c.states, pods, c.nodes, P, N, "spare %s" % spare)
            seen.append((spare, ctx.k1_flush_entries(), int(ctx.k1_trace().shape[0])))
            ctx.close()
    assert seen[0] == seen[2] and seen[1] == seen[3], seen
    assert seen[0][1][0] > 0


def test_no_plan_walk_stops_before_the_inert_classes():
    assert os.path.exists(MEASURE), "build the measurement library: make -C escalator_amd/csrc ABLATIONS=1"
    env = dict(os.environ, ESC_LIB_PATH=MEASURE, ESC_K1_VARIANT="7")
    r = subprocess.run([sys.executable, "-u", os.path.join(HERE, "inert_child.py")], capture_output=True, text=True,
                       timeout=240, env=env, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-3000:]
    out = json.loads([x for x in r.stdout.splitlines() if x.startswith("{")][-1])
    for tag, c in out.items():
        assert c["exact"] and c["plan_words_zero"], (tag, out)
        assert c["entries"] == c["full"] > 0, (tag, out)           # no plan: every row flushed whole
        assert c["bytes"] == c["layout_bytes"] > 0 and c["counted"] > 0, (tag, out)


@pytest.mark.parametrize("graph", [False, True])
def test_sharded_two_contexts_host_exchange(esc, graph):
    """Two ranks' pod shards, the words exchanged through the host: == the whole snapshot, each
    shard's stream bytes its own range's."""
    from escalator_amd import layout
    from escalator_amd.dist import merge_owned, shard_range
    from test_gpu import _packed_subset, check_against_c_oracle
    c = CLUSTERS[True]
    ctxs, words, firsts = [], [], []
    for r in range(2):
        x = esc.Context(c.groups, rank=r, world=2)
        P, N = x.pack(c.pods, c.nodes)
        lo, hi = shard_range(len(c.pods), r, 2)
        x.load(_packed_subset(P, list(range(lo, hi))), N, pod_offset=lo)
        assert x.stream_bytes()[0] == layout.pod_bytes(P, n_gp_of(x), lo, hi), r
        assert any(c.inert[lo:hi]) and not all(c.inert[lo:hi])
        x.set_state(c.states)
        x.use_graph(graph)
        for _ in range(2 if graph else 1):
            x.reduce()
        w, f = x.exchange_download()
        words.append(w)
        firsts.append(f)
        ctxs.append(x)
    W, F = np.sum(words, axis=0), np.min(firsts, axis=0)
    parts = []
    for x in ctxs:
        x.exchange_upload(W, F)
        x.decide()
        parts.append(x.results())
    tot, dec = merge_owned(parts)
    otot = soa.totals(P, N, c.groups)
    odf, odi = soa.decide(c.groups, c.states, otot)
    check_against_c_oracle(tot, dec, otot, odf, odi)
    check(esc, tot, dec, c.groups, c.states, c.pods, c.nodes, P, N, "sharded")


# ------------------------------------------------------------------ pod events
def world(esc, spare=0.25):
    c = CLUSTERS[True]
    return c, PodWorld(esc, c.groups, c.pods, c.nodes, spare)


def lonely_is_empty(w, got):
    """The tainted node that only inert pods are bound to is deletable, as the oracle says
    (World.check has compared the lists with the oracle's already)."""
    assert any(p is not None and p["node_name"] == "lonely" for p in w.pods)
    assert "lonely" in got["rm_list"][0], got["rm_list"][0]


def test_one_pod_from_a_counted_class_to_an_inert_one_and_back(esc):
    """Pod id `me`, bound to a node of group 0, upserted counted -> inert -> counted.  The inert
    class of pods without extra pairs holds 256 pods, so the pod takes the first slot of its
    second tile; on the way back it takes a free slot of the packed small class.  After every
    step: every answer against the oracles and a fresh load, TryRemoveTaintedNodes included, a
    clean audit, the stream bytes against ``layout`` and against the bytes written here."""
    from escalator_amd import layout
    c, w = world(esc)
    me = next(i for i, k in enumerate(c.kinds) if k == "sel_group_pair")
    w.bind([me], ["n15"])                                       # a tainted node of group 0
    n_gp = n_gp_of(w.ctx)
    assert IC.N_INERT[0] == 256

    def stream(tag):
        P = w.ctx.pack([p for p in w.pods if p is not None], [])[0]
        got = w.ctx.stream_bytes()[0]
        assert got == layout.pod_bytes(P, n_gp), (tag, got)
        return got

    got, _ = w.check("loaded")
    lonely_is_empty(w, got)
    b0, r0 = stream("loaded"), w.ctx.pods_room()["per_class"]
    steps = [("inert: daemonset", IC.pod("me", sel=IC.live_sel(0, 0), ds=True, node_name="n15"), -8, INERT0),
             ("counted again", IC.pod("me", sel=IC.live_sel(0, 0), node_name="n15"), 0, SMALL0),
             ("inert: no group pair", IC.pod("me", sel=IC.other_sel(0), node_name="n15"), -8, INERT0),
             ("counted, two extra pairs", IC.pod("me", sel=IC.live_sel(0, 2), node_name="n15"), 4, SMALL0 + 2),
             ("inert, two extra pairs", IC.pod("me", sel=IC.other_sel(2), aff=True, node_name="n15"), -8, INERT0 + 2)]
    for tag, obj, delta, cls in steps:
        assert w.upsert([me], [obj]) == 0, tag
        got, _ = w.check(tag)
        lonely_is_empty(w, got)
        assert stream(tag) == b0 + delta, tag
        r = w.ctx.pods_room()["per_class"]
        for k in (INERT0, SMALL0, INERT0 + 2, SMALL0 + 2):     # its first slot freed, one taken where it is
            assert r[k] == r0[k] + (1 if k == SMALL0 else 0) - (1 if k == cls else 0), (tag, k)
    w.delete([me])
    w.check("deleted")
    assert stream("deleted") == b0 - 8


def test_an_inert_class_fills_up_and_grows(esc):
    """The inert class without extra pairs: 256 pods at spare 0.25, 320 wanted, two tiles, 256
    free positions and 16 spare C slots.  300 more daemonset pods do not fit; esc_pods_grow makes
    the room the load's rule gives, and the same batch then lands in the class, unstreamed."""
    from escalator_amd import layout
    c, w = world(esc)
    n_gp = n_gp_of(w.ctx)
    r = w.ctx.pods_room()
    assert r["per_class"][INERT0] == 2 * 256 - 256 and r["c_free"] == 16
    b0 = w.ctx.stream_bytes()[0]
    n0 = len(w.pods)
    ids = list(range(n0, n0 + 300))
    burst = [IC.pod("b%d" % i, ds=True, cpu=1 + i % 90, node_name="lonely" if i % 7 == 0 else "") for i in ids]
    before = w.ctx.audit()
    assert w.upsert(ids, burst) == E_LIMIT
    assert w.ctx.audit() == before and w.ctx.stream_bytes()[0] == b0
    w.grow(ids, burst)
    assert tiles(want(256, 300, 0.25)) == 3
    assert w.ctx.pods_room()["per_class"][INERT0] == 3 * 256 - 256
    w.check("grown")
    assert w.upsert(ids, burst) == 0
    assert w.ctx.pods_room()["per_class"][INERT0] == 3 * 256 - 556
    got, _ = w.check("burst in")
    lonely_is_empty(w, got)
    assert w.ctx.stream_bytes()[0] == b0 == layout.pod_bytes(w.ctx.pack([p for p in w.pods if p is not None], [])[0], n_gp)


@pytest.mark.parametrize("spare", [0.0, 0.25])
def test_every_pod_inert(esc, spare):
    """No K tile has any weight: without spare room K1 has no workgroup at all (as for an empty
    snapshot), with it the spare C tile's.  Every sum is zero, on every path."""
    c = CLUSTERS[True]
    pods = [p for p, x, k in zip(c.pods, c.inert, c.kinds) if x and "12_bytes" not in k and k != "ds_plain"]
    ctx = esc.Context(c.groups)
    ctx.set_spare(spare)
    P, N = ctx.pack(pods, c.nodes)
    ctx.load(P, N, replicas=2)
    assert ctx.stream_bytes()[0] == 0
    for tag in ("plain", "wide", "graph", "graph again", "calibrated"):
        ctx.force_wide(tag == "wide")
        if tag == "graph":
            ctx.use_graph(True)
        if tag == "calibrated":
            ctx.k1_calibrate(2)
        tot, dec = ctx.decide_all(c.states)
        check(esc, tot, dec, c.groups, c.states, pods, c.nodes, P, N, tag)
        assert not tot["n_pods"].any() and not tot["pod_cpu_m"].any() and not tot["pod_mem_b"].any(), tag
    assert ctx.k1_flush_entries()[0] <= ctx.k1_flush_entries()[1]
