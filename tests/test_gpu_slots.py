"""GPU: K1 (k_pod_reduce) against the C oracle across pod-slot counts.

K1 accumulates into S = n_gp + 1 pod slots: one per distinct group label pair (every group,
the "default" one included, owns or shares a pair) plus one for the default pod filter.  Two
properties of S select K1's code path and are sampled here at their edges:

- the LDS window: at most WINDOW slots fit one launch's LDS, more are taken in several
  launches over windows [g0, g0 + gw) (esc_runtime.hip enqueue_step, POD_WINDOW_MAX);
- the LDS copies: a window of gw <= REPS_MAX_GW slots keeps K1_REPS copies of its partials
  and sums them before the flush, a larger one keeps one (esc_kernels.hip k1_reps).

Every case asserts the slot count it reached (esc_ctx_num_group_pairs + 1) and what its input
holds; tests/test_k1_edges_source.py (CPU) fails when the constants below stop being the
edges of the sources.  Everything is bit-exact."""
import random

import numpy as np
import pytest

from oracle import oracle as O
from oracle import soa
from test_gpu import _bits, _packed_subset, check_against_c_oracle, check_metrics
from test_gpu_select import SEL_TAINT, SEL_UNTAINT, check_selections

pytestmark = pytest.mark.gpu
soa.build()

WINDOW = 10_240          # POD_WINDOW_MAX = LDS_BYTES / 16, LDS_BYTES = 160 * 1024 (esc_runtime.hip)
FC_COL = 32              # pod slots per K3 column (esc_kernels.h)
K1_REPS = 8              # LDS copies of a small window's partials (esc_kernels.hip)
K1_REP_LDS = 65_536      # ... kept while they fit this many bytes (esc_kernels.hip)
COPY_WORDS = (2, 2)      # k1_copy_words(gw) = ceil(gw / FC_COL) * FC_COL * 2 + 2 (esc_kernels.hip)


def k1_copy_words(gw):
    return (gw + FC_COL - 1) // FC_COL * FC_COL * COPY_WORDS[0] + COPY_WORDS[1]


def k1_reps(gw):
    """LDS copies K1 keeps for a window of gw slots (k1_reps, esc_kernels.hip)."""
    return K1_REPS if k1_copy_words(gw) * 8 * K1_REPS <= K1_REP_LDS else 1


REPS_MAX_GW = 480        # the largest window with copies: 15 columns, 8 * 962 words = 61 568 B
assert k1_reps(REPS_MAX_GW) == K1_REPS and k1_reps(REPS_MAX_GW + 1) == 1

# one window on each side of the copies threshold and of a column (FC_COL) boundary
COPIES_S = [129, 256, 449, REPS_MAX_GW, REPS_MAX_GW + 1, 512, 513]
# one full window; a second window of the default slot alone; of 2 slots; of one column; tail
# windows on each side of the copies threshold; exactly two and exactly three windows
WINDOW_S = [WINDOW, WINDOW + 1, WINDOW + 2, WINDOW + FC_COL, WINDOW + REPS_MAX_GW, WINDOW + REPS_MAX_GW + 1,
            2 * WINDOW, 2 * WINDOW + 1]
CALIBRATE_S = [WINDOW + REPS_MAX_GW, 2 * WINDOW + 1]
ORDER_S = WINDOW + 1 + 200
SHARD_S = WINDOW + 61


def windows(S):
    """(g0, gw) of K1's launches for S slots."""
    return [(g0, min(WINDOW, S - g0)) for g0 in range(0, S, WINDOW)]


def synth_groups_for_slots(S):
    """The generator's group count that gives S pod slots (host arithmetic, no device): its
    groups own one pair each, "default" included, except that group g with g % 64 == 62 shares
    the pair of g - 2 (esc_synth.cpp build_groups)."""
    G = S - 1
    while G - len(range(62, G, 64)) + 1 < S:
        G += 1
    return G


@pytest.fixture(scope="module")
def esc():
    import escalator_amd
    return escalator_amd


def slots_of(ctx):
    return ctx.lib.esc_ctx_num_group_pairs(ctx.handle) + 1


def _synth(esc, P, N, S, seed=0xE5CA1A7E00000004, **kw):
    s = esc.Synth(P, N, synth_groups_for_slots(S), config=4, seed=seed, **kw)
    t = soa.group_tables(s.groups)
    assert t["n_gp"] + 1 == S and t["default"] >= 0, (S, t["n_gp"])
    return s, t


def _assert_spread(S, t, otot):
    """The snapshot's pods reach every K1 window: some group of each window (by its pair's
    slot) has pods, and so has the default filter's slot, the last slot of the last window."""
    slot = t["gpair"].astype(np.int64)
    nondef = np.arange(t["G"]) != t["default"]
    for g0, gw in windows(S):
        sel = nondef & (slot >= g0) & (slot < g0 + gw)
        if sel.any():                                   # (a window of the default slot alone has none)
            assert otot[sel, 2].sum() > 0, (S, g0)
    assert otot[t["default"], 2] > 0, S


def _run_sequence(ctx, otot, odf, odi):
    """Three graph replays (both replicas), the exact wide path forced, then the gauges."""
    for _ in range(3):
        ctx.run()
        check_against_c_oracle(*ctx.results(), otot, odf, odi)
    ctx.force_wide(True)
    ctx.run()
    check_against_c_oracle(*ctx.results(), otot, odf, odi)
    ctx.force_wide(False)
    ctx.set_metrics(True)
    ctx.run()
    check_against_c_oracle(*ctx.results(), otot, odf, odi)
    check_metrics(ctx.metrics(), soa.metrics(otot, odf, odi))


@pytest.mark.parametrize("S", COPIES_S)
def test_copies_threshold_one_window(esc, S):
    """One LDS window of S slots on each side of the copies threshold (8 copies up to 480
    slots, one from 481) and of a column boundary."""
    assert len(windows(S)) == 1 and k1_reps(S) == (K1_REPS if S <= REPS_MAX_GW else 1)
    s, t = _synth(esc, 300_000, 20_000, S)
    pods, nodes = s.pods(), s.nodes()
    otot = soa.totals(pods, nodes, s.groups)
    odf, odi = soa.decide(s.groups, s.states, otot)
    _assert_spread(S, t, otot)
    ctx = esc.Context(s)
    assert slots_of(ctx) == S
    ctx.load_synth(s, replicas=2)
    ctx.use_graph(True)
    ctx.set_state(s.states)
    _run_sequence(ctx, otot, odf, odi)


@pytest.mark.parametrize("S", WINDOW_S)
def test_window_edges(esc, S):
    """Slot counts at the LDS window's edges: a full first window (163 840 B of dynamic LDS),
    then a second window of 1 slot (the default slot alone: no pair slot, plim = 0), of 2 (one
    16-B store), of one column, of 480 / 481 slots (copies / one copy beside a first window
    without copies), and exactly two and three windows.  At two of them esc_k1_calibrate
    re-plans K1's shares with its own windowed launches; totals exact before and after."""
    w = windows(S)
    assert len(w) == (S + WINDOW - 1) // WINDOW and w[0][1] == WINDOW
    s, t = _synth(esc, 300_000, 30_000, S)
    pods, nodes = s.pods(), s.nodes()
    otot = soa.totals(pods, nodes, s.groups)
    odf, odi = soa.decide(s.groups, s.states, otot)
    _assert_spread(S, t, otot)
    ctx = esc.Context(s)
    assert slots_of(ctx) == S
    ctx.load_synth(s, replicas=2)
    ctx.use_graph(True)
    ctx.set_state(s.states)
    _run_sequence(ctx, otot, odf, odi)
    if S in CALIBRATE_S:
        ctx.k1_calibrate(2)
        for _ in range(2):
            ctx.run()
            check_against_c_oracle(*ctx.results(), otot, odf, odi)


# ------------------------------------------------------------------ K1 without a work plan
def test_no_plan_walk_full_row_flush():
    """The walk K1 takes when plan_k1 places no plan (PodDev::seg null): equal weight ranges
    per workgroup, every row flushed whole.  ESC_K1_VARIANT=7 on the measurement library runs
    the product kernel that way (a child process, tests/fault_child.py): ~40 groups in one
    window, then S = WINDOW + 1, whose second window is the default filter's slot alone (the
    full-row flush at g0 > 0).  Bit-exact against the C oracle; no compact flush; trace words
    6-7, which only the plan branch writes, stay zero in every workgroup."""
    from test_gpu_faults import run_child
    S = WINDOW + 1
    assert windows(S) == [(0, WINDOW), (WINDOW, 1)]
    r = run_child("noplan", str(synth_groups_for_slots(S)), ESC_K1_VARIANT="7")
    assert 30 <= r["small"]["slots"] <= 42 and r["two_windows"]["slots"] == S, r
    for c in r.values():
        assert c["k_shapes"] >= 3 and c["c_pods"] > 0 and c["workgroups"] > 1, r     # what the input holds
        assert c["exact"], r
        assert c["entries"] == c["full"] > 0, r
        assert c["trace_live"] and c["plan_words_zero"], r


# ------------------------------------------------ pods that straddle windows, from objects
def _pair_sets(P):
    """(lowest, highest) selected pair of every packed pod (NONE, -1 without any)."""
    f = P["flags"].astype(np.uint64)
    nxp = ((f >> 24) & 0x3F).astype(np.int64)
    op = np.concatenate([[0], np.cumsum(nxp)])
    lo = P["pair0"].astype(np.int64)
    lo[P["pair0"] == 0xFFFFFFFF] = 1 << 40
    hi = np.where(P["pair0"] == 0xFFFFFFFF, -1, P["pair0"].astype(np.int64))
    for i in np.nonzero(nxp)[0]:
        x = P["xp_pair"][op[i]:op[i + 1]].astype(np.int64)
        lo[i], hi[i] = min(lo[i], x.min()), max(hi[i], x.max())
    return lo, hi


def _n_extra_records(P):
    f = P["flags"].astype(np.uint64)
    return (((f >> 8) & 0xFF) + ((f >> 16) & 0xFF) + ((f >> 4) & 1)).astype(np.int64)


def _big_tiles(P):
    """64-pod C tiles (pods with > 3 extra records or > 3 extra pairs, in input order) that
    hold more than 128 extra records: the ones k_pod_bigtiles takes (esc_load_pods)."""
    f = P["flags"].astype(np.uint64)
    rec = _n_extra_records(P)
    c = np.nonzero((rec > 3) | (((f >> 24) & 0x3F) > 3))[0]
    return [c[a:a + 64] for a in range(0, len(c), 64) if rec[c[a:a + 64]].sum() > 128]


def _effective_in_packed_range(p):
    """The pod's effective request (sum of containers, max with init containers, + overhead)
    stays inside K1's packed LDS range: cpu in [0, 2^20), mem in [0, 2^44)."""
    cpu = sum(c["cpu"] or 0 for c in p["containers"])
    mem = sum(c["mem"] or 0 for c in p["containers"])
    return 0 <= cpu < (1 << 20) and 0 <= mem < (1 << 44) and \
        all(0 <= (c["cpu"] or 0) < (1 << 20) and 0 <= (c["mem"] or 0) < (1 << 44) for c in p["containers"])


def _in(key, values):
    return {"node_affinity": {"required": [[{"key": key, "op": "In", "values": list(values)}]]},
            "pod_affinity": False, "pod_anti_affinity": False}


def _check_all(ctx, groups, states, P, N):
    otot = soa.totals(P, N, groups)
    odf, odi = soa.decide(groups, states, otot)
    ctx.set_state(states)
    ctx.run()
    tot, dec = ctx.results()
    check_against_c_oracle(tot, dec, otot, odf, odi)
    return tot, dec


def _check_literal(tot, dec, groups, pods, nodes, chosen):
    for g in chosen:
        L = O.scale_node_group(groups[g], {}, pods, nodes)
        t, d = tot[g], dec[g]
        assert (t["n_pods"], t["n_nodes"], t["n_untainted"], t["n_tainted"], t["n_cordoned"], t["first_node"]) == \
            (L["n_pods"], L["n_nodes"], L["n_untainted"], L["n_tainted"], L["n_cordoned"], L["first_node"]), g
        if L["pod_cpu_m"] is not None:                  # (None: the sums pass int64, the overflow gate)
            assert (t["pod_cpu_m"], t["pod_mem_b"], t["node_cpu_m"], t["node_mem_b"]) == \
                (L["pod_cpu_m"], L["pod_mem_b"], L["node_cpu_m"], L["node_mem_b"]), g
        assert int(d["delta"]) == L["delta"] and int(d["n_to_taint"]) == L["n_to_taint"], (g, L)
        assert _bits(d["cpu_pct"]) == _bits(L["cpu_pct"]) and _bits(d["mem_pct"]) == _bits(L["mem_pct"]), g


def test_pods_straddling_windows_from_objects(esc):
    """10 300 single-pair groups (pair k=v<i> is slot i) and a "default" group that shares
    v0's pair (every group has a pair; sharing keeps the slots at 10 301): window 0 holds the
    slots below 10 240, window 1 the 60 groups above and the default slot.  Packed from
    objects: pods whose nodeSelector and node-affinity pairs lie in different windows, both
    ways; default-filter pods; pods outside the packed range with a window-1 pair only (the
    exact wide words); pods with >= 5 containers (C tiles) selecting both windows; one C tile
    past 128 records (k_pod_bigtiles) on window-1 groups.  Against the C oracle for every
    group and the literal scaleNodeGroup for eight; then pod events move pods across the
    window edge and back and delete some (touch_mark's columns in the second window)."""
    NG = 10_300
    spec = {"label_key": "k", "min_nodes": 0, "max_nodes": 1000, "scale_up_pct": 70, "taint_lower_pct": 30,
            "taint_upper_pct": 45, "fast_removal_rate": 4, "slow_removal_rate": 2}
    groups = [dict(spec, name="g%d" % i, label_value="v%d" % i) for i in range(NG)]
    groups.append(dict(spec, name="default", label_value="v0"))
    DEF = NG
    t = soa.group_tables(groups)
    S = t["n_gp"] + 1
    assert S == WINDOW + 61 and list(t["gpair"][:NG]) == list(range(NG)) and t["gpair"][DEF] == 0
    rng = random.Random(10_301)
    low = lambda: rng.choice([0, 1, 5000, WINDOW - 2, WINDOW - 1, rng.randrange(WINDOW)])      # noqa: E731
    high = lambda: rng.choice([WINDOW, WINDOW + 1, NG - 1, rng.randrange(WINDOW, NG)])          # noqa: E731
    small = lambda: {"cpu": rng.randrange(1, 4000), "mem": rng.randrange(1, 1 << 33)}           # noqa: E731
    OVER = WINDOW + 10                                   # the group three overflowing pods select

    def pod(sel=None, aff=None, containers=None, **kw):
        return dict({"containers": containers or [small()], "node_selector": sel, "affinity": aff}, **kw)

    pods, kinds = [], {}

    def add(kind, n, make):
        kinds[kind] = range(len(pods), len(pods) + n)
        pods.extend(make(i) for i in range(n))

    add("plain0", 500, lambda i: pod({"k": "v%d" % low()}))                 # the pods the events move
    add("sel_lo_aff_hi", 250, lambda i: pod({"k": "v%d" % low()}, _in("k", ["v%d" % high()])))
    add("sel_hi_aff_lo", 250, lambda i: pod({"k": "v%d" % high()}, _in("k", ["v%d" % low()])))
    add("default", 300, lambda i: pod())
    big = [{"cpu": 1 << 20, "mem": 5}, {"cpu": 3, "mem": 1 << 44}, {"cpu": (1 << 33) + 1, "mem": (1 << 50) + 9},
           {"cpu": -7, "mem": 100}, {"cpu": 11, "mem": -(1 << 30)}, {"cpu": (1 << 20) + 99, "mem": (1 << 44) + 7}]
    add("wide_hi", 150, lambda i: pod({"k": "v%d" % high()}, containers=[dict(big[i % len(big)])]))
    add("overflow", 3, lambda i: pod({"k": "v%d" % OVER}, containers=[{"cpu": 1, "mem": (1 << 62) + 5}]))
    add("c_both", 300, lambda i: pod({"k": "v%d" % (low() if i % 2 else high())},
                                     _in("k", ["v%d" % low(), "v%d" % high()]),
                                     containers=[small() for _ in range(5 + i % 3)]))
    add("bigtile", 64, lambda i: pod({"k": "v%d" % high()}, containers=[small() for _ in range(9)]))
    add("plain1", 1200, lambda i: pod({"k": "v%d" % (high() if i % 3 == 0 else low())},
                                      init_containers=[{"cpu": rng.randrange(1, 9000), "mem": None}] if i % 7 == 0 else [],
                                      overhead={"cpu": 7, "mem": 11} if i % 5 == 0 else None))
    assert 2_900 <= len(pods) <= 3_100
    edge = [0, 1, WINDOW - 2, WINDOW - 1, WINDOW, WINDOW + 1, OVER, NG - 1]
    nodes = [{"name": "n%d" % j, "labels": {"k": "v%d" % (edge[j % 8] if j < 120 else (low() if j % 2 else high()))},
              "cpu": rng.choice([2000, 4000, 16000]), "mem": rng.choice([8 << 30, 64 << 30]),
              "unschedulable": j % 11 == 0, "taints": ["atlassian.com/escalator"] if j % 5 == 0 else [],
              "created_ns": 10**18 + 1000 * ((j * 37) % 200)} for j in range(200)]
    ctx = esc.Context(groups)
    assert slots_of(ctx) == S and len(windows(S)) == 2
    ctx.set_spare(1.0)
    P, N = ctx.pack(pods, nodes)
    # ---- the composition claimed above, on the packed arrays
    lo, hi = _pair_sets(P)
    strad = (lo < WINDOW) & (hi >= WINDOW)
    for kind in ("sel_lo_aff_hi", "sel_hi_aff_lo"):
        r = kinds[kind]
        assert strad[r.start:r.stop].sum() >= 200, kind
    r = kinds["default"]
    assert np.all(hi[r.start:r.stop] == -1) and len(r) >= 100
    r = kinds["wide_hi"]
    assert np.all(lo[r.start:r.stop] >= WINDOW) and np.all(hi[r.start:r.stop] < NG)
    assert sum(not _effective_in_packed_range(pods[i]) for i in r) >= 100
    rec = _n_extra_records(P)
    r = kinds["c_both"]
    assert np.all(rec[r.start:r.stop] >= 4) and strad[r.start:r.stop].sum() >= 200
    tiles = _big_tiles(P)
    assert tiles and any(np.all(lo[tl] >= WINDOW) for tl in tiles), len(tiles)
    nslot = N["label0"].astype(np.int64)
    assert (nslot < WINDOW).sum() >= 50 and ((nslot >= WINDOW) & (nslot < NG)).sum() >= 50
    # ---- load, decide
    ctx.load(P, N)
    tot, dec = _check_all(ctx, groups, None, P, N)
    chosen = [0, WINDOW - 2, WINDOW - 1, WINDOW, WINDOW + 1, NG - 1, DEF, OVER]
    assert tot["flags"][OVER] & 1
    _check_literal(tot, dec, groups, pods, nodes, chosen)
    assert tot["n_pods"][DEF] == 300 and tot["n_pods"][WINDOW - 1] > 0 and tot["n_pods"][WINDOW] > 0
    # ---- pod events across the window edge: 50 pods to a window-1 pair, back, then 50 deleted
    ids = list(kinds["plain0"])[:50]
    assert np.all(hi[ids] < WINDOW)
    for dest in (lambda i: WINDOW + i % 60, None):
        moved = [dict(pods[i], node_selector={"k": "v%d" % dest(i)}) if dest else pods[i] for i in ids]
        Pe, _ = ctx.pack(moved, [])
        assert np.all(_n_extra_records(Pe) == 0) and len(Pe["xp_pair"]) == 0
        assert np.all((Pe["pair0"] >= WINDOW) == bool(dest))
        assert ctx.pods_upsert(ids, Pe) == 0
        cur = list(pods)
        for k, i in enumerate(ids):
            cur[i] = moved[k]
            for f in ("flags", "cpu0", "mem0", "pair0"):          # no extra records either way: in place
                P[f][i] = Pe[f][k]
        tot, dec = _check_all(ctx, groups, None, P, N)
        _check_literal(tot, dec, groups, cur, nodes, [WINDOW - 1, WINDOW, WINDOW + 1, DEF])
    dels = list(kinds["plain0"])[100:125] + list(kinds["sel_lo_aff_hi"])[:15] + list(kinds["wide_hi"])[:10]
    ctx.pods_delete(dels)
    keep = [i for i in range(len(pods)) if i not in set(dels)]
    tot, dec = _check_all(ctx, groups, None, _packed_subset(P, keep), N)
    _check_literal(tot, dec, groups, [pods[i] for i in keep], nodes, chosen)


# ------------------------------------------------------------ one hot slot on the copies path
@pytest.mark.parametrize("graph", [True, False])
def test_hot_slot_on_copies_path(esc, graph):
    """S = 200 (8 LDS copies): one slot takes 300 000 pods at the packed range's maxima (cpu
    2^20 - 2, mem 2^44 - 2: the largest values the cpu | count << 40 words carry), the others a
    few each: the copy-summing pass and the packed words under the heaviest per-slot load."""
    NG, HOT, N_HOT = 198, 77, 300_000
    spec = {"label_key": "k", "min_nodes": 0, "max_nodes": 100_000, "scale_up_pct": 70, "taint_lower_pct": 30,
            "taint_upper_pct": 45, "fast_removal_rate": 4, "slow_removal_rate": 2}
    groups = [dict(spec, name="g%d" % i, label_value="v%d" % i) for i in range(NG)]
    groups.append(dict(spec, name="default", label_key="", label_value=""))
    t = soa.group_tables(groups)
    S = t["n_gp"] + 1
    assert S == 200 and k1_reps(S) == K1_REPS
    rng = random.Random(200)
    hot = [{"containers": [{"cpu": (1 << 20) - 2, "mem": (1 << 44) - 2}], "node_selector": {"k": "v%d" % HOT}}
           for _ in range(300)]
    thin = [{"containers": [{"cpu": rng.randrange(1, 4000), "mem": rng.randrange(1, 1 << 33)}],
             "node_selector": {"k": "v%d" % (i % NG)} if i % 9 else None} for i in range(600)]
    nodes = [{"name": "n%d" % j, "labels": {"k": "v%d" % (j % NG)}, "cpu": 64_000, "mem": 256 << 30,
              "created_ns": 10**18 + j} for j in range(400)]
    ctx = esc.Context(groups)
    assert slots_of(ctx) == S
    Ph, N = ctx.pack(hot, nodes)
    Pt, _ = ctx.pack(thin, [])
    assert len(Ph["xc_cpu"]) == 0 and len(Ph["xp_pair"]) == 0 and len(Pt["xc_cpu"]) == 0 and len(Pt["xp_pair"]) == 0
    P = {k: np.concatenate([np.tile(Ph[k], N_HOT // 300), Pt[k]]) for k in ("flags", "cpu0", "mem0", "pair0")}
    P.update(xc_cpu=np.zeros(0, np.int64), xc_mem=np.zeros(0, np.int64), xp_pair=np.zeros(0, np.uint32))
    assert (P["pair0"] == HOT).sum() >= N_HOT and np.all(P["cpu0"][:N_HOT] == (1 << 20) - 2) and \
        np.all(P["mem0"][:N_HOT] == (1 << 44) - 2)
    otot = soa.totals(P, N, groups)
    odf, odi = soa.decide(groups, None, otot)
    assert otot[HOT, 2] >= N_HOT and otot[HOT, 0] >= N_HOT * ((1 << 20) - 2)
    ctx.load(P, N, replicas=2)
    ctx.use_graph(graph)
    ctx.set_state(None)
    for _ in range(3):
        ctx.run()
        check_against_c_oracle(*ctx.results(), otot, odf, odi)


# ------------------------------------------- ordering and selections beside a multi-window K1
def test_order_and_selections_beside_two_windows(esc):
    """The ordering in the step and the selections K4 delivers, with K1 in two launches (a
    first window without copies, a tail window of 201 slots with them), through the graph."""
    S = ORDER_S
    assert [gw for _, gw in windows(S)] == [WINDOW, 201] and k1_reps(201) == K1_REPS
    s, t = _synth(esc, 300_000, 30_000, S)
    pods, nodes = s.pods(), s.nodes()
    otot = soa.totals(pods, nodes, s.groups)
    odf, odi = soa.decide(s.groups, s.states, otot)
    _assert_spread(S, t, otot)
    want = soa.order_all(nodes, s.groups)
    ctx = esc.Context(s)
    assert slots_of(ctx) == S
    ctx.load_synth(s, replicas=2)
    ctx.set_state(s.states)
    ctx.set_order_in_step(True)
    ctx.set_selections(2, 64)
    ctx.use_graph(True)
    for _ in range(3):
        ctx.run()
        tot, dec = ctx.results()
        check_against_c_oracle(tot, dec, otot, odf, odi)
        seen = check_selections(ctx, dec, want, nodes["created_ns"], 2, 64)
    assert seen[SEL_TAINT] > 0 and seen[SEL_UNTAINT] > 0, seen
    slot = t["gpair"].astype(np.int64)
    for g in list(np.nonzero(slot >= WINDOW)[0][:20]) + [0, 1, t["G"] - 1]:
        for w in (0, 1):
            assert np.array_equal(ctx.group_order(int(g), w), want[(int(g), w)]), (g, w)


# ----------------------------------------------------------------------------------- sharded
def test_sharded_three_ranks_two_windows(esc):
    """Three ranks' pod shards at S = 10 301 (two K1 windows per rank), exchanged through the
    host: the owners' records make up every group, exactly."""
    from escalator_amd.dist import merge_owned, merge_owned_metrics, shard_range
    S, P, N = SHARD_S, 300_000, 30_000
    assert len(windows(S)) == 2
    full, t = _synth(esc, P, N, S, seed=11)
    G = full.n_groups
    otot = soa.totals(full.pods(), full.nodes(), full.groups)
    odf, odi = soa.decide(full.groups, full.states, otot)
    _assert_spread(S, t, otot)
    ctxs, words, firsts = [], [], []
    for r in range(3):
        lo, hi = shard_range(P, r, 3)
        s = esc.Synth(P, N, G, config=4, seed=11, p_lo=lo, p_hi=hi)
        c = esc.Context(s, rank=r, world=3)
        assert slots_of(c) == S
        c.load_synth(s, pod_offset=lo)
        c.set_state(full.states)
        c.use_graph(True)
        for _ in range(2):
            c.reduce()
        w, f = c.exchange_download()
        words.append(w)
        firsts.append(f)
        ctxs.append((c, s))
    W = np.sum(words, axis=0)
    F = np.min(firsts, axis=0)
    parts, mets = [], []
    for c, _ in ctxs:
        c.set_metrics(True)
        c.exchange_upload(W, F)
        c.decide()
        parts.append(c.results())
        mets.append(c.metrics())
    tot, dec = merge_owned(parts)
    check_against_c_oracle(tot, dec, otot, odf, odi)
    owners = [ctxs[0][0].group_owner(g) for g in range(G)]
    assert set(owners) == {0, 1, 2}
    check_metrics(merge_owned_metrics(mets, owners), soa.metrics(otot, odf, odi))
