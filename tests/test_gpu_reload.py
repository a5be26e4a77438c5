"""GPU: reloading one side of the snapshot alone, and when selections may be read.

esc_load_pods and esc_load_nodes both drop the age index (captured steps hold its buffers).
A pod re-list with the nodes resident (esc_load_pods alone) therefore ends by rebuilding it,
as esc_load_nodes does: the context stays usable with the ordering in the step and with
selections.  esc_selections answers only for a decision that ran with a selection target:
before the first one after esc_set_selections / esc_set_order_in_step / a reload, or after a
decision with the ordering out of the step, it returns ESC_E_STATE, never "no group asks for
a walk".  Everything against the C oracle (oracle/soa.py), bit-exact."""
import numpy as np
import pytest

from oracle import soa
from test_gpu import check_against_c_oracle
from test_gpu_select import SEL_TAINT, SEL_UNTAINT, check_selections

pytestmark = pytest.mark.gpu
soa.build()

P, N, G = 200_000, 20_000, 200
SLACK, CAP = 2, 64


@pytest.fixture(scope="module")
def esc():
    import escalator_amd
    return escalator_amd


class Ref:
    """One (pods, nodes) combination's oracle results."""

    def __init__(self, s, pods, nodes):
        self.pods, self.nodes = pods, nodes
        self.otot = soa.totals(pods, nodes, s.groups)
        self.odf, self.odi = soa.decide(s.groups, s.states, self.otot)
        self.want = soa.order_all(nodes, s.groups)


@pytest.fixture(scope="module")
def snap(esc):
    """A config-4 snapshot, a second pod set for the same groups (another seed: the label
    pairs, hence the pair ids, do not depend on it) and a second node table (taint / cordon
    flags flipped, creation times reassigned), with the oracle's results for the three
    combinations the tests load."""
    s = esc.Synth(P, N, G, config=4, seed=0xE5CA1A7E00000004)
    s2 = esc.Synth(P + 7_001, N, G, config=4, seed=0xE5CA1A7E000000B2)
    pair = lambda gs: [(g["label_key"], g["label_value"]) for g in gs]          # noqa: E731
    assert pair(s.groups) == pair(s2.groups)
    pods, nodes = s.pods(), s.nodes()
    pods2 = {k: v.copy() for k, v in s2.pods().items()}
    assert not np.array_equal(pods2["pair0"][:1000], pods["pair0"][:1000])
    rng = np.random.default_rng(17)
    nodes2 = {k: v.copy() for k, v in nodes.items()}
    ids = rng.choice(N, N // 4, replace=False)
    nodes2["flags"][ids] ^= rng.integers(1, 4, len(ids)).astype(np.uint32) & 3   # taint / cordon bits
    nodes2["created_ns"] = rng.permutation(nodes["created_ns"])
    return {"s": s, "keep": s2, "a": Ref(s, pods, nodes), "pods2": Ref(s, pods2, nodes), "nodes2": Ref(s, pods, nodes2)}


def _context(esc, snap, selections):
    s, a = snap["s"], snap["a"]
    ctx = esc.Context(s)
    ctx.load(a.pods, a.nodes)
    ctx.set_state(s.states)
    ctx.set_order_in_step(True)
    if selections:
        ctx.set_selections(SLACK, CAP)
    return ctx


def _decide(ctx, ref, selections=False):
    ctx.run()
    tot, dec = ctx.results()
    check_against_c_oracle(tot, dec, ref.otot, ref.odf, ref.odi)
    if selections:
        seen = check_selections(ctx, dec, ref.want, ref.nodes["created_ns"], SLACK, CAP)
        assert seen[SEL_TAINT] > 0 and seen[SEL_UNTAINT] > 0, seen
    return dec


def _orders(ctx, ref):
    for g in range(G):
        for w in (0, 1):
            assert np.array_equal(ctx.group_order(g, w), ref.want[(g, w)]), (g, w)


@pytest.mark.parametrize("selections", [False, True])
def test_pods_only_reload_with_order_in_step(esc, snap, selections):
    """load_pods alone with the nodes resident and the ordering in the step: the next
    decisions (plain, then through a newly captured graph) are the oracle's for the new pods
    and the old nodes, with every group's two orders — from the step and from esc_sort_nodes —
    and, when on, the selections."""
    ctx = _context(esc, snap, selections)
    _decide(ctx, snap["a"], selections)
    b = snap["pods2"]
    assert not np.array_equal(b.odi[:, 0], snap["a"].odi[:, 0])      # the reload changes decisions
    ctx.load_pods(b.pods)
    ctx.use_graph(False)
    _decide(ctx, b, selections)
    _orders(ctx, b)
    ctx.use_graph(True)
    for _ in range(2):
        _decide(ctx, b, selections)
    _orders(ctx, b)
    ctx.sort_nodes()
    _orders(ctx, b)


def test_selections_refused_until_a_decision_delivers_them(esc, snap):
    """selections() is ESC_E_STATE whenever the last decision did not run with a selection
    target, and exact again after one normal decision."""
    from escalator_amd._lib import EscError, ESC_E_STATE

    def refused():
        with pytest.raises(EscError) as e:
            ctx.selections()
        assert e.value.code == ESC_E_STATE

    a = snap["a"]
    ctx = _context(esc, snap, False)
    _decide(ctx, a)                                      # (the decision records exist from here on)
    ctx.set_selections(SLACK, CAP)
    refused()                                            # no decision since esc_set_selections
    _decide(ctx, a, True)
    ctx.set_order_in_step(False)
    refused()
    _decide(ctx, a)                                      # decided with no ordering to select from
    refused()
    ctx.set_order_in_step(True)
    refused()
    _decide(ctx, a, True)
    ctx.load_pods(snap["pods2"].pods)                    # a reload: fresh records, nothing decided
    refused()
    _decide(ctx, snap["pods2"], True)
    ctx.load_nodes(a.nodes)
    refused()
    ctx.use_graph(True)
    _decide(ctx, snap["pods2"], True)
    _decide(ctx, snap["pods2"], True)


def test_nodes_only_reload(esc, snap):
    """load_nodes alone with the pods resident (flags and creation times changed): decisions,
    orders and selections follow the new nodes."""
    ctx = _context(esc, snap, True)
    ctx.use_graph(True)
    _decide(ctx, snap["a"], True)
    b = snap["nodes2"]
    assert not np.array_equal(b.otot[:, 6], snap["a"].otot[:, 6])    # untainted counts moved
    ctx.load_nodes(b.nodes)
    for _ in range(2):
        _decide(ctx, b, True)
    _orders(ctx, b)
    ctx.sort_nodes()
    _orders(ctx, b)
