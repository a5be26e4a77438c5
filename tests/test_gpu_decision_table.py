"""GPU: K4's float64 decision arithmetic at its edges (tests/decision_table.py), through
every way a decision is delivered: the compact and the full record, the pinned totals
record (G <= 1 024) and the word arrays above it, a replayed graph, the owner-scoped K4 of a
multi-device context and of per-process ranks.  All cases sit in one context and one
decision; every comparison is equality of integers or of float64 bits, against the literal
oracle on each case's objects and against the C oracle on the packed table."""
import random

import numpy as np
import pytest

import decision_table as DT
from oracle import soa
from test_gpu import _packed_subset, check_metrics

pytestmark = pytest.mark.gpu
soa.build()


@pytest.fixture(scope="module")
def esc():
    import escalator_amd
    return escalator_amd


@pytest.fixture(scope="module")
def table():
    return DT.build()


class Cluster:
    """Cases as one packed cluster with both references for a list of states."""

    def __init__(self, cases):
        from escalator_amd.context import Context
        self.cases = cases
        self.asm = DT.assemble(cases)
        self.groups, self.states = self.asm["groups"], self.asm["states"]
        self.P, self.N = Context(self.groups, device=-1).pack(self.asm["pods"], self.asm["nodes"], self.asm["trackers"])
        self.otot = soa.totals(self.P, self.N, self.groups)
        self._refs = {}

    def refs(self, states=None, key="base"):
        if key not in self._refs:
            odf, odi = soa.decide(self.groups, self.states if states is None else states, self.otot)
            self._refs[key] = (DT.oracle_arrays(self.cases, self.asm["node_base"], states),
                               (self.otot, None, odf, odi, soa.metrics(self.otot, odf, odi)))
        return self._refs[key]

    def check(self, what, tot, dec, met, states=None, key="base"):
        t, df, di = DT.result_arrays(tot, dec)
        for name, (rtot, known, rdf, rdi, mets) in zip(("literal oracle", "C oracle"), self.refs(states, key)):
            DT.compare(self.cases, "%s against the %s" % (what, name), t, df, di, rtot, known, rdf, rdi)
            try:
                check_metrics(met, mets)
            except AssertionError as e:                 # name the case, not only its index
                from escalator_amd._lib import METRIC_NAMES
                g, why = DT.gauge_mismatch(met, mets, METRIC_NAMES) or (None, "check_metrics: %s" % e)
                raise AssertionError("%s against the %s, gauges of group %s: %s\n%s" % (
                    what, name, g, why, DT.describe(self.cases[g]) if g is not None else "")) from None


@pytest.fixture(scope="module")
def full(table):
    return Cluster(table)


@pytest.fixture(scope="module")
def core(table):
    return Cluster(DT.core(table))


def _decide_both_widths(esc, cl, what):
    ctx = esc.Context(cl.groups)
    ctx.load(cl.P, cl.N)
    ctx.set_metrics(True)
    for wide in (False, True):
        ctx.force_wide(wide)
        tot, dec = ctx.decide_all(cl.states)
        cl.check("%s, force_wide %d" % (what, wide), tot, dec, ctx.metrics())
    ctx.close()
    return dec


def test_full_table_word_array_totals(esc, full):
    """G > 1 024: the totals come back through the word arrays."""
    assert len(full.cases) > 1024
    dec = _decide_both_widths(esc, full, "full table")
    assert (dec["delta"] > (1 << 31)).any() and (dec["delta"] == DT.INT64_MIN).any()     # the full record


def test_core_subset_pinned_totals(esc, core):
    """G <= 1 024: K4 writes the totals records to pinned host memory."""
    assert len(core.cases) <= 1024
    _decide_both_widths(esc, core, "core subset")


def test_core_subset_shuffled(esc, table):
    """A K4 block holds 64 groups: another group order puts the wide records, the errors and
    the special values into other lanes and blocks."""
    cases = DT.core(table)
    random.Random(64).shuffle(cases)
    _decide_both_widths(esc, Cluster(cases), "shuffled core subset")


def test_graph_replay_reads_new_states(esc, full):
    """A replayed step reads the parameters of the last set_state: every lock flipped and
    the cached capacities swapped, then back."""
    flipped = DT.flipped_states(full.cases)
    ctx = esc.Context(full.groups)
    ctx.load(full.P, full.N)
    ctx.set_metrics(True)
    ctx.use_graph(True)
    seen = []
    for k, (states, key) in enumerate(((None, "base"), (flipped, "flipped"), (None, "base"))):
        ctx.set_state(full.states if states is None else states)
        ctx.step()
        tot, dec = ctx.results()
        full.check("graph step %d (%s states)" % (k, key), tot, dec, ctx.metrics(), states, key)
        seen.append(dec.tobytes())
    assert seen[0] == seen[2] != seen[1]
    ctx.close()


def test_multi_device_context(esc, full):
    """devices=[0, 0, 0]: every group decided by its owner shard from summed pod words."""
    ctx = esc.Context(full.groups, devices=[0, 0, 0])
    ctx.load(full.P, full.N)
    ctx.set_state(full.states)
    ctx.set_metrics(True)
    ctx.step()
    tot, dec = ctx.results()
    full.check("multi-device context", tot, dec, ctx.metrics())
    assert len({ctx.group_owner(g) for g in range(len(full.cases))}) == 3
    ctx.close()


def test_two_ranks_host_exchange(esc, core):
    """Two per-process ranks, the pod words summed through the host: each rank decides the
    groups it owns (the others come back NOT_OWNED) and the owners' records make up the table."""
    from escalator_amd._lib import ESC_ST_NOT_OWNED, ESC_TF_NOT_OWNED
    from escalator_amd.dist import merge_owned, merge_owned_metrics, shard_range
    world, n_pods, G = 2, len(core.asm["pods"]), len(core.cases)
    ctxs, words, firsts = [], [], []
    for r in range(world):
        lo, hi = shard_range(n_pods, r, world)
        c = esc.Context(core.groups, rank=r, world=world)
        c.load(_packed_subset(core.P, list(range(lo, hi))), core.N, pod_offset=lo)
        c.set_state(core.states)
        c.set_metrics(True)
        c.reduce()
        w, f = c.exchange_download()
        words.append(w)
        firsts.append(f)
        ctxs.append(c)
    W, F = np.sum(words, axis=0), np.min(firsts, axis=0)
    owners = np.array([ctxs[0].group_owner(g) for g in range(G)])
    assert set(owners.tolist()) == {0, 1}
    parts, mets = [], []
    for r, c in enumerate(ctxs):
        c.exchange_upload(W, F)
        c.decide()
        t, d = c.results()
        assert np.array_equal((t["flags"] & ESC_TF_NOT_OWNED) == 0, owners == r), r
        assert (d["status"][owners != r] == ESC_ST_NOT_OWNED).all(), r
        parts.append((t, d))
        mets.append(c.metrics())
    tot, dec = merge_owned(parts)
    core.check("two ranks merged", tot, dec, merge_owned_metrics(mets, owners))
    for c in ctxs:
        c.close()
