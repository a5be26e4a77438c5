"""CPU: ``layout.inert_mask`` and ``layout.pod_bytes`` over hand-built packed pods at every edge
of the definition of an inert pod: a daemonset pod, or a pod that blocks the
default filter (static, a selector, a blocking affinity) none of whose pairs is a group pair.
For each edge one pod just inside and one just outside, with the bytes written here by hand: an
inert pod of the packed small block is never streamed (0 B), every other pod costs what it cost
before (tests/fold_cases.py pins those figures for pods that join a slot)."""
import numpy as np
import pytest

from escalator_amd import layout

N_GP = 5
NONE = 0xFFFFFFFF
DS, ST, SEL, AFF = 1, 2, 4, 8

# (name, flag bits, (cpu0, mem0), pair0, extra pairs, extra regular records, inert, bytes)
ROWS = [
    ("daemonset_no_pair", DS, (100, 1 << 20), NONE, [], [], True, 0),
    ("daemonset_group_pair", DS | SEL, (100, 1 << 20), 2, [], [], True, 0),
    ("daemonset_group_pair_among_extras", DS | SEL, (100, 1 << 20), 1, [3, 9], [], True, 0),
    ("static", ST, (100, 1 << 20), NONE, [], [], True, 0),
    ("static_with_group_pair", ST | SEL, (100, 1 << 20), 0, [], [], False, 8),
    ("selector_last_group_pair", SEL, (100, 1 << 20), N_GP - 1, [], [], False, 8),
    ("selector_first_other_pair", SEL, (100, 1 << 20), N_GP, [], [], True, 0),
    ("affinity_only", AFF, (100, 1 << 20), NONE, [], [], True, 0),
    ("affinity_with_group_pair", AFF | SEL, (100, 1 << 20), 4, [], [], False, 8),
    ("plain_pod_without_pairs", 0, (100, 1 << 20), NONE, [], [], False, 8),      # joins the default slot
    ("one_group_pair_three_others", SEL, (100, 1 << 20), 3, [7, 8, 9], [], False, 8 + 6),
    ("four_other_pairs", SEL, (100, 1 << 20), 6, [7, 8, 9], [], True, 0),
    ("two_other_pairs", SEL, (100, 1 << 20), N_GP, [N_GP + 1], [], True, 0),
    ("group_pair_and_other", SEL, (100, 1 << 20), N_GP - 1, [N_GP], [], False, 8 + 2),
    # inert pods whose request does not fit the packed small block: priced as before
    ("daemonset_mem_2_34", DS, (100, 1 << 34), NONE, [], [], True, 12),
    ("daemonset_cpu_2_14", DS, (1 << 14, 5), NONE, [7], [], True, 12 + 4),
    ("static_plain", ST, (100, (1 << 44) - 1), NONE, [], [], True, 20),
    ("static_folds_to_12", ST, (1 << 13, 5), NONE, [], [(1 << 13, 5)], True, 12),
    ("static_folds_to_8", ST, (100, 5), NONE, [], [(100, 5)], True, 0),
    ("static_record_out_of_range", ST, (100, 5), NONE, [], [(-1, 5)], True, 20 + 16),
]
NAMES = [r[0] for r in ROWS]


def pack(rows):
    flags = [bits | len(recs) << 8 | len(xp) << 24 for _, bits, _, _, xp, recs, _, _ in rows]
    return {"flags": np.array(flags, np.uint32),
            "cpu0": np.array([r[2][0] for r in rows], np.uint32),
            "mem0": np.array([r[2][1] for r in rows], np.int64),
            "pair0": np.array([r[3] for r in rows], np.uint32),
            "xc_cpu": np.array([c for r in rows for c, _ in r[5]], np.int64),
            "xc_mem": np.array([m for r in rows for _, m in r[5]], np.int64),
            "xp_pair": np.array([q for r in rows for q in r[4]], np.uint32)}


@pytest.mark.parametrize("row", ROWS, ids=NAMES)
def test_each_edge_alone(row):
    pods = pack([row])
    assert layout.inert_mask(pods, N_GP).tolist() == [row[6]]
    assert layout.pod_bytes(pods, N_GP) == row[7]


def test_all_together_and_by_range():
    pods = pack(ROWS)
    assert layout.inert_mask(pods, N_GP).tolist() == [r[6] for r in ROWS]
    assert layout.pod_bytes(pods, N_GP) == sum(r[7] for r in ROWS)
    for lo in range(len(ROWS)):                            # a shard's range prices its own pods
        for hi in (lo + 1, len(ROWS)):
            assert layout.pod_bytes(pods, N_GP, lo, hi) == sum(r[7] for r in ROWS[lo:hi]), (lo, hi)


def test_the_mask_follows_the_group_pairs_alone():
    """The same pods in contexts with other group-pair counts: only n_gp moves the edge."""
    pods = pack(ROWS)
    for n_gp in (0, 1, N_GP, N_GP + 1, 10):
        want = []
        for _, bits, _, pair0, xp, _, _, _ in ROWS:
            has = any(q < n_gp for q in [pair0] + xp if q != NONE)
            want.append(bool(bits & DS) or (bool(bits & (ST | SEL | AFF)) and not has))
        assert layout.inert_mask(pods, n_gp).tolist() == want, n_gp
    # a context too wide for the packed small block (>= 2^14 - 1 group pairs) has no 8-B pods,
    # so nothing is left out: every pod is priced in its 12-B or plain layout
    wide = (1 << 14) - 1
    assert layout.pod_bytes(pods, wide) == sum(12 + 4 * len(r[4]) if r[7] < 20 else r[7] for r in ROWS)


def test_no_pods():
    pods = pack([])
    assert layout.inert_mask(pods, N_GP).tolist() == [] and layout.pod_bytes(pods, N_GP) == 0
