"""CPU: layout.compact_positions, the NumPy restatement of esc_pods_compact's order rule, on
hand-written cases with the positions written out by hand (the GPU suite compares every pod's
esc_pod_where with it), and layout.class_ids on one pod of every layout."""
import numpy as np

from escalator_amd import layout

NONE = 0xFFFFFFFF
N_GP = 96                       # buckets 0, 1, 2 (pairs 0..31, 32..63, 64..95) and the last, 3


def positions(cls, src, pair0, live, rehomed=None, n_gp=N_GP, pod_sort=32):
    rehomed = [0] * len(cls) if rehomed is None else rehomed
    return layout.compact_positions(cls, src, pair0, live, rehomed, n_gp, pod_sort).tolist()


def test_holes_at_a_tiles_start_middle_and_end():
    # one class of two tiles, every pod in bucket 0: the live pods close up in old-position order
    n = 512
    live = np.ones(n, bool)
    live[[0, 1, 2]] = False                 # the first tile's start
    live[[100, 101]] = False                # its middle
    live[[254, 255]] = False                # its end
    live[[256]] = False                     # the second tile's start
    live[[511]] = False                     # and end
    got = positions([7] * n, list(range(n)), [5] * n, live)
    want, nxt = [], 0
    for i in range(n):
        want.append(nxt if live[i] else -1)
        nxt += int(live[i])
    assert got == want and got[3] == 0 and got[102] == 97 and got[257] == 249 and max(got) == 502   # 8 holes before slot 257


def test_a_whole_free_first_tile_and_a_whole_free_last_tile():
    n = 768
    live = np.zeros(n, bool)
    live[256:512] = True
    got = positions([0] * n, list(range(n)), [40] * n, live)
    assert got[:256] == [-1] * 256 and got[512:] == [-1] * 256
    assert got[256:512] == list(range(256))
    live[:] = False
    live[:256] = True                       # only the first tile: nothing moves
    assert positions([0] * n, list(range(n)), [40] * n, live)[:256] == list(range(256))


def test_buckets_and_the_last_bucket_edges():
    #        old pos:  0     1   2        3         4      5   6   7
    pair0 = [NONE, N_GP, 95, N_GP - 1, N_GP + 7, 31, 32, 0]
    # bucket:          3     3   2        2         3      0   1   0
    got = positions([3] * 8, list(range(8)), pair0, [1] * 8)
    # bucket 0: old 5, 7; bucket 1: old 6; bucket 2: old 2, 3; the last: old 0, 1, 4
    assert got == [5, 6, 3, 4, 7, 0, 2, 1]
    # n_gp - 1 is a group pair (its own bucket when it starts one), n_gp is not
    assert positions([0, 0], [0, 1], [64, 63], [1, 1], n_gp=65) == [1, 0]
    assert positions([0, 0], [0, 1], [65, 64], [1, 1], n_gp=65) == [1, 0]
    assert positions([0, 0, 0], [0, 1, 2], [66, 65, 64], [1, 1, 1], n_gp=65) == [1, 2, 0]


def test_pod_sort_zero_is_one_bucket():
    got = positions([1] * 5, [4, 3, 2, 1, 0], [90, 0, NONE, 33, 64], [1, 1, 0, 1, 1], pod_sort=0)
    assert got == [3, 2, -1, 1, 0]          # old positions 0, 1, 3, 4 in order; pairs play no part


def test_classes_are_independent_and_dead_entries_take_none():
    cls = [2, 1, 2, 1, -1, 2]
    got = positions(cls, [0, 0, 1, 1, 9, 2], [70, 70, 1, 1, 1, 1], [1, 1, 1, 0, 1, 1])
    assert got == [2, 0, 0, -1, -1, 1]


def test_rehomed_pods_interleave_by_bucket_behind_the_residents():
    #  residents of class 0 at old positions 0, 1, 2, 5 (buckets 1, 0, 2, 0); re-homed pods from C
    #  slots 70, 3, 12 (buckets 0, 2, 0): inside a bucket the residents first, then by C index
    cls = [0, 0, 0, 0, 0, 0, 0]
    src = [0, 1, 2, 5, 70, 3, 12]
    pair0 = [40, 3, 80, 9, 4, 64, 31]
    rehomed = [0, 0, 0, 0, 1, 1, 1]
    got = positions(cls, src, pair0, [1] * 7, rehomed)
    # bucket 0: old 1, old 5, C 12, C 70 -> 0..3; bucket 1: old 0 -> 4; bucket 2: old 2, C 3 -> 5, 6
    assert got == [4, 0, 5, 1, 3, 6, 2]
    # a C index below every old position still follows the residents of its bucket
    assert positions([0, 0], [200, 0], [1, 2], [1, 1], [0, 1]) == [0, 1]


def test_empty_input():
    assert positions([], [], [], []) == []


def test_class_ids_of_every_layout():
    def pods(flags, cpu0, mem0, pair0, xc=(), xm=(), xp=()):
        return {"flags": np.array(flags, np.uint32), "cpu0": np.array(cpu0, np.uint32), "mem0": np.array(mem0, np.int64),
                "pair0": np.array(pair0, np.uint32), "xc_cpu": np.array(xc, np.int64), "xc_mem": np.array(xm, np.int64),
                "xp_pair": np.array(xp, np.uint32)}
    SEL, DS = 1 << 2, 1 << 0
    P = pods([SEL, SEL | 2 << 24, SEL, SEL | 1 << 8, SEL | 1 << 8 | 1 << 24, DS | SEL, SEL | 1 << 24, SEL | 4 << 8, 0],
             [100, 100, 100, 1 << 20, 1 << 20, 100, 100, 1, 100],
             [1 << 20, 1 << 20, 17 << 30, 5, 5, 1 << 20, 1 << 20, 1, 1 << 20],
             [0, 1, 2, 3, 4, 5, 200, 6, NONE],
             xc=[3, 3, 1, 1, 1, 1], xm=[7, 7, 1, 1, 1, 1], xp=[5, 6, 9, 300])
    got = layout.class_ids(P, n_gp=100).tolist()
    # small, small + 2 pairs, 12-B packed, plain (1 record), plain (1 record, 1 pair), inert (daemonset),
    # inert (blocks the default filter, no group pair), the C section (4 records), small (no pair: default slot)
    assert got == [256, 258, 128, 32, 33, 384, 385, -1, 256]
    # in a context of 2^14 - 1 group pairs or more there is no packed small class
    assert layout.class_ids(P, n_gp=(1 << 14) - 1).tolist()[:3] == [128, 130, 128]
