"""Hand-built pods at every edge of the fold rule, shared by
tests/test_fold_layout.py (CPU: ``layout.pod_bytes`` against the bytes written here by hand)
and tests/test_gpu_fold.py (GPU: the same pods through the library against the oracles).

The rule: a K-section pod (at most 3 extra records, at most 3 extra pairs) whose own values
are all in the packed ranges has its records folded into one effective request — regular
containers summed, max with every init container (an absent key takes no part), overhead
added.  Request cpu <= 2^14 - 1 and mem <= 2^34 - 1 (in a context with fewer than 2^14 - 1
group pairs): 8 B + 2 B per extra pair.  Else cpu < 2^20 - 1 and mem < 2^44 - 1: 12 B + 4 B
per extra pair.  Else plain with its records: 20 B + 16 B per record + 4 B per extra pair.

Each case is (name, pod object, bytes in a context with few group pairs, bytes in one with
>= 2^14 - 1 group pairs).  The pods select the group pair ("k", "v0") so that one group
counts them all; objects are the plain-dict schema of escalator_amd/objects.py.
"""
C14, M34 = 1 << 14, 1 << 34
C20, M44 = 1 << 20, 1 << 44


def pod(containers, inits=(), overhead=None, selector=True):
    return {"name": "", "owner_kinds": [], "annotations": {},
            "node_selector": {"k": "v0"} if selector else None, "affinity": None,
            "containers": [{"cpu": c, "mem": m} for c, m in containers],
            "init_containers": [{"cpu": c, "mem": m} for c, m in inits],
            "overhead": None if overhead is None else {"cpu": overhead[0], "mem": overhead[1]},
            "node_name": ""}


PLAIN1, PLAIN2 = 20 + 16, 20 + 32            # plain pod with one / two records

CASES = [
    # no records at all: the first container alone
    ("r0_small", pod([(100, 1 << 20)]), 8, 12),
    # 8-B range by a sum of two regular containers: cpu 2^14 - 1 | 2^14, mem 2^34 - 1 | 2^34
    ("sum_cpu_in8", pod([(C14 - 2, 5), (1, 5)]), 8, 12),
    ("sum_cpu_out8", pod([(C14 - 1, 5), (1, 5)]), 12, 12),
    ("sum_mem_in8", pod([(5, M34 - 2), (5, 1)]), 8, 12),
    ("sum_mem_out8", pod([(5, M34 - 1), (5, 1)]), 12, 12),
    # 12-B range: cpu 2^20 - 2 | 2^20 - 1, mem 2^44 - 2 | 2^44 - 1; just outside: plain, records kept
    ("sum_cpu_in12", pod([(C20 - 3, 5), (1, 5)]), 12, 12),
    ("sum_cpu_out12", pod([(C20 - 3, 5), (2, 5)]), PLAIN1, PLAIN1),
    ("sum_mem_in12", pod([(5, M44 - 3), (5, 1)]), 12, 12),
    ("sum_mem_out12", pod([(5, M44 - 3), (5, 2)]), PLAIN1, PLAIN1),
    # three containers whose sum passes 16 GiB: the 12-B block
    ("sum3_12", pod([(1000, 6 << 30), (1000, 6 << 30), (1000, 6 << 30)]), 12, 12),
    # init containers: one that wins the max (and leaves the 8-B range), one that loses,
    # one with one key absent, one with both absent
    ("init_wins", pod([(100, 100)], inits=[(C14, 50)]), 12, 12),
    ("init_loses", pod([(100, 100)], inits=[(99, 99)]), 8, 12),
    ("init_cpu_absent", pod([(100, 100)], inits=[(None, M34)]), 12, 12),
    ("init_mem_absent", pod([(100, 100)], inits=[(C14 - 1, None)]), 8, 12),
    ("init_both_absent", pod([(100, 100)], inits=[(None, None)]), 8, 12),
    # the max is taken after the regular sum: 60 + 60 beats the init's 100
    ("init_vs_sum", pod([(60, 60), (60, 60)], inits=[(100, 100)]), 8, 12),
    # an overhead that alone pushes the pod over each edge
    ("ovh_in8", pod([(C14 - 2, M34 - 2)], overhead=(1, 1)), 8, 12),
    ("ovh_out8_cpu", pod([(C14 - 1, 5)], overhead=(1, None)), 12, 12),
    ("ovh_out8_mem", pod([(5, M34 - 1)], overhead=(None, 1)), 12, 12),
    ("ovh_out12_cpu", pod([(C20 - 2, 5)], overhead=(1, 1)), PLAIN1, PLAIN1),
    ("ovh_out12_mem", pod([(5, M44 - 2)], overhead=(1, 1)), PLAIN1, PLAIN1),
    # regular + init + overhead together, the overhead added after the max
    ("all_three_kinds", pod([(100, 100), (100, 100)], inits=[(500, 50)], overhead=(C14 - 500, 1)), 12, 12),
    # pods that fail the range test on their own values: unchanged, plain with their records
    ("neg_record", pod([(100, 100), (-5, 100)]), PLAIN1, PLAIN1),
    ("neg_first", pod([(-5, 100)]), PLAIN1, PLAIN1),           # the packer keeps it as a record
    ("big_record", pod([(100, 100), (C20 - 1, 100)]), PLAIN1, PLAIN1),
    ("neg_init", pod([(100, 100)], inits=[(-1, 5)]), PLAIN1, PLAIN1),
    ("big_first", pod([(100, M44 - 1)]), 20, 20),
    # two plain pods whose requests together leave int64 (1.5 * 2^62 + 2^62): alone each is
    # summed exactly, in one snapshot their group's total wraps (ESC_ST_ERR_OVERFLOW)
    ("wrap", pod([(1, (1 << 62) + 5), (1, 1 << 61)]), PLAIN1, PLAIN1),
    ("wrap2", pod([(1, (1 << 62) + 5)]), 20, 20),
    # 4 records: the C section, unchanged (20 + 4 * 16, plus its tile's 8 B of offsets)
    ("c_section", pod([(100, 100)] * 5), 20 + 64, 20 + 64),
]
C_TILE_BYTES = 8                                  # one 64-pod C tile's record offsets

WRAPPING = {"wrap", "wrap2"}                      # together their group's total leaves int64


def pods_of(names=None):
    return [p for n, p, _, _ in CASES if names is None or n in names]


def bytes_of(names=None, many_pairs=False):
    sel = [c for c in CASES if names is None or c[0] in names]
    c_pods = sum(1 for c in sel if c[0] == "c_section")
    return sum(c[3] if many_pairs else c[2] for c in sel) + (c_pods + 63) // 64 * C_TILE_BYTES
