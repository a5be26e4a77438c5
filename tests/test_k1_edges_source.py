"""CPU: the slot counts tests/test_gpu_slots.py calls K1's edges are still the edges.

The GPU cases sit on the LDS window size and on the LDS-copies threshold of k_pod_reduce;
both are compile-time constants of the HIP sources.  They are read from the sources here and
the edges recomputed, so a change of LDS_BYTES, FC_COL, K1_REPS, K1_REP_LDS or k1_copy_words
fails this test instead of quietly leaving the GPU cases in the middle of a range."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "escalator_amd", "csrc")


def _code(name):
    src = open(os.path.join(CSRC, name)).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return "\n".join(line.split("//", 1)[0] for line in src.splitlines())


def _product(expr):
    """'160 * 1024' -> 163840 (integer literals and '*' only)."""
    assert re.fullmatch(r"\s*\d+(\s*\*\s*\d+)*\s*", expr), expr
    out = 1
    for f in expr.split("*"):
        out *= int(f)
    return out


def _constant(code, name):
    m = re.search(r"constexpr\s+\w+\s+(?:\w+\s*=\s*[^,;]+,\s*)*" + name + r"\s*=\s*([^,;]+)[,;]", code)
    assert m, name
    return m.group(1).strip()


def _source_constants():
    rt, kh, kk = _code("esc_runtime.hip"), _code("esc_kernels.h"), _code("esc_kernels.hip")
    lds_bytes = _product(_constant(rt, "LDS_BYTES"))
    m = re.fullmatch(r"LDS_BYTES\s*/\s*(\d+)", _constant(rt, "POD_WINDOW_MAX"))
    assert m, "POD_WINDOW_MAX is no longer LDS_BYTES / <bytes per slot>"
    fc_col = _product(_constant(kh, "FC_COL"))
    reps = _product(_constant(kk, "K1_REPS"))
    rep_lds = _product(_constant(kk, "K1_REP_LDS"))
    m2 = re.search(r"k1_copy_words\(uint32_t gw\)\s*\{\s*return \(gw \+ FC_COL - 1\) / FC_COL \* FC_COL \* (\d+) \+ (\d+);",
                   kk)
    assert m2, "k1_copy_words is no longer ceil(gw / FC_COL) * FC_COL * a + b"
    m3 = re.search(r"k1_reps\(uint32_t gw\)\s*\{\s*return \(uint64_t\)k1_copy_words\(gw\) \* (\d+) \* K1_REPS <= K1_REP_LDS "
                   r"\? K1_REPS : 1u;", kk)
    assert m3, "k1_reps is no longer 'K1_REPS copies of 8-B words while they fit K1_REP_LDS'"
    return {"window": lds_bytes // int(m.group(1)), "lds_bytes": lds_bytes, "slot_bytes": int(m.group(1)),
            "fc_col": fc_col, "reps": reps, "rep_lds": rep_lds, "copy_words": (int(m2.group(1)), int(m2.group(2))),
            "word_bytes": int(m3.group(1))}


def test_slot_test_constants_match_the_sources():
    import test_gpu_slots as T
    c = _source_constants()
    assert (T.WINDOW, T.FC_COL, T.K1_REPS, T.K1_REP_LDS, T.COPY_WORDS) == \
        (c["window"], c["fc_col"], c["reps"], c["rep_lds"], c["copy_words"]), c
    assert c["word_bytes"] == 8 and c["slot_bytes"] == 16
    # the first window of a multi-window context takes the whole LDS as dynamic memory
    assert T.WINDOW * c["slot_bytes"] == c["lds_bytes"] == 163_840 and T.WINDOW % T.FC_COL == 0


def test_slot_test_cases_sit_on_the_edges():
    import test_gpu_slots as T
    c = _source_constants()

    def reps(gw):                                       # recomputed from the sources' figures alone
        a, b = c["copy_words"]
        words = (gw + c["fc_col"] - 1) // c["fc_col"] * c["fc_col"] * a + b
        return c["reps"] if words * c["word_bytes"] * c["reps"] <= c["rep_lds"] else 1

    edge = max(gw for gw in range(1, c["window"] + 1) if reps(gw) > 1)
    assert edge == T.REPS_MAX_GW == 480 and all(reps(gw) > 1 for gw in range(1, edge + 1))
    assert all(T.k1_reps(gw) == reps(gw) for gw in range(1, c["window"] + 1))
    W = c["window"]
    assert {edge, edge + 1} <= set(T.COPIES_S) and all(s <= W for s in T.COPIES_S)
    # both sides of a column boundary without copies, and several columns with them
    assert {16 * c["fc_col"], 16 * c["fc_col"] + 1} <= set(T.COPIES_S) and min(T.COPIES_S) > 4 * c["fc_col"]
    assert {W, W + 1, W + 2, W + c["fc_col"], W + edge, W + edge + 1, 2 * W, 2 * W + 1} == set(T.WINDOW_S)
    assert set(T.CALIBRATE_S) <= set(T.WINDOW_S)
    for s in (T.ORDER_S, T.SHARD_S):
        w = T.windows(s)
        assert len(w) == 2 and w[0] == (0, W) and reps(w[0][1]) == 1 and reps(w[1][1]) > 1
    assert [len(T.windows(s)) for s in T.WINDOW_S] == [1, 2, 2, 2, 2, 2, 2, 3]
    # the generator's group count for a slot target is exact (one slot per own pair + 1)
    for s in T.COPIES_S + T.WINDOW_S + [T.ORDER_S, T.SHARD_S]:
        g = T.synth_groups_for_slots(s)
        assert g - len(range(62, g, 64)) + 1 == s
