"""CPU: the slot counts tests/test_gpu_k1_width.py puts on each side of the one-workgroup-per-CU
edge are still on each side of it, and the product still runs K1 at 512 threads only.

A K1 window whose dynamic LDS (k1_lds_bytes, esc_kernels.hip) is more than half of LDS_BYTES
leaves a CU one workgroup; that is where 1024 threads would raise the waves per SIMD.  The
figures are read from the sources here, in the way tests/test_k1_edges_source.py reads the
window's, and the edge recomputed for every window size."""
import os
import re

from test_k1_edges_source import CSRC, _code, _source_constants


def _lds_bytes_figures():
    kk = _code("esc_kernels.hip")
    m = re.search(r"constexpr size_t k1_lds_bytes\(uint32_t gw\)\s*\{\s*return k1_reps\(gw\) > 1 \? \(size_t\)k1_reps\(gw\) \* "
                  r"k1_copy_words\(gw\) \* (\d+)\s*: \(size_t\)\(gw \+ FC_COL - 1\) / FC_COL \* FC_COL \* (\d+) \* "
                  r"sizeof\(uint64_t\);", kk)
    assert m, "k1_lds_bytes is no longer 'copies * copy words * 8, or whole columns * 2 * 8'"
    return int(m.group(1)), int(m.group(2))


def test_one_workgroup_per_cu_edge_from_the_sources():
    import test_gpu_k1_width as T
    c = _source_constants()
    copy_word_bytes, halves = _lds_bytes_figures()
    assert (copy_word_bytes, halves) == (8, 2)

    def lds(gw):                                        # k1_lds_bytes from the sources' figures alone
        a, b = c["copy_words"]
        cols = (gw + c["fc_col"] - 1) // c["fc_col"] * c["fc_col"]
        words = cols * a + b
        reps = c["reps"] if words * c["word_bytes"] * c["reps"] <= c["rep_lds"] else 1
        return reps * words * copy_word_bytes if reps > 1 else cols * halves * 8

    def per_cu(gw):
        return c["lds_bytes"] // lds(gw)

    W = c["window"]
    assert all(lds(gw) <= c["lds_bytes"] for gw in range(1, W + 1)) and lds(W) == c["lds_bytes"]
    edge = max(gw for gw in range(1, W + 1) if per_cu(gw) >= 2)
    # one edge: two or more workgroups a CU up to it, one from there to the full window
    assert all((per_cu(gw) >= 2) == (gw <= edge) for gw in range(1, W + 1))
    assert edge == T.SWITCH_S == 5_120 and lds(edge) * 2 == c["lds_bytes"]
    # a window with LDS copies is never alone on its CU
    assert c["rep_lds"] <= c["lds_bytes"] // 2
    assert {edge, edge + 1, W, W + 1} == set(T.MIX_S) and set(T.PATH_S) == {edge + 1, W + 1}
    assert [gw for _, gw in T.windows(W + 1)] == [W, 1] and per_cu(1) >= 2


def test_product_runs_512_threads_and_the_width_knob_is_measurement_only():
    rt, kk = _code("esc_runtime.hip"), _code("esc_kernels.hip")
    assert re.search(r"c->k1_variant, c->k1_threads \? c->k1_threads : 512,", rt), "launch_k1 no longer asks for 512 threads"
    assert re.search(r"#else\s*#define ESC_K1W\(A, DC\) ESC_K1\(512, A, DC\)\s*#endif", kk), \
        "the product library's K1 launcher no longer instantiates 512 threads alone"
    assert len(re.findall(r"ESC_K1\(1024,", kk)) == 1 and \
        re.search(r"#if ESC_MEASURE\s*#define ESC_K1W\(A, DC\)[^#]*ESC_K1\(1024, A, DC\)[^#]*#else", kk)
    # ESC_K1_THREADS is read inside an ESC_MEASURE block, next to ESC_K1_VARIANT
    src = open(os.path.join(CSRC, "esc_runtime.hip")).read()
    assert src.count('getenv("ESC_K1_THREADS")') == 1
    at = src.index('getenv("ESC_K1_THREADS")')
    assert src[:at].rfind("#if ESC_MEASURE") > src[:at].rfind("#endif")
    assert 0 < at - src.index('getenv("ESC_K1_VARIANT")') < 300
