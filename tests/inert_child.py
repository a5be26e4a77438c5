"""Child process of tests/test_gpu_inert.py on the MEASUREMENT library (ESC_LIB_PATH =
escalator_amd/libescalator_hip_measure.so) with ESC_K1_VARIANT=7: K1 without a work plan, the
equal-weight walk over the class table, on the cluster of tests/inert_cases.py.  The inert classes
lie behind the walk's last weight, so no workgroup's range reaches them.  Prints one JSON line."""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

import numpy as np  # noqa: E402

import escalator_amd as esc  # noqa: E402
import inert_cases as IC  # noqa: E402
from escalator_amd import layout  # noqa: E402
from oracle import soa  # noqa: E402


def main():
    assert os.environ.get("ESC_K1_VARIANT") == "7"
    soa.build()
    out = {}
    for with_default in (False, True):
        groups = IC.groups(with_default)
        pods, _, _ = IC.pods()
        nodes, states = IC.nodes(), IC.states(len(groups))
        ctx = esc.Context(groups)
        ctx.set_spare(0.25)
        P, N = ctx.pack(pods, nodes)
        ctx.load(P, N)
        tot, dec = ctx.decide_all(states)
        otot = soa.totals(P, N, groups)
        odf, odi = soa.decide(groups, states, otot)
        ok = all(np.array_equal(tot[n], otot[:, k]) for k, n in enumerate(soa.TOT_FIELDS[:12]))
        ok &= np.array_equal(dec["cpu_pct"].view(np.uint64), odf[:, 0].view(np.uint64))
        ok &= np.array_equal(dec["mem_pct"].view(np.uint64), odf[:, 1].view(np.uint64))
        ok &= np.array_equal(dec["delta"], odi[:, 0]) and np.array_equal(dec["n_to_taint"], odi[:, 1])
        entries, full = ctx.k1_flush_entries()
        n_gp = ctx.lib.esc_ctx_num_group_pairs(ctx.handle)
        out["default" if with_default else "no_default"] = {
            "exact": bool(ok), "entries": entries, "full": full, "counted": int(tot["n_pods"].sum()),
            "bytes": ctx.stream_bytes()[0], "layout_bytes": layout.pod_bytes(P, n_gp),
            "plan_words_zero": bool((ctx.k1_trace()[:, 6:8] == 0).all())}
        ctx.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
