"""GPU: the benchmark's command line.  A plain run prints the headline line alone and times
exactly --steps steps; --dump-outputs writes the last timed step's decision, checked here
against the C oracle over the same seeded snapshot; --full adds the parity check and the
per-kernel figures."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from oracle import soa

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PODS, NODES, GROUPS = 300_001, 10_000, 100          # config 2 with its pod count overridden
HEADLINE = {"metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling",
            "vs_baseline", "dtype", "data", "config"}


def run_bench(*extra):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--config", "2", "--pods",
                        str(PODS), "--steps", "3", "--warmup", "1", *extra], capture_output=True, text=True,
                       timeout=240, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [x for x in r.stdout.splitlines() if x.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    return json.loads(lines[0])


def test_plain_run_prints_the_headline_and_dumps_the_decision(tmp_path):
    import escalator_amd as esc
    out = run_bench("--dump-outputs", str(tmp_path / "dump"))
    assert set(out) == HEADLINE, sorted(set(out) ^ HEADLINE)
    assert out["steps"] == 3 and out["warmup"] == 1 and out["n_gpus"] == 1
    assert out["unit"] == "records/s" and out["higher_is_better"] is True and out["dtype"] == "int64"
    assert out["ms_per_step"] > 0
    assert out["value"] == pytest.approx((PODS + NODES) / (out["ms_per_step"] * 1e-3), rel=1e-9)
    got = {f[:-4]: np.load(tmp_path / "dump" / f) for f in sorted(os.listdir(tmp_path / "dump"))}
    assert all(a.dtype == np.float64 for a in got.values())
    assert sum(a.nbytes for a in got.values()) <= 64 << 20
    s = esc.Synth(PODS, NODES, GROUPS, config=2, seed=0xE5CA1A7E00000002, threads=16)
    otot = soa.totals(s.pods(), s.nodes(), s.groups)
    odf, odi = soa.decide(s.groups, s.states, otot)
    for k, name in enumerate(soa.TOT_FIELDS[:12]):
        assert np.array_equal(got["totals_" + name], otot[:, k].astype(np.float64)), name
    assert np.array_equal(got["decision_cpu_pct"].view(np.uint64), odf[:, 0].view(np.uint64))
    assert np.array_equal(got["decision_mem_pct"].view(np.uint64), odf[:, 1].view(np.uint64))
    for k, name in enumerate(["delta", "n_to_taint", "cached_cpu_m", "cached_mem_b", "status", "branch",
                              "taint_status"]):
        assert np.array_equal(got["decision_" + name], odi[:, k].astype(np.float64)), name
    # the selections delivered with the decision: one list per walking group, inside the node table
    which, off, idx = got["selection_which"], got["selection_offsets"], got["selection_nodes"]
    assert len(which) == GROUPS and len(off) == GROUPS + 1 and off[0] == 0 and off[-1] == len(idx)
    assert np.all(np.diff(off) >= 0) and np.all((idx >= 0) & (idx < NODES))
    assert np.all(np.diff(off)[which < 0] == 0)


def test_full_run_adds_parity_and_kernel_figures():
    out = run_bench("--full", "--no-cpu-baseline", "--no-host")
    assert HEADLINE < set(out)
    assert out["steps"] == 3 and out["parity"].startswith("bit-exact vs C oracle")
    assert out["roofline"]["kernel"] == "k_pod_reduce" and out["roofline"]["launch_ms"] > 0
    assert out["stage_ms"]["k_pod_reduce"] > 0 and out["run_once"]["ms"] > 0
