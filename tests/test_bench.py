"""bench.py's command line: a plain run prints the headline alone, --full adds the roofline and the legs,
--dump-outputs writes the last timed step's g and Jacobian values (a fixed seeded sample of the problems
when the batch is larger than the size limit)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import bench

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADLINE = ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step", "steps", "warmup")
B, STEPS = 40, 3


def test_dump_rows_keeps_everything_that_fits():
    np.testing.assert_array_equal(bench.dump_rows(7, 100, limit=700), np.arange(7))


def test_dump_rows_sample_is_fixed_sorted_and_within_the_limit():
    rows = bench.dump_rows(4096, 8 * (3238 + 28144))
    assert len(rows) == bench.DUMP_BYTES // (8 * (3238 + 28144)) == 238
    assert len(rows) * 8 * (3238 + 28144) <= 64 * 1000 * 1000
    assert (np.diff(rows) > 0).all() and rows[0] >= 0 and rows[-1] < 4096
    np.testing.assert_array_equal(rows, bench.dump_rows(4096, 8 * (3238 + 28144)))
    assert len(bench.dump_rows(5, 100, limit=50)) == 1   # never empty


def test_dump_outputs_strips_the_padding(tmp_path):
    m, nnz, ldg, ldv = 5, 19, 16, 32
    rng = np.random.default_rng(1)
    G, V = rng.standard_normal((9, ldg)), rng.standard_normal((9, ldv))
    assert bench.dump_outputs(str(tmp_path / "a"), G, V, m, nnz) == 9
    g, v = np.load(tmp_path / "a" / "g.npy"), np.load(tmp_path / "a" / "jac_values.npy")
    assert g.dtype == v.dtype == np.float64
    np.testing.assert_array_equal(g, G[:, :m])
    np.testing.assert_array_equal(v, V[:, :nnz])
    limit = 4 * 8 * (m + nnz)
    rows = bench.dump_rows(9, 8 * (m + nnz), limit)
    assert bench.dump_outputs(str(tmp_path / "b"), G, V, m, nnz, rank=1, limit=limit) == 4 == len(rows)
    np.testing.assert_array_equal(np.load(tmp_path / "b" / "g_rank1.npy"), G[rows, :m])
    assert sorted(os.listdir(tmp_path / "b")) == ["g_rank1.npy", "jac_values_rank1.npy"]


def _run_bench(*extra):
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(STEPS), "--warmup", "1",
           "--settle-ms", "0", "--batch", str(B)] + list(extra)
    out = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1
    return json.loads(lines[0])


@pytest.mark.gpu
def test_plain_run_prints_the_headline_and_dumps_the_last_step(tmp_path):
    import torch
    from tests.parity import assert_close
    from oracle.oracle import Oracle
    from towr2025_amd import TowrGpuProblem
    from towr2025_amd import formulation as F
    j = _run_bench("--dump-outputs", str(tmp_path))
    for k in HEADLINE:
        assert k in j, k
    assert j["steps"] == STEPS and j["unit"] == "calls/s" and j["dtype"] == "f64" and j["higher_is_better"] is True
    assert j["value"] == pytest.approx(B * STEPS / (j["ms_per_step"] * STEPS * 1e-3))
    for k in ("roofline", "objective", "gait_optimization", "rotvec", "host_batch", "single_call", "cpu_baseline"):
        assert k not in j, f"{k} belongs to --full"
    assert sorted(os.listdir(tmp_path)) == ["g.npy", "jac_values.npy"]
    g, v = np.load(tmp_path / "g.npy"), np.load(tmp_path / "jac_values.npy")
    # the same evaluation made here: the batch of the bench, the x set of its last timed step
    desc = F.anymal_trot().to_desc()
    p = TowrGpuProblem(desc)
    Xh, terrains = bench.make_batch(p, B, first_id=0)
    p.set_batch_terrain(terrains)
    k = (STEPS - 1) % bench.N_X
    dev = torch.device("cuda:0")
    G = torch.zeros((B, p.m), dtype=torch.float64, device=dev)
    V = torch.zeros((B, p.nnz), dtype=torch.float64, device=dev)
    p.eval_batch_device(torch.from_numpy(np.ascontiguousarray(Xh[k])).to(dev), G, V)
    torch.cuda.synchronize()
    assert g.shape == (B, p.m) and v.shape == (B, p.nnz) and g.dtype == v.dtype == np.float64
    np.testing.assert_array_equal(g, G.cpu().numpy())
    np.testing.assert_array_equal(v, V.cpu().numpy())
    p.close()
    for b in (0, B - 1):
        desc.terrain = terrains[b]
        o = Oracle(desc)
        r, _, v_ref = o.eval_jac(Xh[k, b])
        assert_close(o.eval_g(Xh[k, b]), g[b], r, v_ref, v[b], o.m, f"dumped problem {b}")


@pytest.mark.gpu
def test_full_run_adds_the_roofline_and_the_selected_legs():
    j = _run_bench("--full", "--no-cpu", "--no-host", "--no-gait", "--legs", "objective")
    for k in HEADLINE + ("roofline", "objective"):
        assert k in j, k
    assert j["roofline"]["kernel"] in j["roofline"]["kernels"]
    assert "cpu_baseline" not in j and "host_batch" not in j and "rotvec" not in j
