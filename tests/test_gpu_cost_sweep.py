"""towr_cost_kernel and towr_traj_kernel (cost_traj.hip) on swept formulation shapes: COST_GPU_SEEDS of
tests/test_cost_sweep.py (shape_sweep.make_with_costs: which cost kinds, weights, torque weight and cost sample periods,
on shapes whose polynomial counts, durations and phase layouts vary, feet that start in flight or never touch down
among them) and the four built shapes either side of kCostSlotMax (configs.anymal_trot_slot_limit). The CPU file checks
the same descriptions through the host emulation first and asserts what the seed list reaches; DESIGN.md "Cost sweep"
has the table. Only the cost and trajectory entries are called."""
import numpy as np
import pytest

from oracle.oracle import Oracle
from tests.gpu_helpers import _assert_row_bits, _eval, _ldx, _nan, _np_bits, _padded, _rows
from tests.parity import ABS, REL, assert_cost_close
from tests.test_cost_sweep import COST_GPU_SEEDS, SLOT_LIMIT, contact_col, cost_case, instantiation
from towr2025_amd import TowrGpuProblem

pytestmark = pytest.mark.gpu

B_COST = 5
TRAJ_RTOL = TRAJ_ATOL = 1e-10     # tests/test_trajectory.py's device gate


def _cost_ratio(f_ref, f, g_ref, g):
    """Largest |err| / tolerance of assert_cost_close's two comparisons (for the record; the assertion is its own)."""
    rf = abs(f - f_ref) / (REL * max(abs(f), abs(f_ref)) + ABS * max(1.0, abs(f_ref)))
    tol = REL * np.maximum(np.abs(g_ref), np.abs(g)) + ABS * max(1.0, float(np.abs(g_ref).max(initial=0.0)))
    return rf, float(np.max(np.abs(g - g_ref) / tol, initial=0.0))


@pytest.mark.parametrize("case", COST_GPU_SEEDS + sorted(SLOT_LIMIT))
def test_objective_on_swept_shapes(case):
    """B = 5 rows x0 + 0.03 N(0, 1) with an odd ldx, ldgrad = n + 3 and NaN-prefilled outputs, at grid 2 (trips 3 and 2:
    both blocks loop, and with the odd ldx alternate between XStage's aligned and unaligned paths) and at the automatic
    grid (one trip per block). Every row: within assert_cost_close of the oracle, bit-equal to eval_f / eval_grad_f,
    bit-equal between the two grids, the f-only call's F bit-equal, the padding still NaN."""
    desc, info = cost_case(case)
    o = Oracle(desc)
    p = TowrGpuProblem(desc, device=0)
    n, B = p.n, B_COST
    assert n == o.n
    X = _rows(o.initial_x(), B, 9400)
    Xd = _padded(X, _ldx(n))
    auto = (p.cost_grid(False), p.cost_grid(True))
    outs = {}
    for grid in (2, 0):
        p.set_cost_grid(grid)
        Fh, Gh = _eval(p, Xd)
        F0 = _eval(p, Xd, grad=False)
        assert np.isnan(Gh[:, n:]).all(), f"{case} grid {grid}: gradient padding written"
        assert np.array_equal(_np_bits(F0), _np_bits(Fh)), f"{case} grid {grid}: the f-only call's F differs"
        outs[grid] = (Fh, Gh[:, :n])
    p.set_cost_grid(0)
    Fh, Gh = outs[2]
    ref = [(o.eval_f(X[b]), o.eval_grad_f(X[b])) for b in range(B)]
    worst = np.max([_cost_ratio(ref[b][0], Fh[b], ref[b][1], Gh[b]) for b in range(B)], axis=0)
    print(f"{case}: n {n} <{', '.join(instantiation(desc))}> automatic grids f-only {auto[0]} gradient {auto[1]}, "
          f"largest |err| / tolerance f {worst[0]:.3g} gradient {worst[1]:.3g}")
    for b in range(B):
        assert_cost_close(ref[b][0], Fh[b], ref[b][1], Gh[b], f"{case} row {b} vs the oracle")
        _assert_row_bits(f"{case} grid 2 vs eval_f / eval_grad_f", Fh, Gh, b, (p.eval_f(X[b]), p.eval_grad_f(X[b])), n)
        _assert_row_bits(f"{case} automatic grid vs grid 2", outs[0][0], outs[0][1], b, (Fh[b], Gh[b]), n)
    p.close()


def _sample_periods(p):
    """Three sample periods by their sample counts (trajectory_size; the kernel takes 64 samples per block): a multiple
    of 64 (a full last block), 1 modulo 64 (a last block of one sample) and one that needs at least three blocks."""
    T = (p.trajectory_size(1e-3)[0] - 1) * 1e-3     # the horizon to within a sample of 1 ms
    want = {"full last block": lambda ns: ns % 64 == 0, "last block of one": lambda ns: ns % 64 == 1,
            "three blocks": lambda ns: ns > 128 and ns % 64 not in (0, 1)}
    out = {}
    for tag, ok in want.items():
        for k in range(60, 260):
            dt = T / (k + 0.5)
            if dt not in out.values() and ok(p.trajectory_size(dt)[0]):
                out[tag] = dt
                break
    assert len(out) == 3, f"no sample period found for {set(want) - set(out)}"
    return out


@pytest.mark.parametrize("seed", COST_GPU_SEEDS)
def test_trajectory_on_swept_shapes(seed):
    """sample_trajectory against the oracle (test_trajectory.py's 1e-10 gate) at three sample periods whose sample
    counts are 0 and 1 modulo the block's 64 samples and more than two blocks; the is_contact_phase columns (feet that
    start in flight, TrajPhases::c0 = 0, and feet that never touch down among them) for equality; a device batch of 3
    with an odd ldx into a NaN-padded ldo bit-equal to the single calls, the padding untouched."""
    import torch
    desc, info = cost_case(seed)
    o = Oracle(desc)
    p = TowrGpuProblem(desc, device=0)
    n, E = p.n, desc.robot.n_ee
    X = _rows(o.initial_x(), 3, 9500)
    Xd = _padded(X, _ldx(n))
    periods = _sample_periods(p)
    counts = {tag: p.trajectory_size(dt)[0] for tag, dt in periods.items()}
    assert counts["full last block"] % 64 == 0 and counts["last block of one"] % 64 == 1 and counts["three blocks"] > 128
    worst = 0.0
    for tag, dt in periods.items():
        ns, nc = p.trajectory_size(dt)
        assert nc == 19 + 25 * E
        single = []
        for b in range(3):
            ref = o.sample_trajectory(X[b], dt)
            got = p.sample_trajectory(X[b], dt)
            assert got.shape == ref.shape == (ns, nc)
            err = np.abs(got - ref) / (TRAJ_ATOL + TRAJ_RTOL * np.abs(ref))
            worst = max(worst, float(err.max()))
            np.testing.assert_allclose(got, ref, rtol=TRAJ_RTOL, atol=TRAJ_ATOL, err_msg=f"seed {seed} {tag} row {b}")
            for ee in range(E):
                np.testing.assert_array_equal(got[:, contact_col(ee)], ref[:, contact_col(ee)], err_msg=f"seed {seed} {tag} foot {ee}")
            single.append(got)
        OUT = _nan(3, ns * nc + 7)
        p.sample_trajectory_batch_device(Xd, dt, OUT)
        torch.cuda.synchronize()
        out = OUT.cpu().numpy()
        assert np.isnan(out[:, ns * nc:]).all(), f"seed {seed} {tag}: write past the rows"
        for b in range(3):
            assert np.array_equal(_np_bits(out[b, :ns * nc]), _np_bits(single[b].ravel())), f"seed {seed} {tag}: batch row {b}"
    print(f"seed {seed}: samples {counts}, largest |err| / tolerance {worst:.3g}")
    p.close()
