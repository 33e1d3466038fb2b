"""Helpers the GPU tests of the batched solver-step entry points share (test_gpu_jac_products, test_gpu_residual,
test_gpu_step, test_gpu_lbfgs): device operands with NaN padding, bit comparisons, and the formulations / batch
terrains of the configurations they use; the batch set-up of the objective kernel's tests (test_gpu_cost_loop,
test_gpu_cost_sweep: _rows, _ldx, _eval, _clean_rows, _assert_row_bits); and the Jacobian products'
extended-precision reference with its a-priori dot-product gate (_reference, _check_products: tests/test_gpu_jac_products.py has the derivation), shared with the CPU
tests of the product tables and the swept-shape consumer tests. torch is imported where it is used, so the module
imports without it."""
import math

import numpy as np

from towr2025_amd import _capi as capi
from towr2025_amd import formulation as F

U = 2.0 ** -53
EXT = np.finfo(np.longdouble).nmant > 52


def _dev():
    import torch
    return torch.device("cuda:0")


def _nan(rows, cols):
    import torch
    return torch.full((rows, cols), float("nan"), dtype=torch.float64, device=_dev())


def _padded(a, ld):
    """host (B, k) array -> device (B, ld) tensor, NaN beyond column k"""
    import torch
    t = _nan(a.shape[0], ld)
    t[:, :a.shape[1]] = torch.from_numpy(np.ascontiguousarray(a)).to(_dev())
    return t


def _vec(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to(_dev())


def _bits(t):
    import torch
    return t.contiguous().view(torch.int64)


def _same_bits(a, b):
    import torch
    return torch.equal(_bits(a), _bits(b))


def _np_bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _rows(x0, B, seed0):
    return np.stack([x0 + 0.03 * np.random.default_rng(seed0 + b).standard_normal(len(x0)) for b in range(B)])


def _ldx(n):
    return n + 1 if n % 2 == 0 else n


def _eval(p, Xd, grad=True):
    """One eval_cost_batch_device into NaN-prefilled outputs: host (F, GRAD with its padding) or F alone."""
    import torch
    B = Xd.shape[0]
    Fd = _nan(1, B)[0]
    Gd = _nan(B, p.n + 3) if grad else None
    p.eval_cost_batch_device(Xd, Fd, Gd)
    torch.cuda.synchronize()
    return (Fd.cpu().numpy(), Gd.cpu().numpy()) if grad else Fd.cpu().numpy()


def _clean_rows(p, X, rows=None):
    """{b: (F, gradient)} of the clean reference rows: row b copied to a fresh (aligned) one-row tensor and evaluated at
    B = 1. Call it with the cost-grid override off."""
    import torch
    assert X.shape[1] == p.n
    out = {}
    for b in (range(len(X)) if rows is None else rows):
        xd = torch.from_numpy(np.ascontiguousarray(X[b:b + 1])).to("cuda:0")
        assert xd.data_ptr() % 16 == 0
        Fh, Gh = _eval(p, xd)
        assert np.isnan(Gh[:, p.n:]).all()
        assert np.isfinite(Fh[0]) and np.isfinite(Gh[0, :p.n]).all(), f"clean reference row {b} is not finite"
        out[b] = (Fh[0], Gh[0, :p.n].copy())
    return out


def _assert_row_bits(tag, Fh, Gh, b, ref, n):
    f, g = ref
    assert _np_bits(Fh[b:b + 1])[0] == _np_bits(np.array([f]))[0], f"{tag}: F[{b}] {Fh[b]!r} != {f!r}"
    diff = np.flatnonzero(_np_bits(Gh[b, :n]) != _np_bits(g))
    assert diff.size == 0, f"{tag}: row {b} differs in {diff.size} gradient columns, first {diff[0]}: {Gh[b, diff[0]]!r} != {g[diff[0]]!r}"


def _formulation(name):
    """The formulation of a configuration of tests/configs.py and the arguments of its var_bounds_data()."""
    if name == "monoped_procedural":
        f, vs, cs, goal, T = F.procedural_monoped()
        return f, dict(varsets=vs, init_mode=capi.INIT_PROCEDURAL, ee_goal=goal, total_time=T)
    f = {"anymal_trot_2p4s": lambda: F.anymal_trot(),
         "anymal_stairs_gaitopt": lambda: F.anymal_trot(terrain=F.HeightMap.MakeTerrain(F.HeightMap.StairsID), optimize_timings=True)}[name]()
    f.params_.enable_stance_tracking = False
    return f, {}


def _terrains(name, B, rng):
    out = []
    for b in range(B):
        if name == "anymal_all_costs" and b % 2:
            t = F.HeightMap.Flat(rng.uniform(0, 0.3))
        else:
            t = F.HeightMap(F.HeightMap.StairsID, (rng.uniform(0.8, 1.4), 0.4, rng.uniform(0.1, 0.25), rng.uniform(0.1, 0.25), 1.0))
        out.append(t.to_c())
    return out


def _segment_sums(terms, ptr):
    """Sums of terms[ptr[i]:ptr[i+1]]: in extended precision where long double has more than 53 bits (not yet
    rounded to double), else math.fsum per segment; empty segments give 0."""
    out = np.zeros(len(ptr) - 1, dtype=np.longdouble if EXT else np.float64)
    nz = np.flatnonzero(np.diff(ptr) > 0)
    if nz.size and EXT:
        out[nz] = np.add.reduceat(terms, ptr[:-1][nz])
    for i in (() if EXT else nz):
        out[i] = math.fsum(terms[ptr[i]:ptr[i + 1]])
    return out


def _reference(p, V, P, LAM):
    """Per output of host arrays V (B, nnz), P (B, n), LAM (B, m): (Y_ref, tol_Y, Z_ref before rounding, S_Z, k_Z,
    gamma) from the engine's own V, jac_csr() and the vectors."""
    rp, col = p.jac_csr()
    cp, row, idx = p.jac_csc()
    B = V.shape[0]
    ft = np.longdouble if EXT else np.float64
    kY, kZ = np.diff(rp).astype(np.float64), np.diff(cp).astype(np.float64)
    Y, SY, Z, SZ = (np.zeros((B, p.m), ft), np.zeros((B, p.m), ft), np.zeros((B, p.n), ft), np.zeros((B, p.n), ft))
    for b in range(B):
        ty = V[b].astype(ft) * P[b][col].astype(ft)
        tz = (V[b].astype(ft) * LAM[b][np.repeat(np.arange(p.m), np.diff(rp))].astype(ft))[idx]
        assert np.array_equal(row, np.repeat(np.arange(p.m), np.diff(rp))[idx])
        Y[b], SY[b] = _segment_sums(ty, rp), _segment_sums(np.abs(ty), rp)
        Z[b], SZ[b] = _segment_sums(tz, cp), _segment_sums(np.abs(tz), cp)
    gam = lambda k: k * U / (1 - k * U)
    return Y.astype(np.float64), 2 * gam(kY) * SY.astype(np.float64), Z, SZ.astype(np.float64), kZ, gam


def _check_products(tag, p, Yd, Zd, Zad, Z0, ref):
    Y_ref, tolY, Z_ref, SZ, kZ, gam = ref
    Y, Z, Za = Yd.cpu().numpy(), Zd.cpu().numpy(), Zad.cpu().numpy()
    assert np.isnan(Y[:, p.m:]).all() and np.isnan(Z[:, p.n:]).all() and np.isnan(Za[:, p.n:]).all(), f"{tag}: padding written"
    Y, Z, Za = Y[:, :p.m], Z[:, :p.n], Za[:, :p.n]
    tolZ = 2 * gam(kZ) * SZ
    tolZa = 2 * gam(kZ + 1) * (SZ + np.abs(Z0))
    eY, eZ = np.abs(Y - Y_ref), np.abs(Z - Z_ref.astype(np.float64))
    eZa = np.abs(Za - (Z_ref + Z0).astype(np.float64))   # (the pre-filled Z joins the sum before the one rounding)
    worst = max(np.max(np.where(tolY > 0, eY / np.where(tolY > 0, tolY, 1), 0), initial=0.0),
                np.max(np.where(tolZ > 0, eZ / np.where(tolZ > 0, tolZ, 1), 0), initial=0.0),
                np.max(np.where(kZ > 0, eZa / np.where(tolZa > 0, tolZa, 1), 0), initial=0.0))
    print(f"{tag}: largest |err| / bound {worst:.3f}")
    assert (eY <= tolY).all() and (eZ <= tolZ).all(), f"{tag}: outside the dot-product bound ({worst:.3f})"
    assert (eZa <= tolZa)[:, kZ > 0].all(), f"{tag}: accumulate outside the bound ({worst:.3f})"
    rp, _ = p.jac_csr()
    empty_r, empty_c = np.diff(rp) == 0, kZ == 0
    assert (Y[:, empty_r] == 0.0).all() and not np.signbit(Y[:, empty_r]).any(), f"{tag}: empty rows are not 0.0"
    assert (Z[:, empty_c] == 0.0).all(), f"{tag}: empty columns are not 0.0"
    assert np.array_equal(Za[:, empty_c].view(np.int64), Z0[:, empty_c].view(np.int64)), f"{tag}: accumulate touched an empty column"
