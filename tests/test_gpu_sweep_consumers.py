"""The solver-step consumers (jprod.hip, resid.hip, step.hip, lbfgs.hip and the fused entries of auglag.hip) on shapes of
the seeded sweep (tests/shape_sweep.py) instead of the parity configurations' default shape: hundreds of empty rows
(194, 39, 66), empty constraint sets in the middle of the row table (175: 4, 126: 3), a pattern smaller than one
2048-entry chunk (154), fewer columns than a block has lanes (196: n = 78), the largest n (93: 1173, odd), the record
path and its tile-path fallbacks (13, 131, 126, 10, 0). B = 3, padded leading dimensions with NaN padding.

No tolerance of its own: the gates are those of tests/test_gpu_jac_products.py (tests/gpu_helpers.py),
tests/test_gpu_residual.py, tests/test_gpu_step.py and tests/test_gpu_lbfgs.py, and bit-equality. The products' bits
are also compared with the host walk of the product tables (tests/host_emu/emu.hip emu_jac_products): jprod.hip
promises one fixed tree of additions per output, and the walk is that tree."""
import functools

import numpy as np
import pytest

from tests import jp_emu
from tests import test_gpu_lbfgs as LB
from tests import test_gpu_residual as RES
from tests import test_gpu_step as STEP
from tests.gpu_helpers import _check_products, _nan, _np_bits, _padded, _reference, _same_bits, _vec
from tests.shape_sweep import make
from towr2025_amd import TowrGpuProblem

pytestmark = pytest.mark.gpu

CONSUMER_SEEDS = [154, 196, 16, 194, 13, 131, 126, 10, 0, 93, 39, 175, 66]
LBFGS_SEEDS = [196, 93]   # n = 78: fewer columns than one wave pair; n = 1173: the largest, odd
B = 3


def _lds(p):
    return (p.nnz + 15) // 16 * 16 + 16, p.m + 5, p.n + 3   # ldv, ldy, ldz


@functools.lru_cache(maxsize=None)
def _case(seed):
    """The seed's handle, its own g and Jacobian values at x0 and two seeded perturbations, standard-normal P / LAM / Z0
    and the separate product calls' outputs."""
    import torch
    desc = make(seed)[0].to_desc()
    p = TowrGpuProblem(desc, device=0)
    ldv, ldy, ldz = _lds(p)
    x0 = p.initial_x()
    X = np.stack([x0 + (0.05 * np.random.default_rng(7000 + 10 * seed + b).standard_normal(p.n) if b else 0.0) for b in range(B)])
    rng = np.random.default_rng(20261020 + seed)
    P, LAM, Z0 = rng.standard_normal((B, p.n)), rng.standard_normal((B, p.m)), rng.standard_normal((B, p.n))
    Xd, Pd, LAMd = _padded(X, p.n + 1), _padded(P, p.n + 7), _padded(LAM, p.m + 9)
    Gd, Vd = _nan(B, p.m + 2), _nan(B, ldv)
    p.eval_batch_device(Xd, Gd, Vd)
    Yd, Zd, Zad = _nan(B, ldy), _nan(B, ldz), _padded(Z0, ldz)
    p.jac_vec_batch_device(Vd, Pd, Yd)
    p.jac_tvec_batch_device(Vd, LAMd, Zd)
    p.jac_tvec_batch_device(Vd, LAMd, Zad, accumulate=True)
    torch.cuda.synchronize()
    V = Vd.cpu().numpy()[:, :p.nnz].copy()
    assert np.isfinite(V).all() and np.isnan(Vd.cpu().numpy()[:, p.nnz:]).all()
    info = p.constraint_info()
    return dict(p=p, desc=desc, X=X, P=P, LAM=LAM, Z0=Z0, Xd=Xd, Pd=Pd, LAMd=LAMd, Gd=Gd, Vd=Vd, Yd=Yd, Zd=Zd, Zad=Zad, V=V,
                info=info, row0=[r0 for _, _, r0, _ in info] + [p.m], ns=desc.n_constraints)


@pytest.mark.parametrize("seed", CONSUMER_SEEDS)
def test_products(seed):
    """jac_vec, jac_tvec and accumulate on the engine's own V: within the dot-product bound, bit-equal to the host walk
    of the tables, and the fused chunked entry bit-identical to them for chunks of 1, 2 and the automatic size."""
    import torch
    c = _case(seed)
    p = c["p"]
    ldv, ldy, ldz = _lds(p)
    _check_products(f"seed {seed}", p, c["Yd"], c["Zd"], c["Zad"], c["Z0"], _reference(p, c["V"], c["P"], c["LAM"]))
    Y, Z, Za = jp_emu.products(c["desc"], c["V"], c["P"], c["LAM"], c["Z0"])
    for got, want, what in ((c["Yd"], Y, "J p"), (c["Zd"], Z, "J^T lam"), (c["Zad"], Za, "J^T lam accumulated")):
        np.testing.assert_array_equal(_np_bits(got.cpu().numpy()[:, :want.shape[1]]), _np_bits(want),
                                      err_msg=f"seed {seed}: {what} is not the tables' tree of additions")
    try:
        for k in (1, 2, 0):
            p.set_products_chunk(k)
            G, Yk, Zk, Zak = _nan(B, p.m + 2), _nan(B, ldy), _nan(B, ldz), _padded(c["Z0"], ldz)
            p.eval_products_batch_device(c["Xd"], G=G, LAM=c["LAMd"], Z=Zk, P=c["Pd"], Y=Yk)
            p.eval_products_batch_device(c["Xd"], LAM=c["LAMd"], Z=Zak, accumulate=True)
            torch.cuda.synchronize()
            assert _same_bits(G, c["Gd"]) and _same_bits(Yk, c["Yd"]), f"seed {seed} chunk {k}: G / Y differ from the separate calls"
            assert _same_bits(Zk, c["Zd"]) and _same_bits(Zak, c["Zad"]), f"seed {seed} chunk {k}: Z differs from the separate calls"
    finally:
        p.set_products_chunk(0)


def _drawn_g(lo, up, rng):
    """G (B, m) around the bounds: a third of the rows sit exactly on a bound (or on the middle of a two-sided row) and
    are satisfied, the others are spread to either side by more than the bounds' width."""
    has_l, has_u = lo > -1e19, up < 1e19
    base = np.where(has_l & has_u, 0.5 * (lo + up), np.where(has_l, lo, np.where(has_u, up, 0.0)))
    spread = 1.0 + np.where(has_l & has_u, up - lo, 0.0)
    G = base + spread * rng.standard_normal((B, lo.size))
    return np.where(rng.random((B, lo.size)) < 1 / 3, base, G)


@pytest.mark.parametrize("seed", CONSUMER_SEEDS)
def test_residual_and_multipliers(seed):
    """The handle's bounds, G drawn so that every sign class is both violated and satisfied: SUM and LAMP
    against the numpy reference of tests/test_gpu_residual.py; an empty set's maximum is +0.0."""
    import torch
    c = _case(seed)
    p, ns, row0, LAM = c["p"], c["ns"], c["row0"], c["LAM"]
    lo, up = p.constraint_bounds()
    G = _drawn_g(lo, up, np.random.default_rng(31 + seed))
    v = RES.reference(G, lo, up, None, 1.0, row0)["v"]
    classes = {"lower-only": (lo > -1e19) & ~(up < 1e19), "upper-only": ~(lo > -1e19) & (up < 1e19),
               "two-sided": (lo > -1e19) & (up < 1e19) & (lo < up), "equality": lo == up}
    for what, rows in classes.items():   # (every shape of the list has all four)
        assert rows.any() and (v[:, rows] > 0).any() and (v[:, rows] == 0).any(), f"seed {seed}: {what} rows are not both violated and satisfied"
    Gd = _padded(G, p.m + 2)
    empty = [s for s, (_, _, _, rows) in enumerate(c["info"]) if rows == 0]
    for rho in RES.RHOS:
        SUM, LAMP = _nan(B, 4 + ns + 3), _nan(B, p.m + 5)
        p.residual_batch_device(Gd, SUM, LAM=c["LAMd"], rho=rho, LAMP=LAMP)
        SUMs = _nan(B, 4 + ns + 1)
        p.residual_batch_device(Gd, SUMs)
        torch.cuda.synchronize()
        RES.check(f"seed {seed} rho={rho:g}", p, SUM, LAMP, RES.reference(G, lo, up, LAM, rho, row0), G, LAM, rho, row0)
        RES.check(f"seed {seed} summary", p, SUMs, None, RES.reference(G, lo, up, None, 1.0, row0), G, None, 1.0, row0)
        S = SUM.cpu().numpy()
        for s in empty:
            assert (_np_bits(S[:, 4 + s]) == 0).all(), f"seed {seed}: the maximum of empty set {s} is not +0.0"
    assert np.isnan(Gd.cpu().numpy()[:, p.m:]).all()


@pytest.mark.parametrize("seed", CONSUMER_SEEDS)
def test_projected_step(seed):
    """Explicit per-problem XL / XU drawn here (a quarter of the columns fixed, a quarter unbounded on either or both
    sides, the others in a box the step leaves on either side or stays in), a scalar and a per-problem step length:
    XP and SUM against the numpy reference of tests/test_gpu_step.py."""
    import torch
    c = _case(seed)
    p, X = c["p"], c["X"]
    n, ns = p.n, c["desc"].n_varsets
    col0 = [c0 for _, _, c0, _ in p.varset_info()] + [n]
    rng = np.random.default_rng(53 + seed)
    D = 0.8 * rng.standard_normal((B, n))
    kind = rng.integers(0, 8, (B, n))           # 0, 1: fixed; 2: no lower; 3: no upper; 4: neither; 5..7: a box
    half = 0.2 * rng.random((B, n)) + 0.01
    mid = X + 0.1 * rng.standard_normal((B, n))
    LO = np.where(kind <= 1, mid, np.where((kind == 2) | (kind == 4), -1e20, mid - half))
    UP = np.where(kind <= 1, mid, np.where((kind == 3) | (kind == 4), 1e20, mid + half))
    XL, XU = _padded(LO, n + 4), _padded(UP, n + 4)
    Xd, Dd = c["Xd"], _padded(D, n + 7)
    al = rng.uniform(0.05, 1.0, B)
    al[0] = 0.0
    for tag, alpha, dev_alpha in (("scalar alpha", STEP.ALPHA, STEP.ALPHA), ("per-problem alpha", al, _vec(al))):
        ref = STEP.reference(X, D, alpha, LO, UP, col0)
        STEP.assert_inputs_exercise_the_clamp(ref, f"seed {seed} {tag}")
        assert (ref["low"] & ~ref["fixed"]).any() and (ref["high"] & ~ref["fixed"]).any() and (ref["free"] & (LO > -1e19)).any()
        SUM, XP = _nan(B, 5 + ns + 3), _nan(B, n + 5)
        p.step_batch_device(Xd, Dd, SUM, XP=XP, alpha=dev_alpha, XL=XL, XU=XU)
        torch.cuda.synchronize()
        STEP.check(f"seed {seed} {tag}", p, SUM, XP, ref, ns)
    assert np.isnan(XL.cpu().numpy()[:, n:]).all() and np.isnan(XU.cpu().numpy()[:, n:]).all() and np.isnan(Dd.cpu().numpy()[:, n:]).all()


@pytest.mark.parametrize("mem", [1, 5])
@pytest.mark.parametrize("seed", LBFGS_SEEDS)
def test_lbfgs_update_and_direction(seed, mem):
    """The update's and the direction's cases and gates of tests/test_gpu_lbfgs.py on the seed's handle (its own
    variable bounds)."""
    LB.check_update(f"sweep_seed_{seed}", B, mem)
    LB.check_direction(f"sweep_seed_{seed}", B, mem)
