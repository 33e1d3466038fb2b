"""The tiled direct Gauss-Newton direction on the device (towr_gpu_gn_direction_tiled_batch_device: the block Cholesky
factorisation of rho (J^T W J)_ff + mu I on 16 x 16 tiles) and the resident loop that uses it
(towr_gpu_alsolve_gn_tiled_iterate_batch_device). Padded leading dimensions with NaN padding, NaN-filled outputs, a
NaN-filled workspace.

Operands and gates: tests/test_gpu_gn_direct.py's (rho_b = 10 (1 + b), mu = 1e-6). The held columns of D, the held
count, the code and SUM[7] are exact; D is not compared forwards: the backward error max |g_f - (H D)_f| with H assembled
in long double from the device's V must be <= 8 x the larger backward error of the two float64 evaluations of
tests/chol_ref.py, measured on the reference and never on the kernel. The bits are this entry's own: they are compared
with themselves (position, stream, wrows, run), not with the envelope entry's or a host restatement's. Breakdown columns
are asserted where they are exact: a NaN (tests/tile_chol_ref.py's column) and a pivot that is exactly 0. Largest gate
ratio per case on MI355X: DESIGN 4n."""
import functools

import numpy as np
import pytest

from tests import alsolve_ref as R
from tests import chol_ref as CH
from tests import lbfgs_ref
from tests import test_gpu_gn as GN
from tests import tile_chol_ref as TC
from tests.configs import cost_descs
from tests.gpu_helpers import _dev, _nan, _np_bits, _same_bits, _terrains, _vec
from tests.test_gpu_alsolve import FUSED_PAR, SOLVE_PAR, _assert_same, _start, _state
from tests.test_gpu_gn_direct import PGN_50, SOLVE_K
from tests.test_gpu_lbfgs import _ints, _problem
from towr2025_amd import TowrGpuProblem, alsolve_params, gn_params
from towr2025_amd import formulation as F

pytestmark = pytest.mark.gpu

MU = 1e-6
# (name, B, wrows): the baseline; n = 78, five block rows, 14 live rows in the last tile; rows without entries and the
# smallest pivot mu itself; three launches with the last partial, 2 live rows in the last tile; 59-tile block rows
CASES = [("monoped_procedural", 3, 3), ("sweep_seed_196", 3, 3), ("sweep_seed_154", 3, 3), ("anymal_trot_2p4s", 5, 2),
         ("anymal_stairs_gaitopt", 2, 2)]


@functools.lru_cache(maxsize=None)
def _operands(name, B):
    p, lo, up, _ = _problem(name)
    c = GN.build_operands(p, lo, up, B)
    c["info"] = p.gn_factor_info()
    c["tile"] = p.gn_tile_info()
    return c


def _run(c, mu=MU, rows=None, stream=None, V=None, GR=None, RUN=None, run_stride=1, wrows=None, LAMP=None):
    """The device call on the problems `rows` (default: all) into NaN-filled D (n + 5) and SUM (8 + 3)."""
    import torch
    n = c["n"]
    idx = slice(None) if rows is None else torch.tensor(list(rows), device=_dev())
    sel = lambda t: t if rows is None else t[idx].contiguous()
    Vd, GRd = sel(c["Vd"] if V is None else V), sel(c["GRd"] if GR is None else GR)
    B = GRd.shape[0]
    D, SUM = _nan(B, n + 5), _nan(B, 8 + 3)
    ldw = c["tile"]["ldw_min"]
    W = _nan(B if wrows is None else wrows, ldw + 3)
    if stream is not None:
        stream.wait_stream(torch.cuda.current_stream())
    XL, XU = (sel(c["XLd"]), sel(c["XUd"])) if "XLd" in c else (None, None)   # (explicit bounds: tests/test_gpu_sweep_chol.py)
    c["p"].gn_tiled_direction_batch_device(gn_params(mu=mu), Vd, sel(c["LPd"] if LAMP is None else LAMP), GRd, D, SUM, W,
                                           rho=sel(c["RHOd"]), X=sel(c["Xd"]), XL=XL, XU=XU, RUN=RUN, run_stride=run_stride,
                                           stream=stream)
    torch.cuda.synchronize()
    assert np.isnan(W.cpu().numpy()[:, ldw:]).all(), "the workspace's padding was written"
    return D, SUM


@functools.lru_cache(maxsize=None)
def _baseline(name, B, wrows):
    return _run(_operands(name, B), wrows=wrows)


@pytest.mark.parametrize("name,B,wrows", CASES)
def test_direction_against_numpy(name, B, wrows):
    c = _operands(name, B)
    n = c["n"]
    assert c["tile"]["nt"] == -(-n // 16) and c["tile"]["ldw_min"] >= 256 * c["tile"]["tiles"]
    D, SUM = _baseline(name, B, wrows)
    Dh, Sh = D.cpu().numpy(), SUM.cpu().numpy()
    assert np.isnan(Dh[:, n:]).all() and np.isnan(Sh[:, 8:]).all(), "padding written"
    worst = 0.0
    for b in range(B):
        tag = f"{name} B={B} problem {b}"
        a0 = (c["P"], c["V"][b], c["LAMP"][b], c["rho"][b], c["GR"][b], MU, c["info"]["pos"], c["info"]["first"])
        f64 = [CH.direction(*a0, held=c["held"][b], reverse=rev) for rev in (False, True)]
        assert all(f["code"] == 1 for f in f64), f"{tag}: the float64 references do not solve: {[f['code'] for f in f64]}"
        g, held, S = c["GR"][b], c["held"][b], Sh[b]
        assert (S[0], S[4], S[5], S[7]) == (1.0, held.sum(), 1.0, -1.0), f"{tag}: solved / held / code / column {S[:8]}"
        assert np.array_equal(_np_bits(Dh[b, :n][held]), _np_bits(g[held])), f"{tag}: held columns"
        assert S[3] > 0, f"{tag}: the slope sum g D = {S[3]}"
        assert 0 < S[2] <= S[6], f"{tag}: pivots {S[2]}, {S[6]}"
        a = (c["P"], c["V"][b], c["LAMP"][b], c["rho"][b], g, MU, held)
        H = CH.system(c["P"], c["V"][b], c["LAMP"][b], c["rho"][b], MU)
        gate = 8 * max(CH.backward_error(*a, f["D"], H=H) for f in f64)
        err = CH.backward_error(*a, Dh[b, :n], H=H)
        bb = float(np.sum(g[~held].astype(np.longdouble) ** 2))
        slope = float(np.sum(g.astype(np.longdouble) * Dh[b, :n].astype(np.longdouble)))
        print(f"{tag}: backward error {err:.3e} gate {gate:.3e} ratio {err / gate:.3e}; pivots {S[2]:.3e} .. {S[6]:.3e}; max |g| {np.max(np.abs(g)):.3e}")
        assert err <= gate, f"{tag}: backward error {err:.3e} gate {gate:.3e}"
        assert abs(S[1] - bb) <= 8 * n * 2.0 ** -53 * bb and abs(S[3] - slope) <= 8 * n * 2.0 ** -53 * float(np.sum(np.abs(g * Dh[b, :n])))
        worst = max(worst, err / gate)
    print(f"{name} B={B}: largest backward error / gate {worst:.3e}")


@pytest.mark.parametrize("name,B,wrows", CASES)
def test_bits_and_isolation(name, B, wrows):
    check_bits_and_isolation(_operands(name, B), wrows)


def check_bits_and_isolation(c, wrows):
    """On the operands c (this file's, or tests/test_gpu_sweep_chol.py's)."""
    import torch
    p, n, nnz, B = c["p"], c["n"], c["nnz"], c["B"]
    x = c["X"][0]
    v_ref = p.eval_jac_values(x)
    p.eval_g_keep_jac(x)
    D0, S0 = _run(c)
    v = p.eval_jac_values_kept(x)
    assert np.array_equal(v.view(np.int64), v_ref.view(np.int64)), "the kept Jacobian was dropped"
    assert (S0[:, 5] == 1).all()
    D1, S1 = _run(c, wrows=wrows)
    assert _same_bits(D0, D1) and _same_bits(S0, S1), "run to run, and the case's wrows"
    for wr in (1, 2, B):
        D1, S1 = _run(c, wrows=wr)
        assert _same_bits(D0, D1) and _same_bits(S0, S1), f"wrows = {wr}"
    order = list(range(B))[::-1]
    D2, S2 = _run(c, rows=order, wrows=2)
    inv = torch.tensor(order, device=_dev())
    assert _same_bits(D0[inv], D2) and _same_bits(S0[inv], S2), "another batch position"
    for b in (B - 1, 0):
        D3, S3 = _run(c, rows=[b], stream=torch.cuda.Stream(device=_dev()))
        assert _same_bits(D0[b:b + 1], D3) and _same_bits(S0[b:b + 1], S3), f"problem {b} as a B = 1 call on another stream"
    # a NaN in one problem's V, in a row whose lam+ is zero and a free column: code 2 at the reference's column, D == GR
    # there, no other problem's bits change
    bad = B - 1
    P = c["P"]
    k = int(np.flatnonzero((c["LAMP"][bad] == 0)[P.row] & ~c["held"][bad][P.col])[0])
    Vn = c["Vd"].clone()
    Vn[bad, k] = float("nan")
    D4, S4 = _run(c, V=Vn, wrows=wrows)
    s = S4[bad].cpu().numpy()
    assert (s[0], s[5]) == (0.0, 2.0) and 0 <= s[7] < n, f"NaN in V: solved / code / column {s[:8]}"
    assert _same_bits(D4[bad, :n], c["GRd"][bad, :n]), "NaN in V: D must be GR"
    others = torch.tensor([b for b in range(B) if b != bad], device=_dev())
    assert _same_bits(D4[others], D0[others]) and _same_bits(S4[others], S0[others]), "NaN in V reached another problem"
    ref = TC.direction(P, Vn[bad, :nnz].cpu().numpy(), c["LAMP"][bad], c["rho"][bad], c["GR"][bad], MU, c["info"]["pos"],
                       c["info"]["first"], held=c["held"][bad])
    assert (ref["code"], ref["bcol"]) == (2, int(s[7])), f"NaN in V: the reference breaks down at {ref['bcol']}, the device at {s[7]}"
    # RUN: a problem whose entry is >= 2 keeps its NaN fill
    vals = np.array([2, 0, 1, 3, 77])[np.arange(B) % 5]
    RUN = _ints(np.stack([vals, np.full(B, 9), np.full(B, 9), np.full(B, 9)], axis=1).reshape(-1))
    D5, S5 = _run(c, RUN=RUN, run_stride=4, wrows=wrows)
    skip = torch.from_numpy(vals >= 2).to(_dev())
    assert skip.any() and (~skip).any()
    assert torch.isnan(D5[skip]).all() and torch.isnan(S5[skip]).all(), "a skipped problem was written"
    assert _same_bits(D5[~skip], D0[~skip]) and _same_bits(S5[~skip], S0[~skip]), "RUN changed a running problem's bits"


@pytest.mark.parametrize("name,B,wrows", CASES)
def test_breakdown_and_nothing_to_solve(name, B, wrows):
    """mu = 0 with lam+ = 0 in problem 1: its matrix is zero on the free columns, so the first free permuted column has the
    pivot exactly 0 — code 2, SUM[7] that column, D == GR, no other problem's bits change (the others' own breakdown
    columns at mu = 0 are rounding noise and are not asserted). And GR = +-0 on every free column of problem 1 (mu = 1e-6):
    code 3, D == GR with the signs of the zeros, no factorisation."""
    check_breakdown_and_nothing_to_solve(_operands(name, B), wrows)


def check_breakdown_and_nothing_to_solve(c, wrows):
    """On the operands c (this file's, or tests/test_gpu_sweep_chol.py's)."""
    import torch
    n, pos, B = c["n"], c["info"]["pos"], c["B"]
    D0, S0 = _run(c, mu=0.0, wrows=wrows)
    others = torch.tensor([b for b in range(B) if b != 1], device=_dev())
    LP0 = c["LPd"].clone()
    LP0[1] = 0.0
    D1, S1 = _run(c, mu=0.0, LAMP=LP0, wrows=wrows)
    s = S1[1].cpu().numpy()
    held = c["held"][1]
    assert (s[0], s[2], s[4], s[5], s[6], s[7]) == (0.0, 0.0, held.sum(), 2.0, 0.0, pos[~held].min()), s[:8]
    assert _same_bits(D1[1, :n], c["GRd"][1, :n]), "lam+ = 0, mu = 0: D must be GR"
    assert _same_bits(D1[others], D0[others]) and _same_bits(S1[others], S0[others])
    # code 3
    g0 = np.where(held, c["GR"][1], 0.0)
    g0[np.flatnonzero(~held)[::2]] = -0.0
    assert np.array_equal(lbfgs_ref.held_mask(c["X"][1], g0, c["lo"][1], c["up"][1]), held)
    GR0 = c["GRd"].clone()
    GR0[1, :n] = torch.from_numpy(g0).to(_dev())
    D2, S2 = _run(c, wrows=wrows)
    D3, S3 = _run(c, GR=GR0, wrows=wrows)
    s = S3[1].cpu().numpy()
    assert (s[0], s[1], s[2], s[4], s[5], s[6], s[7]) == (0.0, 0.0, 0.0, held.sum(), 3.0, 0.0, -1.0), s[:8]
    assert _same_bits(D3[1, :n], GR0[1, :n]), "code 3: D must be GR"
    assert _same_bits(D3[others], D2[others]) and _same_bits(S3[others], S2[others])


# ---- the fused entry ---------------------------------------------------------------------------------------------------
TILED_ITERS = 3


def _pieces_iteration(p, par, gn, st, DC, GSUM, W, Gs, Vs):
    """tests/test_gpu_gn_direct.py's, with the tiled direction."""
    import torch
    B, n = st.B, p.n
    p.eval_cost_batch_device(st.XC, st.FC, GRAD=st.GRC)
    p.eval_batch_device(st.XC, Gs, Vs)
    rho = st.RHO.cpu().numpy()
    for b in range(B):
        p.residual_batch_device(Gs[b:b + 1], st.RSUM[b:b + 1], LAM=st.LAM[b:b + 1], rho=float(rho[b]), LAMP=st.LAMP[b:b + 1])
    p.jac_tvec_batch_device(Vs, st.LAMP, st.GRC, accumulate=True)
    p.gn_tiled_direction_batch_device(gn, Vs, st.LAMP, st.GRC, DC, GSUM, W, rho=st.RHO, X=st.XC, RUN=st.ISTATE, run_stride=4)
    p.linesearch_batch_device(par, st)
    p.auglag_outer_batch_device(par, st)
    flags = st.ISTATE.view(B, 4)[:, 1]
    acc = (flags & 1) != 0
    retry = ~acc & ((flags & 4) != 0)
    st.D[acc, :n] = DC[acc, :n]
    st.D[retry, :n] = st.GR[retry, :n]
    p.step_batch_device(st.X, st.D, st.SSUM, XP=st.XC, alpha=st.ALPHA)
    torch.cuda.synchronize()


def test_fused_entry_is_bit_identical_to_the_pieces():
    """TILED_ITERS alsolve_gn_tiled_iterate(iters=1) calls against the public calls in sequence, in every state array, DC
    and GSUM after every iteration, at the automatic products chunk and at chunk 2 (a ragged last chunk, wrows = 2 within
    it), with batch terrains set and a RHO row of distinct values; iters=3 against three calls."""
    import torch
    name, B = "anymal_all_costs", 5
    f = F.with_costs(F.anymal_trot())
    f.params_.enable_stance_tracking = False
    p = TowrGpuProblem(cost_descs()[name], device=0, data=f.var_bounds_data())
    lo, up = p.variable_bounds()
    p.set_batch_terrain(_terrains(name, B, np.random.default_rng(7)))
    n, mem = p.n, FUSED_PAR["mem"]
    ldw = p.gn_tile_info()["ldw_min"]
    par = alsolve_params(**FUSED_PAR)
    gn = gn_params(mu=1e-2)
    h0 = _start(p, lo, up, B, mem, 7300)

    def fresh():
        st = _state(p, B, mem, h0)
        p.alsolve_init(par, st)
        st.RHO.copy_(_vec(10.0 * (1.0 + 0.25 * np.arange(B))))
        return st, _nan(B, n + 3), _nan(B, 8 + 2)

    Gs, Vs = _nan(B, p.m + 1), _nan(B, p.nnz + 5)
    (ref, DCr, GSr), want, codes = fresh(), [], []
    Wr = _nan(B, ldw + 1)
    for k in range(TILED_ITERS):
        _pieces_iteration(p, par, gn, ref, DCr, GSr, Wr, Gs, Vs)
        want.append((ref.clone(), DCr.clone(), GSr.clone()))
        codes.append(ref.LSUM[:, 0].cpu().numpy().astype(int).tolist())
    print(f"{name}: LSUM[0] per iteration {codes}; direction codes at the end {GSr[:, 5].tolist()}")
    assert (GSr[:, 5] == 1).all() and np.isnan(GSr.cpu().numpy()[:, 8:]).all() and np.isnan(DCr.cpu().numpy()[:, n:]).all()
    try:
        for chunk, wrows in ((0, 3), (2, 2)):
            p.set_products_chunk(chunk)
            W = _nan(wrows, ldw + 2)
            st, DC, GS = fresh()
            for k in range(TILED_ITERS):
                p.alsolve_gn_tiled_iterate(par, st, gn, DC, GS, W)
                torch.cuda.synchronize()
                what = f"{name} chunk {chunk} wrows {wrows} iteration {k}"
                _assert_same(st, want[k][0], what)
                assert _same_bits(DC, want[k][1]) and _same_bits(GS, want[k][2]), f"{what}: DC / GSUM"
            st, DC, GS = fresh()
            p.alsolve_gn_tiled_iterate(par, st, gn, DC, GS, W, iters=3)
            torch.cuda.synchronize()
            _assert_same(st, want[2][0], f"{name} chunk {chunk} iters=3")
            assert _same_bits(DC, want[2][1]) and _same_bits(GS, want[2][2]), f"{name} chunk {chunk} iters=3: DC / GSUM"
    finally:
        p.set_products_chunk(0)


# ---- a short solve -----------------------------------------------------------------------------------------------------
def test_short_solve_converges():
    """tests/test_gpu_gn_direct.py's short solve with alsolve_gn_tiled_iterate: monoped_procedural, B = 6, wrows = 4 (two
    launches per iteration), the starts x0 + 0.05 randn(900 + b), SOLVE_PAR, mu = 1e-6, at most SOLVE_K = 100 iterations.
    Asserted: no NaN appears, an accepted base never raises M0, every problem's max violation ends below the
    preconditioned CG loop's CPU figure for its seed (PGN_50), at least 5 of the 6 problems end TOWR_AL_CONVERGED. The
    iteration counts are printed."""
    name, B = "monoped_procedural", 6
    p, lo, up, _ = _problem(name)
    n, mem = p.n, SOLVE_PAR["mem"]
    par = alsolve_params(**SOLVE_PAR)
    gn = gn_params(mu=MU)
    x0 = p.initial_x()
    h0 = dict(X=np.stack([x0 + 0.05 * np.random.default_rng(900 + b).standard_normal(n) for b in range(B)]), LAM=np.zeros((B, p.m)))
    st = _state(p, B, mem, h0)
    DC, GS = _nan(B, n + 3), _nan(B, 8 + 2)
    W = _nan(4, p.gn_tile_info()["ldw_min"])
    p.alsolve_init(par, st)
    done = np.zeros(B, dtype=int)
    for k in range(SOLVE_K):
        p.alsolve_gn_tiled_iterate(par, st, gn, DC, GS, W)
        sc, ls = st.SCAL.cpu().numpy()[:, :8], st.LSUM.cpu().numpy()[:, :8]
        assert not np.isnan(sc).any() and not np.isnan(ls).any() and not np.isnan(GS.cpu().numpy()[:, :8]).any(), f"iteration {k}: NaN"
        acc = ls[:, 0] == 2
        assert (ls[acc, 2] <= ls[acc, 3]).all(), f"iteration {k}: an accepted base raised M0"
        phases = np.array(st.ISTATE.view(B, 4)[:, 0].tolist())
        done = np.where((done == 0) & (phases >= R.CONVERGED), k + 1, done)
        if (phases >= R.CONVERGED).all():
            break
    last = st.SCAL.cpu().numpy()[:, 4]
    print(f"phases {phases.tolist()} after {done.tolist()} iterations; max violation {last.tolist()}; direction codes {GS[:, 5].tolist()}")
    assert np.isfinite(st.X.cpu().numpy()[:, :n]).all()
    assert (last < np.array(PGN_50)).all(), f"not below the preconditioned loop's violation: {last.tolist()}"
    assert (phases == R.CONVERGED).sum() >= 5, phases.tolist()
