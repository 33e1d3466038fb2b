"""The Gauss-Newton direction on the device (towr_gpu_gn_direction_batch_device) and the resident loop that uses it
(towr_gpu_alsolve_gn_iterate_batch_device) against tests/gn_ref.py, the numpy restatement of include/towr_gpu.h. Every
case uses padded leading dimensions with NaN padding and NaN-filled outputs. The shapes are those of
tests/test_gpu_lbfgs.py, for its reasons.

Operands: the device's own CSR values at clamp(x0 + 0.05 sigma), lam+ of the residual kernel for LAM = 0.1 randn and
rho_b = 10 (1 + b) (the RHO row), GR = J^T lam+, the handle's bounds; mu = {1e-2, 1e-6} max diag(rho_0 J_0^T W_0 J_0),
ncg in {1, 3, 8}, tol = 0.

Gates. The held columns of D, the steps, the held count and the stop code are exact. The free columns of D and
SUM[1..3] (bb, rr, the slope) cannot be bounded a priori (the conditioning of the CG recursion enters), so the gate is
the one of tests/test_gpu_lbfgs.py, measured on the reference and never on the kernel: err against the long double
reference <= 8 max(e64, gamma_n scale), e64 = the larger error of two float64 evaluations of the reference with
different summation orders, scale = max |value| (of D: over its free columns). On these operands e64 / scale stays below 1e-14, so the gate is
gamma_n scale-sized. It still refuses a wrong system: a reference that treats every row as active lies more than
1000 gates away on every problem checked (asserted on the CPU inside the test; measured >= 1.9e3, on gait-opt
>= 6e6). Largest err / gate seen on MI355X: 8.4e-3 (per case: DESIGN 4k). The gate and the comparison live in
tests/gn_gate.py (shared with the CPU tests of the kernel's host walk, tests/test_gn_emu.py); the device's bits against
that walk, the swept shapes and the stop codes 2 (without a NaN) and 3 are in tests/test_gpu_sweep_gn.py."""
import functools

import numpy as np
import pytest

from tests import alsolve_ref as R
from tests import gn_gate as GATE
from tests import gn_ref as G
from tests import lbfgs_ref
from tests.configs import cost_descs
from tests.gpu_helpers import _dev, _nan, _np_bits, _padded, _same_bits, _terrains, _vec
from tests.test_gpu_alsolve import FUSED_PAR, SOLVE_PAR, _assert_same, _start, _state, empty_sets
from tests.test_gpu_lbfgs import _gamma, _ints, _problem
from towr2025_amd import TowrGpuProblem, alsolve_params, gn_params
from towr2025_amd import formulation as F

pytestmark = pytest.mark.gpu

LD = np.longdouble
CASES = [("monoped_procedural", 1), ("monoped_procedural", 3), ("anymal_trot_2p4s", 37), ("anymal_stairs_gaitopt", 3)]
MUS = (1e-2, 1e-6)
NCGS = (1, 3, 8)
COMBOS = [(mk, ncg) for mk in MUS for ncg in NCGS]


@functools.lru_cache(maxsize=None)
def _operands(name, B):
    """Device and host copies of one case's operands, the pattern, the held masks and mu's base."""
    p, lo, up, _ = _problem(name)
    return build_operands(p, lo, up, B)


def build_operands(p, lo, up, B, redraw=None):
    """_operands on a handle with its variable bounds. `redraw`: when the handle's bounds hold no column at these
    operands, redraw(X) -> per-problem (XL, XU) (B, n) that the call then takes explicitly (XLd / XUd in the result)."""
    import torch
    n, m, nnz = p.n, p.m, p.nnz
    rng = np.random.default_rng(8100 + B)
    X = R.clamp(p.initial_x() + 0.05 * rng.standard_normal((B, n)), lo, up)
    LAM = 0.1 * rng.standard_normal((B, m))
    rho = 10.0 * (1.0 + np.arange(B))
    Xd, Gd, Vd = _padded(X, n + 1), _nan(B, m + 2), _nan(B, nnz + 3)
    p.eval_batch_device(Xd, Gd, Vd)
    LAMd, LPd, RS = _padded(LAM, m + 5), _nan(B, m + 4), _nan(B, 4 + p.desc.n_constraints + 1)
    for b in range(B):
        p.residual_batch_device(Gd[b:b + 1], RS[b:b + 1], LAM=LAMd[b:b + 1], rho=float(rho[b]), LAMP=LPd[b:b + 1])
    GRd = _nan(B, n + 7)
    p.jac_tvec_batch_device(Vd, LPd, GRd)
    torch.cuda.synchronize()
    V, LAMP, GR = Vd.cpu().numpy()[:, :nnz], LPd.cpu().numpy()[:, :m], GRd.cpu().numpy()[:, :n]
    return finish_operands(p, lo, up, B, X, V, LAMP, GR, rho, Xd, Vd, LPd, GRd, redraw)


def finish_operands(p, lo, up, B, X, V, LAMP, GR, rho, Xd, Vd, LPd, GRd, redraw=None):
    """The checks on the operands and the dict the helpers below take. lo / up: (n) or per problem (B, n)."""
    n, m, nnz = p.n, p.m, p.nnz
    assert np.isfinite(V).all() and np.isfinite(LAMP).all() and np.isfinite(GR).all()
    rp, col = p.jac_csr()
    P = G.Pattern(rp, col, n)
    lo, up = np.broadcast_to(lo, (B, n)), np.broadcast_to(up, (B, n))
    held = np.stack([lbfgs_ref.held_mask(X[b], GR[b], lo[b], up[b]) for b in range(B)])
    extra = {}
    if redraw is not None and not held.any():
        lo, up = redraw(X)
        held = np.stack([lbfgs_ref.held_mask(X[b], GR[b], lo[b], up[b]) for b in range(B)])
        extra = dict(XLd=_padded(lo, n + 4), XUd=_padded(up, n + 4))
    w0 = G.weights(LAMP[0])
    mu_base = float(np.max(rho[0] * np.bincount(P.col, weights=w0[P.row] * V[0] * V[0], minlength=n)))
    inactive = int((LAMP == 0).sum())
    assert mu_base > 0 and inactive > 0 and held.any(), "no curvature, no inactive row or no held column: the case shows nothing"
    return dict(p=p, lo=lo, up=up, n=n, m=m, nnz=nnz, B=B, X=X, V=V, LAMP=LAMP, GR=GR, rho=rho, P=P, held=held, mu_base=mu_base,
                Xd=Xd, Vd=Vd, LPd=LPd, GRd=GRd, RHOd=_vec(rho), **extra)


def _run(c, gn, rows=None, stream=None, V=None, GR=None, RUN=None, run_stride=1, LAMP=None):
    """The device call on the problems `rows` (default: all) into NaN-filled D (n + 5) and SUM (6 + 3)."""
    import torch
    n = c["n"]
    idx = slice(None) if rows is None else torch.tensor(list(rows), device=_dev())
    sel = lambda t: t if rows is None else t[idx].contiguous()
    Vd, GRd = sel(c["Vd"] if V is None else V), sel(c["GRd"] if GR is None else GR)
    B = GRd.shape[0]
    D, SUM = _nan(B, n + 5), _nan(B, 6 + 3)
    if stream is not None:
        stream.wait_stream(torch.cuda.current_stream())
    XL, XU = (sel(c["XLd"]), sel(c["XUd"])) if "XLd" in c else (None, None)   # (explicit bounds: tests/test_gpu_sweep_gn.py)
    c["p"].gn_direction_batch_device(gn, Vd, sel(c["LPd"] if LAMP is None else LAMP), GRd, D, SUM, rho=sel(c["RHOd"]), X=sel(c["Xd"]),
                                     XL=XL, XU=XU, RUN=RUN, run_stride=run_stride, stream=stream)
    torch.cuda.synchronize()
    return D, SUM


def _refs(c, b, ncg, mu, tol):
    kw = dict(held=c["held"][b])
    a = (c["P"], c["V"][b], c["LAMP"][b], c["rho"][b], c["GR"][b], ncg, mu, tol)
    return (G.direction(*a, dtype=LD, **kw), [G.direction(*a, reverse=rev, **kw) for rev in (False, True)])


_gate = GATE.gate   # (the gate and the comparison live in tests/gn_gate.py, importable without torch)


def _check_problem(tag, c, b, Dh, S, ld, f64):
    """Row b of the device outputs against the references; returns the largest err / gate."""
    n = c["n"]
    assert np.isnan(Dh[n:]).all() and np.isnan(S[6:]).all(), f"{tag}: padding written"
    return GATE.check_values(tag, n, c["GR"][b], c["held"][b], Dh, S, ld, f64)


@pytest.mark.parametrize("name,B", CASES)
def test_direction_against_numpy(name, B):
    """Every (mu, ncg) combination in one call per combination; at B = 37 a combination is checked on the problems
    b % 6 == its index and on the first and last problem (every problem is checked in some combination)."""
    c = _operands(name, B)
    n = c["n"]
    worst, e64_rel, teeth = 0.0, 0.0, np.inf
    for ci, (mk, ncg) in enumerate(COMBOS):
        mu = mk * c["mu_base"]
        D, SUM = _run(c, gn_params(ncg=ncg, mu=mu, tol=0.0))
        Dh, S = D.cpu().numpy(), SUM.cpu().numpy()
        for b in range(B):
            if B > 6 and b % 6 != ci and b not in (0, B - 1):
                continue
            ld, f64 = _refs(c, b, ncg, mu, 0.0)
            tag = f"{name} B={B} mu={mk:g} ncg={ncg} problem {b}"
            assert ld["steps"] == ncg and ld["code"] == 0, f"{tag}: the reference stopped early {ld['steps'], ld['code']}"
            worst = max(worst, _check_problem(tag, c, b, Dh[b], S[b], ld, f64))
            # teeth, on the CPU: the system with every row active lies far outside the gate
            v, gate, rel = _gate(ld, f64, "D", n)
            e64_rel = max(e64_rel, rel)
            wrong = G.direction(c["P"], c["V"][b], c["LAMP"][b], c["rho"][b], c["GR"][b], ncg, mu, 0.0, held=c["held"][b], dtype=LD,
                                ignore_w=True)["D"]
            away = float(np.max(np.abs(wrong - v))) / gate
            assert away > 1000, f"{tag}: ignoring W lies only {away:.3g} gates away"
            teeth = min(teeth, away)
    print(f"{name} B={B}: largest err / gate {worst:.3e}; largest e64 / scale {e64_rel:.3e}; ignoring W >= {teeth:.3g} gates away")


@pytest.mark.parametrize("name,B", CASES)
def test_early_stop(name, B):
    """tol between two consecutive rr / bb of problem 0's long double run (their geometric mean): the three references
    and the device stop at the same step on every problem, and no reference residual lies within 1e-6 of the tie."""
    c = _operands(name, B)
    mu = MUS[0] * c["mu_base"]
    hist = [float(v) for v in _refs(c, 0, 8, mu, 0.0)[0]["hist"]]
    k = next(i for i in range(2, 8) if hist[i] < min(hist[:i]))
    tol = float(np.sqrt(np.sqrt(hist[k] * min(hist[:k]))))
    D, SUM = _run(c, gn_params(ncg=8, mu=mu, tol=tol))
    Dh, S = D.cpu().numpy(), SUM.cpu().numpy()
    steps, worst = [], 0.0
    for b in range(B):
        ld, f64 = _refs(c, b, 8, mu, tol)
        for r in [ld] + f64:
            assert min(abs(float(h) / (tol * tol) - 1.0) for h in r["hist"]) > 1e-6, f"{name} problem {b}: a stop decision is a tie"
        worst = max(worst, _check_problem(f"{name} B={B} tol={tol:.3e} problem {b}", c, b, Dh[b], S[b], ld, f64))
        steps.append((ld["steps"], ld["code"]))
    assert steps[0] == (k, 1), steps
    print(f"{name} B={B}: tol {tol:.3e}; (steps, code) per problem {steps}; largest err / gate {worst:.3e}")


@pytest.mark.parametrize("name,B", [c for c in CASES if c[1] > 1])
def test_bits_and_isolation(name, B):
    import torch
    c = _operands(name, B)
    p, n, nnz = c["p"], c["n"], c["nnz"]
    gn = gn_params(ncg=8, mu=MUS[1] * c["mu_base"], tol=0.0)
    x = c["X"][0]
    v_ref = p.eval_jac_values(x)
    p.eval_g_keep_jac(x)
    D0, S0 = _run(c, gn)
    v = p.eval_jac_values_kept(x)
    assert np.array_equal(v.view(np.int64), v_ref.view(np.int64)), "the kept Jacobian was dropped"
    assert (S0[:, 0] == 8).all() and np.isnan(D0[:, n:].cpu().numpy()).all() and np.isnan(S0[:, 6:].cpu().numpy()).all()
    D1, S1 = _run(c, gn)
    assert _same_bits(D0, D1) and _same_bits(S0, S1), "run to run"
    order = list(range(B))[::-1]
    D2, S2 = _run(c, gn, rows=order)
    inv = torch.tensor(order, device=_dev())
    assert _same_bits(D0[inv], D2) and _same_bits(S0[inv], S2), "another batch position"
    for b in (B - 1, 0):
        D3, S3 = _run(c, gn, rows=[b], stream=torch.cuda.Stream(device=_dev()))
        assert _same_bits(D0[b:b + 1], D3) and _same_bits(S0[b:b + 1], S3), f"problem {b} as a B = 1 call on another stream"
    # a NaN in one problem's GR (a column that is not fixed) or V: code 2 and D == GR there, no other problem's bits change
    col = int(np.flatnonzero(c["lo"][1] < c["up"][1])[5])   # (of problem 1, whose GR takes the NaN: the bounds are per problem rows)
    GRn, Vn = c["GRd"].clone(), c["Vd"].clone()
    GRn[1, col] = float("nan")
    Vn[0, nnz // 2] = float("nan")
    for what, kw, bad, gr in (("GR", dict(GR=GRn), 1, GRn), ("V", dict(V=Vn), 0, c["GRd"])):
        D4, S4 = _run(c, gn, **kw)
        s = S4[bad].cpu().numpy()
        assert (s[0], s[5]) == (0.0, 2.0), f"NaN in {what}: steps / code {s[:6]}"
        assert _same_bits(D4[bad, :n], gr[bad, :n]), f"NaN in {what}: D must be GR"
        others = torch.tensor([b for b in range(B) if b != bad], device=_dev())
        assert _same_bits(D4[others], D0[others]) and _same_bits(S4[others], S0[others]), f"NaN in {what} reached another problem"
    # RUN: a problem whose entry is >= 2 keeps its NaN fill
    vals = np.array([0, 1, 2, 3, 4, 77, -5])[np.arange(B) % 7]
    RUN = _ints(np.stack([vals, np.full(B, 9), np.full(B, 9), np.full(B, 9)], axis=1).reshape(-1))
    D5, S5 = _run(c, gn, RUN=RUN, run_stride=4)
    skip = torch.from_numpy(vals >= 2).to(_dev())
    assert skip.any() and (~skip).any()
    assert torch.isnan(D5[skip]).all() and torch.isnan(S5[skip]).all(), "a skipped problem was written"
    assert _same_bits(D5[~skip], D0[~skip]) and _same_bits(S5[~skip], S0[~skip]), "RUN changed a running problem's bits"
    # X = None: every column is free; the scalar rho
    Df, Sf = _nan(B, n + 5), _nan(B, 6 + 3)
    p.gn_direction_batch_device(gn, c["Vd"], c["LPd"], c["GRd"], Df, Sf, rho=10.0)
    torch.cuda.synchronize()
    assert (Sf[:, 4] == 0).all() and (Sf[:, 0] == 8).all()
    ld = G.direction(c["P"], c["V"][0], c["LAMP"][0], 10.0, c["GR"][0], 8, MUS[1] * c["mu_base"], 0.0, dtype=LD)
    f64 = [G.direction(c["P"], c["V"][0], c["LAMP"][0], 10.0, c["GR"][0], 8, MUS[1] * c["mu_base"], 0.0, reverse=rev) for rev in (False, True)]
    v, gate, _ = _gate(ld, f64, "D", n)
    assert float(np.max(np.abs(Df[0, :n].cpu().numpy().astype(LD) - v))) <= gate, "every column free"


# ---- the fused entry ---------------------------------------------------------------------------------------------------
GN_ITERS = 12


def _pieces_iteration(p, par, gn, st, DC, GSUM, Gs, Vs):
    """One iteration by the public calls; the residual takes a scalar rho: one B = 1 call per problem. The select is
    done with torch row copies."""
    import torch
    B, n = st.B, p.n
    p.eval_cost_batch_device(st.XC, st.FC, GRAD=st.GRC)
    p.eval_batch_device(st.XC, Gs, Vs)
    rho = st.RHO.cpu().numpy()
    for b in range(B):
        p.residual_batch_device(Gs[b:b + 1], st.RSUM[b:b + 1], LAM=st.LAM[b:b + 1], rho=float(rho[b]), LAMP=st.LAMP[b:b + 1])
    p.jac_tvec_batch_device(Vs, st.LAMP, st.GRC, accumulate=True)
    p.gn_direction_batch_device(gn, Vs, st.LAMP, st.GRC, DC, GSUM, rho=st.RHO, X=st.XC, RUN=st.ISTATE, run_stride=4)
    p.linesearch_batch_device(par, st)
    p.auglag_outer_batch_device(par, st)
    flags = st.ISTATE.view(B, 4)[:, 1]
    acc = (flags & 1) != 0
    retry = ~acc & ((flags & 4) != 0)
    st.D[acc, :n] = DC[acc, :n]
    st.D[retry, :n] = st.GR[retry, :n]
    p.step_batch_device(st.X, st.D, st.SSUM, XP=st.XC, alpha=st.ALPHA)
    torch.cuda.synchronize()


@pytest.mark.parametrize("name,B", [("anymal_all_costs", 5), ("anymal_stairs_gaitopt_costs", 3)])
def test_fused_entry_is_bit_identical_to_the_pieces(name, B):
    """GN_ITERS alsolve_gn_iterate(iters=1) calls against the public calls in sequence, in every state array, DC and
    GSUM after every iteration, at the automatic products chunk and at chunk 2 (a ragged last chunk), with batch
    terrains set and a RHO row of distinct values; iters=3 against three calls; then one forced iteration (M0 lowered so
    that the trial is refused: a shrink that keeps D, and a fall through alpha_min that takes D <- GR); then frozen
    problems, whose bits stop changing."""
    gait = name == "anymal_stairs_gaitopt_costs"
    f = F.with_costs(F.anymal_trot(terrain=F.HeightMap.MakeTerrain(F.HeightMap.StairsID), optimize_timings=True) if gait else F.anymal_trot())
    f.params_.enable_stance_tracking = False
    p = TowrGpuProblem(cost_descs()[name], device=0, data=f.var_bounds_data())
    lo, up = p.variable_bounds()
    p.set_batch_terrain(_terrains(name, B, np.random.default_rng(7)))
    check_fused(name, p, lo, up, B, GN_ITERS, {1, 2}, frozen=True)


def check_fused(name, p, lo, up, B, iters, need, frozen=False):
    """`iters` alsolve_gn_iterate(iters=1) calls on the handle p against the public calls in sequence (every state
    array, DC and GSUM after every iteration, products chunks 0 and 2, a RHO row of distinct values), iters=3 against
    three calls, then one forced iteration (see the test above). `need`: the line-search codes (LSUM[0]) that must occur
    in the first `iters` iterations. The maximum of a constraint set without rows stays +0.0 in RSUM through every
    residual call of the loop. `frozen`: also the frozen-problems run. Returns the codes per iteration."""
    import torch
    n, mem = p.n, FUSED_PAR["mem"]
    par = alsolve_params(**FUSED_PAR)
    gn = gn_params(ncg=6, mu=1e-2, tol=1e-3)
    h0 = _start(p, lo, up, B, mem, 7300)
    empty = empty_sets(p)

    def fresh(par=par):
        st = _state(p, B, mem, h0)
        p.alsolve_init(par, st)
        st.RHO.copy_(_vec(10.0 * (1.0 + 0.25 * np.arange(B))))
        return st, _nan(B, n + 3), _nan(B, 6 + 2)

    def force(st):
        """Problem 0 falls through alpha_min with a pair in the history, problem 1 shrinks; both refuse the trial."""
        st.SCAL[:2, 0] = -1e300
        st.ISTATE.view(B, 4)[:2, 0] = R.SEARCH
        st.HMETA.view(B, 2)[0] = _ints(np.array([1, 1]))
        st.ALPHA[0], st.ALPHA[1] = par.alpha_min, 1.0

    Gs, Vs = _nan(B, p.m + 1), _nan(B, p.nnz + 5)
    (ref, DCr, GSr), want, codes = fresh(), [], []
    for k in range(iters + 1):
        if k == iters:
            force(ref)
            d_before = ref.D.clone()
        _pieces_iteration(p, par, gn, ref, DCr, GSr, Gs, Vs)
        want.append((ref.clone(), DCr.clone(), GSr.clone()))
        codes.append(ref.LSUM[:, 0].cpu().numpy().astype(int).tolist())
    print(f"{name}: LSUM[0] per iteration {codes}; CG steps / codes at the end {GSr[:, 0].tolist()} / {GSr[:, 5].tolist()}")
    flat = {c for row in codes[:iters] for c in row}
    assert need <= flat, f"codes {sorted(need - flat)} do not occur in the run: the comparison would show nothing"
    assert (GSr[:, 0] > 0).all() and np.isnan(GSr.cpu().numpy()[:, 6:]).all() and np.isnan(DCr.cpu().numpy()[:, n:]).all()
    assert codes[iters][:2] == [4, 3], codes[iters]
    assert _same_bits(ref.D[0, :n], ref.GR[0, :n]) and _same_bits(ref.D[1], d_before[1]), "the forced select"
    try:
        for chunk in (0, 2):
            p.set_products_chunk(chunk)
            st, DC, GS = fresh()
            for k in range(iters + 1):
                if k == iters:
                    force(st)
                p.alsolve_gn_iterate(par, st, gn, DC, GS)
                torch.cuda.synchronize()
                what = f"{name} chunk {chunk} iteration {k}"
                _assert_same(st, want[k][0], what)
                assert _same_bits(DC, want[k][1]) and _same_bits(GS, want[k][2]), f"{what}: DC / GSUM"
                for s_ in empty:
                    assert (_np_bits(st.RSUM.cpu().numpy()[:, 4 + s_]) == 0).all(), f"{what}: the maximum of empty set {s_} is not +0.0"
            st, DC, GS = fresh()
            p.alsolve_gn_iterate(par, st, gn, DC, GS, iters=3)
            torch.cuda.synchronize()
            _assert_same(st, want[2][0], f"{name} chunk {chunk} iters=3")
            assert _same_bits(DC, want[2][1]) and _same_bits(GS, want[2][2]), f"{name} chunk {chunk} iters=3: DC / GSUM"
    finally:
        p.set_products_chunk(0)
    if not frozen:
        return codes
    # frozen: max_outer = 1 ends every problem MAXED; from then on no bit changes, DC and GSUM included
    par2 = alsolve_params(**{**FUSED_PAR, "max_inner": 3, "max_outer": 1})
    st, DC, GS = fresh(par2)
    p.alsolve_gn_iterate(par2, st, gn, DC, GS, iters=40)
    torch.cuda.synchronize()
    assert st.ISTATE.view(B, 4)[:, 0].tolist() == [R.MAXED] * B, st.ISTATE.view(B, 4).tolist()
    p.alsolve_gn_iterate(par2, st, gn, DC, GS, iters=2)          # (the frozen code LSUM[0] = 0 and XC = P(X) settle here)
    keep, DCk, GSk = st.clone(), DC.clone(), GS.clone()
    p.alsolve_gn_iterate(par2, st, gn, DC, GS, iters=3)
    torch.cuda.synchronize()
    _assert_same(st, keep, "frozen problems")
    assert _same_bits(DC, DCk) and _same_bits(GS, GSk), "frozen problems: DC / GSUM"
    return codes


# ---- a short solve -----------------------------------------------------------------------------------------------------
GN_SOLVE = dict(ncg=100, mu=1e-2, tol=1e-3)
GN_SOLVE_K = 50
LBFGS_150 = (19.966277, 21.103334, 19.909981)


def test_short_solve_beats_the_lbfgs_loop():
    """monoped_procedural, B = 3, the starts and SOLVE_PAR of tests/test_gpu_alsolve.py's short solve (shrink = 0.1), the
    GN direction with ncg = 100, mu = 1e-2, tol = 1e-3, GN_SOLVE_K = 50 iterations of alsolve_gn_iterate(iters=1) with
    SCAL read between the calls. Asserted: no NaN appears, an accepted base never raises M0, every problem's max
    violation (SCAL[4]) ends below its value after the first evaluation — and below what the L-BFGS loop of
    tests/alsolve_ref.py reaches after 150 iterations with the same parameters.

    From the CPU reference driven by the CPU oracle (both float64 summation orders, the smaller figure kept for the
    L-BFGS loop): L-BFGS, 150 iterations: 19.966277 / 21.103334 / 19.909981 (19.966286 / 21.103446 / 19.910032 in the
    other order). tests/gn_ref.py's loop with the parameters above, 50 iterations: 10.721 / 10.997 / 10.905 and
    10.757 / 11.014 / 10.909 from first violations 1660.4 / 2534.2 / 1912.5, every trial accepted at alpha0. With
    ncg = 60 and mu = 1e-3 the same loop ends at 13.5 / 14.0 / 12.9, with ncg = 30 at 18.7 / 19.5 / 18.7: the CG budget is
    what buys the margin. The iterates are NOT compared with the reference: a rounding difference may steer a decision."""
    name, B = "monoped_procedural", 3
    p, lo, up, _ = _problem(name)
    n, mem = p.n, SOLVE_PAR["mem"]
    par = alsolve_params(**SOLVE_PAR)
    gn = gn_params(**GN_SOLVE)
    x0 = p.initial_x()
    h0 = dict(X=np.stack([x0 + 0.05 * np.random.default_rng(900 + b).standard_normal(n) for b in range(B)]), LAM=np.zeros((B, p.m)))
    st = _state(p, B, mem, h0)
    DC, GS = _nan(B, n + 3), _nan(B, 6 + 2)
    p.alsolve_init(par, st)
    first, codes = None, []
    for k in range(GN_SOLVE_K):
        p.alsolve_gn_iterate(par, st, gn, DC, GS)
        sc, ls = st.SCAL.cpu().numpy()[:, :8], st.LSUM.cpu().numpy()[:, :8]
        assert not np.isnan(sc).any() and not np.isnan(ls).any() and not np.isnan(GS.cpu().numpy()[:, :6]).any(), f"iteration {k}: NaN"
        acc = ls[:, 0] == 2
        assert (ls[acc, 2] <= ls[acc, 3]).all(), f"iteration {k}: an accepted base raised M0"
        codes.append(ls[:, 0].astype(int).tolist())
        if k == 0:
            first = sc[:, 4].copy()
    last = st.SCAL.cpu().numpy()[:, 4]
    print(f"max violation: first {first.tolist()} last {last.tolist()} ratio {(first / last).tolist()}; L-BFGS after 150: {LBFGS_150}; "
          f"phases {st.ISTATE.view(B, 4)[:, 0].tolist()}; codes {sorted({c for r in codes for c in r})}; CG steps {GS[:, 0].tolist()}")
    assert np.isfinite(st.X.cpu().numpy()[:, :n]).all()
    assert (last < first).all()
    assert (last < np.array(LBFGS_150)).all(), f"not below the L-BFGS loop's 150-iteration violation: {last.tolist()}"
