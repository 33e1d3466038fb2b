"""The resident AL loop on the device (towr_gpu_linesearch_batch_device, towr_gpu_auglag_outer_batch_device,
towr_gpu_alsolve_init_batch_device, towr_gpu_alsolve_iterate_batch_device) against tests/alsolve_ref.py, the numpy
restatement of include/towr_gpu.h. Every state array has a padded leading dimension with NaN padding; outputs start
NaN-filled. The shapes are those of tests/test_gpu_lbfgs.py, for its reasons.

Gates. Everything the two kernels decide, copy or compute with one rounded operation is exact: phases, flags, counters,
ALPHA, RHO, the copies, SCAL (M0 = MC is one float64 addition, pg an integer maximum), LSUM[0, 2, 3, 6, 7]; HS, HY, HMETA
and USUM are bit-equal to a separate towr_gpu_lbfgs_update_batch_device call on the same operands. The three sums
(LSUM[1] gs, [4] sy, [5] yy) are sums of n terms: |got - ref| <= 2 gamma_n sum |term| + 8 u sum |term| against the long
double reference, the bound tests/test_gpu_lbfgs.py uses for the update's sums. No decision is a rounding tie: the
operands put MC a whole c1 |gs| (k = 2) or half of it (k = 0.5) from the Armijo bound, and the test asserts that the
long double and both float64 references take the same branch for every problem."""
import numpy as np
import pytest

from tests import alsolve_ref as R
from tests.configs import config_descs, cost_descs
from tests.gpu_helpers import _dev, _nan, _np_bits, _padded, _same_bits, _terrains, _vec
from tests.test_gpu_lbfgs import _gamma, _ints, _problem
from towr2025_amd import AlSolveState, TowrGpuProblem, alsolve_params
from towr2025_amd import formulation as F

pytestmark = pytest.mark.gpu

U = 2.0 ** -53
LD = np.longdouble
CASES = [("monoped_procedural", 3), ("anymal_trot_2p4s", 37), ("anymal_stairs_gaitopt", 3)]
ROWS = ("X", "GR", "XC", "GRC", "D", "LAM", "LAMP", "HS", "HY", "SCAL", "RSUM", "SSUM", "DSUM", "USUM", "LSUM")
ALL = ROWS + ("ALPHA", "RHO", "FC", "HMETA", "ISTATE")


def _state(p, B, mem, host=None):
    """An AlSolveState with padded leading dimensions, NaN everywhere (ISTATE and HMETA zero), then `host` (name ->
    (B, k) array) copied into the leading columns."""
    import torch
    n, m = p.n, p.m
    s = AlSolveState()
    s.B, s.mem = B, mem
    for k in ("X", "GR", "XC", "GRC", "D"):
        setattr(s, k, _nan(B, n + 3))
    s.LAM, s.LAMP = _nan(B, m + 5), _nan(B, m + 5)
    s.HS, s.HY = _nan(B * mem, n + 2), _nan(B * mem, n + 2)
    s.HMETA, s.ISTATE = _ints(np.zeros(2 * B)), _ints(np.zeros(4 * B))
    for k in ("ALPHA", "RHO", "FC"):
        setattr(s, k, torch.full((B,), float("nan"), dtype=torch.float64, device=_dev()))
    s.SCAL, s.LSUM, s.USUM, s.DSUM = _nan(B, 8 + 1), _nan(B, 8 + 2), _nan(B, 6 + 1), _nan(B, 5 + 2)
    s.RSUM, s.SSUM = _nan(B, 4 + p.desc.n_constraints + 3), _nan(B, 5 + p.desc.n_varsets + 3)
    for k, a in (host or {}).items():
        t = getattr(s, k)
        a = np.asarray(a)
        if t.dtype == torch.int32:
            t.copy_(_ints(a.reshape(-1)))
        elif t.dim() == 1:
            t.copy_(_vec(a))
        else:
            t[:, :a.shape[1]] = _vec(a)
    return s


def _host(s):
    return {k: getattr(s, k).cpu().numpy().copy() for k in ALL}


def _assert_same(a, b, what, keys=ALL):
    import torch
    for k in keys:
        x, y = getattr(a, k), getattr(b, k)
        assert torch.equal(x, y) if x.dtype == torch.int32 else _same_bits(x, y), f"{what}: {k}"


def _ref_problem(h, b, n, m, mem):
    """Problem b of a host copy as a state of tests/alsolve_ref.py."""
    return dict(X=h["X"][b, :n].copy(), GR=h["GR"][b, :n].copy(), XC=h["XC"][b, :n].copy(), GRC=h["GRC"][b, :n].copy(),
                D=h["D"][b, :n].copy(), LAM=h["LAM"][b, :m].copy(), LAMP=h["LAMP"][b, :m].copy(),
                HS=h["HS"][b * mem:(b + 1) * mem].copy(), HY=h["HY"][b * mem:(b + 1) * mem].copy(), HMETA=h["HMETA"][2 * b:2 * b + 2].copy(),
                ALPHA=np.float64(h["ALPHA"][b]), RHO=np.float64(h["RHO"][b]), FC=np.float64(h["FC"][b]), SCAL=h["SCAL"][b, :8].copy(),
                ISTATE=h["ISTATE"][4 * b:4 * b + 4].copy(), RSUM=h["RSUM"][b].copy(), SSUM=h["SSUM"][b].copy(), DSUM=h["DSUM"][b].copy(),
                USUM=h["USUM"][b, :6].copy(), LSUM=h["LSUM"][b, :8].copy())


def _par_dict(par):
    return {k: getattr(par, k) for k in R.DEFAULTS}


# ---- the line search ---------------------------------------------------------------------------------------------------
KINDS = ("restart", "accept", "accept_refused", "shrink", "reset", "stalled", "frozen", "garbage", "nan_mc")
LS_PAR = dict(mem=3, c1=0.25, shrink=0.5, alpha0=1.0, alpha_min=0.2, curv_eps=1e-12)


def _linesearch_operands(p, lo, up, B, mem, rnd):
    """Round `rnd` of the synthetic operands: problem b takes branch KINDS[(b + 3 rnd) % 9]."""
    n, m = p.n, p.m
    rng = np.random.default_rng(4000 + 100 * rnd + B)
    x0 = p.initial_x()
    X = np.clip(x0 + 0.05 * rng.standard_normal((B, n)), lo, up)
    GR = rng.standard_normal((B, n))
    D = GR * rng.uniform(0.5, 2.0, (B, n))
    XC = R.clamp(X - 1e-2 * D, lo, up)
    S = XC - X
    GRC = GR + rng.uniform(0.5, 2.0, (B, n)) * S
    kinds = [KINDS[(b + 3 * rnd) % 9] for b in range(B)]
    h = dict(X=X, GR=GR, D=D, XC=XC, GRC=GRC, HS=rng.standard_normal((B * mem, n)), HY=rng.standard_normal((B * mem, n)),
             LAM=rng.standard_normal((B, m)), LAMP=rng.standard_normal((B, m)), ALPHA=np.full(B, 0.5), RHO=np.full(B, 10.0),
             SCAL=np.tile([0.0, 0.3, 0.1, 0.1, 0.2, 0.9, 0.0, 0.0], (B, 1)), RSUM=np.zeros((B, 4)), FC=np.zeros(B),
             HMETA=np.zeros((B, 2), dtype=np.int32), ISTATE=np.zeros((B, 4), dtype=np.int32))
    for b, kind in enumerate(kinds):
        if kind == "accept_refused":
            GRC[b] = GR[b] - 1.5 * S[b]                       # negative curvature: sy < 0
        gs = np.sum(GR[b] * S[b])
        assert gs < 0
        m0, phi = rng.uniform(1, 2), rng.uniform(0.1, 0.5)
        k = 2.0 if kind in ("restart", "accept", "accept_refused", "frozen", "garbage") else 0.5
        h["SCAL"][b, 0] = m0
        h["RSUM"][b] = (rng.uniform(0.01, 0.1), 0.0, -1.0, phi)
        h["FC"][b] = np.nan if kind == "nan_mc" else m0 + k * LS_PAR["c1"] * gs - phi
        h["ISTATE"][b] = ({"restart": R.RESTART, "frozen": (R.CONVERGED, R.STALLED, R.MAXED)[b % 3], "garbage": (77, -5)[b % 2]}.get(kind, R.SEARCH),
                          5, 3 + b, b % 4)
        h["HMETA"][b] = {"reset": (1 + b % mem, b % mem), "stalled": ((0, 0), (99, 1))[b % 2]}.get(kind, (min(b % (mem + 2), mem), b % mem))
        if kind in ("reset", "stalled"):
            h["ALPHA"][b] = 0.3
    return h, kinds


@pytest.mark.parametrize("name,B", CASES)
def test_linesearch_against_numpy(name, B):
    check_linesearch(name, B)


def check_linesearch(name, B):
    """The line search on the handle `name` of tests/test_gpu_lbfgs.py _problem (a configuration or "sweep_seed_N")."""
    import torch
    p, lo, up, _ = _problem(name)
    n, m, mem = p.n, p.m, LS_PAR["mem"]
    par = alsolve_params(**LS_PAR)
    pd = _par_dict(par)
    per_problem_bounds = name == "monoped_procedural"      # (B, n + 2) rows of XL / XU here, the handle's own elsewhere
    XL = _padded(np.tile(lo, (B, 1)), n + 2) if per_problem_bounds else None
    XU = _padded(np.tile(up, (B, 1)), n + 2) if per_problem_bounds else None
    seen, worst = set(), 0.0
    for rnd in range(-(-9 // B) if B < 9 else 1):
        h0, kinds = _linesearch_operands(p, lo, up, B, mem, rnd)
        st = _state(p, B, mem, h0)
        before = _host(st)
        # the pair offered by the update kernel itself, on copies of the history
        HS2, HY2, M2, US2 = st.HS.clone(), st.HY.clone(), st.HMETA.clone(), _nan(B, 7)
        p.lbfgs_update_batch_device(st.X, st.XC, st.GR, st.GRC, HS2, HY2, M2, US2, mem, curv_eps=par.curv_eps)
        torch.cuda.synchronize()
        HS2, HY2, M2, US2 = HS2.cpu().numpy(), HY2.cpu().numpy(), M2.cpu().numpy(), US2.cpu().numpy()
        p.linesearch_batch_device(par, st, XL=XL, XU=XU)
        torch.cuda.synchronize()
        got = _host(st)
        for b, kind in enumerate(kinds):
            refs = {}
            for key, (dt, rev) in dict(ld=(LD, False), f64=(np.float64, False), rev=(np.float64, True)).items():
                rs = _ref_problem(before, b, n, m, mem)
                refs[key] = (rs, R.linesearch(rs, pd, lo, up, dt, rev))
            rs, info = refs["ld"]
            code = info["code"]
            assert refs["f64"][1]["code"] == code == refs["rev"][1]["code"], f"{name} problem {b} ({kind}): the references disagree"
            assert code == dict(restart=1, accept=2, accept_refused=2, shrink=3, reset=4, stalled=5, frozen=0, garbage=0, nan_mc=3)[kind]
            seen.add(kind)
            tag = f"{name} round {rnd} problem {b} ({kind})"
            assert list(got["ISTATE"][4 * b:4 * b + 4]) == list(rs["ISTATE"]), tag
            assert _np_bits(got["ALPHA"][b]) == _np_bits(rs["ALPHA"]), tag
            for k in ("X", "GR"):
                assert np.array_equal(_np_bits(got[k][b, :n]), _np_bits(rs[k])), f"{tag}: {k}"
            assert np.array_equal(_np_bits(got["SCAL"][b, :8]), _np_bits(rs["SCAL"])), f"{tag}: SCAL {got['SCAL'][b]} {rs['SCAL']}"
            took = kind in ("accept", "accept_refused")
            # the history: the update call's bits on an accepted base, untouched otherwise (HMETA zeroed by restart / reset)
            rows = slice(b * mem, (b + 1) * mem)
            for k, upd in (("HS", HS2), ("HY", HY2)):
                assert np.array_equal(_np_bits(got[k][rows]), _np_bits(upd[rows] if took else before[k][rows])), f"{tag}: {k}"
            want_meta = M2[2 * b:2 * b + 2] if took else ([0, 0] if kind in ("restart", "reset") else before["HMETA"][2 * b:2 * b + 2])
            assert list(got["HMETA"][2 * b:2 * b + 2]) == list(want_meta), tag
            assert list(got["HMETA"][2 * b:2 * b + 2]) == list(rs["HMETA"]), tag
            assert np.array_equal(_np_bits(got["USUM"][b]), _np_bits(US2[b] if took else before["USUM"][b])), f"{tag}: USUM"
            if kind == "accept":
                assert US2[b, 3] == 1.0
            if kind == "accept_refused":
                assert US2[b, 3] == 0.0 and US2[b, 5] == -1.0
            # LSUM
            L = got["LSUM"][b]
            if code == 0:
                assert L[0] == 0.0 and np.isnan(L[1:]).all(), tag
            else:
                for i in (0, 2, 3, 6, 7):
                    assert _np_bits(L[i]) == _np_bits(rs["LSUM"][i]), f"{tag}: LSUM[{i}] {L[i]} {rs['LSUM'][i]}"
                for i, key, ab in ((1, "gs", "abs_gs"), (4, "sy", "abs_sy"), (5, "yy", None)):
                    absterm = info[ab] if ab else info["yy"]
                    bound = (2 * _gamma(n) + 8 * U) * float(absterm)
                    err = abs(float(LD(L[i]) - info[key]))
                    assert err <= bound, f"{tag}: LSUM[{i}] err {err:.3e} bound {bound:.3e}"
                    worst = max(worst, err / bound if bound else 0.0)
        # nothing else moved: the other arrays, the padding, bytes past the summary widths
        for k in ("XC", "GRC", "D", "LAM", "LAMP", "RHO", "FC", "RSUM", "SSUM", "DSUM"):
            assert np.array_equal(_np_bits(got[k]), _np_bits(before[k])), f"{name}: {k} changed"
        for k, w in (("X", n), ("GR", n), ("HS", n), ("HY", n), ("SCAL", 8), ("LSUM", 8), ("USUM", 6)):
            assert np.isnan(got[k][:, w:]).all(), f"{name}: padding of {k} written"
    assert seen == set(KINDS), seen
    print(f"{name}: largest sum err / bound {worst:.3e}")


# ---- the outer update --------------------------------------------------------------------------------------------------
OUTER_PAR = dict(mem=3, max_inner=5, max_outer=3, rho_grow=10.0, rho_max=500.0, eta_star=1e-3, omega_star=1e-3, eta_shrink=0.5,
                 omega_shrink=0.1)
#               pg      eta     omega  viol     phase      flags inner outer rho
OUTER_CASES = {"converged":      (1e-4, 0.1, 0.1, 1e-4, R.SEARCH, 3, 2, 0, 10.0),
               "lam":            (0.05, 0.1, 0.1, 0.05, R.SEARCH, 3, 2, 0, 10.0),
               "lam_floor":      (0.0015, 0.0015, 0.002, 1e-3, R.SEARCH, 3, 2, 0, 10.0),
               "rho":            (0.05, 0.1, 0.1, 0.5, R.SEARCH, 3, 2, 0, 10.0),
               "rho_capped":     (0.05, 0.1, 0.1, 0.5, R.SEARCH, 3, 2, 0, 100.0),
               "nan_viol":       (0.05, 0.1, 0.1, np.nan, R.SEARCH, 3, 2, 0, 10.0),
               "forced":         (0.7, 0.1, 0.1, 0.05, R.SEARCH, 1, 5, 0, 10.0),
               "max_outer":      (0.05, 0.1, 0.1, 0.5, R.SEARCH, 3, 2, 2, 10.0),
               "idle_pg":        (0.7, 0.1, 0.1, 0.05, R.SEARCH, 3, 4, 0, 10.0),
               "idle_flag":      (0.05, 0.1, 0.1, 0.05, R.SEARCH, 2, 2, 0, 10.0),
               "idle_nan_pg":    (np.nan, 0.1, 0.1, 0.05, R.SEARCH, 3, 2, 0, 10.0),
               "idle_restart":   (0.05, 0.1, 0.1, 0.05, R.RESTART, 3, 2, 0, 10.0),
               "idle_frozen":    (0.05, 0.1, 0.1, 0.05, R.CONVERGED, 3, 2, 0, 10.0),
               "idle_garbage":   (0.05, 0.1, 0.1, 0.05, 99, 3, 2, 0, 10.0)}


@pytest.mark.parametrize("name,B", CASES)
def test_outer_against_numpy(name, B):
    check_outer(name, B)


def check_outer(name, B):
    """The outer update on the handle `name` of tests/test_gpu_lbfgs.py _problem."""
    import torch
    p, lo, up, _ = _problem(name)
    n, m, mem = p.n, p.m, OUTER_PAR["mem"]
    par = alsolve_params(**OUTER_PAR)
    pd = _par_dict(par)
    names = list(OUTER_CASES)
    did_all = set()
    for rnd in range(-(-len(names) // B)):
        rng = np.random.default_rng(6000 + rnd)
        mine = [names[(b + B * rnd) % len(names)] for b in range(B)]
        c = np.array([OUTER_CASES[k] for k in mine])
        h0 = dict(LAM=rng.standard_normal((B, m)), LAMP=rng.standard_normal((B, m)), ALPHA=np.full(B, 0.5), RHO=c[:, 8],
                  SCAL=np.column_stack([np.ones(B), c[:, 0], c[:, 1], c[:, 2], c[:, 3], np.full(B, 0.9), np.zeros(B), np.zeros(B)]),
                  ISTATE=c[:, 4:8].astype(np.int32), HMETA=np.tile([2, 1], (B, 1)))
        st = _state(p, B, mem, h0)
        before = _host(st)
        p.auglag_outer_batch_device(par, st)
        torch.cuda.synchronize()
        got = _host(st)
        for b, k in enumerate(mine):
            rs = _ref_problem(before, b, n, m, mem)
            did = R.outer(rs, pd)
            did_all.add((k, did))
            tag = f"{name} problem {b} ({k})"
            assert (did is None) == k.startswith("idle"), tag
            assert list(got["ISTATE"][4 * b:4 * b + 4]) == list(rs["ISTATE"]) and list(got["HMETA"][2 * b:2 * b + 2]) == list(rs["HMETA"]), tag
            for key, val in (("ALPHA", rs["ALPHA"]), ("RHO", rs["RHO"])):
                assert _np_bits(got[key][b]) == _np_bits(val), f"{tag}: {key}"
            assert np.array_equal(_np_bits(got["SCAL"][b, :8]), _np_bits(rs["SCAL"])), f"{tag}: SCAL"
            assert np.array_equal(_np_bits(got["LAM"][b, :m]), _np_bits(rs["LAM"])), f"{tag}: LAM"
        for k in ROWS + ("FC",):
            if k not in ("LAM", "SCAL"):
                assert np.array_equal(_np_bits(got[k]), _np_bits(before[k])), f"{name}: {k} changed"
        assert np.isnan(got["LAM"][:, m:]).all() and np.isnan(got["SCAL"][:, 8:]).all(), f"{name}: padding written"
    want = {"converged": "converged", "lam": "lam", "lam_floor": "lam", "rho": "rho", "rho_capped": "rho", "nan_viol": "rho",
            "forced": "lam", "max_outer": "rho"}
    assert did_all == {(k, want.get(k)) for k in names}


# ---- per-problem rho ---------------------------------------------------------------------------------------------------
def _start(p, lo, up, B, mem, seed, sigma=0.05):
    n, m = p.n, p.m
    rng = np.random.default_rng(seed)
    x0 = p.initial_x()
    X = np.stack([x0 + sigma * np.random.default_rng(seed + 1 + b).standard_normal(n) for b in range(B)])
    return dict(X=X, LAM=0.1 * rng.standard_normal((B, m)))


@pytest.mark.parametrize("name,B", [("monoped_procedural", 3), ("anymal_trot_2p4s", 37)])
def test_per_problem_rho_equals_the_scalar_calls(name, B):
    """The evaluation inside one iteration with a RHO row of distinct values against B = 1 calls of the public
    towr_gpu_eval_auglag_batch_device with that scalar rho, row by row and bit for bit, in two batch orders."""
    import torch
    p, lo, up, _ = _problem(name)
    n, m, mem = p.n, p.m, 2
    par = alsolve_params(mem=mem)
    h0 = _start(p, lo, up, B, mem, 7100)
    rho = 1.0 + 0.37 * np.arange(B)
    outs = []
    for order in (np.arange(B), np.arange(B)[::-1]):
        st = _state(p, B, mem, {k: v[order] for k, v in h0.items()})
        p.alsolve_init(par, st)
        st.RHO.copy_(_vec(rho[order]))
        XC, LAM = st.XC.clone(), st.LAM.clone()
        p.alsolve_iterate(par, st, iters=1)
        torch.cuda.synchronize()
        inv = np.argsort(order)
        outs.append({k: getattr(st, k)[torch.from_numpy(inv).to(_dev())] for k in ("LAMP", "RSUM", "GRC", "FC")})
        if order[0] != 0:
            continue
        nc = p.desc.n_constraints
        for b in range(B):
            Fb, Gb = torch.full((1,), float("nan"), dtype=torch.float64, device=_dev()), _nan(1, n + 3)
            LPb, RSb = _nan(1, m + 5), _nan(1, 4 + nc + 3)
            p.eval_cost_batch_device(XC[b:b + 1], Fb, GRAD=Gb)
            p.eval_auglag_batch_device(XC[b:b + 1], RSb, Gb, LAM=LAM[b:b + 1], rho=float(rho[b]), LAMP=LPb, accumulate=True)
            for k, t in (("LAMP", LPb), ("RSUM", RSb), ("GRC", Gb)):
                assert _same_bits(getattr(st, k)[b:b + 1], t), f"{name} problem {b}: {k}"
            assert _same_bits(st.FC[b:b + 1], Fb), f"{name} problem {b}: FC"
        assert np.isfinite(st.LAMP.cpu().numpy()[:, :m]).all()
    for k in outs[0]:
        assert _same_bits(outs[0][k], outs[1][k]), f"{name}: {k} depends on the position in the batch"


# ---- the fused entry ---------------------------------------------------------------------------------------------------
def _pieces_iteration(p, par, st):
    """One iteration by the public calls. The evaluation takes a scalar rho: one call per distinct RHO value, its rows
    kept; the direction is unmasked: the rows whose flag bit 1 is clear keep their D and DSUM."""
    import torch
    B, mem = st.B, st.mem
    p.eval_cost_batch_device(st.XC, st.FC, GRAD=st.GRC)
    rho = st.RHO.cpu().numpy()
    G0, LP, RS = st.GRC.clone(), st.LAMP.clone(), st.RSUM.clone()
    for r in np.unique(rho):
        g, lp, rs = G0.clone(), LP.clone(), RS.clone()
        p.eval_auglag_batch_device(st.XC, rs, g, LAM=st.LAM, rho=float(r), LAMP=lp, accumulate=True)
        rows = torch.from_numpy(np.flatnonzero(rho == r)).to(_dev())
        st.GRC[rows], st.LAMP[rows], st.RSUM[rows] = g[rows], lp[rows], rs[rows]
    p.linesearch_batch_device(par, st)
    p.auglag_outer_batch_device(par, st)
    run = torch.nonzero(st.ISTATE.view(B, 4)[:, 1] & 2).flatten()
    D, DS = st.D.clone(), st.DSUM.clone()
    p.lbfgs_direction_batch_device(st.GR, st.HS, st.HY, st.HMETA, D, DS, mem, X=st.X)
    st.D[run], st.DSUM[run] = D[run], DS[run]
    p.step_batch_device(st.X, st.D, st.SSUM, XP=st.XC, alpha=st.ALPHA)
    torch.cuda.synchronize()


FUSED_PAR = dict(mem=3, shrink=0.03, curv_eps=1e-14, max_inner=12, max_outer=4, alpha_min=1e-16, rho_grow=3.0)
FUSED_ITERS = 24


@pytest.mark.parametrize("name,B", [("anymal_all_costs", 5), ("anymal_stairs_gaitopt_costs", 3)])
def test_fused_entry_is_bit_identical_to_the_pieces(name, B):
    """FUSED_ITERS iterate(iters=1) calls against the public calls in sequence, in every state array after every
    iteration, at the automatic products chunk and at chunk 2 (a ragged last chunk), with batch terrains set and a RHO row
    of distinct values; iterate(iters=3) against three iterate(iters=1)."""
    gait = name == "anymal_stairs_gaitopt_costs"
    f = F.with_costs(F.anymal_trot(terrain=F.HeightMap.MakeTerrain(F.HeightMap.StairsID), optimize_timings=True) if gait else F.anymal_trot())
    f.params_.enable_stance_tracking = False
    p = TowrGpuProblem(cost_descs()[name], device=0, data=f.var_bounds_data())
    lo, up = p.variable_bounds()
    p.set_batch_terrain(_terrains(name, B, np.random.default_rng(7)))
    check_fused(name, p, lo, up, B, FUSED_ITERS, {1, 2, 3})


def empty_sets(p):
    """The constraint sets without rows."""
    return [s for s, (_, _, _, rows) in enumerate(p.constraint_info()) if rows == 0]


def check_fused(name, p, lo, up, B, iters, need):
    """`iters` iterate(iters=1) calls on the handle p against the public calls in sequence (every state array after
    every iteration, products chunks 0 and 2, a RHO row of distinct values), then iterate(iters=3) against three calls.
    `need`: the line-search codes (LSUM[0]) that must occur in the run. The maximum of a constraint set without rows stays
    +0.0 in RSUM through every residual call of the loop. Returns the codes per iteration."""
    import torch
    mem = FUSED_PAR["mem"]
    par = alsolve_params(**FUSED_PAR)
    h0 = _start(p, lo, up, B, mem, 7300)
    empty = empty_sets(p)

    def fresh():
        st = _state(p, B, mem, h0)
        p.alsolve_init(par, st)
        st.RHO.copy_(_vec(10.0 * (1.0 + 0.25 * np.arange(B))))
        return st
    want, ref, codes = [], fresh(), []
    xc = ref.XC.cpu().numpy()[:, :p.n]
    assert (xc >= lo).all() and (xc <= up).all() and np.isnan(ref.XC.cpu().numpy()[:, p.n:]).all()
    for k in range(iters):
        _pieces_iteration(p, par, ref)
        want.append(ref.clone())
        codes.append(ref.LSUM[:, 0].cpu().numpy().astype(int).tolist())
    print(f"{name}: LSUM[0] per iteration {codes}; phases {ref.ISTATE.view(B, 4)[:, 0].tolist()} outer {ref.ISTATE.view(B, 4)[:, 3].tolist()}")
    flat = {c for row in codes for c in row}
    assert need <= flat, f"codes {sorted(need - flat)} do not occur in the run: the comparison would show nothing"
    assert (want[-1].HMETA.view(B, 2)[:, 0] > 0).any() or any((w.DSUM[:, 0] > 0).any() for w in want), "no pair was ever used"
    try:
        for chunk in (0, 2):
            p.set_products_chunk(chunk)
            st = fresh()
            for k in range(iters):
                p.alsolve_iterate(par, st)
                torch.cuda.synchronize()
                _assert_same(st, want[k], f"{name} chunk {chunk} iteration {k}")
                for s_ in empty:
                    assert (_np_bits(st.RSUM.cpu().numpy()[:, 4 + s_]) == 0).all(), f"{name} iteration {k}: the maximum of empty set {s_} is not +0.0"
            st = fresh()
            p.alsolve_iterate(par, st, iters=3)
            torch.cuda.synchronize()
            _assert_same(st, want[2], f"{name} chunk {chunk} iters=3")
    finally:
        p.set_products_chunk(0)
    return codes


def test_fused_rows_do_not_depend_on_batch_stream_or_run():
    """A row's bits after a few iterations: in the batch, alone (B = 1) on another stream, and run to run; and the kept
    Jacobian survives the calls."""
    import torch
    name, B, K = "anymal_stairs_gaitopt", 3, 6
    _, lo, up, vb = _problem(name)
    p = TowrGpuProblem(config_descs()[name], device=0, data=vb)
    mem = FUSED_PAR["mem"]
    par = alsolve_params(**FUSED_PAR)
    h0 = _start(p, lo, up, B, mem, 7500)
    x = h0["X"][1]
    v_ref = p.eval_jac_values(x)
    p.eval_g_keep_jac(x)

    def run(rows, stream=None):
        st = _state(p, len(rows), mem, {k: v[rows] for k, v in h0.items()})
        if stream is not None:
            stream.wait_stream(torch.cuda.current_stream())
        p.alsolve_init(par, st, stream=stream)
        p.alsolve_iterate(par, st, iters=K, stream=stream)
        torch.cuda.synchronize()
        return st
    a = run([0, 1, 2])
    v = p.eval_jac_values_kept(x)
    assert np.array_equal(v.view(np.int64), v_ref.view(np.int64)), "the kept Jacobian was dropped"
    b = run([0, 1, 2])
    _assert_same(a, b, "run to run")
    one = run([1], torch.cuda.Stream(device=_dev()))
    for k in ALL:
        t, o = getattr(a, k), getattr(one, k)
        per = t.shape[0] // B
        assert torch.equal(t[per:2 * per].view(torch.int32 if t.dtype == torch.int32 else torch.int64),
                           o.view(torch.int32 if o.dtype == torch.int32 else torch.int64)), f"B = 1 on another stream: {k}"
    assert np.isfinite(a.X.cpu().numpy()[:, :p.n]).all() and (a.ISTATE.view(B, 4)[:, 2] > 0).all()


# ---- a short solve -----------------------------------------------------------------------------------------------------
SOLVE_PAR = dict(mem=8, shrink=0.1, rho0=10.0, curv_eps=1e-14, max_inner=200, alpha_min=1e-16)
SOLVE_K = 150


def test_short_solve_reduces_the_violation():
    """monoped_procedural, B = 3, x0 perturbed by 0.05 sigma, SOLVE_K iterations of iterate(iters=1) with SCAL read
    between the calls. Asserted: no NaN appears, an accepted base never raises M0, and every problem's max violation
    (SCAL[4]) ends below its value after the first evaluation. tests/alsolve_ref.py driven by the CPU oracle with these
    parameters drops it from 1.66e3 / 2.53e3 / 1.91e3 to 20.0 / 21.1 / 19.9 (83x / 120x / 96x) in both float64 summation
    orders, so the assertion has room. The iterates are NOT compared with the reference: a rounding
    difference in a sum may steer an accept / reject decision, after which the two runs are different, equally valid
    solves. A second run with max_inner = 12 and max_outer = 1 drives every problem to MAXED; from then on no bit of a
    frozen problem's state changes."""
    import torch
    name, B = "monoped_procedural", 3
    p, lo, up, _ = _problem(name)
    n, mem = p.n, SOLVE_PAR["mem"]
    par = alsolve_params(**SOLVE_PAR)
    x0 = p.initial_x()
    h0 = dict(X=np.stack([x0 + 0.05 * np.random.default_rng(900 + b).standard_normal(n) for b in range(B)]), LAM=np.zeros((B, p.m)))
    st = _state(p, B, mem, h0)
    p.alsolve_init(par, st)
    first = None
    for k in range(SOLVE_K):
        p.alsolve_iterate(par, st)
        sc, ls = st.SCAL.cpu().numpy()[:, :8], st.LSUM.cpu().numpy()[:, :8]
        assert not np.isnan(sc).any() and not np.isnan(ls).any(), f"iteration {k}: NaN"
        acc = ls[:, 0] == 2
        assert (ls[acc, 2] <= ls[acc, 3]).all(), f"iteration {k}: an accepted base raised M0"
        if k == 0:
            first = sc[:, 4].copy()
    last = st.SCAL.cpu().numpy()[:, 4]
    print(f"max violation: first {first.tolist()} last {last.tolist()} ratio {(first / last).tolist()}; "
          f"phases {st.ISTATE.view(B, 4)[:, 0].tolist()} inner {st.ISTATE.view(B, 4)[:, 2].tolist()}")
    assert np.isfinite(st.X.cpu().numpy()[:, :n]).all()
    assert (last < first).all()

    par2 = alsolve_params(**{**SOLVE_PAR, "max_inner": 12, "max_outer": 1})
    st = _state(p, B, mem, h0)
    p.alsolve_init(par2, st)
    p.alsolve_iterate(par2, st, iters=60)
    torch.cuda.synchronize()
    assert st.ISTATE.view(B, 4)[:, 0].tolist() == [R.MAXED] * B, st.ISTATE.view(B, 4).tolist()
    p.alsolve_iterate(par2, st, iters=2)                      # (the frozen code LSUM[0] = 0 and XC = P(X) settle here)
    keep = st.clone()
    p.alsolve_iterate(par2, st, iters=3)
    torch.cuda.synchronize()
    _assert_same(st, keep, "frozen problems")
