"""tests/gn_ref.py (the numpy restatement of the Gauss-Newton direction and of the loop that uses it) against a dense
solve of H d = g, every stop code of the recursion, and the loop on the convex QP of tests/test_alsolve_ref.py. No GPU."""
import numpy as np
import pytest

from tests import alsolve_ref as R
from tests import gn_ref as G
from tests import lbfgs_ref
from tests.test_alsolve_ref import _evaluator, _kkt_direct, _qp

MODES = [(np.float64, False), (np.float64, True), (np.longdouble, False)]


def _sparse_problem(seed=20261021, m=14, n=9):
    """A random sparse J (an empty row, an empty column), lam+ with inactive rows, a point with held columns."""
    rng = np.random.default_rng(seed)
    mask = rng.uniform(size=(m, n)) < 0.4
    mask[3] = False                     # a row without entries
    mask[:, 5] = False                  # a column without entries
    mask[0, 0] = mask[1, 1] = True
    Jd = np.where(mask, rng.standard_normal((m, n)), 0.0)
    row_ptr = np.concatenate([[0], np.cumsum(mask.sum(1))])
    col = np.concatenate([np.flatnonzero(r) for r in mask])
    vals = Jd[mask]                     # (row-major: CSR order)
    lamp = rng.standard_normal(m)
    lamp[[2, 7, 8]] = 0.0
    lamp[9] = -0.0                      # -0.0 == 0.0: inactive
    g = rng.standard_normal(n)
    x = rng.uniform(-0.5, 0.5, n)
    lo, up = np.full(n, -1.0), np.full(n, 1.0)
    x[2], g[2] = lo[2], 0.7             # on its lower bound, the gradient pointing out: held
    x[6], g[6] = up[6], -0.4            # on its upper bound: held
    x[4], g[4] = lo[4], -0.3            # on its lower bound, the gradient pointing in: free
    lo[7] = up[7] = x[7]                # fixed: held
    return G.Pattern(row_ptr, col, n), Jd, vals, lamp, g, x, lo, up


def test_pattern_products_match_dense():
    P, Jd, vals, *_ = _sparse_problem()
    rng = np.random.default_rng(1)
    p, t = rng.standard_normal(P.n), rng.standard_normal(P.m)
    for rev in (False, True):
        assert np.allclose(G.jvec(P, vals, p, rev), Jd @ p, rtol=0, atol=1e-14)
        assert np.allclose(G.jtvec(P, vals, t, rev), Jd.T @ t, rtol=0, atol=1e-14)
    assert G.jvec(P, vals, p)[3] == 0.0 and G.jtvec(P, vals, t)[5] == 0.0


@pytest.mark.parametrize("dtype,reverse", MODES)
def test_direction_solves_the_dense_system(dtype, reverse):
    P, Jd, vals, lamp, g, x, lo, up = _sparse_problem()
    held = lbfgs_ref.held_mask(x, g, lo, up)
    assert list(np.flatnonzero(held)) == [2, 6, 7]
    free = ~held
    w = (lamp != 0).astype(float)
    assert w.sum() == P.m - 4
    rho, mu = 7.0, 0.5
    H = rho * (Jd.T * w) @ Jd
    H = H[np.ix_(free, free)] + mu * np.eye(free.sum())
    want = np.linalg.solve(H, g[free])
    d = G.direction(P, vals, lamp, rho, g, ncg=int(free.sum()), mu=mu, tol=0.0, held=held, dtype=dtype, reverse=reverse)
    assert d["steps"] == free.sum() and d["code"] == 0 and d["nheld"] == 3
    assert np.array_equal(d["D"][held].astype(np.float64), g[held])
    err = np.max(np.abs(d["D"][free].astype(np.float64) - want)) / np.max(np.abs(want))
    assert err < 1e-8, err
    assert float(d["rr"]) < 1e-16 * float(d["bb"])
    assert abs(float(d["slope"]) - (g[held] @ g[held] + g[free] @ want)) < 1e-8 * abs(g[free] @ want)
    assert abs(float(d["bb"]) - g[free] @ g[free]) < 1e-14 * (g @ g)
    # every row active is another system: the restatement does read the weights
    other = G.direction(P, vals, lamp, rho, g, ncg=int(free.sum()), mu=mu, tol=0.0, held=held, dtype=dtype, reverse=reverse, ignore_w=True)
    assert np.max(np.abs((other["D"] - d["D"])[free])) > 1e-2 * np.max(np.abs(want))
    # the residual falls monotonically in the H^-1 norm only, but the history has one entry per step and starts at 1
    assert len(d["hist"]) == d["steps"] + 1 and d["hist"][0] == 1


@pytest.mark.parametrize("dtype,reverse", MODES)
def test_every_stop_code(dtype, reverse):
    P, Jd, vals, lamp, g, x, lo, up = _sparse_problem()
    held = lbfgs_ref.held_mask(x, g, lo, up)
    kw = dict(held=held, dtype=dtype, reverse=reverse)
    # 0: ncg exhausted
    d = G.direction(P, vals, lamp, 7.0, g, ncg=2, mu=1e-3, tol=0.0, **kw)
    assert (d["steps"], d["code"]) == (2, 0) and np.array_equal(d["D"][held].astype(np.float64), g[held])
    # 1: the tolerance, between two residuals of the run above
    full = G.direction(P, vals, lamp, 7.0, g, ncg=6, mu=1e-3, tol=0.0, **kw)
    hist = [float(v) for v in full["hist"]]
    k = next(i for i in range(1, 6) if hist[i] < min(hist[:i]))      # the first step that sets a new minimum
    tol = np.sqrt(np.sqrt(hist[k] * min(hist[:k])))
    d = G.direction(P, vals, lamp, 7.0, g, ncg=6, mu=1e-3, tol=tol, **kw)
    assert (d["steps"], d["code"]) == (k, 1)
    # 1 at it == 0 (tol >= 1): no step completed, D == GR
    d = G.direction(P, vals, lamp, 7.0, g, ncg=6, mu=1e-3, tol=1.0, **kw)
    assert (d["steps"], d["code"]) == (0, 1) and np.array_equal(d["D"].astype(np.float64), g) and d["rr"] == d["bb"]
    # 2: no curvature (no active row, mu = 0), at it == 0: D == GR
    d = G.direction(P, vals, np.zeros(P.m), 7.0, g, ncg=6, mu=0.0, tol=0.0, **kw)
    assert (d["steps"], d["code"]) == (0, 2) and np.array_equal(d["D"].astype(np.float64), g)
    assert float(d["slope"]) == pytest.approx(float(g @ g), rel=1e-14)
    # 2: a NaN in the values, in the gradient, in rho
    vn = vals.copy()
    vn[4] = np.nan
    gn = g.copy()
    gn[0] = np.nan
    for v_, g_, rho_ in ((vn, g, 7.0), (vals, gn, 7.0), (vals, g, np.nan)):
        d = G.direction(P, v_, lamp, rho_, g_, ncg=6, mu=1e-3, tol=0.0, **kw)
        assert (d["steps"], d["code"]) == (0, 2)
        assert np.array_equal(d["D"].astype(np.float64).view(np.int64), g_.view(np.int64))
    # 3: nothing to solve (the gradient is zero on every free column)
    g0 = np.where(held, g, 0.0)
    d = G.direction(P, vals, lamp, 7.0, g0, ncg=6, mu=1e-3, tol=0.0, **kw)
    assert (d["steps"], d["code"]) == (0, 3) and np.array_equal(d["D"].astype(np.float64), g0) and d["bb"] == 0
    s = G.summary(d)
    assert np.array_equal(s[[0, 1, 2, 4, 5]], [0, 0, 0, 3, 3]) and s[3] == pytest.approx(float(g0 @ g0), rel=1e-14)
    # without X every column is free
    d = G.direction(P, vals, lamp, 7.0, g, ncg=1, mu=1e-3, tol=0.0, held=None, dtype=dtype, reverse=reverse)
    assert d["nheld"] == 0 and d["steps"] == 1


def _gn_evaluator(Q, c, A, gl, gu):
    inner = _evaluator(Q, c, A, gl, gu)

    def evaluate(x, lam, rho):
        return inner(x, lam, rho) + (A.reshape(-1).copy(),)
    return evaluate


@pytest.mark.parametrize("dtype,reverse", MODES)
def test_gn_loop_converges_on_the_qp(dtype, reverse):
    """The loop with the GN direction on the QP of tests/test_alsolve_ref.py. The objective's Hessian Q is not part of
    the GN system; mu = the largest eigenvalue of Q stands in for it (H then dominates the true Hessian, so the unit
    step descends)."""
    Q, c, A, lo, up, gl, gu = _qp()
    xs, lams = _kkt_direct(Q, c, A, lo, up, gl, gu)
    par = R.params(mem=4, max_inner=200, max_outer=30, rho0=2.0, rho_grow=4.0, eta_star=1e-6, omega_star=1e-6, alpha_min=1e-12)
    gn = dict(ncg=6, mu=float(np.linalg.eigvalsh(Q)[-1]), tol=1e-8)
    P = G.Pattern.dense(3, 6)
    st = R.new_state(6, 3, par["mem"], x0=np.full(6, 3.0))
    R.init(st, par, lo, up)
    trace, m0 = [], []
    for _ in range(3000):
        G.iterate(st, par, gn, P, _gn_evaluator(Q, c, A, gl, gu), lo, up, 1, dtype, reverse, trace)
        m0.append((trace[-1][0], st["LSUM"][3], st["LSUM"][2]))
        if st["ISTATE"][0] >= R.CONVERGED:
            break
    assert st["ISTATE"][0] == R.CONVERGED, (st["ISTATE"], st["SCAL"], len(trace))
    assert np.max(np.abs(st["X"] - xs)) < 1e-5 and np.max(np.abs(st["LAMP"] - lams)) < 1e-4
    assert all(mc <= before for code, before, mc in m0 if code == 2)
    assert {1, 2} <= {t[0] for t in trace} and "converged" == trace[-1][1]
    # frozen: the direction is no longer computed and nothing of the state moves
    keep = {k: np.copy(v) for k, v in st.items()}
    G.iterate(st, par, gn, P, _gn_evaluator(Q, c, A, gl, gu), lo, up, 2, dtype, reverse, trace)
    assert trace[-1][0] == 0
    for k in ("X", "GR", "LAM", "RHO", "SCAL", "ISTATE", "D", "DC", "GSUM", "ALPHA", "XC"):
        assert np.array_equal(keep[k], st[k]), k


def test_select_follows_the_flags():
    st = dict(ISTATE=np.array([R.SEARCH, 0, 0, 0], dtype=np.int32), D=np.array([1.0, 2.0]), DC=np.array([3.0, 4.0]), GR=np.array([5.0, 6.0]))
    for flags, want in ((1 | 2 | 4, "DC"), (1 | 2, "DC"), (2 | 4, "GR"), (0, "D"), (2, "D")):
        s = {k: v.copy() for k, v in st.items()}
        s["ISTATE"][1] = flags
        G.select(s)
        assert np.array_equal(s["D"], st[want]), flags
