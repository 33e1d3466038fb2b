"""tests/alsolve_ref.py (the numpy restatement of the resident AL loop) against a box-and-range-constrained convex QP
whose KKT point numpy solves directly, and every branch of the two state machines on hand-made states. No GPU."""
import numpy as np
import pytest

from tests import alsolve_ref as R

INF = 1e20


def _qp():
    """min 0.5 x'Qx + c'x, lo <= x <= up, gl <= Ax <= gu, built so that the active set at the solution is known: x_0 on
    its upper bound, row 0 an equality, row 1 on its upper side, row 2 inactive."""
    rng = np.random.default_rng(20261020)
    n, m = 6, 3
    Mx = rng.standard_normal((n, n))
    Q = Mx @ Mx.T + n * np.eye(n)
    A = rng.standard_normal((m, n))
    xs = rng.uniform(-0.5, 0.5, n)
    lo, up = np.full(n, -2.0), np.full(n, 2.0)
    lo[3] = -INF                      # a side that does not count
    up[0] = xs[0]
    lam = np.array([0.7, 1.3, 0.0])   # row 1 on its upper side: lam > 0
    z = np.zeros(n)
    z[0] = 0.9                        # the bound's multiplier (upper: > 0)
    c = -(Q @ xs + A.T @ lam + z)
    g = A @ xs
    gl = np.array([g[0], -INF, g[2] - 1.0])
    gu = np.array([g[0], g[1], g[2] + 1.0])
    return Q, c, A, lo, up, gl, gu


def _kkt_direct(Q, c, A, lo, up, gl, gu):
    """The KKT point with the active set above, by one linear solve; the KKT conditions are then checked."""
    n = Q.shape[0]
    free = np.arange(1, n)
    act = [0, 1]
    K = np.block([[Q[np.ix_(free, free)], A[np.ix_(act, free)].T], [A[np.ix_(act, free)], np.zeros((2, 2))]])
    rhs = np.concatenate([-(c[free] + Q[free, 0] * up[0]), np.array([gl[0], gu[1]]) - A[act, 0] * up[0]])
    sol = np.linalg.solve(K, rhs)
    x = np.concatenate([[up[0]], sol[:n - 1]])
    lam = np.array([sol[n - 1], sol[n], 0.0])
    z0 = -(Q @ x + c + A.T @ lam)[0]
    g = A @ x
    assert z0 > 0 and lam[1] > 0 and gl[2] < g[2] < gu[2] and np.all(x[1:] > lo[1:]) and np.all(x[1:] < up[1:])
    return x, lam


def _evaluator(Q, c, A, gl, gu):
    def evaluate(x, lam, rho):
        g = A @ x
        t = g + lam / rho
        r = t - R.clamp(t, gl, gu)
        lamp = rho * r
        phi = np.sum(0.5 * rho * r * r - 0.5 * lam * lam / rho)
        has_l, has_u = gl > -R.SIDE_INF, gu < R.SIDE_INF
        viol = max(0.0, np.max(np.where(has_l, gl - g, 0.0)), np.max(np.where(has_u, g - gu, 0.0)))
        return 0.5 * x @ Q @ x + c @ x, Q @ x + c + A.T @ lamp, lamp, viol, phi
    return evaluate


@pytest.mark.parametrize("dtype,reverse", [(np.float64, False), (np.float64, True), (np.longdouble, False)])
def test_qp_converges_to_the_kkt_point(dtype, reverse):
    Q, c, A, lo, up, gl, gu = _qp()
    xs, lams = _kkt_direct(Q, c, A, lo, up, gl, gu)
    par = R.params(mem=4, max_inner=40, max_outer=30, rho0=2.0, rho_grow=4.0, eta_star=1e-6, omega_star=1e-6, alpha_min=1e-12)
    st = R.new_state(6, 3, par["mem"], x0=np.full(6, 3.0))   # outside the box: init clamps
    R.init(st, par, lo, up)
    assert np.all(st["XC"] <= up) and np.all(st["XC"] >= np.where(lo > -1e19, lo, -np.inf))
    trace, m0 = [], []
    for _ in range(600):
        R.iterate(st, par, _evaluator(Q, c, A, gl, gu), lo, up, 1, dtype, reverse, trace)
        m0.append((trace[-1][0], st["LSUM"][3], st["LSUM"][2]))
        if st["ISTATE"][0] >= R.CONVERGED:
            break
    assert st["ISTATE"][0] == R.CONVERGED, (st["ISTATE"], st["SCAL"])
    assert np.max(np.abs(st["X"] - xs)) < 1e-5 and np.max(np.abs(st["LAMP"] - lams)) < 1e-4
    assert st["ALPHA"] == 0.0 and st["ISTATE"][1] == 0
    # the merit at the base never increases between two outer updates: an accepted base's MC is at most the M0 before
    assert all(mc <= before for code, before, mc in m0 if code == 2)
    codes = {t[0] for t in trace}
    assert {1, 2, 3} <= codes and "lam" in {t[1] for t in trace} and "converged" == trace[-1][1]
    # frozen: a further iteration changes nothing but LSUM[0] / the flags
    keep = {k: np.copy(v) for k, v in st.items()}
    R.iterate(st, par, _evaluator(Q, c, A, gl, gu), lo, up, 2, dtype, reverse, trace)
    assert trace[-1][0] == 0
    for k in ("X", "GR", "LAM", "RHO", "SCAL", "ISTATE", "HMETA", "HS", "HY", "ALPHA", "XC"):
        assert np.array_equal(keep[k], st[k]), k


def _search_state(par, n=5, m=2, seed=1):
    rng = np.random.default_rng(seed)
    st = R.new_state(n, m, par["mem"], rng.uniform(-1, 1, n))
    st["GR"] = rng.standard_normal(n)
    st["D"] = st["GR"].copy()
    st["XC"] = st["X"] - 0.5 * st["GR"]
    st["GRC"] = st["GR"] * 0.5            # y = -0.5 g, s = -0.5 g: sy > 0
    st["ISTATE"][:] = (R.SEARCH, 0, 3, 1)
    st["ALPHA"], st["RHO"] = np.float64(0.5), np.float64(10.0)
    st["SCAL"][:] = (1.0, 0.3, 0.1, 0.1, 0.2, 0.9, 0, 0)
    st["RSUM"][:] = (0.05, 0, 0, 0.25)
    return st


def _set_mc(st, par, k):
    """FC such that MC = M0 + k c1 gs."""
    gs = np.sum(st["GR"] * (st["XC"] - st["X"]))
    st["FC"] = np.float64(st["SCAL"][0] + k * par["c1"] * gs - st["RSUM"][3])
    return gs


def test_every_linesearch_branch():
    par = R.params(mem=3, c1=0.25, alpha_min=0.2)
    lo, up = np.full(5, -INF), np.full(5, INF)
    seen = set()
    # restart
    st = _search_state(par)
    st["ISTATE"][0] = R.RESTART
    st["HMETA"][:] = (2, 1)
    st["FC"] = np.float64(2.0)
    xc, grc = st["XC"].copy(), st["GRC"].copy()
    seen.add(R.linesearch(st, par, lo, up)["code"])
    assert list(st["ISTATE"]) == [R.SEARCH, 7, 4, 1] and list(st["HMETA"]) == [0, 0] and st["ALPHA"] == par["alpha0"]
    assert np.array_equal(st["X"], xc) and np.array_equal(st["GR"], grc)
    assert st["SCAL"][0] == 2.25 and st["SCAL"][4] == 0.05 and st["SCAL"][5] == 2.0 and st["SCAL"][1] == np.max(np.abs((xc - grc) - xc))
    assert list(st["LSUM"][[0, 1, 4, 5, 6]]) == [1, 0, 0, 0, 0]
    # accept, the pair stored
    st = _search_state(par)
    _set_mc(st, par, 2.0)
    s_pair = st["XC"] - st["X"]
    seen.add(R.linesearch(st, par, lo, up)["code"])
    assert list(st["ISTATE"]) == [R.SEARCH, 3, 4, 1] and list(st["HMETA"]) == [1, 1] and st["LSUM"][6] == 1 and st["USUM"][3] == 1
    assert np.array_equal(st["HS"][0], s_pair)
    # accept, the pair refused by curvature (y = 0)
    st = _search_state(par)
    st["GRC"] = st["GR"].copy()
    _set_mc(st, par, 2.0)
    info = R.linesearch(st, par, lo, up)
    assert info["code"] == 2 and list(st["HMETA"]) == [0, 0] and st["LSUM"][6] == 0 and st["USUM"][5] == -1
    # shrink
    st = _search_state(par)
    _set_mc(st, par, 0.5)
    keep = {k: np.copy(v) for k, v in st.items()}
    seen.add(R.linesearch(st, par, lo, up)["code"])
    assert st["ALPHA"] == 0.25 and list(st["ISTATE"]) == [R.SEARCH, 0, 4, 1]
    for k in ("X", "GR", "D", "HS", "HY", "HMETA", "SCAL"):
        assert np.array_equal(keep[k], st[k])
    # history reset: below alpha_min with a pair held
    st = _search_state(par)
    _set_mc(st, par, 0.5)
    st["ALPHA"], st["HMETA"][:] = np.float64(0.3), (1, 1)
    seen.add(R.linesearch(st, par, lo, up)["code"])
    assert st["ALPHA"] == par["alpha0"] and list(st["ISTATE"]) == [R.SEARCH, 6, 4, 1] and list(st["HMETA"]) == [0, 0]
    # stalled: below alpha_min, nothing held
    st = _search_state(par)
    _set_mc(st, par, 0.5)
    st["ALPHA"] = np.float64(0.3)
    seen.add(R.linesearch(st, par, lo, up)["code"])
    assert st["ALPHA"] == 0 and list(st["ISTATE"]) == [R.STALLED, 0, 4, 1]
    # a NaN merit rejects; an uphill step (gs > 0) rejects whatever the merit
    st = _search_state(par)
    st["FC"] = np.float64(np.nan)
    assert R.linesearch(st, par, lo, up)["code"] == 3
    st = _search_state(par)
    st["XC"] = st["X"] + 0.5 * st["GR"]
    st["FC"] = np.float64(-1e9)
    assert R.linesearch(st, par, lo, up)["code"] == 3
    # frozen and garbage phases
    for ph in (R.CONVERGED, R.STALLED, R.MAXED, 77, -3):
        st = _search_state(par)
        st["ISTATE"][:2] = (ph, 5)
        st["LSUM"][:] = 9.0
        keep = {k: np.copy(v) for k, v in st.items()}
        seen.add(R.linesearch(st, par, lo, up)["code"])
        assert list(st["ISTATE"]) == [ph, 0, 3, 1] and list(st["LSUM"]) == [0.0] + [9.0] * 7
        for k in st:
            if k not in ("ISTATE", "LSUM"):
                assert np.array_equal(keep[k], st[k], equal_nan=True), k
    assert seen == {0, 1, 2, 3, 4, 5}
    # pg respects the box: a column on its bound with the gradient pointing out does not count
    st = _search_state(par)
    _set_mc(st, par, 2.0)
    lo2 = st["XC"] - np.array([0, 1e-3, INF, INF, INF])
    st["GRC"] = np.array([5.0, 5.0, 0.1, -0.2, 0.0])
    xc = st["XC"].copy()
    R.linesearch(st, par, lo2, up)
    assert st["SCAL"][1] == abs((xc[3] + 0.2) - xc[3]) < 0.21   # (not the 5.0 of the two columns the box stops)


def test_every_outer_branch():
    par = R.params(mem=3, max_inner=5, max_outer=3, rho_grow=10.0, rho_max=500.0, eta_star=1e-3, omega_star=1e-3, eta_shrink=0.5,
                   omega_shrink=0.1)
    seen, phases = set(), set()

    def case(scal, istate, rho=10.0):
        st = _search_state(par)
        st["SCAL"][:] = scal
        st["ISTATE"][:] = istate
        st["RHO"] = np.float64(rho)
        st["LAMP"] = np.array([3.0, -4.0])
        st["HMETA"][:] = (2, 1)
        keep = {k: np.copy(v) for k, v in st.items()}
        did = R.outer(st, par)
        seen.add(did)
        phases.add(int(st["ISTATE"][0]))
        return st, keep, did
    #          M0   pg    eta  omega viol f
    st, _, did = case((1.0, 1e-4, 0.1, 0.1, 1e-4, 0, 0, 0), (R.SEARCH, 3, 2, 0))
    assert did == "converged" and list(st["ISTATE"]) == [R.CONVERGED, 0, 2, 0] and st["ALPHA"] == 0 and list(st["HMETA"]) == [2, 1]
    st, _, did = case((1.0, 0.05, 0.1, 0.1, 0.05, 0, 0, 0), (R.SEARCH, 3, 2, 0))
    assert did == "lam" and list(st["LAM"]) == [3.0, -4.0] and st["SCAL"][2] == 0.05 and st["SCAL"][3] == 0.1 * 0.1
    assert list(st["ISTATE"]) == [R.RESTART, 0, 0, 1] and list(st["HMETA"]) == [0, 0] and st["ALPHA"] == 0 and st["RHO"] == 10.0
    st, _, did = case((1.0, 0.0015, 0.0015, 0.002, 1e-3, 0, 0, 0), (R.SEARCH, 3, 2, 0))   # the schedules stop at the stars
    assert did == "lam" and st["SCAL"][2] == 1e-3 and st["SCAL"][3] == 1e-3
    st, keep, did = case((1.0, 0.05, 0.1, 0.1, 0.5, 0, 0, 0), (R.SEARCH, 3, 2, 0))
    assert did == "rho" and st["RHO"] == 100.0 and np.array_equal(st["LAM"], keep["LAM"]) and st["SCAL"][2] == 0.1
    st, _, did = case((1.0, 0.05, 0.1, 0.1, 0.5, 0, 0, 0), (R.SEARCH, 3, 2, 0), rho=100.0)
    assert did == "rho" and st["RHO"] == 500.0                                           # capped
    st, keep, did = case((1.0, 0.05, 0.1, 0.1, np.nan, 0, 0, 0), (R.SEARCH, 3, 2, 0))
    assert did == "rho" and st["RHO"] == 100.0 and np.array_equal(st["LAM"], keep["LAM"])
    st, _, did = case((1.0, 0.7, 0.1, 0.1, 0.05, 0, 0, 0), (R.SEARCH, 1, 5, 0))          # pg > omega, forced by max_inner
    assert did == "lam" and list(st["ISTATE"]) == [R.RESTART, 0, 0, 1]
    st, _, did = case((1.0, 0.05, 0.1, 0.1, 0.5, 0, 0, 0), (R.SEARCH, 3, 2, 2))          # max_outer reached
    assert did == "rho" and list(st["ISTATE"]) == [R.MAXED, 0, 0, 3]
    for scal, ist in (((1.0, 0.7, 0.1, 0.1, 0.05, 0, 0, 0), (R.SEARCH, 3, 4, 0)),        # pg > omega, inner < max_inner
                      ((1.0, 0.05, 0.1, 0.1, 0.05, 0, 0, 0), (R.SEARCH, 2, 2, 0)),       # no base accepted in this iteration
                      ((1.0, np.nan, 0.1, 0.1, 0.05, 0, 0, 0), (R.SEARCH, 3, 2, 0)),     # a NaN pg is not <= omega
                      ((1.0, 0.05, 0.1, 0.1, 0.05, 0, 0, 0), (R.RESTART, 3, 2, 0)),
                      ((1.0, 0.05, 0.1, 0.1, 0.05, 0, 0, 0), (R.CONVERGED, 3, 2, 0)),
                      ((1.0, 0.05, 0.1, 0.1, 0.05, 0, 0, 0), (99, 3, 2, 0))):
        st, keep, did = case(scal, ist)
        assert did is None
        for k in st:
            assert np.array_equal(keep[k], st[k], equal_nan=True), k
    assert seen == {None, "converged", "lam", "rho"} and {R.CONVERGED, R.RESTART, R.MAXED} <= phases


def test_loop_reaches_stalled_and_maxed():
    """STALLED and MAXED through the loop itself: a merit that never decreases, and max_outer = 1."""
    Q, c, A, lo, up, gl, gu = _qp()
    ev = _evaluator(Q, c, A, gl, gu)
    par = R.params(mem=2, max_outer=1, max_inner=3, alpha_min=1e-3)
    st = R.new_state(6, 3, 2, np.zeros(6))
    R.init(st, par, lo, up)
    trace = []
    R.iterate(st, par, ev, lo, up, 12, trace=trace)
    assert st["ISTATE"][0] == R.MAXED and st["ISTATE"][3] == 1
    calls = [0]

    def rising(x, lam, rho):   # f grows with every call: nothing is ever accepted after the restart
        calls[0] += 1
        f, gr, lamp, viol, phi = ev(x, lam, rho)
        return f + calls[0], gr, lamp, viol, phi
    par = R.params(mem=2, alpha_min=1e-2, max_inner=1000, omega0=1e-12, omega_star=1e-12)
    st = R.new_state(6, 3, 2, np.zeros(6))
    R.init(st, par, lo, up)
    trace = []
    R.iterate(st, par, rising, lo, up, 12, trace=trace)
    assert st["ISTATE"][0] == R.STALLED and st["ALPHA"] == 0 and [t[0] for t in trace][:9] == [1, 3, 3, 3, 3, 3, 3, 5, 0]
