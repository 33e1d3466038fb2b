"""tests/chol_ref.py (the numpy restatement of the direct Gauss-Newton direction and of the loop that uses it) against a
dense solve of H d = g, every code, two deliberately wrong systems; the ordering and envelope of
towr_gpu_gn_factor_info on layout-only handles of every configuration and sweep seed; and a short solve of
monoped_procedural driven by the CPU oracle. No GPU."""
import functools

import numpy as np
import pytest

from tests import alsolve_ref as R
from tests import chol_ref as CH
from tests import gn_ref as G
from tests import lbfgs_ref
from tests.configs import config_descs
from tests.shape_sweep import make
from tests.test_gn_ref import MODES, _sparse_problem
from tests.test_pgn_ref import SOLVE_PAR, _monoped
from towr2025_amd import TowrGpuProblem
from towr2025_amd import _capi as capi

SWEEP_SEEDS = (154, 196, 16, 194, 13, 131, 126, 10, 0, 93, 39, 175, 66)   # DESIGN 4k's table (tests/test_gpu_sweep_consumers.py)
SOLVE_MU = 1e-6
SOLVE_K = 100
SOLVE_SEEDS = (900, 901, 902, 903, 904, 905)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def _orderings(P):
    """The identity and a seeded permutation, each with its envelope."""
    out = []
    for pos in (np.arange(P.n), np.random.default_rng(5).permutation(P.n)):
        first, env, bw = CH.envelope(P, pos)
        out.append((pos, first))
    return out


def _gate(P, vals, lamp, rho, g, mu, held, pos, first):
    """8 x the larger backward error of the two float64 references (the factor of tests/gn_gate.py)."""
    errs = []
    for rev in (False, True):
        d = CH.direction(P, vals, lamp, rho, g, mu, pos, first, held=held, reverse=rev)
        assert d["code"] == 1
        errs.append(CH.backward_error(P, vals, lamp, rho, g, mu, held, d["D"]))
    return 8 * max(errs)


@pytest.mark.parametrize("dtype,reverse", MODES)
def test_direction_solves_the_dense_system(dtype, reverse):
    P, Jd, vals, lamp, g, x, lo, up = _sparse_problem()
    held = lbfgs_ref.held_mask(x, g, lo, up)
    assert list(np.flatnonzero(held)) == [2, 6, 7]
    free = ~held
    w = (lamp != 0).astype(float)
    rho, mu = 7.0, 0.5
    H = rho * (Jd.T * w) @ Jd
    Hf = H[np.ix_(free, free)] + mu * np.eye(free.sum())
    want = np.linalg.solve(Hf, g[free])
    for pos, first in _orderings(P):
        d = CH.direction(P, vals, lamp, rho, g, mu, pos, first, held=held, dtype=dtype, reverse=reverse)
        assert d["solved"] and d["code"] == 1 and d["nheld"] == 3 and d["bcol"] == -1
        assert np.array_equal(_bits(d["D"][held]), _bits(g[held]))
        err = np.max(np.abs(d["D"][free].astype(np.float64) - want)) / np.max(np.abs(want))
        assert err < 1e-12, err
        assert abs(float(d["slope"]) - (g[held] @ g[held] + g[free] @ want)) < 1e-12 * abs(g @ g)
        assert abs(float(d["bb"]) - g[free] @ g[free]) < 1e-14 * (g @ g)
        # the pivots are those of the dense factor of the permuted matrix (held rows are the identity: pivot 1)
        assert 0 < d["pmin"] <= d["pmax"] and d["pmin"] >= mu * (1 - 1e-12)
        s = CH.summary(d)
        assert s.shape == (8,) and np.array_equal(s[[0, 4, 5, 7]], [1, 3, 1, -1])
        assert float(d["slope"]) > 0
        # two wrong systems lie far outside the gate: every row active, and no column held
        gate = _gate(P, vals, lamp, rho, g, mu, held, pos, first)
        assert CH.backward_error(P, vals, lamp, rho, g, mu, held, d["D"]) <= gate
        for kw in (dict(ignore_w=True), dict(ignore_held=True)):
            other = CH.direction(P, vals, lamp, rho, g, mu, pos, first, held=held, dtype=dtype, reverse=reverse, **kw)
            assert other["code"] == 1
            far = CH.backward_error(P, vals, lamp, rho, g, mu, held, other["D"])
            assert far > 1000 * gate, (kw, far, gate)


def test_assembly_inside_the_envelope():
    """The assembled matrix: rho J^T W J + mu I on free columns, the identity on held ones, +0.0 where two columns share
    no row, nothing outside the envelope."""
    P, Jd, vals, lamp, g, x, lo, up = _sparse_problem()
    held = lbfgs_ref.held_mask(x, g, lo, up)
    w = (lamp != 0).astype(float)
    H = CH.assemble(P, vals, lamp, 7.0, 0.5, held)
    want = 7.0 * (Jd.T * w) @ Jd + 0.5 * np.eye(P.n)
    want[held, :] = 0
    want[:, held] = 0
    want[held, held] = 1
    assert np.allclose(H, want, rtol=1e-14, atol=1e-15)
    S = CH.structure(P)
    assert np.array_equal(_bits(H[~S]), _bits(np.zeros((~S).sum())))
    for pos, first in _orderings(P):
        inv = np.argsort(pos)
        Sp = S[np.ix_(inv, inv)]
        q, c = np.nonzero(np.tril(Sp))
        assert (first[q] <= c).all()


@pytest.mark.parametrize("dtype,reverse", MODES)
def test_every_code(dtype, reverse):
    P, Jd, vals, lamp, g, x, lo, up = _sparse_problem()
    held = lbfgs_ref.held_mask(x, g, lo, up)
    pos, first = _orderings(P)[1]
    kw = dict(held=held, dtype=dtype, reverse=reverse)
    # 2: column 5 has no entry and is free; at mu = 0 its pivot is exactly 0
    assert not held[5]
    d = CH.direction(P, vals, lamp, 7.0, g, 0.0, pos, first, **kw)
    assert (d["code"], d["solved"], d["bcol"]) == (2, False, pos[5]) and np.array_equal(_bits(d["D"]), _bits(g))
    assert float(d["slope"]) == pytest.approx(float(g @ g), rel=1e-14)
    s = CH.summary(d)
    assert np.array_equal(s[[0, 4, 5, 7]], [0, 3, 2, pos[5]])
    # 2: a NaN in an inactive row still reaches the matrix (the product w * (v * v) keeps it), in rho, in an active row
    vi, vn = vals.copy(), vals.copy()
    inactive = int(np.flatnonzero((lamp == 0) & (np.diff(P.row_ptr) > 0))[0])
    vi[P.row_ptr[inactive]] = np.nan
    vn[4] = np.nan
    for v_, rho_ in ((vi, 7.0), (vn, 7.0), (vals, np.nan)):
        d = CH.direction(P, v_, lamp, rho_, g, 0.5, pos, first, **kw)
        assert d["code"] == 2 and d["bcol"] >= 0 and not d["solved"]
        assert np.array_equal(_bits(d["D"]), _bits(g))
    # 3: nothing to solve (the gradient is zero on every free column, -0.0 included): no factorisation
    g0 = np.where(held, g, 0.0)
    g0[0] = -0.0
    d = CH.direction(P, vi, lamp, 7.0, g0, 0.5, pos, first, **kw)
    assert (d["code"], d["solved"], d["bcol"], d["bb"]) == (3, False, -1, 0) and np.array_equal(_bits(d["D"]), _bits(g0))
    assert np.array_equal(CH.summary(d)[[0, 1, 2, 4, 5, 6, 7]], [0, 0, 0, 3, 3, 0, -1])
    # without X every column is free
    d = CH.direction(P, vals, lamp, 7.0, g, 0.5, pos, first, held=None, dtype=dtype, reverse=reverse)
    assert d["nheld"] == 0 and d["code"] == 1


# ---- the ordering and the envelope of towr_gpu_gn_factor_info, on layout-only handles --------------------------------
SCIPY_MARGIN = 1.25   # another start node and other tie-breaks than scipy's reverse_cuthill_mckee


@functools.lru_cache(maxsize=None)
def _layout_handle(name):
    if name.startswith("sweep_seed_"):
        f = make(int(name[len("sweep_seed_"):]))[0]
        f.params_.enable_stance_tracking = False
        return TowrGpuProblem(f.to_desc(), device=-1)
    return TowrGpuProblem(config_descs()[name], device=-1)


ORDER_CASES = list(config_descs()) + [f"sweep_seed_{s}" for s in SWEEP_SEEDS]


def _jtj(h):
    """(rows, columns) of the structural nonzeros of J^T J of a handle's pattern."""
    rp, col = h.jac_csr()
    return np.nonzero(CH.structure(G.Pattern(rp, col, h.n)))


@pytest.mark.parametrize("name", ORDER_CASES)
def test_factor_info(name):
    h = _layout_handle(name)
    n = h.n
    info = h.gn_factor_info()
    pos, first = info["pos"].astype(np.int64), info["first"].astype(np.int64)
    assert info["ordering"] == capi.GN_ORDER_RCM
    assert np.array_equal(np.sort(pos), np.arange(n))
    q = np.arange(n)
    assert (first >= 0).all() and (first <= q).all()
    assert info["envelope"] == int((q - first + 1).sum()) and info["bandwidth"] == int((q - first).max())
    assert info["ldw_min"] >= info["envelope"]
    # every structural nonzero of J^T J lies inside the envelope, and no row's envelope starts before its first one
    r, c = _jtj(h)
    pq, pc = pos[r], pos[c]
    low = pc <= pq
    assert (first[pq[low]] <= pc[low]).all()
    tight = q.copy()
    np.minimum.at(tight, pq[low], pc[low])
    assert np.array_equal(tight, first)
    # the same answer the second time (the tables are built once), and NULL outputs are accepted
    again = h.gn_factor_info()
    assert np.array_equal(again["pos"], info["pos"]) and np.array_equal(again["first"], info["first"])
    assert h._lib.towr_gpu_gn_factor_info(h._h, None, None, None, None, None, None) == capi.TOWR_OK


@pytest.mark.parametrize("name", ORDER_CASES)
def test_envelope_against_scipy(name):
    """The envelope is at most 1.25 x that of scipy's reverse Cuthill-McKee on the same pattern (the ratios: DESIGN 4m)."""
    sp = pytest.importorskip("scipy.sparse")
    from scipy.sparse.csgraph import reverse_cuthill_mckee
    h = _layout_handle(name)
    n, q = h.n, np.arange(h.n)
    r, c = _jtj(h)
    perm = reverse_cuthill_mckee(sp.csr_matrix((np.ones(r.size), (r, c)), shape=(n, n)), symmetric_mode=True)
    spos = np.empty(n, dtype=np.int64)
    spos[perm] = q
    sfirst = q.copy()
    np.minimum.at(sfirst, spos[r], spos[c])
    senv = int((q - sfirst + 1).sum())
    env = h.gn_factor_info()["envelope"]
    print(f"{name}: n {n} envelope {env} scipy {senv} ratio {env / senv:.3f}")
    assert env <= SCIPY_MARGIN * senv


# ---- the short solve, driven by the CPU oracle ----------------------------------------------------------------------
def solve_monoped_direct(seed, reverse, K=SOLVE_K, mu=SOLVE_MU):
    """Up to K iterations of chol_ref.iterate from x0 + 0.05 randn(seed), LAM = 0, the handle's variable bounds, the
    handle's ordering: (phase, iterations run, max violation at the base, refused trials)."""
    o, P, x0, lo, up, evaluate = _monoped()
    info = _layout_handle("monoped_procedural").gn_factor_info()
    gn = dict(mu=mu, pos=info["pos"], first=info["first"])
    par = R.params(**SOLVE_PAR)
    x0 = x0 + 0.05 * np.random.default_rng(seed).standard_normal(o.n)
    st = R.new_state(o.n, o.m, par["mem"], x0, n_rsum=4 + o.desc.n_constraints, n_ssum=5 + o.desc.n_varsets)
    R.init(st, par, lo, up)
    trace = []
    for k in range(K):
        CH.iterate(st, par, gn, P, evaluate, lo, up, 1, np.float64, reverse, trace)
        assert not np.isnan(st["SCAL"]).any() and not np.isnan(st["LSUM"]).any(), f"iteration {k}: NaN"
        if trace[-1][0] == 2:
            assert st["LSUM"][2] <= st["LSUM"][3], f"iteration {k}: an accepted base raised M0"
        if st["ISTATE"][0] >= R.CONVERGED:
            break
    codes = [t[0] for t in trace]
    return int(st["ISTATE"][0]), len(trace), float(st["SCAL"][4]), codes.count(3)


@pytest.mark.parametrize("seed", SOLVE_SEEDS)
def test_short_solve_on_monoped(seed):
    """monoped_procedural driven by the CPU oracle: SOLVE_PAR (eta_star = omega_star = 1e-6), mu = 1e-6, the starts
    x0 + 0.05 randn(seed), LAM = 0, the handle's variable bounds and ordering, at most K = 100 iterations of
    tests/chol_ref.iterate in float64 with ascending sums. Asserted: TOWR_AL_CONVERGED, no NaN, an accepted base never
    raises M0. The measured iteration counts and the reversed-order outcome stand in DESIGN 4m."""
    phase, iters, viol, refused = solve_monoped_direct(seed, False)
    print(f"seed {seed}: phase {phase} after {iters} iterations, max violation {viol:.3e}, refused trials {refused}")
    assert phase == R.CONVERGED, (phase, iters, viol)
