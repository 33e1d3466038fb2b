"""tests/tile_chol_ref.py (the numpy restatement of the tiled direct Gauss-Newton direction and of the loop that uses it)
against a dense solve of H d = g with padding rows in the last tile, every code, two deliberately wrong systems; the tile
envelope of towr_gpu_gn_tile_info on layout-only handles of every configuration and sweep seed; and the short solve of
monoped_procedural driven by the CPU oracle. No GPU."""
import numpy as np
import pytest

from tests import alsolve_ref as R
from tests import chol_ref as CH
from tests import lbfgs_ref
from tests import tile_chol_ref as TC
from tests.test_chol_ref import ORDER_CASES, SOLVE_K, SOLVE_MU, SOLVE_SEEDS, _bits, _gate, _layout_handle, _orderings
from tests.test_gn_ref import _sparse_problem
from tests.test_pgn_ref import SOLVE_PAR, _monoped
from towr2025_amd import _capi as capi

# the stored tiles per configuration, as measured on the host for the tile envelope's design
TILES = {"monoped_procedural": 79, "biped_walk_2s": 274, "anymal_trot_2p4s": 585, "anymal_stairs_gaitopt": 1928,
         "hopper_gait_torque": 1283, "anymal_gait_torque": 1927, "sweep_seed_196": 15, "sweep_seed_154": 48}
DTYPES = (np.float64, np.longdouble)
PAD_SHAPE = dict(m=60, n=37)   # three block rows, 5 live rows in the last tile


@pytest.mark.parametrize("name", ORDER_CASES)
def test_tile_info(name):
    h = _layout_handle(name)
    n = h.n
    f = h.gn_factor_info()
    first = f["first"].astype(np.int64)
    info = h.gn_tile_info()
    nt = -(-n // 16)
    assert info["tile"] == 16 == capi.GN_TILE and info["nt"] == nt
    bfirst = info["bfirst"].astype(np.int64)
    want = np.array([first[16 * I:min(n, 16 * I + 16)].min() // 16 for I in range(nt)])
    assert np.array_equal(bfirst, want) and (bfirst <= np.arange(nt)).all()
    assert info["tiles"] == int((np.arange(nt) - bfirst + 1).sum())
    assert info["ldw_min"] >= 256 * info["tiles"]
    rnt, rbfirst, rtiles = TC.tile_tables(first, n)
    assert (rnt, rtiles) == (nt, info["tiles"]) and np.array_equal(rbfirst, bfirst)
    # every entry of the scalar envelope lies in a stored tile: row q's first column is not left of its block row's
    q = np.arange(n)
    assert (first // 16 >= bfirst[q // 16]).all()
    if name in TILES:
        assert info["tiles"] == TILES[name]
    # the same answer the second time (the tables are built once), and NULL outputs are accepted
    again = h.gn_tile_info()
    assert np.array_equal(again["bfirst"], info["bfirst"]) and again["tiles"] == info["tiles"]
    assert h._lib.towr_gpu_gn_tile_info(h._h, None, None, None, None, None) == capi.TOWR_OK


def test_tile_table_names():
    assert set(TILES) <= set(ORDER_CASES)


@pytest.mark.parametrize("dtype", DTYPES)
def test_direction_solves_the_dense_system(dtype):
    P, Jd, vals, lamp, g, x, lo, up = _sparse_problem(**PAD_SHAPE)
    assert P.n % 16 != 0
    held = lbfgs_ref.held_mask(x, g, lo, up)
    assert list(np.flatnonzero(held)) == [2, 6, 7]
    free = ~held
    w = (lamp != 0).astype(float)
    rho, mu = 7.0, 0.5
    H = rho * (Jd.T * w) @ Jd
    Hf = H[np.ix_(free, free)] + mu * np.eye(free.sum())
    want = np.linalg.solve(Hf, g[free])
    for pos, first in _orderings(P):
        d = TC.direction(P, vals, lamp, rho, g, mu, pos, first, held=held, dtype=dtype)
        assert d["solved"] and d["code"] == 1 and d["nheld"] == 3 and d["bcol"] == -1
        assert np.array_equal(_bits(d["D"][held]), _bits(g[held]))
        err = np.max(np.abs(d["D"][free].astype(np.float64) - want)) / np.max(np.abs(want))
        assert err < 1e-12, err
        assert abs(float(d["slope"]) - (g[held] @ g[held] + g[free] @ want)) < 1e-12 * abs(g @ g)
        # the pivots are those of the scalar factorisation up to rounding (the padding's pivots, 1.0, are not counted)
        ref = CH.direction(P, vals, lamp, rho, g, mu, pos, first, held=held, dtype=dtype)
        assert d["pmin"] == pytest.approx(ref["pmin"], rel=1e-10) and d["pmax"] == pytest.approx(ref["pmax"], rel=1e-10)
        assert np.array_equal(TC.summary(d)[[0, 4, 5, 7]], [1, 3, 1, -1])
        # inside the envelope direction's gate; the two wrong systems lie far outside it
        gate = _gate(P, vals, lamp, rho, g, mu, held, pos, first)
        assert CH.backward_error(P, vals, lamp, rho, g, mu, held, d["D"]) <= gate
        for kw in (dict(ignore_w=True), dict(ignore_held=True)):
            other = TC.direction(P, vals, lamp, rho, g, mu, pos, first, held=held, dtype=dtype, **kw)
            assert other["code"] == 1
            far = CH.backward_error(P, vals, lamp, rho, g, mu, held, other["D"])
            assert far > 1000 * gate, (kw, far, gate)


def test_tiles_hold_the_envelope_and_the_padding():
    P, Jd, vals, lamp, g, x, lo, up = _sparse_problem(**PAD_SHAPE)
    held = lbfgs_ref.held_mask(x, g, lo, up)
    H = CH.assemble(P, vals, lamp, 7.0, 0.5, held)
    for pos, first in _orderings(P):
        inv = np.argsort(pos)
        nt, bfirst, tiles = TC.tile_tables(first, P.n)
        assert nt == 3 and tiles == int((np.arange(nt) - bfirst + 1).sum())
        A = TC.into_tiles(H[np.ix_(inv, inv)], bfirst)
        assert A.shape == (48, 48)
        assert np.array_equal(_bits(A[:P.n, :P.n]), _bits(np.tril(H[np.ix_(inv, inv)])))
        assert np.array_equal(A[P.n:, P.n:], np.eye(48 - P.n)) and not A[P.n:, :P.n].any()
        M = TC.stored_mask(P.n, bfirst)
        q = np.arange(P.n)
        assert all(M[r, first[r]:r + 1].all() for r in q)


@pytest.mark.parametrize("dtype", DTYPES)
def test_every_code(dtype):
    P, Jd, vals, lamp, g, x, lo, up = _sparse_problem(**PAD_SHAPE)
    held = lbfgs_ref.held_mask(x, g, lo, up)
    pos, first = _orderings(P)[1]
    kw = dict(held=held, dtype=dtype)
    # 2: column 5 has no entry and is free; at mu = 0 its pivot is exactly 0
    assert not held[5]
    d = TC.direction(P, vals, lamp, 7.0, g, 0.0, pos, first, **kw)
    assert (d["code"], d["solved"], d["bcol"]) == (2, False, pos[5]) and np.array_equal(_bits(d["D"]), _bits(g))
    assert np.array_equal(TC.summary(d)[[0, 4, 5, 7]], [0, 3, 2, pos[5]])
    # 2: a NaN in an inactive row still reaches the matrix
    vi = vals.copy()
    inactive = int(np.flatnonzero((lamp == 0) & (np.diff(P.row_ptr) > 0))[0])
    vi[P.row_ptr[inactive]] = np.nan
    d = TC.direction(P, vi, lamp, 7.0, g, 0.5, pos, first, **kw)
    assert d["code"] == 2 and d["bcol"] >= 0 and not d["solved"] and np.array_equal(_bits(d["D"]), _bits(g))
    # 3: nothing to solve (the gradient is zero on every free column, -0.0 included): no factorisation
    g0 = np.where(held, g, 0.0)
    g0[0] = -0.0
    d = TC.direction(P, vi, lamp, 7.0, g0, 0.5, pos, first, **kw)
    assert (d["code"], d["solved"], d["bcol"], d["bb"]) == (3, False, -1, 0) and np.array_equal(_bits(d["D"]), _bits(g0))
    assert np.array_equal(TC.summary(d)[[0, 1, 2, 4, 5, 6, 7]], [0, 0, 0, 3, 3, 0, -1])


# ---- the short solve, driven by the CPU oracle ----------------------------------------------------------------------
def solve_monoped_tiled(seed, K=SOLVE_K, mu=SOLVE_MU):
    """tests/test_chol_ref.solve_monoped_direct with tile_chol_ref.iterate."""
    o, P, x0, lo, up, evaluate = _monoped()
    info = _layout_handle("monoped_procedural").gn_factor_info()
    gn = dict(mu=mu, pos=info["pos"], first=info["first"])
    par = R.params(**SOLVE_PAR)
    x0 = x0 + 0.05 * np.random.default_rng(seed).standard_normal(o.n)
    st = R.new_state(o.n, o.m, par["mem"], x0, n_rsum=4 + o.desc.n_constraints, n_ssum=5 + o.desc.n_varsets)
    R.init(st, par, lo, up)
    trace = []
    for k in range(K):
        TC.iterate(st, par, gn, P, evaluate, lo, up, 1, np.float64, trace)
        assert not np.isnan(st["SCAL"]).any() and not np.isnan(st["LSUM"]).any(), f"iteration {k}: NaN"
        if trace[-1][0] == 2:
            assert st["LSUM"][2] <= st["LSUM"][3], f"iteration {k}: an accepted base raised M0"
        if st["ISTATE"][0] >= R.CONVERGED:
            break
    return int(st["ISTATE"][0]), len(trace), float(st["SCAL"][4])


def test_short_solve_on_monoped():
    """tests/test_chol_ref.py's short solve (seeds 900..905, SOLVE_PAR, mu = 1e-6, K = 100) through the tiled reference:
    at least 5 of 6 reach TOWR_AL_CONVERGED (both of chol_ref's orders reach all six, in 67 / 9 / 39 / 32 / 10 / 12
    iterations). The iteration counts are printed, not asserted."""
    out = [solve_monoped_tiled(seed) for seed in SOLVE_SEEDS]
    for seed, (phase, iters, viol) in zip(SOLVE_SEEDS, out):
        print(f"seed {seed}: phase {phase} after {iters} iterations, max violation {viol:.3e}")
    assert sum(phase == R.CONVERGED for phase, _, _ in out) >= 5, out
