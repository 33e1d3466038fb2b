"""tests/lbfgs_ref.py against textbook L-BFGS (CPU): on small n, all columns free and all pairs used, the two-loop
result equals H g with H the dense matrix built by the BFGS inverse update applied pair by pair from gamma I, and
H y_newest = s_newest (the secant equation); the ring, the curvature test and the held columns of the header."""
import numpy as np
import pytest

from tests import lbfgs_ref as R

LD = np.longdouble
EPS_LD = float(np.finfo(LD).eps)


def _pairs(n, k, seed):
    """k pairs of a convex quadratic (y = A s, A SPD with a spectrum in about [1, 30]): every s y > 0."""
    rng = np.random.default_rng(seed)
    Q = rng.standard_normal((n, n))
    A = Q @ Q.T / n + np.diag(rng.uniform(1.0, 20.0, n))
    S = rng.standard_normal((k, n))
    return S, S @ A, rng.standard_normal(n)


def _dense(S, Y, order):
    """H from gamma I by the BFGS inverse update over the pairs `order` (oldest first), in long double."""
    n = S.shape[1]
    newest = order[-1]
    s, y = S[newest].astype(LD), Y[newest].astype(LD)
    H = (s @ y) / (y @ y) * np.eye(n, dtype=LD)
    I = np.eye(n, dtype=LD)
    for k in order:
        s, y = S[k].astype(LD), Y[k].astype(LD)
        rho = 1 / (s @ y)
        H = (I - rho * np.outer(s, y)) @ H @ (I - rho * np.outer(y, s)) + rho * np.outer(s, s)
    return H


@pytest.mark.parametrize("n,mem,count,nxt", [(7, 5, 5, 0), (12, 5, 3, 3), (12, 3, 3, 1), (9, 1, 1, 0), (16, 4, 4, 2)])
def test_two_loop_equals_the_dense_bfgs_inverse(n, mem, count, nxt):
    S, Y, g = _pairs(n, mem, 100 * n + mem)
    order = [(nxt - i) % mem for i in range(count, 0, -1)]              # oldest first
    H = _dense(S, Y, order)
    ref = R.direction(g, S, Y, [count, nxt], dtype=LD)
    assert ref["used"] == list(range(1, count + 1)) and ref["nheld"] == 0
    want = H @ g.astype(LD)
    scale = float(np.abs(want).max())
    # both sides are O(mem n^2) long double operations on a matrix of condition below 1e3: 1e4 eps is far above
    # their rounding and far below float64's 2^-53 = 2000 eps
    assert float(np.abs(ref["D"] - want).max()) <= 1e4 * EPS_LD * scale
    newest = order[-1]
    sec = R.direction(Y[newest], S, Y, [count, nxt], dtype=LD)          # the secant equation H y = s
    assert float(np.abs(sec["D"] - S[newest]).max()) <= 1e4 * EPS_LD * float(np.abs(S[newest]).max())
    assert float(np.abs(H @ Y[newest].astype(LD) - S[newest]).max()) <= 1e4 * EPS_LD * float(np.abs(S[newest]).max())
    d64 = R.direction(g, S, Y, [count, nxt])                            # float64, both orders: near the long double result
    d64r = R.direction(g, S, Y, [count, nxt], reverse=True)
    for d in (d64, d64r):
        assert d["D"].dtype == np.float64 and float(np.abs(d["D"] - want).max()) <= 1e-12 * scale
    gam = (S[newest].astype(LD) @ Y[newest].astype(LD)) / (Y[newest].astype(LD) @ Y[newest].astype(LD))
    assert abs(ref["gamma"] - gam) <= 1e3 * EPS_LD * gam


def test_empty_garbage_and_unused_pairs():
    S, Y, g = _pairs(10, 3, 5)
    for meta in ([0, 0], [0, 2], [-7, 99], [4, 0], [1, 3]):
        d = R.direction(g, S, Y, meta)
        if meta[0] == 0 or R.meta_or_empty(*meta, 3) == (0, 0):
            assert np.array_equal(d["D"].view(np.uint64), g.view(np.uint64)) and d["used"] == [] and d["gamma"] == 1.0
    Y2 = Y.copy()
    Y2[1] = -Y2[1]                                                       # slot 1: negative curvature, unused
    d = R.direction(g, S, Y2, [3, 0])                                    # i = 1, 2, 3 -> slots 2, 1, 0
    assert d["used"] == [1, 3] and d["c"][1] < 0
    keep = R.direction(g, np.delete(S, 1, 0), np.delete(Y, 1, 0), [2, 0])   # ... the same as a history without it
    assert np.array_equal(d["D"], keep["D"])
    Y3 = Y.copy()
    Y3[2, 4] = np.nan                                                    # a NaN in the newest pair: unused, the rest proceeds
    d = R.direction(g, S, Y3, [3, 0])
    assert d["used"] == [2, 3] and np.isfinite(d["D"]).all()
    gn = g.copy()
    gn[3] = np.nan                                                       # a NaN gradient entry reaches every free column
    assert np.isnan(R.direction(gn, S, Y, [3, 0])["D"]).all()
    dropped = R.direction(g, S, Y, [3, 0], drop=2)
    assert dropped["used"] == [1, 3] and not np.allclose(dropped["D"], R.direction(g, S, Y, [3, 0])["D"])


def test_held_columns():
    n = 11
    S, Y, g = _pairs(n, 3, 9)
    lo, up = np.full(n, -1e20), np.full(n, 1e20)
    x = np.zeros(n)
    lo[0], g[0] = 0.0, 1.0                                               # on the lower side, pointing out: held
    lo[1], g[1] = 0.0, -1.0                                              # on the lower side, pointing in: free
    up[2], g[2] = 0.0, -2.0                                              # on the upper side, pointing out: held
    up[3], g[3] = 0.0, 2.0                                               # ... pointing in: free
    lo[4] = up[4] = 0.5                                                  # fixed: held wherever x is
    lo[5], up[5], g[5] = 0.0, 1e19, 1.0                                  # an upper side that does not count; the lower does
    lo[6], g[6] = -np.inf, 1.0                                           # no side counts
    held = R.held_mask(x, g, lo, up)
    assert held.tolist() == [True, False, True, False, True, True, False, False, False, False, False]
    gn = g.copy()
    gn[0] = np.nan                                                       # a NaN gradient is free
    assert not R.held_mask(x, gn, lo, up)[0] and not R.held_mask(None, g, lo, up).any()
    d = R.direction(g, S, Y, [3, 0], held=held, dtype=LD)
    assert d["nheld"] == 4 and np.array_equal(d["D"][held], g[held].astype(LD))
    f = ~held                                                            # the recursion on the free columns alone
    sub = R.direction(g[f], S[:, f], Y[:, f], [3, 0], dtype=LD)
    assert np.array_equal(d["D"][f], sub["D"]) and d["gamma"] == sub["gamma"] and d["gg"] == sub["gg"]
    assert d["slope"] == np.sum(g.astype(LD) * d["D"])


def test_update_ring_and_curvature_test():
    n, mem = 6, 3
    rng = np.random.default_rng(3)
    HS, HY, meta = np.full((mem, n + 2), np.nan), np.full((mem, n + 2), np.nan), np.array([0, 0], dtype=np.int32)
    slots = []
    for t in range(mem + 2):
        x, s = rng.standard_normal(n), rng.standard_normal(n)
        out, _ = R.update(x, x + s, 2.0 * x, 2.0 * (x + s), 0.25, HS, HY, meta)      # y = 2 s: sy / yy = 0.5 > 0.25
        assert out[3] == 1.0 and out[5] == t % mem and out[4] == min(t + 1, mem)
        assert np.array_equal(HS[t % mem, :n], (x + s) - x) and np.isnan(HS[:, n:]).all()
        slots.append(int(out[5]))
    assert slots == [0, 1, 2, 0, 1] and meta.tolist() == [3, 2]
    before = (HS.copy(), HY.copy(), meta.copy())
    x, s = rng.standard_normal(n), rng.standard_normal(n)
    for xn, grn, eps in ((x + s, 2.0 * x - 2.0 * s, 0.0),                # negative curvature
                         (x + s, 2.0 * (x + s), 0.75),                   # curv_eps above sy / yy = 0.5
                         (np.where(np.arange(n) == 2, np.nan, x + s), 2.0 * (x + s), 0.0)):   # a NaN
        out, _ = R.update(x, xn, 2.0 * x, grn, eps, HS, HY, meta)
        assert out[3] == 0.0 and out[5] == -1.0 and out[4] == 3
        assert all(np.array_equal(a.view(np.uint8), b.view(np.uint8)) for a, b in zip(before, (HS, HY, meta)))
    garbage = np.array([-7, 99], dtype=np.int32)                         # garbage meta: an empty history
    out, _ = R.update(x, x + s, 2.0 * x, 2.0 * (x + s), 0.0, HS, HY, garbage)
    assert out[5] == 0.0 and garbage.tolist() == [1, 1 % mem]
