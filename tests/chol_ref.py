"""numpy restatement of the direct Gauss-Newton direction of include/towr_gpu.h
(towr_gpu_gn_direction_direct_batch_device: the assembly of H = rho (J^T W J)_ff + mu I into the envelope of an ordering,
the envelope Cholesky factorisation, the two triangular solves, the codes and SUM) and of the iteration that uses it
(towr_gpu_alsolve_gn_direct_iterate_batch_device), one problem at a time. `dtype` / `reverse` as in tests/gn_ref.py: the
arithmetic (np.float64 or np.longdouble) and a second summation order of every sum (the terms reversed). The line
search, the outer update, the select and the step are those of tests/alsolve_ref.py / tests/gn_ref.py.
tests/test_chol_ref.py checks this file against a dense solve."""
import numpy as np

from tests import alsolve_ref, gn_ref, lbfgs_ref

_sum = lbfgs_ref._sum


def structure(P):
    """The pattern of J^T J as a dense boolean matrix (two columns share a row), the diagonal included."""
    S = np.eye(P.n, dtype=bool)
    for i in range(P.m):
        c = P.col[P.row_ptr[i]:P.row_ptr[i + 1]]
        S[np.ix_(c, c)] = True
    return S


def envelope(P, pos):
    """first[q] of the ordering `pos` (pos[j] = the permuted position of column j): the smallest permuted column of
    permuted row q of the lower triangle of J^T J. Returns (first, envelope entries, bandwidth)."""
    pos = np.asarray(pos, dtype=np.int64)
    S = structure(P)
    inv = np.argsort(pos)
    Sp = S[np.ix_(inv, inv)]
    first = np.argmax(Sp, axis=1).astype(np.int64)          # the first True of a row; the diagonal is True
    q = np.arange(P.n)
    assert (first <= q).all()
    return first, int((q - first + 1).sum()), int((q - first).max(initial=0))


def assemble(P, vals, lamp, rho, mu, held, dtype=np.float64, reverse=False, ignore_w=False):
    """H in the columns' own order, dense: rho * sum_i w_i (v_ij v_ik) over the rows in ascending (reversed: descending)
    order, + mu on the diagonal, +0.0 where two columns share no row; the identity on held rows and columns."""
    n = P.n
    w = np.ones(P.m, dtype=dtype) if ignore_w else gn_ref.weights(lamp, dtype)
    vd = np.asarray(vals).astype(dtype)
    A = np.zeros((n, n), dtype=dtype)
    S = np.zeros((n, n), dtype=bool)
    rows = range(P.m - 1, -1, -1) if reverse else range(P.m)
    with np.errstate(invalid="ignore", over="ignore"):
        for i in rows:
            a, b = P.row_ptr[i], P.row_ptr[i + 1]
            if a == b:
                continue
            c, v = P.col[a:b], vd[a:b]
            ix = np.ix_(c, c)
            A[ix] += w[i] * np.outer(v, v)
            S[ix] = True
        H = np.where(S, dtype(rho) * A, dtype(0.0))
        H[np.diag_indices(n)] = dtype(rho) * np.diag(A) + dtype(mu)
    if held is not None and held.any():
        H[held, :] = 0.0
        H[:, held] = 0.0
        H[held, held] = 1.0
    return H


def factor_solve(Hp, gp, first, heldq, dtype=np.float64, reverse=False):
    """The envelope Cholesky factorisation of the permuted Hp (its lower triangle inside the envelope `first`), columns
    ascending, and the two solves with the permuted right-hand side gp. Returns dict(d (permuted; None on a
    breakdown), code, bcol, pmin, pmax)."""
    n = Hp.shape[0]
    first = np.asarray(first, dtype=np.int64)
    L = np.tril(Hp).astype(dtype)
    Lr = L[:, ::-1].copy() if reverse else None   # the columns mirrored: a reversed sum reads it forwards
    last = np.arange(n)
    for q in range(n):
        last[first[q]:q] = q                      # (q ascending: the last writer is the largest row)
    y, d = np.zeros(n, dtype=dtype), np.zeros(n, dtype=dtype)
    pmin, pmax = np.inf, 0.0
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        for c in range(n):
            f = first[c]
            lc = L[c, f:c].copy()
            piv = L[c, c] - _sum(lc * lc, reverse)
            if not piv > 0:
                return dict(d=None, code=2, bcol=c, pmin=pmin, pmax=pmax)
            if not heldq[c]:
                pmin, pmax = min(pmin, float(piv)), max(pmax, float(piv))
            lcc = np.sqrt(piv)
            L[c, c] = lcc
            y[c] = (gp[c] - _sum(lc * y[f:c], reverse)) / lcc
            r0, r1 = c + 1, last[c] + 1
            if r1 > r0:                           # (L is zero left of first[r], outside the envelope: those terms add 0)
                s = Lr[r0:r1, n - c:n - f] @ lc[::-1] if reverse else L[r0:r1, f:c] @ lc
                inside = first[r0:r1] <= c        # a row whose envelope does not reach c keeps its zero
                L[r0:r1, c] = np.where(inside, (L[r0:r1, c] - s) / lcc, L[r0:r1, c])
                if reverse:
                    Lr[r0:r1, n - 1 - c] = L[r0:r1, c]
        for c in range(n - 1, -1, -1):
            rows = np.arange(c + 1, last[c] + 1)
            t = (L[rows, c] * d[rows])[::-1]      # descending r is the stated order
            d[c] = (y[c] - _sum(t, reverse)) / L[c, c]
    return dict(d=d, code=1, bcol=-1, pmin=pmin, pmax=pmax)


def direction(P, vals, lamp, rho, g, mu, pos, first, held=None, dtype=np.float64, reverse=False, ignore_w=False,
              ignore_held=False):
    """The direct direction. `ignore_w` (every row active) and `ignore_held` (no column held) are deliberately wrong
    systems, for checking that a gate refuses them. Returns dict(D, solved, bb, pmin, slope, nheld, code, pmax, bcol,
    free)."""
    n = P.n
    pos = np.asarray(pos, dtype=np.int64)
    held = np.zeros(n, dtype=bool) if held is None else np.asarray(held, dtype=bool)
    used = np.zeros(n, dtype=bool) if ignore_held else held
    free = ~held
    gd = np.asarray(g).astype(dtype)
    inv = np.argsort(pos)
    with np.errstate(invalid="ignore", over="ignore"):
        bb = _sum(gd[free] * gd[free], reverse)
    out = dict(code=3, bcol=-1, pmin=np.inf, pmax=0.0)
    d = None
    if not bb == 0:
        H = assemble(P, vals, lamp, rho, mu, used, dtype, reverse, ignore_w)
        out = factor_solve(H[np.ix_(inv, inv)], gd[inv], first, used[inv], dtype, reverse)
        d = out["d"]
    D = gd.copy()
    if d is not None:
        D[~used] = d[pos[~used]]
    with np.errstate(invalid="ignore", over="ignore"):
        slope = _sum(gd * D, reverse)
    pmin = 0.0 if np.isinf(out["pmin"]) else out["pmin"]
    return dict(D=D, solved=out["code"] == 1, bb=bb, pmin=pmin, slope=slope, nheld=int(held.sum()), code=out["code"],
                pmax=out["pmax"], bcol=out["bcol"], free=free)


def summary(d):
    """SUM[0..7] of a direction() result, as float64."""
    return np.array([1.0 if d["solved"] else 0.0, d["bb"], d["pmin"], d["slope"], d["nheld"], d["code"], d["pmax"], d["bcol"]],
                    dtype=np.float64)


def system(P, vals, lamp, rho, mu):
    """H = rho J^T W J + mu I over all columns, assembled in long double from the values as they are."""
    return assemble(P, vals, lamp, rho, mu, None, np.longdouble)


def backward_error(P, vals, lamp, rho, g, mu, held, D, H=None):
    """max |g_f - (H D)_f| over the free columns, H = system(...) (or the caller's copy of it): what a direction is held
    to (the system's condition number makes a forward comparison meaningless)."""
    LD = np.longdouble
    H = system(P, vals, lamp, rho, mu) if H is None else H
    free = ~np.asarray(held, dtype=bool)
    r = np.asarray(g).astype(LD)[free] - H[np.ix_(free, free)] @ np.asarray(D).astype(LD)[free]
    return float(np.max(np.abs(r), initial=0.0))


def iterate(st, par, gn, P, evaluate, lo, up, iters=1, dtype=np.float64, reverse=False, trace=None):
    """gn_ref.iterate with the direction above: gn = dict(mu, pos, first). GSUM has 8 entries."""
    st.setdefault("DC", np.zeros_like(st["X"]))
    st.setdefault("GSUM", np.zeros(8))
    for _ in range(iters):
        f, gr, lamp, viol, phi, vals = evaluate(st["XC"], st["LAM"], float(st["RHO"]))
        st["FC"], st["GRC"], st["LAMP"] = np.float64(f), np.array(gr, dtype=np.float64), np.array(lamp, dtype=np.float64)
        st["RSUM"][0], st["RSUM"][3] = viol, phi
        if int(st["ISTATE"][0]) < 2:                                # RUN = the phase: frozen problems are skipped
            held = lbfgs_ref.held_mask(st["XC"], st["GRC"], lo, up)
            d = direction(P, vals, st["LAMP"], st["RHO"], st["GRC"], gn["mu"], gn["pos"], gn["first"], held, dtype, reverse)
            st["DC"], st["GSUM"] = d["D"].astype(np.float64), summary(d)
        info = alsolve_ref.linesearch(st, par, lo, up, dtype, reverse)
        did = alsolve_ref.outer(st, par)
        gn_ref.select(st)
        with np.errstate(invalid="ignore", over="ignore"):
            st["XC"] = alsolve_ref.clamp(st["X"] - np.float64(st["ALPHA"]) * st["D"], lo, up)
        if trace is not None:
            trace.append((info["code"], did, int(st["ISTATE"][0])))
    return st
