"""numpy restatement of the Gauss-Newton direction of include/towr_gpu.h (towr_gpu_gn_direction_batch_device) and of
the iteration that uses it (towr_gpu_alsolve_gn_iterate_batch_device), one problem at a time. `dtype` / `reverse` as in
tests/lbfgs_ref.py: the arithmetic of the products, the sums and the recursion (np.float64 or np.longdouble), and a
second summation order of every sum (the terms reversed). The line search, the outer update and the step are those of
tests/alsolve_ref.py. tests/test_gn_ref.py checks this file against a dense solve."""
import numpy as np

from tests import alsolve_ref, lbfgs_ref

_sum = lbfgs_ref._sum


class Pattern:
    """A CSR pattern (row_ptr (m + 1), col (nnz), n columns) with its by-column order."""

    def __init__(self, row_ptr, col, n):
        self.row_ptr = np.asarray(row_ptr, dtype=np.int64)
        self.col = np.asarray(col, dtype=np.int64)
        self.n, self.m = int(n), len(self.row_ptr) - 1
        self.row = np.repeat(np.arange(self.m, dtype=np.int64), np.diff(self.row_ptr))
        self.perm = np.argsort(self.col, kind="stable")          # by column, rows ascending
        self.col_ptr = np.concatenate([[0], np.cumsum(np.bincount(self.col, minlength=self.n))]).astype(np.int64)

    @classmethod
    def dense(cls, m, n):
        return cls(np.arange(m + 1) * n, np.tile(np.arange(n), m), n)


def _seg_sums(t, ptr, reverse):
    """out[i] = the sum of t[ptr[i]:ptr[i + 1]] (0 for an empty segment), in ascending or in reversed order."""
    out = np.zeros(len(ptr) - 1, dtype=t.dtype)
    nz = np.flatnonzero(ptr[1:] > ptr[:-1])
    if nz.size == 0:
        return out
    if reverse:
        out[nz[::-1]] = np.add.reduceat(t[::-1], (t.size - ptr[1:][nz])[::-1])
    else:
        out[nz] = np.add.reduceat(t, ptr[:-1][nz])
    return out


def jvec(P, vals, p, reverse=False):
    return _seg_sums(vals * p[P.col], P.row_ptr, reverse)


def jtvec(P, vals, t, reverse=False):
    return _seg_sums((vals * t[P.row])[P.perm], P.col_ptr, reverse)


def weights(lamp, dtype=np.float64):
    """w_i = 1 where lam+_i != 0 (a NaN is active), else 0."""
    return (np.asarray(lamp) != 0.0).astype(dtype)


def direction(P, vals, lamp, rho, g, ncg, mu, tol, held=None, dtype=np.float64, reverse=False, ignore_w=False):
    """The CG recursion on H = rho (J^T W J)_ff + mu I from d = 0. `ignore_w`: every row active although the formulas
    weight them — a deliberately wrong system, for checking that a gate refuses one. Returns dict(D, steps, bb, rr,
    slope, nheld, code, hist (rr / bb before every step and after the last), free)."""
    n = P.n
    free = np.ones(n, dtype=bool) if held is None else ~held
    w = np.ones(P.m, dtype=dtype) if ignore_w else weights(lamp, dtype)
    vd, gd = np.asarray(vals).astype(dtype), np.asarray(g).astype(dtype)
    rho, mu, tol = dtype(rho), dtype(mu), dtype(tol)
    zero = np.zeros(n, dtype=dtype)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        p = np.where(free, gd, zero)
        r, d = p.copy(), zero.copy()
        bb = _sum(gd[free] * gd[free], reverse)
        rr, steps, code = bb, 0, 0
        hist = [dtype(1.0)]
        if bb == 0:
            code = 3
        else:
            for _ in range(int(ncg)):
                if rr <= tol * tol * bb:
                    code = 1
                    break
                t = w * jvec(P, vd, p, reverse)
                hp = np.where(free, rho * jtvec(P, vd, t, reverse) + mu * p, zero)
                php = _sum((p * hp)[free], reverse)
                if not php > 0:
                    code = 2
                    break
                a = rr / php
                d = np.where(free, d + a * p, zero)
                r = np.where(free, r - a * hp, zero)
                rn = _sum((r * r)[free], reverse)
                p = np.where(free, r + (rn / rr) * p, zero)
                rr = rn
                steps += 1
                hist.append(rr / bb)
        D = gd.copy()
        if steps:
            D[free] = d[free]
        slope = _sum(gd * D, reverse)
    return dict(D=D, steps=steps, bb=bb, rr=rr, slope=slope, nheld=int((~free).sum()), code=code, hist=hist, free=free)


def summary(d):
    """SUM[0..5] of a direction() result, as float64."""
    return np.array([d["steps"], d["bb"], d["rr"], d["slope"], d["nheld"], d["code"]], dtype=np.float64)


def select(st):
    """The select behind the outer update: D <- DC on an accepted base, else D <- GR on a history reset."""
    flags = int(st["ISTATE"][1])
    if flags & 1:
        st["D"] = st["DC"].copy()
    elif flags & 4:
        st["D"] = st["GR"].copy()


def iterate(st, par, gn, P, evaluate, lo, up, iters=1, dtype=np.float64, reverse=False, trace=None):
    """`iters` iterations on one problem's state (alsolve_ref.new_state plus DC and GSUM, added here when missing).
    evaluate(x, lam, rho) -> (f, grad of the augmented Lagrangian, lam+, max violation, phi, the CSR values of J at x).
    gn = dict(ncg, mu, tol). `trace` as in alsolve_ref.iterate."""
    st.setdefault("DC", np.zeros_like(st["X"]))
    st.setdefault("GSUM", np.zeros(6))
    for _ in range(iters):
        f, gr, lamp, viol, phi, vals = evaluate(st["XC"], st["LAM"], float(st["RHO"]))
        st["FC"], st["GRC"], st["LAMP"] = np.float64(f), np.array(gr, dtype=np.float64), np.array(lamp, dtype=np.float64)
        st["RSUM"][0], st["RSUM"][3] = viol, phi
        if int(st["ISTATE"][0]) < 2:                                # RUN = the phase: frozen problems are skipped
            held = lbfgs_ref.held_mask(st["XC"], st["GRC"], lo, up)
            d = direction(P, vals, st["LAMP"], st["RHO"], st["GRC"], gn["ncg"], gn["mu"], gn["tol"], held, dtype, reverse)
            st["DC"], st["GSUM"] = d["D"].astype(np.float64), summary(d)
        info = alsolve_ref.linesearch(st, par, lo, up, dtype, reverse)
        did = alsolve_ref.outer(st, par)
        select(st)
        with np.errstate(invalid="ignore", over="ignore"):
            st["XC"] = alsolve_ref.clamp(st["X"] - np.float64(st["ALPHA"]) * st["D"], lo, up)
        if trace is not None:
            trace.append((info["code"], did, int(st["ISTATE"][0])))
    return st
