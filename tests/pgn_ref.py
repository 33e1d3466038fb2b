"""numpy restatement of the Jacobi-preconditioned Gauss-Newton direction of include/towr_gpu.h
(towr_gpu_gn_direction_pc_batch_device with TOWR_GN_PC_JACOBI) and of the iteration that uses it
(towr_gpu_alsolve_gn_pc_iterate_batch_device), one problem at a time. `dtype` / `reverse` as in tests/gn_ref.py, whose
pattern, products, weights, select and loop this file uses. direction() returns gn_ref.direction's keys plus rz, pc and
nzero, so tests/gn_gate.check_values takes it unchanged. tests/test_pgn_ref.py checks this file against a dense solve."""
import numpy as np

from tests import alsolve_ref, gn_ref, lbfgs_ref

_sum = lbfgs_ref._sum


def diagonal(P, vals, w, reverse=False):
    """dg_j = sum_i w_i * (v_ij * v_ij) over column j, rows ascending (or reversed)."""
    return gn_ref._seg_sums((w[P.row] * (vals * vals))[P.perm], P.col_ptr, reverse)


def direction(P, vals, lamp, rho, g, ncg, mu, tol, held=None, dtype=np.float64, reverse=False):
    """The preconditioned CG recursion on H = rho (J^T W J)_ff + mu I from d = 0 with M = rho diag(J^T W J) + mu (1 where
    that is exactly 0). Returns gn_ref.direction's dict plus rz (the final r.z), pc (M on free columns, 0 on held ones)
    and nzero (the free columns whose M was replaced)."""
    n = P.n
    free = np.ones(n, dtype=bool) if held is None else ~held
    w = gn_ref.weights(lamp, dtype)
    vd, gd = np.asarray(vals).astype(dtype), np.asarray(g).astype(dtype)
    rho, mu, tol = dtype(rho), dtype(mu), dtype(tol)
    zero, one = np.zeros(n, dtype=dtype), np.ones(n, dtype=dtype)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        M = rho * diagonal(P, vd, w, reverse) + mu
        replaced = free & (M == 0)
        M = np.where(replaced, one, M)
        Mf = np.where(free, M, one)                  # (held columns: nothing is divided)
        r = np.where(free, gd, zero)
        z = np.where(free, r / Mf, zero)
        p, d = z.copy(), zero.copy()
        bb = _sum(gd[free] * gd[free], reverse)
        rz = _sum((r * z)[free], reverse)
        rr, steps, code = bb, 0, 0
        hist = [dtype(1.0)]
        if bb == 0:
            code = 3
        else:
            for _ in range(int(ncg)):
                if rr <= tol * tol * bb:
                    code = 1
                    break
                t = w * gn_ref.jvec(P, vd, p, reverse)
                hp = np.where(free, rho * gn_ref.jtvec(P, vd, t, reverse) + mu * p, zero)
                php = _sum((p * hp)[free], reverse)
                if not php > 0:
                    code = 2
                    break
                a = rz / php
                d = np.where(free, d + a * p, zero)
                r = np.where(free, r - a * hp, zero)
                z = np.where(free, r / Mf, zero)
                rn = _sum((r * r)[free], reverse)
                rzn = _sum((r * z)[free], reverse)
                p = np.where(free, z + (rzn / rz) * p, zero)
                rz, rr = rzn, rn
                steps += 1
                hist.append(rr / bb)
        D = gd.copy()
        if steps:
            D[free] = d[free]
        slope = _sum(gd * D, reverse)
    return dict(D=D, steps=steps, bb=bb, rr=rr, slope=slope, nheld=int((~free).sum()), code=code, hist=hist, free=free,
                rz=rz, pc=np.where(free, M, zero), nzero=int(replaced.sum()))


def summary(d):
    """SUM[0..7] of a direction() result, as float64."""
    return np.concatenate([gn_ref.summary(d), np.array([d["rz"], d["nzero"]], dtype=np.float64)])


def iterate(st, par, gn, P, evaluate, lo, up, iters=1, dtype=np.float64, reverse=False, trace=None):
    """gn_ref.iterate with the preconditioned direction (st also takes PC; GSUM has 8 entries)."""
    st.setdefault("DC", np.zeros_like(st["X"]))
    st.setdefault("PC", np.zeros_like(st["X"]))
    st.setdefault("GSUM", np.zeros(8))
    for _ in range(iters):
        f, gr, lamp, viol, phi, vals = evaluate(st["XC"], st["LAM"], float(st["RHO"]))
        st["FC"], st["GRC"], st["LAMP"] = np.float64(f), np.array(gr, dtype=np.float64), np.array(lamp, dtype=np.float64)
        st["RSUM"][0], st["RSUM"][3] = viol, phi
        if int(st["ISTATE"][0]) < 2:                                # RUN = the phase: frozen problems are skipped
            held = lbfgs_ref.held_mask(st["XC"], st["GRC"], lo, up)
            d = direction(P, vals, st["LAMP"], st["RHO"], st["GRC"], gn["ncg"], gn["mu"], gn["tol"], held, dtype, reverse)
            st["DC"], st["PC"], st["GSUM"] = d["D"].astype(np.float64), d["pc"].astype(np.float64), summary(d)
        info = alsolve_ref.linesearch(st, par, lo, up, dtype, reverse)
        did = alsolve_ref.outer(st, par)
        gn_ref.select(st)
        with np.errstate(invalid="ignore", over="ignore"):
            st["XC"] = alsolve_ref.clamp(st["X"] - np.float64(st["ALPHA"]) * st["D"], lo, up)
        if trace is not None:
            trace.append((info["code"], did, int(st["ISTATE"][0])))
    return st
