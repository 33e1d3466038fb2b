"""numpy restatement of the resident AL loop of include/towr_gpu.h, one problem at a time: the line search
(towr_gpu_linesearch_batch_device), the outer update (towr_gpu_auglag_outer_batch_device), the initialisation and the
iteration (towr_gpu_alsolve_iterate_batch_device) with the evaluation behind a callback. `dtype` / `reverse` as in
tests/lbfgs_ref.py: the arithmetic and the order of the sums (and of the accept test taken on them); everything the
state stores is float64, and pg, MC, the trial lengths and the outer update are float64 operations in every mode, as
on the device. tests/test_alsolve_ref.py runs the loop on a convex QP with a known KKT point."""
import numpy as np

from tests import lbfgs_ref

RESTART, SEARCH, CONVERGED, STALLED, MAXED = range(5)
SIDE_INF = lbfgs_ref.SIDE_INF

DEFAULTS = dict(mem=5, max_inner=50, max_outer=20, c1=1e-4, shrink=0.5, alpha0=1.0, alpha_min=1e-10, curv_eps=1e-8,
                rho0=10.0, rho_grow=10.0, rho_max=1e8, eta0=0.1, eta_shrink=0.1, eta_star=1e-6,
                omega0=0.1, omega_shrink=0.1, omega_star=1e-6)


def params(**kw):
    assert not set(kw) - set(DEFAULTS), kw
    return {**DEFAULTS, **kw}


def clamp(t, lo, up):
    """t clamped to the sides that count (a NaN stays NaN)."""
    has_l, has_u = lo > -SIDE_INF, up < SIDE_INF
    with np.errstate(invalid="ignore"):
        xp = np.where(has_l & (t < lo), lo, t)
        return np.where(has_u & (xp > up), up, xp)


def proj_grad(x, g, lo, up):
    """pg = max_j |clamp(x - g) - x|, NaN on top (the step kernel's [0] with a = 1)."""
    s = np.abs(clamp(x - g, lo, up) - x)
    return np.float64(np.nan) if np.isnan(s).any() else (s.max() if s.size else np.float64(0.0))


def new_state(n, m, mem, x0, lam0=None, n_rsum=4, n_ssum=5):
    z = np.zeros
    return dict(X=np.array(x0, dtype=np.float64), GR=z(n), XC=z(n), GRC=z(n), D=z(n), LAM=z(m) if lam0 is None else np.array(lam0, float),
                LAMP=z(m), HS=z((mem, n)), HY=z((mem, n)), HMETA=np.zeros(2, dtype=np.int32), ALPHA=np.float64(0), RHO=np.float64(0),
                FC=np.float64(0), SCAL=z(8), ISTATE=np.zeros(4, dtype=np.int32), RSUM=z(n_rsum), SSUM=z(n_ssum), DSUM=z(5), USUM=z(6),
                LSUM=z(8))


def init(st, par, lo, up):
    st["ISTATE"][:] = (RESTART, 0, 0, 0)
    st["HMETA"][:] = 0
    st["RHO"], st["ALPHA"] = np.float64(par["rho0"]), np.float64(0.0)
    st["SCAL"][:] = (0, 0, par["eta0"], par["omega0"], 0, 0, 0, 0)
    st["XC"] = clamp(st["X"], lo, up)
    st["D"] = np.zeros_like(st["X"])


def linesearch(st, par, lo, up, dtype=np.float64, reverse=False):
    """The line search on one problem's state (changed in place). Returns dict(code, gs, abs_gs, sy, yy, abs_sy, margin):
    the sums as `dtype`, the sums of the absolute terms (for the error bounds) and margin = (M0 + c1 gs) - MC (the
    distance from the Armijo tie, NaN outside SEARCH)."""
    IS, SC, mem = st["ISTATE"], st["SCAL"], par["mem"]
    phase = int(IS[0])
    if phase not in (RESTART, SEARCH):
        IS[1] = 0
        st["LSUM"][0] = 0.0
        return dict(code=0)
    fc, viol = np.float64(st["FC"]), np.float64(st["RSUM"][0])
    with np.errstate(invalid="ignore", over="ignore"):
        mc = fc + np.float64(st["RSUM"][3])
    m0, pg_old = SC[0], SC[1]
    count, nxt = lbfgs_ref.meta_or_empty(st["HMETA"][0], st["HMETA"][1], mem)
    info = dict(gs=dtype(0), abs_gs=dtype(0), sy=dtype(0), yy=dtype(0), abs_sy=dtype(0), margin=np.nan)
    take, store = True, False
    if phase == SEARCH:
        with np.errstate(invalid="ignore", over="ignore"):
            s = st["XC"] - st["X"]
            gd, sd = st["GR"].astype(dtype), s.astype(dtype)
            gs = lbfgs_ref._sum(gd * sd, reverse)
            rhs = dtype(m0) + dtype(par["c1"]) * gs
            take = bool(gs <= 0) and bool(dtype(mc) <= rhs)
            info.update(gs=gs, abs_gs=np.sum(np.abs(gd * sd)), margin=rhs - dtype(mc))
        # the pair's sums always (LSUM[4..5]); the history changes only on an accepted base
        meta = st["HMETA"].copy() if take else np.array([count, nxt])
        HS, HY = (st["HS"], st["HY"]) if take else (st["HS"].copy(), st["HY"].copy())
        out, abs_sy = lbfgs_ref.update(st["X"], st["XC"], st["GR"], st["GRC"], par["curv_eps"], HS, HY, meta, dtype, reverse)
        info.update(sy=out[0], yy=out[2], abs_sy=abs_sy)
        if take:
            store = bool(out[3])
            if store:
                st["HMETA"][:] = meta
            st["USUM"][:6] = out.astype(np.float64)
    if take:
        st["X"], st["GR"] = st["XC"].copy(), st["GRC"].copy()
        pg = proj_grad(st["X"], st["GR"], lo, up)
        if phase == RESTART:
            st["HMETA"][:] = 0
            IS[0] = SEARCH
            code, flags = 1, 1 | 2 | 4
        else:
            code, flags = 2, 1 | 2
        SC[0], SC[1], SC[4], SC[5] = mc, pg, viol, fc
        st["ALPHA"] = np.float64(par["alpha0"])
    else:
        pg, flags = pg_old, 0
        with np.errstate(invalid="ignore"):
            a = np.float64(st["ALPHA"]) * np.float64(par["shrink"])
        if a >= par["alpha_min"]:
            st["ALPHA"], code = a, 3
        elif count > 0:
            st["HMETA"][:] = 0
            st["ALPHA"], flags, code = np.float64(par["alpha0"]), 2 | 4, 4
        else:
            IS[0] = STALLED
            st["ALPHA"], code = np.float64(0.0), 5
    IS[1] = flags
    IS[2] += 1
    st["LSUM"][:8] = (code, np.float64(info["gs"]), mc, m0, np.float64(info["sy"]), np.float64(info["yy"]), 1.0 if store else 0.0, pg)
    info["code"] = code
    return info


def outer(st, par):
    """The outer update on one problem's state. Returns what it did: None (not acting), 'converged', 'lam' or 'rho'."""
    IS, SC = st["ISTATE"], st["SCAL"]
    pg, eta, omega, viol = SC[1], SC[2], SC[3], SC[4]
    if int(IS[0]) != SEARCH or not (int(IS[1]) & 1) or not (pg <= omega or int(IS[2]) >= par["max_inner"]):
        return None
    st["ALPHA"] = np.float64(0.0)
    IS[1] = 0
    if viol <= eta and viol <= par["eta_star"] and pg <= par["omega_star"]:
        IS[0] = CONVERGED
        return "converged"
    if viol <= eta:
        st["LAM"] = st["LAMP"].copy()
        te, to = eta * np.float64(par["eta_shrink"]), omega * np.float64(par["omega_shrink"])
        SC[2] = te if te > par["eta_star"] else par["eta_star"]
        SC[3] = to if to > par["omega_star"] else par["omega_star"]
        did = "lam"
    else:
        with np.errstate(over="ignore"):
            tr = np.float64(st["RHO"]) * np.float64(par["rho_grow"])
        st["RHO"] = np.float64(tr if tr < par["rho_max"] else par["rho_max"])
        did = "rho"
    IS[3] += 1
    IS[2] = 0
    st["HMETA"][:] = 0
    IS[0] = MAXED if int(IS[3]) >= par["max_outer"] else RESTART
    return did


def iterate(st, par, evaluate, lo, up, iters=1, dtype=np.float64, reverse=False, trace=None):
    """`iters` iterations on one problem. evaluate(x, lam, rho) -> (f, grad of the augmented Lagrangian, lam+, max
    violation, phi). `trace`: a list that receives (LSUM[0] code, outer's answer, phase after) per iteration."""
    for _ in range(iters):
        f, gr, lamp, viol, phi = evaluate(st["XC"], st["LAM"], float(st["RHO"]))
        st["FC"], st["GRC"], st["LAMP"] = np.float64(f), np.array(gr, dtype=np.float64), np.array(lamp, dtype=np.float64)
        st["RSUM"][0], st["RSUM"][3] = viol, phi
        info = linesearch(st, par, lo, up, dtype, reverse)
        did = outer(st, par)
        if int(st["ISTATE"][1]) & 2:
            held = lbfgs_ref.held_mask(st["X"], st["GR"], lo, up)
            d = lbfgs_ref.direction(st["GR"], st["HS"], st["HY"], st["HMETA"], held, dtype, reverse)
            st["D"] = d["D"].astype(np.float64)
        with np.errstate(invalid="ignore", over="ignore"):
            st["XC"] = clamp(st["X"] - np.float64(st["ALPHA"]) * st["D"], lo, up)
        if trace is not None:
            trace.append((info["code"], did, int(st["ISTATE"][0])))
    return st
