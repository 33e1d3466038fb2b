"""numpy restatement of the stop rule of include/towr_gpu.h (towr_gpu_alsolve_stop_batch_device), one problem at a
time, and the iterations of tests/gn_ref.py, tests/chol_ref.py and tests/tile_chol_ref.py with the rule between
alsolve_ref.linesearch and alsolve_ref.outer (towr_gpu_alsolve_solve_ex_batch_device's iterations). The rule is IEEE
comparisons and one float64 product, so the device's bits are restated exactly. With stop = None the iterations are
those files' own, bit for bit. tests/test_stop_ref.py walks every branch."""
import numpy as np

from tests import alsolve_ref, chol_ref, gn_ref, lbfgs_ref, tile_chol_ref

ACCEPTABLE, INFEASIBLE = 5, 6
# the parameters of DESIGN 4p's runs: values for tests and documentation, not a default of the library
EXAMPLE = dict(acc_eta=1e-6, acc_omega=1e-4, acc_iters=15, infeas_keep=0.99, infeas_rho=1e4)
OFF = dict(acc_eta=0.0, acc_omega=0.0, acc_iters=0, infeas_keep=1.0, infeas_rho=np.inf)


def params(**kw):
    assert not set(kw) - set(OFF), kw
    return {**OFF, **kw}


def stop(st, par, sp):
    """The rule on one problem's state (changed in place). Returns what it did: None (not acting, or nothing but the run
    length), 'acceptable', 'infeasible' or 'recorded' (SCAL[7] = viol: the outer update grows RHO next)."""
    IS, SC = st["ISTATE"], st["SCAL"]
    if int(IS[0]) != alsolve_ref.SEARCH:
        return None
    flags, inner = int(IS[1]), int(IS[2])
    pg, eta, omega, viol = SC[1], SC[2], SC[3], SC[4]
    if sp["acc_iters"] > 0:
        within = bool(viol <= sp["acc_eta"]) and bool(pg <= sp["acc_omega"])       # (a NaN: False)
        run = SC[6] + np.float64(1.0) if within else np.float64(0.0)
        SC[6] = run
        if run >= np.float64(sp["acc_iters"]):
            IS[0], IS[1] = ACCEPTABLE, 0
            st["ALPHA"] = np.float64(0.0)
            return "acceptable"
    grow = bool(flags & 1) and (bool(pg <= omega) or inner >= par["max_inner"]) and not bool(viol <= eta)
    if not grow:
        return None
    last = SC[7]
    with np.errstate(invalid="ignore", over="ignore"):
        keep = np.float64(sp["infeas_keep"]) * last
    if bool(last > 0.0) and bool(viol >= keep) and bool(np.float64(st["RHO"]) >= sp["infeas_rho"]):
        IS[0], IS[1] = INFEASIBLE, 0
        st["ALPHA"] = np.float64(0.0)
        return "infeasible"
    SC[7] = viol
    return "recorded"


def iterate(st, par, sp, evaluate, lo, up, direct, gsum, iters=1, dtype=np.float64, reverse=False, trace=None):
    """The GN iteration of tests/gn_ref.py around a direction: direct(vals, held) -> (DC, GSUM) at (XC, GRC, LAMP, RHO) of
    `st`. sp None: no stop rule. `trace` receives (LSUM[0] code, outer's answer, phase after, the rule's answer)."""
    st.setdefault("DC", np.zeros_like(st["X"]))
    st.setdefault("GSUM", np.zeros(gsum))
    for _ in range(iters):
        f, gr, lamp, viol, phi, vals = evaluate(st["XC"], st["LAM"], float(st["RHO"]))
        st["FC"], st["GRC"], st["LAMP"] = np.float64(f), np.array(gr, dtype=np.float64), np.array(lamp, dtype=np.float64)
        st["RSUM"][0], st["RSUM"][3] = viol, phi
        if int(st["ISTATE"][0]) < 2:                                # RUN = the phase: frozen problems are skipped
            held = lbfgs_ref.held_mask(st["XC"], st["GRC"], lo, up)
            st["DC"], st["GSUM"] = direct(vals, held)
        info = alsolve_ref.linesearch(st, par, lo, up, dtype, reverse)
        rule = stop(st, par, sp) if sp is not None else None
        did = alsolve_ref.outer(st, par)
        gn_ref.select(st)
        with np.errstate(invalid="ignore", over="ignore"):
            st["XC"] = alsolve_ref.clamp(st["X"] - np.float64(st["ALPHA"]) * st["D"], lo, up)
        if trace is not None:
            trace.append((info["code"], did, int(st["ISTATE"][0]), rule))
    return st


def gn_iterate(st, par, sp, gn, P, evaluate, lo, up, iters=1, dtype=np.float64, reverse=False, trace=None):
    """gn_ref.iterate with the rule: gn = dict(ncg, mu, tol)."""
    def direct(vals, held):
        d = gn_ref.direction(P, vals, st["LAMP"], st["RHO"], st["GRC"], gn["ncg"], gn["mu"], gn["tol"], held, dtype, reverse)
        return d["D"].astype(np.float64), gn_ref.summary(d)
    return iterate(st, par, sp, evaluate, lo, up, direct, 6, iters, dtype, reverse, trace)


def chol_iterate(st, par, sp, gn, P, evaluate, lo, up, iters=1, dtype=np.float64, reverse=False, trace=None):
    """chol_ref.iterate with the rule: gn = dict(mu, pos, first)."""
    def direct(vals, held):
        d = chol_ref.direction(P, vals, st["LAMP"], st["RHO"], st["GRC"], gn["mu"], gn["pos"], gn["first"], held, dtype, reverse)
        return d["D"].astype(np.float64), chol_ref.summary(d)
    return iterate(st, par, sp, evaluate, lo, up, direct, 8, iters, dtype, reverse, trace)


def tile_iterate(st, par, sp, gn, P, evaluate, lo, up, iters=1, dtype=np.float64, trace=None):
    """tile_chol_ref.iterate with the rule: gn = dict(mu, pos, first)."""
    def direct(vals, held):
        d = tile_chol_ref.direction(P, vals, st["LAMP"], st["RHO"], st["GRC"], gn["mu"], gn["pos"], gn["first"], held, dtype)
        return d["D"].astype(np.float64), tile_chol_ref.summary(d)
    return iterate(st, par, sp, evaluate, lo, up, direct, 8, iters, dtype, False, trace)


def stop_batch(h, par, sp, B):
    """The rule on problems [0, B) of a host copy h = dict(ISTATE (4 B ints), SCAL (B, >= 8), ALPHA (B), RHO (B)), in
    place: what the device call leaves in those arrays."""
    for b in range(B):
        st = dict(ISTATE=h["ISTATE"][4 * b:4 * b + 4], SCAL=h["SCAL"][b], ALPHA=np.float64(h["ALPHA"][b]), RHO=np.float64(h["RHO"][b]))
        stop(st, par, sp)
        h["ALPHA"][b] = st["ALPHA"]
    return h
