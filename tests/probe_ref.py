"""numpy restatement of the probe stage of include/towr_gpu.h (towr_gpu_alsolve_probe_batch_device), one problem at a
time, and the iterations of tests/stop_ref.py with the stage in front (towr_gpu_alsolve_solve_probe_batch_device's
iterations). The stage tests lengths of the line search's own ladder with a merit callback and leaves ALPHA, XC and the
inner counter where the loop without probes stands after the rejections it found: every float64 operation of the header
is restated (the ladder's rounded products, the step's expression, the line search's test), so with the device's own
merit and `device_tree` as the sum the device's bytes are restated exactly. tests/test_probe_ref.py walks every branch."""
import numpy as np

from tests import alsolve_ref, stop_ref

PROBE_MAX = 8
NAN = np.float64(np.nan)
LANES, WAVE = 256, 64   # the line search's block and the wave


def device_tree(terms):
    """The sum of `terms` (float64, column order) on the line search's tree: lane l adds columns l, l + 256, ... in
    ascending order, a halving tree over each wave of 64 lanes, then the four waves added in wave order."""
    t = np.asarray(terms, dtype=np.float64)
    pad = np.zeros(-(-max(t.size, 1) // LANES) * LANES)
    pad[:t.size] = t                        # (+0.0 beyond n: the partial starts at +0.0, so adding it changes no bit)
    with np.errstate(invalid="ignore", over="ignore"):
        acc = np.zeros(LANES)
        for row in pad.reshape(-1, LANES):
            acc = acc + row
        w = acc.reshape(LANES // WAVE, WAVE).copy()
        o = WAVE // 2
        while o > 0:
            w[:, :o] = w[:, :o] + w[:, o:2 * o]
            o //= 2
        out = w[0, 0]
        for k in range(1, LANES // WAVE):
            out = out + w[k, 0]
    return np.float64(out)


def al_merit(o, gl, gu):
    """merit(x, lam, rho) = f + phi from an oracle's f and g alone: the expressions of the evaluations in
    tests/test_pgn_ref.py and tests/test_stop_ref.py, so the bits of their f + phi, without a Jacobian."""
    def merit(x, lam, rho):
        g = o.eval_g(x)
        t = g + lam / rho
        r = t - alsolve_ref.clamp(t, gl, gu)
        phi = np.sum(0.5 * rho * r * r - 0.5 * lam * lam / rho)
        with np.errstate(invalid="ignore", over="ignore"):
            return np.float64(o.eval_f(x)) + np.float64(phi)
    return merit


def merit_of(evaluate):
    """merit(x, lam, rho) from an evaluation callback of tests/stop_ref.iterate: FC + RSUM[3] as the line search adds them."""
    def merit(x, lam, rho):
        e = evaluate(x, lam, rho)
        with np.errstate(invalid="ignore", over="ignore"):
            return np.float64(e[0]) + np.float64(e[4])
    return merit


def probe(st, par, T, merit, lo, up, gsum=np.sum):
    """The stage on one problem's state (changed in place): merit(x, lam, rho) -> f + phi, gsum the sum of gs (np.sum: the
    order of alsolve_ref.linesearch in float64; device_tree: the device's). Returns PSUM[0..7], or None for a problem that
    is not in SEARCH (the device writes PSUM[0] = 0 and nothing else)."""
    assert 1 <= T <= PROBE_MAX
    IS = st["ISTATE"]
    if int(IS[0]) != alsolve_ref.SEARCH:
        return None
    shrink, amin, c1 = np.float64(par["shrink"]), np.float64(par["alpha_min"]), np.float64(par["c1"])
    m0 = np.float64(st["SCAL"][0])
    with np.errstate(invalid="ignore", over="ignore"):
        a = [np.float64(st["ALPHA"])]
        for _ in range(T):
            a.append(a[-1] * shrink)
        v = 1                                                  # t = 0 always counts
        while v <= T and a[v] >= amin:                         # (a NaN ends the run)
            v += 1

        def cand(al):
            xt = alsolve_ref.clamp(st["X"] - al * st["D"], lo, up)
            return xt, np.float64(gsum(st["GR"] * (xt - st["X"])))

        code = 0
        for t in range(min(v, T)):
            xt, gs = cand(a[t])
            mc = np.float64(merit(xt, st["LAM"], float(st["RHO"])))
            if bool(gs <= 0) and bool(mc <= m0 + c1 * gs):     # (a NaN anywhere: False)
                code, tstar = 1, t
                break
        if code == 0 and v == T + 1:                           # none passed: the next, untested length
            code, tstar, mc = 2, T, NAN
            xt, gs = cand(a[T])
        elif code == 0:                                        # none passed: the last valid length stays (xt, mc, gs are its)
            code, tstar = 3, v - 1
    st["ALPHA"] = a[tstar]
    st["XC"] = xt
    IS[2] += tstar
    return np.array([code, tstar, T if code == 2 else tstar + 1, a[tstar], mc, gs, 0.0, 0.0], dtype=np.float64)


def iterate(st, par, sp, T, evaluate, lo, up, direct, gsum_width, iters=1, merit=None, trace=None, psums=None):
    """`iters` iterations of stop_ref.iterate (float64, ascending sums) with the stage in front of each. T None or 0: no
    stage. merit None: from `evaluate`. `psums` receives the stage's return per iteration."""
    merit = merit or merit_of(evaluate)
    for _ in range(iters):
        ps = probe(st, par, T, merit, lo, up) if T else None
        if psums is not None:
            psums.append(ps)
        stop_ref.iterate(st, par, sp, evaluate, lo, up, direct, gsum_width, 1, np.float64, False, trace)
    return st


def probe_batch(h, par, T, merit, lo, up, n, m, gsum=device_tree):
    """The stage on the problems of a host copy h = dict(X, D, GR, XC (B, >= n), LAM (B, >= m), ALPHA, RHO (B), SCAL
    (B, >= 8), ISTATE (4 B ints), PSUM (B, >= 8)), in place: what the device call leaves in ALPHA, XC, ISTATE and PSUM.
    merit(b, x, lam, rho); lo, up: (n,) or (B, n)."""
    B = h["ALPHA"].shape[0]
    for b in range(B):
        l, u = (lo[b], up[b]) if np.ndim(lo) == 2 else (lo, up)
        st = dict(ISTATE=h["ISTATE"][4 * b:4 * b + 4], SCAL=h["SCAL"][b], ALPHA=np.float64(h["ALPHA"][b]), RHO=np.float64(h["RHO"][b]),
                  X=h["X"][b, :n], D=h["D"][b, :n], GR=h["GR"][b, :n], LAM=h["LAM"][b, :m], XC=None)
        ps = probe(st, par, T, lambda x, lam, rho: merit(b, x, lam, rho), l, u, gsum)
        if ps is None:
            h["PSUM"][b, 0] = 0.0
            continue
        h["PSUM"][b, :8] = ps
        h["ALPHA"][b] = st["ALPHA"]
        h["XC"][b, :n] = st["XC"]
    return h
