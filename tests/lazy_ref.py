"""numpy restatement of the verdict stage of include/towr_gpu.h (towr_gpu_alsolve_verdict_batch_device), one problem at
a time, and the GN iterations of tests/stop_ref.py / tests/probe_ref.py with the stage ahead of the direction
(towr_gpu_alsolve_gn_lazy_iterate_batch_device's iterations): the direction is computed only where the verdict is 0. The
stage is the line search's accept test: one float64 sum, one rounded product, one rounded addition and IEEE comparisons,
so with `device_tree` as the sum the device's words are restated exactly. tests/test_lazy_ref.py walks every branch."""
import numpy as np

from tests import alsolve_ref, probe_ref, stop_ref
from tests.probe_ref import device_tree

RUN, SKIP = 0, 2   # the words of VERDICT: a RUN mask for the direction entries (run_stride 1)


def verdict(st, par, gsum=device_tree):
    """The stage on one problem's state (not changed): 0 where the line search behind it will accept a base, else 2. st
    holds ISTATE, X, GR, XC, FC, RSUM and SCAL as the line search finds them; gsum is the sum of gs (device_tree: the
    device's tree; np.sum: the order of alsolve_ref.linesearch in float64)."""
    phase = int(st["ISTATE"][0])
    if phase == alsolve_ref.RESTART:
        return RUN
    if phase != alsolve_ref.SEARCH:
        return SKIP
    with np.errstate(invalid="ignore", over="ignore"):
        gs = np.float64(gsum(st["GR"] * (st["XC"] - st["X"])))
        mc = np.float64(st["FC"]) + np.float64(st["RSUM"][3])
        m0 = np.float64(st["SCAL"][0])
        c1gs = np.float64(par["c1"]) * gs
        take = bool(gs <= 0.0) and bool(mc <= m0 + c1gs)   # (a NaN anywhere: False)
    return RUN if take else SKIP


def iterate(st, par, sp, T, evaluate, lo, up, direct, gsum_width, iters=1, merit=None, trace=None, psums=None, verdicts=None,
            gsum=np.sum):
    """`iters` iterations of probe_ref.iterate (T None or 0: of stop_ref.iterate) with the verdict ahead of the direction:
    `direct` is called only on verdict 0, else DC and GSUM stay as they are. st["NDIR"] counts the zeros and `verdicts`
    receives the word of every iteration (2 for a frozen problem, whose direction the loop never calls). gsum: np.sum, the
    order of the reference's own line search."""
    st.setdefault("DC", np.zeros_like(st["X"]))
    st.setdefault("GSUM", np.zeros(gsum_width))
    st.setdefault("NDIR", 0)
    word = [SKIP]

    def lazy_direct(vals, held):   # (stop_ref.iterate calls it behind the evaluation: FC, GRC and RSUM are the candidate's)
        word[0] = verdict(st, par, gsum)
        if word[0] != RUN:
            return st["DC"], st["GSUM"]
        st["NDIR"] += 1
        return direct(vals, held)

    for _ in range(iters):
        word[0] = SKIP
        probe_ref.iterate(st, par, sp, T, evaluate, lo, up, lazy_direct, gsum_width, 1, merit, trace, psums)
        if verdicts is not None:
            verdicts.append(word[0])
    return st


def verdict_batch(h, par, n, gsum=device_tree):
    """The stage on the problems of a host copy h = dict(X, GR, XC (B, >= n), FC (B), SCAL (B, >= 8), RSUM (B, >= 4),
    ISTATE (4 B ints), VERDICT (B ints), NDIR (B ints) or None), in place: what the device call leaves in VERDICT and NDIR."""
    B = h["FC"].shape[0]
    for b in range(B):
        st = dict(ISTATE=h["ISTATE"][4 * b:4 * b + 4], X=h["X"][b, :n], GR=h["GR"][b, :n], XC=h["XC"][b, :n], FC=h["FC"][b],
                  RSUM=h["RSUM"][b], SCAL=h["SCAL"][b])
        w = verdict(st, par, gsum)
        h["VERDICT"][b] = w
        if w == RUN and h.get("NDIR") is not None:
            h["NDIR"][b] += 1
    return h
