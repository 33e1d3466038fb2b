"""numpy restatement of the L-BFGS formulas of include/towr_gpu.h (towr_gpu_lbfgs_update_batch_device and
towr_gpu_lbfgs_direction_batch_device), one problem at a time. `dtype` is the arithmetic of the sums and of the
recursion: np.float64 or np.longdouble (s = xn - x and y = grn - gr are float64 subtractions in both, as on the device).
`reverse` sums the columns in reversed order (numpy's pairwise sum over the reversed terms): a second summation order
of the same sums, for measuring how far two float64 evaluations lie apart. tests/test_lbfgs_ref.py checks this file
against the dense BFGS inverse update."""
import numpy as np

SIDE_INF = 1e19


def _sum(t, reverse):
    return np.sum(t[::-1]) if reverse else np.sum(t)


def meta_or_empty(count, nxt, mem):
    """An out-of-range {count, next} is an empty history."""
    return (int(count), int(nxt)) if 0 <= count <= mem and 0 <= nxt < mem else (0, 0)


def update(x, xn, gr, grn, curv_eps, HS, HY, meta, dtype=np.float64, reverse=False):
    """Offer the pair (xn - x, grn - gr) to the history HS, HY (mem, >= n), meta = [count, next] (all changed in place
    when the pair is accepted). Returns SUM[0..5] (as `dtype`) and sum |s y| (for the error bound and the tie check)."""
    n, mem = x.shape[0], HS.shape[0]
    with np.errstate(invalid="ignore"):
        s, y = xn - x, grn - gr
        sd, yd = s.astype(dtype), y.astype(dtype)
        sy, ss, yy = _sum(sd * yd, reverse), _sum(sd * sd, reverse), _sum(yd * yd, reverse)
        accept = bool(sy > dtype(curv_eps) * yy)
    count, nxt = meta_or_empty(meta[0], meta[1], mem)
    slot = -1
    if accept:
        slot = nxt
        HS[slot, :n], HY[slot, :n] = s, y
        meta[0], meta[1] = min(count + 1, mem), (nxt + 1) % mem
        count = int(meta[0])
    out = np.array([sy, ss, yy, 1.0 if accept else 0.0, count, slot], dtype=dtype)
    return out, np.sum(np.abs(sd * yd))


def held_mask(x, g, lo, up):
    """The held columns: on a side that counts with the gradient pointing out of the box, or fixed. x None: none."""
    if x is None:
        return np.zeros(g.shape, dtype=bool)
    has_l, has_u = lo > -SIDE_INF, up < SIDE_INF
    with np.errstate(invalid="ignore"):
        return (has_l & (x <= lo) & (g > 0)) | (has_u & (x >= up) & (g < 0)) | (has_l & has_u & (lo == up))


def direction(g, HS, HY, meta, held=None, dtype=np.float64, reverse=False, drop=None):
    """The two-loop recursion on the free columns. HS, HY (mem, >= n), meta = [count, next]. `drop`: the pair i (1 =
    newest) to leave out although the formulas use it — a deliberately wrong recursion, for checking that a gate
    refuses one. Returns dict(D, used (the i's), gamma, slope, nheld, gg, c (per i), abs_c (sum_free |s y| per i))."""
    n, mem = g.shape[0], HS.shape[0]
    count, nxt = meta_or_empty(meta[0], meta[1], mem)
    free = np.ones(n, dtype=bool) if held is None else ~held
    gd = g.astype(dtype)
    q = gd[free].copy()
    used, al, cs, c_all, abs_c = [], {}, {}, [], []
    gamma = dtype(1.0)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        for i in range(1, count + 1):
            slot = (nxt - i) % mem
            s, y = HS[slot, :n][free].astype(dtype), HY[slot, :n][free].astype(dtype)
            c = _sum(s * y, reverse)
            c_all.append(c)
            abs_c.append(np.sum(np.abs(s * y)))
            if not c > 0 or i == drop:
                continue
            a = _sum(s * q, reverse) / c
            if not used:
                gamma = c / _sum(y * y, reverse)
            used.append(i)
            al[i], cs[i] = a, c
            q = q - a * y
        r = gamma * q if used else q
        for i in reversed(used):
            slot = (nxt - i) % mem
            s, y = HS[slot, :n][free].astype(dtype), HY[slot, :n][free].astype(dtype)
            beta = _sum(y * r, reverse) / cs[i]
            r = r + (al[i] - beta) * s
        D = gd.copy()
        D[free] = r
        slope = _sum(gd * D, reverse)
        gg = _sum(gd[free] * gd[free], reverse)
    return dict(D=D, used=used, gamma=gamma, slope=slope, nheld=int((~free).sum()), gg=gg, c=c_all, abs_c=abs_c, free=free)
