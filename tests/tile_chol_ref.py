"""numpy restatement of the tiled direct Gauss-Newton direction of include/towr_gpu.h
(towr_gpu_gn_tile_info's tile envelope; towr_gpu_gn_direction_tiled_batch_device: the assembly of
H = rho (J^T W J)_ff + mu I into 16 x 16 tiles, the block Cholesky factorisation in the header's order, the two block
solves, the codes and SUM) and of the iteration that uses it (towr_gpu_alsolve_gn_tiled_iterate_batch_device), one
problem at a time, in np.float64 or np.longdouble. The order of every sum is the header's, except inside a group of four
products, which the device forms in one v_mfma_f64_16x16x4_f64 and this file as a 16 x 4 by 4 x 16 numpy product: the
device's bits are not restated here. The assembly, the held rule, the line search, the outer update, the select and the
step are those of tests/chol_ref.py / tests/alsolve_ref.py / tests/gn_ref.py. tests/test_tile_chol_ref.py checks this
file against a dense solve."""
import numpy as np

from tests import alsolve_ref, chol_ref, gn_ref, lbfgs_ref

TILE = 16


def tile_tables(first, n, tile=TILE):
    """(nt, bfirst, tiles) of the scalar envelope `first` (n entries): bfirst[I] = min first[q] // tile over the rows of
    block row I, tiles = sum_I (I - bfirst[I] + 1)."""
    first = np.asarray(first, dtype=np.int64)
    nt = (n + tile - 1) // tile
    bfirst = np.array([int(first[tile * I:min(n, tile * (I + 1))].min()) // tile for I in range(nt)], dtype=np.int64)
    assert (bfirst <= np.arange(nt)).all()
    return nt, bfirst, int((np.arange(nt) - bfirst + 1).sum())


def stored_mask(n, bfirst, tile=TILE):
    """The stored tiles' entries on and under the diagonal as a (tile nt, tile nt) boolean matrix."""
    nt = len(bfirst)
    M = np.zeros((tile * nt, tile * nt), dtype=bool)
    for I in range(nt):
        M[tile * I:tile * (I + 1), tile * bfirst[I]:tile * (I + 1)] = True
    return np.tril(M)


def into_tiles(Hp, bfirst, dtype=np.float64, tile=TILE):
    """The permuted Hp (n, n) as the padded lower triangle the tiles hold: the identity on the padding's diagonal, 0
    elsewhere in it; nothing of Hp's lower triangle may lie outside the stored tiles."""
    n, nt = Hp.shape[0], len(bfirst)
    A = np.eye(tile * nt, dtype=dtype)
    A[:n, :n] = np.tril(Hp)
    outside = ~stored_mask(n, bfirst, tile)
    low = np.tril(np.ones_like(outside))
    with np.errstate(invalid="ignore"):
        assert not (A[outside & low] != 0).any(), "an entry of the lower triangle outside the tile envelope"
    return A


def factor_solve(Hp, gp, bfirst, heldq, dtype=np.float64, tile=TILE):
    """The block Cholesky factorisation of the permuted Hp inside the tile envelope `bfirst`, left-looking by block
    column, and the two block solves with the permuted right-hand side gp, in the header's order. Returns dict(d
    (permuted, n entries; None on a breakdown), code, bcol, pmin, pmax)."""
    n, nt = Hp.shape[0], len(bfirst)
    T = tile
    A = into_tiles(Hp, bfirst, dtype, T)
    g = np.zeros(T * nt, dtype=dtype)
    g[:n] = gp
    counted = np.zeros(T * nt, dtype=bool)
    counted[:n] = ~np.asarray(heldq, dtype=bool)
    below = [[I for I in range(J + 1, nt) if bfirst[I] <= J] for J in range(nt)]
    blk = lambda I: slice(T * I, T * (I + 1))
    y = np.zeros(T * nt, dtype=dtype)
    pmin, pmax = np.inf, 0.0
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        for J in range(nt):
            # the tile products, K ascending, four k at a time
            for I in [J] + below[J]:
                t = A[blk(I), blk(J)].copy()
                for K in range(max(bfirst[I], bfirst[J]), J):
                    a, b = A[blk(I), blk(K)], A[blk(J), blk(K)]
                    for kk in range(0, T, 4):
                        t = t - a[:, kk:kk + 4] @ b[:, kk:kk + 4].T
                A[blk(I), blk(J)] = t
            # the forward solve's sum in four partial sums (k mod 4), combined (p0 + p1) + (p2 + p3)
            p = np.zeros((T, 4), dtype=dtype)
            for K in range(bfirst[J], J):
                terms = A[blk(J), blk(K)] * y[blk(K)][None, :]
                for kk in range(0, T, 4):
                    p = p + terms[:, kk:kk + 4]
            t_ = g[blk(J)] - ((p[:, 0] + p[:, 1]) + (p[:, 2] + p[:, 3]))
            # the diagonal tile, unblocked
            D = A[blk(J), blk(J)].copy()
            for k in range(T):
                piv = D[k, k]
                if not piv > 0:
                    return dict(d=None, code=2, bcol=T * J + k, pmin=pmin, pmax=pmax)
                if counted[T * J + k]:
                    pmin, pmax = min(pmin, float(piv)), max(pmax, float(piv))
                l = np.sqrt(piv)
                D[k, k] = l
                D[k + 1:, k] = D[k + 1:, k] / l
                t_[k] = t_[k] / l
                t_[k + 1:] = t_[k + 1:] - D[k + 1:, k] * t_[k]
                for c in range(k + 1, T):
                    D[c:, c] = D[c:, c] - D[c:, k] * D[c, k]
            D = np.tril(D)
            A[blk(J), blk(J)] = D
            y[blk(J)] = t_
            # the panel: X L_JJ^T = A by columns ascending, the products subtracted one by one
            for I in below[J]:
                X = A[blk(I), blk(J)].copy()
                for c in range(T):
                    s = X[:, c].copy()
                    for k in range(c):
                        s = s - X[:, k] * D[c, k]
                    X[:, c] = s / D[c, c]
                A[blk(I), blk(J)] = X
        # the backward solve, block columns descending
        acc = np.zeros(T * nt, dtype=dtype)
        d = np.zeros(T * nt, dtype=dtype)
        for J in range(nt - 1, -1, -1):
            D = A[blk(J), blk(J)]
            t_ = y[blk(J)] - acc[blk(J)]
            for k in range(T - 1, -1, -1):
                t_[k] = t_[k] / D[k, k]
                t_[:k] = t_[:k] - D[k, :k] * t_[k]
            d[blk(J)] = t_
            for K in range(bfirst[J], J):
                terms = A[blk(J), blk(K)] * t_[:, None]        # (r, c): L_rc d_r
                s = np.zeros(T, dtype=dtype)
                for r in range(T - 1, -1, -1):
                    s = s + terms[r]
                acc[blk(K)] = acc[blk(K)] + s
    return dict(d=d[:n], code=1, bcol=-1, pmin=pmin, pmax=pmax)


def direction(P, vals, lamp, rho, g, mu, pos, first, held=None, dtype=np.float64, ignore_w=False, ignore_held=False):
    """The tiled direction: chol_ref.direction with the factorisation above (bb, the assembly and the slope sum are that
    file's ascending sums). `ignore_w` / `ignore_held`: the two deliberately wrong systems."""
    n = P.n
    pos = np.asarray(pos, dtype=np.int64)
    held = np.zeros(n, dtype=bool) if held is None else np.asarray(held, dtype=bool)
    used = np.zeros(n, dtype=bool) if ignore_held else held
    free = ~held
    gd = np.asarray(g).astype(dtype)
    inv = np.argsort(pos)
    with np.errstate(invalid="ignore", over="ignore"):
        bb = np.sum(gd[free] * gd[free])
    out = dict(code=3, bcol=-1, pmin=np.inf, pmax=0.0)
    d = None
    if not bb == 0:
        H = chol_ref.assemble(P, vals, lamp, rho, mu, used, dtype, False, ignore_w)
        _, bfirst, _ = tile_tables(first, n)
        out = factor_solve(H[np.ix_(inv, inv)], gd[inv], bfirst, used[inv], dtype)
        d = out["d"]
    D = gd.copy()
    if d is not None:
        D[~used] = d[pos[~used]]
    with np.errstate(invalid="ignore", over="ignore"):
        slope = np.sum(gd * D)
    pmin = 0.0 if np.isinf(out["pmin"]) else out["pmin"]
    return dict(D=D, solved=out["code"] == 1, bb=bb, pmin=pmin, slope=slope, nheld=int(held.sum()), code=out["code"],
                pmax=out["pmax"], bcol=out["bcol"], free=free)


summary = chol_ref.summary


def iterate(st, par, gn, P, evaluate, lo, up, iters=1, dtype=np.float64, trace=None):
    """chol_ref.iterate with the direction above: gn = dict(mu, pos, first). GSUM has 8 entries."""
    st.setdefault("DC", np.zeros_like(st["X"]))
    st.setdefault("GSUM", np.zeros(8))
    for _ in range(iters):
        f, gr, lamp, viol, phi, vals = evaluate(st["XC"], st["LAM"], float(st["RHO"]))
        st["FC"], st["GRC"], st["LAMP"] = np.float64(f), np.array(gr, dtype=np.float64), np.array(lamp, dtype=np.float64)
        st["RSUM"][0], st["RSUM"][3] = viol, phi
        if int(st["ISTATE"][0]) < 2:                                # RUN = the phase: frozen problems are skipped
            held = lbfgs_ref.held_mask(st["XC"], st["GRC"], lo, up)
            d = direction(P, vals, st["LAMP"], st["RHO"], st["GRC"], gn["mu"], gn["pos"], gn["first"], held, dtype)
            st["DC"], st["GSUM"] = d["D"].astype(np.float64), summary(d)
        info = alsolve_ref.linesearch(st, par, lo, up, dtype, False)
        did = alsolve_ref.outer(st, par)
        gn_ref.select(st)
        with np.errstate(invalid="ignore", over="ignore"):
            st["XC"] = alsolve_ref.clamp(st["X"] - np.float64(st["ALPHA"]) * st["D"], lo, up)
        if trace is not None:
            trace.append((info["code"], did, int(st["ISTATE"][0])))
    return st
