"""The queued solve's entry points at the C-ABI boundary (no GPU, a layout-only handle, fake pointers: nothing runs): the
symbols and the struct exist, every refusal include/towr_gpu.h lists for towr_gpu_alsolve_retire_key_batch_device,
towr_gpu_alsolve_move_rows_batch_device and towr_gpu_alsolve_solve_queue_batch_device is TOWR_ERR_INVALID with a message,
and valid arguments are TOWR_ERR_NO_DEVICE — every check comes before the device is bound."""
import ctypes as C

import pytest

from tests.configs import config_descs
from tests.test_alsolve_capi import BAD_PARAMS, PTRS
from tests.test_gn_capi import INV, NAN, NODEV, Q
from tests.test_solve_capi import DC, GSUM, METHODS, PC, QW, STEP, _apart, _rows
from towr2025_amd import TowrGpuProblem, _capi as capi, alsolve_params, alsolve_stop_params, gn_params

QUEUE_PTRS = ("X0", "ID", "AGE", "KEY", "X_OUT", "LAM_OUT", "RHO_OUT", "SCAL_OUT", "ISTATE_OUT", "ITERS_OUT")
OPTIONAL = ("LAM0", "GL", "GU", "XL", "XU", "GLW", "GUW", "XLW", "XUW")


@pytest.fixture(scope="module")
def p():
    return TowrGpuProblem(config_descs()["monoped_procedural"], device=-1)


def _queue(p, N=5, per_problem=False, **kw):
    """A valid towr_solve_queue_t on fake pointers, every array at its own address; per_problem: N bound rows each with
    their work rows. `kw` replaces fields."""
    q = capi.SolveQueue(N=N)
    for i, k in enumerate(QUEUE_PTRS + OPTIONAL):
        setattr(q, k, Q + (60 + i) * STEP)
    for k in OPTIONAL:
        setattr(q, k, None)
    q.ldx0, q.ldxo, q.ldl0, q.ldlo = p.n, p.n + 1, 0, p.m
    if per_problem:
        for i, k in enumerate(OPTIONAL):
            setattr(q, k, Q + (80 + i) * STEP)
        q.ldl0, q.ldgb, q.ldxb, q.ldgw, q.ldxw = p.m, p.m, p.n + 2, p.m + 1, p.n
    for k, v in kw.items():
        setattr(q, k, v)
    return q


def _solve(p, method=capi.SOLVE_GN_TILED, max_iters=4, check_every=2, compact=1, par="default", st="default", d="default", B=2,
           q="default", LOG=Q, report="default", opts="default", stop=None, **dkw):
    par = alsolve_params() if par == "default" else par
    st = _apart(p) if st == "default" else st
    q = _queue(p) if q == "default" else q
    if opts == "default":
        opts = capi.SolveOpts(method=method, max_iters=max_iters, check_every=check_every, compact=compact)
    if d == "default":
        d = capi.SolveDir()
        d.gn = C.pointer(gn_params(ncg=3, mu=1e-6, tol=1e-3))
        d.precond, d.wrows, d.DC, d.GSUM, d.ldgs, d.PC, d.W = capi.GN_PC_JACOBI, 1, DC, GSUM, 8, PC, QW
        d.ldw = p.gn_tile_info()["ldw_min"]
        for k, v in dkw.items():
            setattr(d, k, v)
    rep = capi.SolveReport() if report == "default" else report
    return p._lib.towr_gpu_alsolve_solve_queue_batch_device(
        p._h, B, None if opts is None else C.byref(opts), par, None if stop is None else C.byref(stop), st,
        None if d is None else C.byref(d), None if q is None else C.byref(q), C.c_void_p(LOG) if LOG else None,
        None if rep is None else C.byref(rep), None)


def test_symbols_structs_and_methods():
    lib = capi.load_library()
    for name in ("towr_gpu_alsolve_retire_key_batch_device", "towr_gpu_alsolve_move_rows_batch_device",
                 "towr_gpu_alsolve_solve_queue_batch_device"):
        assert hasattr(lib, name) and name in capi.SYMBOLS
    assert capi.ABI_VERSION == 4 and lib.towr_gpu_abi_version() == 4          # additive: the version stays
    assert C.sizeof(capi.AlSolveStateC) == 29 * 8 and C.sizeof(capi.AlSolveStop) == 40
    assert (C.sizeof(capi.Rows), C.sizeof(capi.SolveOpts), C.sizeof(capi.SolveDir), C.sizeof(capi.SolveReport)) == (24, 16, 64, 48)
    assert C.sizeof(capi.SolveQueue) == 8 + 27 * 8
    header = open(capi.__file__.replace("towr2025_amd/_capi.py", "include/towr_gpu.h")).read()
    assert "#define TOWR_MOVE_MAX_ARRAYS 16" in header and capi.MOVE_MAX_ARRAYS == 16
    body = header[header.index("int32_t N, reserved;"):header.index("} towr_solve_queue_t;")]
    names = [k for k, _ in capi.SolveQueue._fields_]
    assert [body.index(k) for k in names] == sorted(body.index(k) for k in names), "the mirror's field order"
    for m in ("alsolve_retire_key", "alsolve_move_rows", "alsolve_solve_queue"):
        assert callable(getattr(TowrGpuProblem, m))


def test_retire_key_refusals(p):
    f, h, qp = p._lib.towr_gpu_alsolve_retire_key_batch_device, p._h, C.c_void_p(Q)
    err = lambda: p._lib.towr_gpu_last_error(h)
    assert f(h, 3, qp, qp, 0, 8, qp, None) == NODEV and f(h, 0, qp, qp, 4, -1, qp, None) == NODEV
    assert f(h, -1, qp, qp, 0, 8, qp, None) == INV and err()
    assert f(h, 3, qp, qp, -1, 8, qp, None) == INV and b"add" in err()
    for args in ((None, qp, qp), (qp, None, qp), (qp, qp, None)):
        assert f(h, 3, args[0], args[1], 0, 8, args[2], None) == INV and b"null" in err()
    assert f(None, 3, qp, qp, 0, 8, qp, None) == INV


def _move(p, slot, out, ID=Q, r0=0, count=1, n=None, reverse=0, slot_arr="default", out_arr="default"):
    s = _rows(*slot) if slot_arr == "default" else slot_arr
    o = _rows(*out) if out_arr == "default" else out_arr
    return p._lib.towr_gpu_alsolve_move_rows_batch_device(p._h, C.c_void_p(ID) if ID else None, r0, count,
                                                          len(slot) if n is None else n, s, o, reverse, None)


def test_move_rows_refusals(p):
    lib, h = p._lib, p._h
    err = lambda: lib.towr_gpu_last_error(h)
    slot = [(Q, 64, 64), (Q + STEP, 16, 8), (Q + 2 * STEP + 4, 8, 8), (Q + 3 * STEP, 8, 4)]
    out = [(Q + 8 * STEP, 128, 64), (Q + 9 * STEP, 8, 8), (Q + 10 * STEP, 12, 8), (Q + 11 * STEP + 4, 4, 4)]
    assert _move(p, slot, out) == NODEV and _move(p, slot, out, reverse=1, r0=7, count=0) == NODEV and _move(p, [], []) == NODEV
    many = lambda k, base: [(base + i * STEP, 8, 8) for i in range(k)]
    assert _move(p, many(16, Q), many(16, Q + 100 * STEP)) == NODEV
    assert _move(p, many(17, Q), many(17, Q + 100 * STEP)) == INV and b"n_arrays" in err()
    assert _move(p, slot, out, n=-1) == INV and b"n_arrays" in err()
    assert _move(p, slot, out, ID=None) == INV and b"ID" in err()
    assert _move(p, slot, out, r0=-1) == INV and _move(p, slot, out, count=-1) == INV and b"negative" in err()
    for r in (-1, 2):
        assert _move(p, slot, out, reverse=r) == INV and b"reverse" in err()
    assert _move(p, slot, out, slot_arr=None) == INV and _move(p, slot, out, out_arr=None) == INV and b"null" in err()
    assert _move(p, [(Q, 64, 64)], [(Q + STEP, 64, 32)]) == INV and b"differ" in err()
    for what, d in (("base", (0, 8, 8)), ("base", (Q + 2, 8, 8)), ("base", (Q + 1, 8, 8)), ("row_bytes", (Q, 8, 0)),
                    ("row_bytes", (Q, 8, -8)), ("row_bytes", (Q, 8, 6)), ("ld_bytes", (Q, 0, 8)), ("ld_bytes", (Q, -8, 8)),
                    ("ld_bytes", (Q, 10, 8)), ("smaller", (Q, 8, 16)), ("smaller", (Q, 60, 64))):
        good = (Q + 5 * STEP, max(d[2], 8), d[2])
        for s, o in (([slot[1], d], [out[1], good]), ([slot[1], good], [out[1], d])):
            assert _move(p, s, o) == INV and what.encode() in err(), (what, d)


def test_queue_valid_arguments_reach_the_device_check(p):
    for method in METHODS:
        assert _solve(p, method=method) == NODEV, method
        assert _solve(p, method=method, q=_queue(p, per_problem=True), B=3, wrows=2) == NODEV, method
        assert _solve(p, method=method, compact=0, max_iters=1, check_every=1, B=1) == NODEV, method
    assert _solve(p, stop=alsolve_stop_params(acc_eta=1e-3, acc_omega=1e-2, acc_iters=3)) == NODEV
    assert _solve(p, max_iters=12, check_every=4) == NODEV
    # an empty queue names no arrays and needs no slot
    empty = capi.SolveQueue(N=0)
    assert _solve(p, q=empty) == NODEV and _solve(p, q=empty, B=0) == NODEV
    # one shared row, and work rows that are not needed may be anything
    g, x = Q + 90 * STEP, Q + 91 * STEP
    assert _solve(p, q=_queue(p, GL=g, GU=g, ldgb=0, XL=x, XU=x, ldxb=0)) == NODEV
    assert _solve(p, method=capi.SOLVE_LBFGS, d=capi.SolveDir()) == NODEV


def test_queue_refusals(p):
    lib, h, n, m = p._lib, p._h, p.n, p.m
    err = lambda: lib.towr_gpu_last_error(h)
    # the driver's own
    for kw in (dict(opts=None), dict(d=None), dict(q=None), dict(LOG=None), dict(report=None)):
        assert _solve(p, **kw) == INV and b"null opts, dir, queue, LOG or report" in err(), kw
    for method in (-1, 5):
        assert _solve(p, method=method) == INV and b"method" in err()
    for k in (0, -1):
        assert _solve(p, check_every=k) == INV and b"check_every" in err()
    for M, K in ((0, 2), (-2, 2), (3, 2), (5, 4), (2, 4)):
        assert _solve(p, max_iters=M, check_every=K) == INV and b"positive multiple" in err(), (M, K)
    for c in (-1, 2):
        assert _solve(p, compact=c) == INV and b"compact" in err()
    assert _solve(p, q=_queue(p, N=-1)) == INV and b"N is negative" in err()
    for B in (0, -1):
        assert _solve(p, B=B) == INV and err(), B
    assert _solve(p, B=0) == INV and b"slots" in err()
    for k in QUEUE_PTRS:
        assert _solve(p, q=_queue(p, **{k: None})) == INV and b"queue: null" in err(), k
    for k, v in (("ldx0", n - 1), ("ldxo", n - 1), ("ldlo", m - 1)):
        assert _solve(p, q=_queue(p, **{k: v})) == INV and b"below" in err(), k
    assert _solve(p, q=_queue(p, LAM0=Q + 70 * STEP, ldl0=m - 1)) == INV and b"ldl0" in err()
    assert _solve(p, q=_queue(p, LAM0=Q + 70 * STEP, ldl0=m)) == NODEV
    b0 = Q + 90 * STEP
    for what, kw in (("only one", dict(GL=b0)), ("only one", dict(GU=b0)), ("only one", dict(XL=b0)), ("only one", dict(XU=b0)),
                     ("ldb", dict(GL=b0, GU=b0 + STEP, ldgb=m - 1)), ("ldb", dict(XL=b0, XU=b0 + STEP, ldxb=n - 1)),
                     ("ldb", dict(GL=b0, GU=b0 + STEP, ldgb=-1)), ("ldb", dict(XL=b0, XU=b0 + STEP, ldxb=-1)),
                     ("work rows", dict(GL=b0, GU=b0 + STEP, ldgb=m)), ("work rows", dict(XL=b0, XU=b0 + STEP, ldxb=n))):
        assert _solve(p, q=_queue(p, **kw)) == INV and what.encode() in err(), (what, kw)
    for k, v in (("GLW", None), ("GUW", None), ("XLW", None), ("XUW", None), ("ldgw", m - 1), ("ldxw", n - 1)):
        assert _solve(p, q=_queue(p, per_problem=True, **{k: v})) == INV and b"work rows" in err(), k
    # what the method's iterate entry refuses
    for method in METHODS:
        assert _solve(p, method=method, par=None) == INV and b"params" in err(), method
        assert _solve(p, method=method, st=None) == INV and b"state" in err(), method
        for field, v in BAD_PARAMS[::7]:
            assert _solve(p, method=method, par=alsolve_params(**{field: v})) == INV and b"params" in err(), (method, field, v)
        for k in PTRS:
            assert _solve(p, method=method, st=_apart(p, **{k: None})) == INV and b"state" in err(), (method, k)
        for k, v in (("ldx", n - 1), ("ldh", n - 1), ("ldsc", 7), ("ldus", 5), ("ldls", 7), ("ldl", m - 1),
                     ("ldrs", 3 + p.desc.n_constraints), ("ldss", 4 + p.desc.n_varsets), ("ldds", 4)):
            assert _solve(p, method=method, st=_apart(p, **{k: v})) == INV and b"state" in err(), (method, k)
        assert _solve(p, method=method, stop=alsolve_stop_params(acc_eta=NAN)) == INV and err(), method
        assert _solve(p, method=method, stop=alsolve_stop_params(infeas_keep=0.0)) == INV and err(), method
    for method in METHODS[1:]:
        assert _solve(p, method=method, gn=None) == INV and b"gn" in err(), method
        assert _solve(p, method=method, DC=None) == INV and _solve(p, method=method, GSUM=None) == INV, method
        assert _solve(p, method=method, gn=C.pointer(gn_params(ncg=3, mu=NAN))) == INV and b"mu" in err(), method
        assert _solve(p, method=method, ldgs=5) == INV, method
    for method in (capi.SOLVE_GN, capi.SOLVE_GN_PC):
        assert _solve(p, method=method, gn=C.pointer(gn_params(ncg=0))) == INV and b"ncg" in err(), method
    assert _solve(p, method=capi.SOLVE_GN_PC, precond=2) == INV and b"precond" in err()
    assert _solve(p, method=capi.SOLVE_GN_PC, PC=None) == INV and b"PC" in err()
    assert _solve(p, method=capi.SOLVE_GN_PC, PC=DC) == INV and b"overlaps" in err()
    for method in (capi.SOLVE_GN_DIRECT, capi.SOLVE_GN_TILED):
        assert _solve(p, method=method, W=None) == INV and b"W" in err(), method
        assert _solve(p, method=method, wrows=0) == INV and b"wrows" in err(), method
        assert _solve(p, method=method, ldw=7) == INV and b"ldw" in err(), method
        assert _solve(p, method=method, W=DC) == INV and b"overlaps" in err(), method
    # an array that fails the swap's or the move's checks: one buffer behind two fields, misaligned rows
    assert _solve(p, st=_apart(p, GRC=Q + STEP)) == INV and b"swap" in err() and b"overlap" in err()
    assert _solve(p, st=_apart(p, ISTATE=Q + 2)) == INV and b"swap" in err()
    assert _solve(p, q=_queue(p, AGE=Q + 61 * STEP)) == INV and b"overlap" in err()                         # (ID's address)
    assert _solve(p, q=_queue(p, ID=Q + 61 * STEP + 2)) == INV and b"swap" in err()
    assert _solve(p, q=_queue(p, per_problem=True, GUW=Q + 85 * STEP)) == INV and b"overlap" in err()      # (GLW's address)
    for k in ("X0", "X_OUT", "RHO_OUT", "ISTATE_OUT", "ITERS_OUT"):
        assert _solve(p, q=_queue(p, **{k: Q + 99 * STEP + 2})) == INV and b"move" in err(), k
