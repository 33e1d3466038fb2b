"""The probe stage's entry points at the C-ABI boundary (no GPU, a layout-only handle, fake pointers: nothing runs): the
symbols and the struct exist, every refusal include/towr_gpu.h lists for towr_gpu_alsolve_probe_batch_device and
towr_gpu_alsolve_solve_probe_batch_device is TOWR_ERR_INVALID with a message, valid arguments are TOWR_ERR_NO_DEVICE —
the checks come before the device is bound — and probe == NULL is accepted as towr_gpu_alsolve_solve_ex_batch_device is."""
import ctypes as C

import pytest

from tests.configs import config_descs
from tests.test_alsolve_capi import BAD_PARAMS, PTRS
from tests.test_gn_capi import INV, NODEV, Q
from tests.test_solve_capi import BOUNDS, DC, GSUM, METHODS, PC, QW, STEP, _apart
from towr2025_amd import TowrGpuProblem, _capi as capi, alsolve_params, gn_params

PSUM = Q + 50 * STEP


@pytest.fixture(scope="module")
def p():
    return TowrGpuProblem(config_descs()["monoped_procedural"], device=-1)


def _probe(p, T=4, par="default", st="default", probe="default", B=1, bounds=(None, None, 0, None, None, 0), psum=PSUM, ldps=8):
    par = alsolve_params() if par == "default" else par
    st = _apart(p) if st == "default" else st
    pr = capi.AlSolveProbe(trials=T) if probe == "default" else probe
    return p._lib.towr_gpu_alsolve_probe_batch_device(p._h, B, par, None if pr is None else C.byref(pr), st, *bounds,
                                                      C.c_void_p(psum) if psum else None, ldps, None)


def _solve(p, T=4, method=capi.SOLVE_GN_TILED, max_iters=3, check_every=2, compact=1, par="default", st="default", probe="default",
           B=1, bounds=(None, None, 0, None, None, 0), psum=PSUM, ldps=8, stop=None, **dkw):
    par = alsolve_params() if par == "default" else par
    st = _apart(p) if st == "default" else st
    pr = capi.AlSolveProbe(trials=T) if probe == "default" else probe
    opts = capi.SolveOpts(method=method, max_iters=max_iters, check_every=check_every, compact=compact)
    d = capi.SolveDir()
    d.gn = C.pointer(gn_params(ncg=3, mu=1e-6, tol=1e-3))
    d.precond, d.wrows, d.DC, d.GSUM, d.ldgs, d.PC, d.W = capi.GN_PC_JACOBI, 1, DC, GSUM, 8, PC, QW
    d.ldw = p.gn_tile_info()["ldw_min"]
    for k, v in dkw.items():
        setattr(d, k, v)
    rep = capi.SolveReport()
    return p._lib.towr_gpu_alsolve_solve_probe_batch_device(
        p._h, B, C.byref(opts), par, None if stop is None else C.byref(stop), None if pr is None else C.byref(pr), st, C.byref(d),
        *bounds, C.c_void_p(psum) if psum else None, ldps, C.c_void_p(Q), C.byref(rep), None)


def test_symbols_and_struct():
    lib = capi.load_library()
    for name in ("towr_gpu_alsolve_probe_batch_device", "towr_gpu_alsolve_solve_probe_batch_device"):
        assert hasattr(lib, name) and name in capi.SYMBOLS
    assert C.sizeof(capi.AlSolveProbe) == 8 and capi.PROBE_MAX == 8
    assert capi.ABI_VERSION == 4 and lib.towr_gpu_abi_version() == 4
    assert C.sizeof(capi.AlSolveStateC) == 29 * 8 and C.sizeof(capi.SolveOpts) == 16          # the existing structs are unchanged
    header = open(capi.__file__.replace("towr2025_amd/_capi.py", "include/towr_gpu.h")).read()
    assert "#define TOWR_PROBE_MAX 8" in header and "typedef struct { int32_t trials, reserved; } towr_alsolve_probe_t;" in header
    assert "PROBED ITERATIONS" in header                                                       # the stop rule's run length
    for m in ("alsolve_probe", "alsolve_solve"):
        assert callable(getattr(TowrGpuProblem, m))


def test_probe_valid_arguments_reach_the_device_check(p):
    q = [C.c_void_p(b) for b in BOUNDS]
    for T in (1, 4, 8):
        assert _probe(p, T=T) == NODEV, T
    assert _probe(p, B=0) == NODEV and _probe(p, ldps=11, B=3) == NODEV
    assert _probe(p, bounds=(q[0], q[1], p.m, q[2], q[3], p.n), B=2) == NODEV
    assert _probe(p, bounds=(q[0], q[1], 0, q[2], q[3], 0), B=2) == NODEV


def test_probe_refusals(p):
    lib, h, n, m = p._lib, p._h, p.n, p.m
    err = lambda: lib.towr_gpu_last_error(h)
    for T in (0, -1, 9, 2 ** 31 - 1):
        assert _probe(p, T=T) == INV and b"trials" in err(), T
    assert _probe(p, probe=None) == INV and b"null probe" in err()
    assert _probe(p, psum=None) == INV and b"PSUM" in err()
    for ld in (7, 0, -8):
        assert _probe(p, ldps=ld) == INV and b"ldps" in err(), ld
    # what the iterate entry refuses
    assert _probe(p, B=-1) == INV
    assert _probe(p, par=None) == INV and b"params" in err()
    assert _probe(p, st=None) == INV and b"state" in err()
    for field, v in BAD_PARAMS:
        assert _probe(p, par=alsolve_params(**{field: v})) == INV and b"params" in err(), (field, v)
    for k in PTRS:
        assert _probe(p, st=_apart(p, **{k: None})) == INV and b"state" in err(), k
    for k, v in (("ldx", n - 1), ("ldh", n - 1), ("ldsc", 7), ("ldus", 5), ("ldls", 7), ("ldl", m - 1),
                 ("ldrs", 3 + p.desc.n_constraints), ("ldss", 4 + p.desc.n_varsets), ("ldds", 4)):
        assert _probe(p, st=_apart(p, **{k: v})) == INV and b"state" in err(), k
    q = C.c_void_p(BOUNDS[0])
    for what, args in (("only GL", (q, None, 0, None, None, 0)), ("only GU", (None, q, 0, None, None, 0)),
                       ("0 < ldgb < m", (q, q, m - 1, None, None, 0)), ("only XL", (None, None, 0, q, None, 0)),
                       ("only XU", (None, None, 0, None, q, 0)), ("0 < ldxb < n", (None, None, 0, q, q, n - 1))):
        assert _probe(p, bounds=args) == INV and err(), what
    assert lib.towr_gpu_alsolve_probe_batch_device(None, 1, alsolve_params(), C.byref(capi.AlSolveProbe(trials=2)), _apart(p),
                                                   None, None, 0, None, None, 0, C.c_void_p(PSUM), 8, None) == INV


def test_solve_with_and_without_probe(p):
    lib, h = p._lib, p._h
    err = lambda: lib.towr_gpu_last_error(h)
    from towr2025_amd import alsolve_stop_params
    for method in METHODS:
        assert _solve(p, method=method) == NODEV, method
        assert _solve(p, method=method, compact=0, T=1) == NODEV and _solve(p, method=method, T=8, stop=alsolve_stop_params()) == NODEV
        # probe == NULL: the _ex entry, which reads neither PSUM nor ldps
        assert _solve(p, method=method, probe=None, psum=None, ldps=0) == NODEV, method
        for T in (0, 9):
            assert _solve(p, method=method, T=T) == INV and b"trials" in err(), (method, T)
        assert _solve(p, method=method, psum=None) == INV and b"PSUM" in err(), method
        assert _solve(p, method=method, ldps=7) == INV and b"ldps" in err(), method
        # what the _ex entry refuses, with and without a probe
        for pr in ("default", None):
            assert _solve(p, method=method, probe=pr, B=-1) == INV, method
            assert _solve(p, method=method, probe=pr, check_every=0) == INV and b"check_every" in err(), method
            assert _solve(p, method=method, probe=pr, st=_apart(p, ldsc=7)) == INV and b"state" in err(), method
            assert _solve(p, method=method, probe=pr, stop=alsolve_stop_params(acc_iters=-1)) == INV and b"stop" in err(), method
    assert _solve(p, method=5) == INV and b"method" in err()
