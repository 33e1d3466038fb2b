"""The stop rule's entry points at the C-ABI boundary (no GPU, a layout-only handle, fake pointers: nothing runs): the
symbols, the struct and the two phase words exist, every refusal include/towr_gpu.h lists for
towr_gpu_alsolve_stop_batch_device and towr_gpu_alsolve_solve_ex_batch_device is TOWR_ERR_INVALID with a message, valid
arguments are TOWR_ERR_NO_DEVICE, and solve_ex with stop == NULL answers every argument as the plain solve entry does."""
import ctypes as C

import pytest

from tests import stop_ref as S
from tests.configs import config_descs
from tests.test_alsolve_capi import BAD_PARAMS, _state
from tests.test_gn_capi import INV, NAN, NODEV, Q
from tests.test_solve_capi import METHODS, _apart, _solve
from tests import test_solve_capi as TS
from towr2025_amd import TowrGpuProblem, _capi as capi, alsolve_params, alsolve_stop_params, gn_params

INF = float("inf")
# every field the header refuses
BAD_STOP = [("acc_eta", -1e-9), ("acc_eta", NAN), ("acc_omega", -1.0), ("acc_omega", NAN), ("acc_iters", -1),
            ("infeas_keep", 0.0), ("infeas_keep", -0.5), ("infeas_keep", 1.0000001), ("infeas_keep", NAN), ("infeas_keep", INF),
            ("infeas_rho", -1.0), ("infeas_rho", NAN)]
GOOD_STOP = [dict(), S.EXAMPLE, dict(acc_eta=0.0, acc_omega=0.0, acc_iters=1), dict(acc_eta=INF, acc_omega=INF, acc_iters=2 ** 31 - 1),
             dict(infeas_keep=1.0, infeas_rho=0.0), dict(infeas_keep=5e-324, infeas_rho=INF)]


@pytest.fixture(scope="module")
def p():
    return TowrGpuProblem(config_descs()["monoped_procedural"], device=-1)


def _stop(p, sp="default", par="default", st="default", B=1):
    sp = alsolve_stop_params(**S.EXAMPLE) if sp == "default" else sp
    par = alsolve_params() if par == "default" else par
    st = _state(p) if st == "default" else st
    return p._lib.towr_gpu_alsolve_stop_batch_device(p._h, B, par, sp, st, None)


def _solve_ex(p, sp="default", method=capi.SOLVE_GN_TILED, max_iters=3, check_every=2, compact=1, par="default", st="default",
              d="default", B=1, bounds=(None, None, 0, None, None, 0), LOG=Q, report="default", opts="default", **dkw):
    """tests/test_solve_capi._solve through the new entry."""
    sp = alsolve_stop_params(**S.EXAMPLE) if sp == "default" else sp
    par = alsolve_params() if par == "default" else par
    st = _apart(p) if st == "default" else st
    if opts == "default":
        opts = capi.SolveOpts(method=method, max_iters=max_iters, check_every=check_every, compact=compact)
    if d == "default":
        d = capi.SolveDir()
        d.gn = C.pointer(gn_params(ncg=3, mu=1e-6, tol=1e-3))
        d.precond, d.wrows, d.DC, d.GSUM, d.ldgs, d.PC, d.W = capi.GN_PC_JACOBI, 1, TS.DC, TS.GSUM, 8, TS.PC, TS.QW
        d.ldw = p.gn_tile_info()["ldw_min"]
        for k, v in dkw.items():
            setattr(d, k, v)
    rep = capi.SolveReport() if report == "default" else report
    return p._lib.towr_gpu_alsolve_solve_ex_batch_device(
        p._h, B, None if opts is None else C.byref(opts), par, sp, st, None if d is None else C.byref(d), *bounds,
        C.c_void_p(LOG) if LOG else None, None if rep is None else C.byref(rep), None)


def test_symbols_struct_and_phases():
    lib = capi.load_library()
    for name in ("towr_gpu_alsolve_stop_batch_device", "towr_gpu_alsolve_solve_ex_batch_device"):
        assert hasattr(lib, name) and name in capi.SYMBOLS
    assert capi.ABI_VERSION == 4 and lib.towr_gpu_abi_version() == 4
    assert C.sizeof(capi.AlSolveStop) == 40 and C.sizeof(capi.SolveReport) == 48 and C.sizeof(capi.AlSolveStateC) == 29 * 8
    assert [f[0] for f in capi.AlSolveStop._fields_] == ["acc_eta", "acc_omega", "acc_iters", "reserved", "infeas_keep", "infeas_rho"]
    header = open(capi.__file__.replace("towr2025_amd/_capi.py", "include/towr_gpu.h")).read()
    assert "#define TOWR_AL_ACCEPTABLE 5" in header and "#define TOWR_AL_INFEASIBLE 6" in header
    assert (capi.AL_ACCEPTABLE, capi.AL_INFEASIBLE) == (5, 6) == (S.ACCEPTABLE, S.INFEASIBLE)
    assert "#define TOWR_GPU_ABI_VERSION 4" in header
    for m in ("alsolve_stop", "alsolve_solve"):
        assert callable(getattr(TowrGpuProblem, m))
    off = alsolve_stop_params()
    assert off.acc_iters == 0 and off.infeas_rho == INF and off.infeas_keep == 1.0


def test_stop_valid_arguments_reach_the_device_check(p):
    for kw in GOOD_STOP:
        assert _stop(p, sp=alsolve_stop_params(**kw)) == NODEV, kw
    assert _stop(p, B=0) == NODEV and _stop(p, B=4097) == NODEV
    # only ISTATE, SCAL, HMETA, ALPHA and RHO are needed
    only = _state(p, **{k: None for k in ("X", "GR", "XC", "GRC", "D", "LAM", "LAMP", "HS", "HY", "FC", "RSUM", "SSUM", "DSUM",
                                           "USUM", "LSUM")}, ldx=0, ldl=0, ldh=0, ldrs=0, ldss=0, ldds=0, ldus=0, ldls=0)
    assert _stop(p, st=only) == NODEV


def test_stop_refusals(p):
    lib, h = p._lib, p._h
    err = lambda: lib.towr_gpu_last_error(h)
    for field, v in BAD_STOP:
        assert _stop(p, sp=alsolve_stop_params(**{**S.EXAMPLE, field: v})) == INV and b"stop" in err() and field.encode() in err(), (field, v)
    assert _stop(p, sp=None) == INV and b"null stop" in err()
    assert _stop(p, par=None) == INV and b"params" in err()
    assert _stop(p, st=None) == INV and b"state" in err()
    assert _stop(p, B=-1) == INV and err()
    assert lib.towr_gpu_alsolve_stop_batch_device(None, 1, alsolve_params(), alsolve_stop_params(), _state(p), None) == INV
    for field, v in BAD_PARAMS:
        assert _stop(p, par=alsolve_params(**{field: v})) == INV and b"params" in err(), (field, v)
    for k in ("ISTATE", "SCAL", "HMETA", "ALPHA", "RHO"):
        assert _stop(p, st=_state(p, **{k: None})) == INV and b"state" in err(), k
    assert _stop(p, st=_state(p, ldsc=7)) == INV and b"ldsc" in err()


def test_solve_ex_refusals_and_valid_arguments(p):
    lib, h = p._lib, p._h
    err = lambda: lib.towr_gpu_last_error(h)
    for method in METHODS:
        for kw in GOOD_STOP:
            assert _solve_ex(p, sp=alsolve_stop_params(**kw), method=method) == NODEV, (method, kw)
        for field, v in BAD_STOP:
            sp = alsolve_stop_params(**{**S.EXAMPLE, field: v})
            assert _solve_ex(p, sp=sp, method=method) == INV and b"stop" in err() and field.encode() in err(), (method, field, v)
            assert _solve_ex(p, sp=sp, method=method, max_iters=0, B=0) == INV, (method, field, v)     # before anything is looked at
    # the plain entry's own refusals, with a stop
    assert _solve_ex(p, opts=None) == INV and _solve_ex(p, d=None) == INV and _solve_ex(p, LOG=None) == INV and _solve_ex(p, report=None) == INV
    assert _solve_ex(p, method=5) == INV and b"method" in err()
    assert _solve_ex(p, check_every=0) == INV and b"check_every" in err()
    assert _solve_ex(p, st=_apart(p, ldsc=7)) == INV and b"state" in err()
    assert _solve_ex(p, st=_apart(p, GRC=Q + TS.STEP)) == INV and b"overlap" in err()


def test_solve_ex_without_stop_answers_as_the_plain_entry(p):
    """stop == NULL: the same code and the same message as towr_gpu_alsolve_solve_batch_device for valid arguments and
    for a refusal of every layer (the driver's own, the iterate entry's, the swap's)."""
    lib, h = p._lib, p._h
    cases = [dict(), dict(B=0, max_iters=0), dict(method=capi.SOLVE_LBFGS, d=capi.SolveDir()), dict(method=capi.SOLVE_GN, ldgs=6),
             dict(opts=None), dict(report=None), dict(method=-1), dict(max_iters=-1), dict(check_every=0), dict(compact=2),
             dict(B=-1), dict(par=None), dict(st=None), dict(par=alsolve_params(mem=0)), dict(st=_apart(p, ldx=p.n - 1)),
             dict(gn=None), dict(method=capi.SOLVE_GN_PC, precond=2), dict(wrows=0), dict(ldw=7), dict(st=_apart(p, ISTATE=Q + 2)),
             dict(DC=Q + 5 * TS.STEP)]
    for kw in cases:
        a = _solve(p, **kw)
        ma = lib.towr_gpu_last_error(h)
        b = _solve_ex(p, sp=None, **kw)
        mb = lib.towr_gpu_last_error(h)
        assert a == b and ma == mb and a in (INV, NODEV), (kw, a, b, ma, mb)
