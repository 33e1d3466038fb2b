"""The resident-loop entry points at the C-ABI boundary (no GPU, a layout-only handle, fake pointers: nothing runs): the
symbols exist, every refusal include/towr_gpu.h lists is TOWR_ERR_INVALID with a message, and valid arguments are
TOWR_ERR_NO_DEVICE — the checks come before the device is bound."""
import ctypes as C

import pytest

from tests.configs import config_descs
from towr2025_amd import AlSolveState, TowrGpuProblem, _capi as capi, alsolve_params

INV, NODEV = capi.TOWR_ERR_INVALID, capi.TOWR_ERR_NO_DEVICE
Q = 4096
NAN = float("nan")
PTRS = ("X", "GR", "XC", "GRC", "D", "LAM", "LAMP", "HS", "HY", "HMETA", "ALPHA", "RHO", "FC", "SCAL", "ISTATE", "RSUM", "SSUM",
        "DSUM", "USUM", "LSUM")
USED = {"ls": ("X", "GR", "XC", "GRC", "HS", "HY", "HMETA", "ALPHA", "FC", "SCAL", "ISTATE", "RSUM", "USUM", "LSUM"),
        "outer": ("LAM", "LAMP", "HMETA", "ALPHA", "RHO", "SCAL", "ISTATE"),
        "all": PTRS}


@pytest.fixture(scope="module")
def p():
    return TowrGpuProblem(config_descs()["monoped_procedural"], device=-1)


def _state(p, **kw):
    c = capi.AlSolveStateC()
    for k in PTRS:
        setattr(c, k, Q)
    c.ldx, c.ldl, c.ldh, c.ldsc = p.n, p.m, p.n, 8
    c.ldrs, c.ldss, c.ldds, c.ldus, c.ldls = 4 + p.desc.n_constraints, 5 + p.desc.n_varsets, 5, 6, 8
    for k, v in kw.items():
        setattr(c, k, v)
    return c


def _calls(p):
    lib, h = p._lib, p._h
    return {"ls": lambda par, st, B=1: lib.towr_gpu_linesearch_batch_device(h, B, par, st, None, None, 0, None),
            "outer": lambda par, st, B=1: lib.towr_gpu_auglag_outer_batch_device(h, B, par, st, None),
            "init": lambda par, st, B=1: lib.towr_gpu_alsolve_init_batch_device(h, B, par, st, None, None, 0, None),
            "iter": lambda par, st, B=1: lib.towr_gpu_alsolve_iterate_batch_device(h, B, 1, par, st, None, None, 0, None, None, 0,
                                                                                  None)}


def test_symbols_structs_and_methods():
    lib = capi.load_library()
    for name in ("towr_gpu_linesearch_batch_device", "towr_gpu_auglag_outer_batch_device", "towr_gpu_alsolve_init_batch_device",
                 "towr_gpu_alsolve_iterate_batch_device"):
        assert hasattr(lib, name) and name in capi.SYMBOLS
    assert capi.ABI_VERSION == 4 and lib.towr_gpu_abi_version() == 4
    assert C.sizeof(capi.AlSolveParams) == 16 + 14 * 8 and C.sizeof(capi.AlSolveStateC) == 29 * 8
    assert (capi.AL_RESTART, capi.AL_SEARCH, capi.AL_CONVERGED, capi.AL_STALLED, capi.AL_MAXED) == (0, 1, 2, 3, 4)
    for m in ("linesearch_batch_device", "auglag_outer_batch_device", "alsolve_init", "alsolve_iterate"):
        assert callable(getattr(TowrGpuProblem, m))
    assert callable(AlSolveState.allocate)


def test_valid_arguments_reach_the_device_check(p):
    par, st = alsolve_params(), _state(p)
    for name, call in _calls(p).items():
        assert call(par, st) == NODEV, name
        assert call(par, st, 0) == NODEV, name   # B = 0 is TOWR_OK only where there is a device
        assert call(par, st, -1) == INV, name
    # the fields an entry does not use may be NULL
    calls = _calls(p)
    assert calls["ls"](par, _state(p, D=None, LAM=None, LAMP=None, RHO=None, SSUM=None, DSUM=None, ldl=0, ldss=0, ldds=0, ldrs=4)) == NODEV
    only = {k: None for k in PTRS if k not in USED["outer"]}
    assert calls["outer"](par, _state(p, ldx=0, ldh=0, ldrs=0, ldss=0, ldds=0, ldus=0, ldls=0, **only)) == NODEV
    lib, h, n, m = p._lib, p._h, p.n, p.m
    qp = C.c_void_p(Q)
    assert lib.towr_gpu_alsolve_iterate_batch_device(h, 1, 0, par, st, qp, qp, m, qp, qp, n, None) == NODEV
    assert lib.towr_gpu_alsolve_iterate_batch_device(h, 1, 3, par, st, qp, qp, 0, qp, qp, 0, None) == NODEV
    assert lib.towr_gpu_linesearch_batch_device(h, 1, par, st, qp, qp, n, None) == NODEV


BAD_PARAMS = [("mem", 0), ("mem", capi.LBFGS_MAX_MEM + 1), ("max_inner", 0), ("max_outer", 0), ("c1", 0.0), ("c1", 1.0), ("c1", NAN),
              ("shrink", 0.0), ("shrink", 1.0), ("shrink", NAN), ("alpha0", 0.0), ("alpha0", NAN), ("alpha_min", 0.0),
              ("alpha_min", 2.0), ("alpha_min", NAN), ("curv_eps", -1e-300), ("curv_eps", NAN), ("rho0", 0.0), ("rho0", NAN),
              ("rho_grow", 0.5), ("rho_grow", NAN), ("rho_max", 1.0), ("rho_max", NAN), ("eta0", 0.0), ("eta0", 1.5), ("eta0", NAN),
              ("eta_shrink", 0.0), ("eta_shrink", 1.5), ("eta_shrink", NAN), ("eta_star", 0.0), ("eta_star", NAN), ("omega0", 0.0),
              ("omega0", 1.5), ("omega0", NAN), ("omega_shrink", 0.0), ("omega_shrink", 1.5), ("omega_shrink", NAN),
              ("omega_star", 0.0), ("omega_star", NAN)]


def test_every_params_refusal(p):
    lib, h, st = p._lib, p._h, _state(p)
    for name, call in _calls(p).items():
        assert call(None, st) == INV and b"params" in lib.towr_gpu_last_error(h), name
        for field, v in BAD_PARAMS:
            assert call(alsolve_params(**{field: v}), st) == INV, (name, field, v)
            assert b"params" in lib.towr_gpu_last_error(h), (name, field, v)
    # the closed ends of the ranges are valid
    ok = alsolve_params(mem=capi.LBFGS_MAX_MEM, max_inner=1, max_outer=1, alpha0=1e-3, alpha_min=1e-3, curv_eps=0.0, rho_grow=1.0,
                        rho0=5.0, rho_max=5.0, eta0=1.0, eta_shrink=1.0, omega0=1.0, omega_shrink=1.0)
    assert _calls(p)["iter"](ok, st) == NODEV


def test_every_state_refusal(p):
    lib, h, n, m = p._lib, p._h, p.n, p.m
    par, calls = alsolve_params(), _calls(p)
    for name, call in calls.items():
        assert call(par, None) == INV and b"state" in lib.towr_gpu_last_error(h), name
    lds = {"ls": [("ldx", n - 1), ("ldh", n - 1), ("ldsc", 7), ("ldrs", 3), ("ldus", 5), ("ldls", 7)],
           "outer": [("ldl", m - 1), ("ldsc", 7)]}
    lds["all"] = lds["ls"] + lds["outer"] + [("ldrs", 3 + p.desc.n_constraints), ("ldss", 4 + p.desc.n_varsets), ("ldds", 4)]
    for name, used in (("ls", "ls"), ("outer", "outer"), ("init", "all"), ("iter", "all")):
        for k in USED[used]:
            assert calls[name](par, _state(p, **{k: None})) == INV, (name, k)
            assert b"state" in lib.towr_gpu_last_error(h), (name, k)
        for k, v in lds[used]:
            assert calls[name](par, _state(p, **{k: v})) == INV, (name, k)
            assert b"state" in lib.towr_gpu_last_error(h), (name, k)


def test_bounds_and_iters_refusals(p):
    lib, h, n, m = p._lib, p._h, p.n, p.m
    par, st, qp = alsolve_params(), _state(p), C.c_void_p(Q)
    it = lib.towr_gpu_alsolve_iterate_batch_device
    for what, args in (("only GL", (qp, None, 0, None, None, 0)), ("only GU", (None, qp, 0, None, None, 0)),
                       ("0 < ldgb < m", (qp, qp, m - 1, None, None, 0)), ("only XL", (None, None, 0, qp, None, 0)),
                       ("only XU", (None, None, 0, None, qp, 0)), ("0 < ldxb < n", (None, None, 0, qp, qp, n - 1))):
        assert it(h, 1, 1, par, st, *args, None) == INV and lib.towr_gpu_last_error(h), what
    assert it(h, 1, -1, par, st, None, None, 0, None, None, 0, None) == INV and b"iters" in lib.towr_gpu_last_error(h)
    for fn in (lib.towr_gpu_linesearch_batch_device, lib.towr_gpu_alsolve_init_batch_device):
        assert fn(h, 1, par, st, qp, None, 0, None) == INV
        assert fn(h, 1, par, st, None, qp, 0, None) == INV
        assert fn(h, 1, par, st, qp, qp, n - 1, None) == INV and lib.towr_gpu_last_error(h)


def test_params_helper():
    from towr2025_amd import TowrGpuError
    with pytest.raises(TowrGpuError, match="unknown field"):
        alsolve_params(rho=1.0)
    assert alsolve_params(mem=7).mem == 7
