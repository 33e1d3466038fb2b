"""The tiled direct Gauss-Newton entry points at the C-ABI boundary (no GPU, a layout-only handle, fake pointers: nothing
runs), as tests/test_gn_direct_capi.py does for the envelope ones: the symbols exist, towr_gpu_gn_tile_info answers on a
layout-only handle, every refusal include/towr_gpu.h lists for towr_gpu_gn_direction_tiled_batch_device and
towr_gpu_alsolve_gn_tiled_iterate_batch_device is TOWR_ERR_INVALID with a message (ldw_min being the tile one), and valid
arguments are TOWR_ERR_NO_DEVICE — the checks come before the device is bound."""
import ctypes as C

import numpy as np
import pytest

from tests.configs import config_descs
from tests.test_alsolve_capi import BAD_PARAMS, PTRS, _state
from tests.test_gn_capi import INV, NAN, NODEV, Q
from towr2025_amd import TowrGpuProblem, _capi as capi, alsolve_params, gn_params

QW = 1 << 30           # W's fake address: far from Q, which stands for every other operand (a W row must overlap none)
QV = 1 << 28           # an operand moved away from Q, with room below it for a W row
BAD_MU = [-1e-300, -1.0, NAN]


@pytest.fixture(scope="module")
def p():
    return TowrGpuProblem(config_descs()["monoped_procedural"], device=-1)


@pytest.fixture(scope="module")
def env(p):
    return p.gn_tile_info()["ldw_min"]


def _dir_args(p, **kw):
    """Valid arguments of towr_gpu_gn_direction_tiled_batch_device by name (fake pointers), with `kw` replacing some."""
    qp = C.c_void_p(Q)
    ldw = p.gn_tile_info()["ldw_min"]
    a = dict(B=1, gn=gn_params(ncg=0, mu=1e-6, tol=NAN), V=qp, ldv=p.nnz, LAMP=qp, ldlp=p.m, RHO=None, rho=10.0,
             X=qp, ldx=p.n, GR=qp, ldgr=p.n, XL=None, XU=None, ldb=0, RUN=None, run_stride=0, D=qp, ldd=p.n, SUM=qp, lds=8,
             W=C.c_void_p(QW), ldw=ldw, wrows=1)
    assert not set(kw) - set(a), kw
    a.update(kw)
    return a


def _direction(p, **kw):
    a = _dir_args(p, **kw)
    gn = a["gn"]
    return p._lib.towr_gpu_gn_direction_tiled_batch_device(
        p._h, a["B"], None if gn is None else C.byref(gn), a["V"], a["ldv"], a["LAMP"], a["ldlp"], a["RHO"], a["rho"],
        a["X"], a["ldx"], a["GR"], a["ldgr"], a["XL"], a["XU"], a["ldb"], a["RUN"], a["run_stride"], a["D"], a["ldd"], a["SUM"],
        a["lds"], a["W"], a["ldw"], a["wrows"], None)


def _iterate(p, par=None, st=None, gn="default", DC=Q, GSUM=Q, ldgs=8, W=QW, ldw=None, wrows=1, B=1, iters=1,
             bounds=(None, None, 0, None, None, 0)):
    par = alsolve_params() if par is None else par
    st = _state(p) if st is None else st
    gn = gn_params(ncg=0, mu=1e-6, tol=NAN) if gn == "default" else gn      # (ncg and tol are not read)
    ldw = p.gn_tile_info()["ldw_min"] if ldw is None else ldw
    return p._lib.towr_gpu_alsolve_gn_tiled_iterate_batch_device(
        p._h, B, iters, par, st, None if gn is None else C.byref(gn), C.c_void_p(DC) if DC else None,
        C.c_void_p(GSUM) if GSUM else None, ldgs, C.c_void_p(W) if W else None, ldw, wrows, *bounds, None)


def test_symbols_constants_and_methods():
    lib = capi.load_library()
    for name in ("towr_gpu_gn_tile_info", "towr_gpu_gn_direction_tiled_batch_device",
                 "towr_gpu_alsolve_gn_tiled_iterate_batch_device"):
        assert hasattr(lib, name) and name in capi.SYMBOLS
    assert capi.ABI_VERSION == 4 and lib.towr_gpu_abi_version() == 4
    assert C.sizeof(capi.GnParams) == 24 and C.sizeof(capi.AlSolveStateC) == 29 * 8      # both structs are unchanged
    header = open(capi.__file__.replace("towr2025_amd/_capi.py", "include/towr_gpu.h")).read()
    assert "#define TOWR_GN_TILE 16" in header and capi.GN_TILE == 16
    for m in ("gn_tile_info", "gn_tiled_direction_batch_device", "alsolve_gn_tiled_iterate"):
        assert callable(getattr(TowrGpuProblem, m))


def test_tile_info_on_a_layout_only_handle(p):
    info = p.gn_tile_info()
    n = p.n
    nt = -(-n // 16)
    first = p.gn_factor_info()["first"]
    assert (info["tile"], info["nt"]) == (16, nt)
    assert np.array_equal(info["bfirst"], [first[16 * I:16 * I + 16].min() // 16 for I in range(nt)])
    assert info["tiles"] == int((np.arange(nt) - info["bfirst"] + 1).sum())
    assert info["ldw_min"] == 256 * info["tiles"] > p.gn_factor_info()["ldw_min"]      # (the tile one is the larger)
    assert p._lib.towr_gpu_gn_tile_info(p._h, None, None, None, None, None) == capi.TOWR_OK
    assert p._lib.towr_gpu_gn_tile_info(None, None, None, None, None, None) == INV


def test_the_envelope_ldw_min_is_refused(p, env):
    """The envelope entry's ldw_min is smaller than the tile one: a workspace sized by it is refused here."""
    small = p.gn_factor_info()["ldw_min"]
    assert small < env
    assert _direction(p, ldw=small) == INV and b"towr_gpu_gn_tile_info" in p._lib.towr_gpu_last_error(p._h)
    assert _iterate(p, ldw=small) == INV and b"towr_gpu_gn_tile_info" in p._lib.towr_gpu_last_error(p._h)


def test_valid_arguments_reach_the_device_check(p, env):
    qp = C.c_void_p(Q)
    n, nnz = p.n, p.nnz
    assert _direction(p) == NODEV
    assert _direction(p, B=0) == NODEV
    assert _direction(p, X=None, ldx=0) == NODEV
    assert _direction(p, RHO=qp, rho=NAN) == NODEV
    assert _direction(p, XL=qp, XU=qp, ldb=n) == NODEV and _direction(p, RUN=qp, run_stride=4) == NODEV
    assert _direction(p, gn=gn_params(ncg=-5, mu=0.0, tol=-1.0)) == NODEV      # mu = 0 is valid; ncg and tol are not read
    assert _direction(p, ldw=env + 3, lds=11, wrows=7, B=3) == NODEV
    assert _direction(p, W=C.c_void_p(Q + 8 * nnz)) == NODEV                   # W right behind the longest row (V's)
    assert _direction(p, V=C.c_void_p(QV), W=C.c_void_p(QV - 8 * env)) == NODEV   # W's row ends where V begins
    assert _iterate(p) == NODEV and _iterate(p, B=0) == NODEV and _iterate(p, iters=0) == NODEV
    assert _iterate(p, gn=gn_params(ncg=-5, mu=0.0, tol=-1.0)) == NODEV
    assert _iterate(p, bounds=(qp, qp, p.m, qp, qp, n), wrows=5, B=2) == NODEV


def test_every_direction_refusal(p, env):
    lib, h, n, m, nnz = p._lib, p._h, p.n, p.m, p.nnz
    qp = C.c_void_p(Q)
    # the tiled entry's own (the direct entry's, on the tile ldw_min)
    assert _direction(p, W=None) == INV and b"W" in lib.towr_gpu_last_error(h)
    assert _direction(p, ldw=env - 1) == INV and b"ldw" in lib.towr_gpu_last_error(h)
    for bad in (0, -1):
        assert _direction(p, wrows=bad) == INV and b"wrows" in lib.towr_gpu_last_error(h), bad
    for lds in (5, 6, 7):
        assert _direction(p, lds=lds) == INV and b"summary" in lib.towr_gpu_last_error(h), lds
    for mu in BAD_MU:
        assert _direction(p, gn=gn_params(ncg=3, mu=mu)) == INV and b"mu" in lib.towr_gpu_last_error(h), mu
    # a used W row shares a byte with an input, with D or with SUM: its first, its last, a later row's
    assert _direction(p, W=qp) == INV and b"overlaps" in lib.towr_gpu_last_error(h)
    assert _direction(p, W=C.c_void_p(Q + 8 * (nnz - 1))) == INV                            # V's last entry
    qv = C.c_void_p(QV)
    assert _direction(p, V=qv, W=C.c_void_p(QV - 8 * (env - 1))) == INV                     # the row's last entry on V's first
    two = C.c_void_p(QV - 8 * (2 * env - 1))                                                # row 1's last entry on V's first
    assert _direction(p, V=qv, B=2, wrows=2, W=two) == INV and _direction(p, V=qv, B=2, wrows=1, W=two) == NODEV
    assert _direction(p, V=qv, B=1, wrows=2, W=two) == NODEV                                # (B = 1 uses one row)
    assert _direction(p, B=2, W=C.c_void_p(Q + 8 * (nnz + 1))) == INV                       # row 1 of V
    # everything towr_gpu_gn_direction_batch_device refuses (but gn's ncg and tol, which are not read)
    assert _direction(p, B=-1) == INV
    for k in ("gn", "V", "LAMP", "GR", "D", "SUM"):
        assert _direction(p, **{k: None}) == INV and lib.towr_gpu_last_error(h), k
    for rho in (0.0, -1.0, NAN):
        assert _direction(p, rho=rho) == INV and b"rho" in lib.towr_gpu_last_error(h), rho
    for k, v in (("ldv", nnz - 1), ("ldlp", m - 1), ("ldx", n - 1), ("ldgr", n - 1), ("ldd", n - 1)):
        assert _direction(p, **{k: v}) == INV and lib.towr_gpu_last_error(h), k
    assert _direction(p, XL=qp) == INV and _direction(p, XU=qp) == INV
    assert _direction(p, XL=qp, XU=qp, ldb=n - 1) == INV and b"ldb" in lib.towr_gpu_last_error(h)
    assert _direction(p, X=None, ldx=0, XL=qp) == INV


def test_every_iterate_refusal(p, env):
    lib, h, n, m = p._lib, p._h, p.n, p.m
    qp = C.c_void_p(Q)
    # the tiled entry's own (the direct entry's, on the tile ldw_min)
    assert _iterate(p, W=None) == INV and b"W" in lib.towr_gpu_last_error(h)
    assert _iterate(p, ldw=env - 1) == INV and b"ldw" in lib.towr_gpu_last_error(h)
    assert _iterate(p, wrows=0) == INV and b"wrows" in lib.towr_gpu_last_error(h)
    for ldgs in (5, 6, 7):
        assert _iterate(p, ldgs=ldgs) == INV, ldgs
    for mu in BAD_MU:
        assert _iterate(p, gn=gn_params(ncg=3, mu=mu)) == INV and b"mu" in lib.towr_gpu_last_error(h), mu
    assert _iterate(p, W=Q) == INV and b"overlaps" in lib.towr_gpu_last_error(h)          # DC, GSUM
    st = _state(p, XC=QV)
    assert _iterate(p, st=st, W=QV - 8 * (env - 1)) == INV and _iterate(p, st=st, W=QV - 8 * env) == NODEV
    for k in ("XC", "GRC", "LAMP"):                                                       # (each at an address of its own)
        assert _iterate(p, st=_state(p, **{k: 1 << 28}), W=1 << 28) == INV and b"overlaps" in lib.towr_gpu_last_error(h), k
        assert _iterate(p, st=_state(p, **{k: 1 << 28})) == NODEV, k
    assert _iterate(p, GSUM=1 << 28, W=1 << 28) == INV and _iterate(p, DC=1 << 28, W=1 << 28) == INV
    # everything towr_gpu_alsolve_gn_iterate_batch_device refuses (but gn's ncg and tol)
    assert _iterate(p, B=-1) == INV
    assert _iterate(p, iters=-1) == INV and b"iters" in lib.towr_gpu_last_error(h)
    assert _iterate(p, gn=None) == INV and b"gn" in lib.towr_gpu_last_error(h)
    assert _iterate(p, DC=None) == INV and _iterate(p, GSUM=None) == INV
    f = p._lib.towr_gpu_alsolve_gn_tiled_iterate_batch_device
    w = C.c_void_p(QW)
    assert f(h, 1, 1, None, _state(p), C.byref(gn_params()), qp, qp, 8, w, env, 1, None, None, 0, None, None, 0, None) == INV
    assert b"params" in lib.towr_gpu_last_error(h)
    for field, v in BAD_PARAMS:
        assert _iterate(p, par=alsolve_params(**{field: v})) == INV and b"params" in lib.towr_gpu_last_error(h), (field, v)
    assert f(h, 1, 1, alsolve_params(), None, C.byref(gn_params()), qp, qp, 8, w, env, 1, None, None, 0, None, None, 0, None) == INV
    assert b"state" in lib.towr_gpu_last_error(h)
    for k in PTRS:
        assert _iterate(p, st=_state(p, **{k: None})) == INV and b"state" in lib.towr_gpu_last_error(h), k
    for k, v in (("ldx", n - 1), ("ldh", n - 1), ("ldsc", 7), ("ldus", 5), ("ldls", 7), ("ldl", m - 1),
                 ("ldrs", 3 + p.desc.n_constraints), ("ldss", 4 + p.desc.n_varsets), ("ldds", 4)):
        assert _iterate(p, st=_state(p, **{k: v})) == INV and b"state" in lib.towr_gpu_last_error(h), k
    for what, args in (("only GL", (qp, None, 0, None, None, 0)), ("only GU", (None, qp, 0, None, None, 0)),
                       ("0 < ldgb < m", (qp, qp, m - 1, None, None, 0)), ("only XL", (None, None, 0, qp, None, 0)),
                       ("only XU", (None, None, 0, None, qp, 0)), ("0 < ldxb < n", (None, None, 0, qp, qp, n - 1))):
        assert _iterate(p, bounds=args) == INV and lib.towr_gpu_last_error(h), what
