"""The L-BFGS entry points at the C-ABI boundary (no GPU, a layout-only handle, fake pointers: nothing runs): the
symbols exist, every refusal include/towr_gpu.h lists is TOWR_ERR_INVALID with a message, and valid arguments are
TOWR_ERR_NO_DEVICE — the checks come before the device is bound."""
import ctypes as C

import pytest

from tests.configs import config_descs
from towr2025_amd import TowrGpuError, TowrGpuProblem, _capi as capi

INV, NODEV = capi.TOWR_ERR_INVALID, capi.TOWR_ERR_NO_DEVICE
Q = C.c_void_p(4096)


@pytest.fixture(scope="module")
def p():
    return TowrGpuProblem(config_descs()["monoped_procedural"], device=-1)


def _update_ok(p):
    n = p.n          # mem, X, ldx, XN, ldxn, GR, ldgr, GRN, ldgrn, curv_eps, HS, HY, ldh, HMETA, SUM, lds
    return [3, Q, n, Q, n, Q, n, Q, n, 1e-8, Q, Q, n, Q, Q, 6]


def _direction_ok(p):
    n = p.n          # mem, X, ldx, GR, ldgr, XL, XU, ldb, HS, HY, ldh, HMETA, D, ldd, SUM, lds
    return [3, Q, n, Q, n, None, None, 0, Q, Q, n, Q, Q, n, Q, 5]


def _fused_ok(p):
    n, m = p.n, p.m
    # 0 mem, 1 X, 2 ldx, 3 XPREV, 4 ldxprev, 5 GRPREV, 6 ldgrprev, 7 GL, 8 GU, 9 ldgb, 10 LAM, 11 ldl, 12 rho, 13 ALPHA,
    # 14 alpha, 15 XL, 16 XU, 17 ldxb, 18 curv_eps, 19 HS, 20 HY, 21 ldh, 22 HMETA, 23 F, 24 GR, 25 ldgr, 26 RSUM, 27 ldrs,
    # 28 USUM, 29 ldus, 30 DSUM, 31 ldds, 32 XP, 33 ldxp, 34 SSUM, 35 ldss
    return [3, Q, n, Q, n, Q, n, None, None, 0, Q, m, 1.0, None, 1.0, None, None, 0, 1e-8, Q, Q, n, Q, Q, Q, n,
            Q, 4 + p.desc.n_constraints, Q, 6, Q, 5, Q, n, Q, 5 + p.desc.n_varsets]


def _but(ok, *changes):
    a = list(ok)
    for i, v in changes:
        a[i] = v
    return a


def test_symbols_and_constant():
    lib = capi.load_library()
    for name in ("towr_gpu_lbfgs_update_batch_device", "towr_gpu_lbfgs_direction_batch_device",
                 "towr_gpu_auglag_lbfgs_step_batch_device"):
        assert hasattr(lib, name) and name in capi.SYMBOLS
    assert capi.LBFGS_MAX_MEM == 16 and capi.ABI_VERSION == 4 and lib.towr_gpu_abi_version() == 4
    for m in ("lbfgs_update_batch_device", "lbfgs_direction_batch_device", "auglag_lbfgs_step_batch_device"):
        assert callable(getattr(TowrGpuProblem, m))


def _refused(call, h, lib, ok, cases):
    for what, ch in cases:
        assert call(h, 1, *_but(ok, *ch), None) == INV, what
        assert lib.towr_gpu_last_error(h), what


def test_update_argument_checks(p):
    lib, h, n = p._lib, p._h, p.n
    call = lib.towr_gpu_lbfgs_update_batch_device
    ok = _update_ok(p)
    assert call(h, 1, *ok, None) == NODEV
    _refused(call, h, lib, ok, [("null X", [(1, None)]), ("null XN", [(3, None)]), ("null GR", [(5, None)]), ("null GRN", [(7, None)]),
                               ("null HS", [(10, None)]), ("null HY", [(11, None)]), ("null HMETA", [(13, None)]),
                               ("null SUM", [(14, None)]), ("mem 0", [(0, 0)]), ("mem 17", [(0, capi.LBFGS_MAX_MEM + 1)]),
                               ("mem -1", [(0, -1)]), ("ldx", [(2, n - 1)]), ("ldxn", [(4, n - 1)]), ("ldgr", [(6, n - 1)]),
                               ("ldgrn", [(8, n - 1)]), ("ldh", [(12, n - 1)]), ("lds", [(15, 5)]),
                               ("curv_eps < 0", [(9, -1e-300)]), ("curv_eps NaN", [(9, float("nan"))])])
    assert b"curv_eps" in lib.towr_gpu_last_error(h)
    assert call(h, -1, *ok, None) == INV
    assert call(h, 0, *ok, None) == NODEV                      # B = 0 is TOWR_OK only where there is a device
    assert call(h, 1, *_but(ok, (0, 1), (9, 0.0)), None) == NODEV
    assert call(h, 1, *_but(ok, (0, capi.LBFGS_MAX_MEM)), None) == NODEV


def test_direction_argument_checks(p):
    lib, h, n = p._lib, p._h, p.n
    call = lib.towr_gpu_lbfgs_direction_batch_device
    ok = _direction_ok(p)
    assert call(h, 1, *ok, None) == NODEV
    _refused(call, h, lib, ok, [("null GR", [(3, None)]), ("null HS", [(8, None)]), ("null HY", [(9, None)]),
                               ("null HMETA", [(11, None)]), ("null D", [(12, None)]), ("null SUM", [(14, None)]),
                               ("mem 0", [(0, 0)]), ("mem 17", [(0, capi.LBFGS_MAX_MEM + 1)]), ("ldx", [(2, n - 1)]),
                               ("ldgr", [(4, n - 1)]), ("ldh", [(10, n - 1)]), ("ldd", [(13, n - 1)]), ("lds", [(15, 4)]),
                               ("only XL", [(5, Q)]), ("only XU", [(6, Q)]), ("0 < ldb < n", [(5, Q), (6, Q), (7, n - 1)])])
    assert call(h, -1, *ok, None) == INV
    assert call(h, 1, *_but(ok, (1, None), (2, 0)), None) == NODEV            # X = NULL: every column free, no ldx
    assert call(h, 1, *_but(ok, (5, Q), (6, Q), (7, n)), None) == NODEV
    assert call(h, 1, *_but(ok, (5, Q), (6, Q)), None) == NODEV               # ldb = 0: one shared row


def test_fused_argument_checks(p):
    lib, h, n, m = p._lib, p._h, p.n, p.m
    call = lib.towr_gpu_auglag_lbfgs_step_batch_device
    ok = _fused_ok(p)
    assert call(h, 1, *ok, None) == NODEV
    ldr, lss = 4 + p.desc.n_constraints, 5 + p.desc.n_varsets
    _refused(call, h, lib, ok, [("null X", [(1, None)]), ("ldx", [(2, n - 1)]), ("only XPREV", [(5, None)]), ("only GRPREV", [(3, None)]),
                               ("ldxprev", [(4, n - 1)]), ("ldgrprev", [(6, n - 1)]), ("only GL", [(7, Q)]), ("only GU", [(8, Q)]),
                               ("0 < ldgb < m", [(7, Q), (8, Q), (9, m - 1)]), ("ldl", [(11, m - 1)]), ("rho", [(12, 0.0)]),
                               ("NaN alpha", [(14, float("nan"))]), ("only XL", [(15, Q)]), ("only XU", [(16, Q)]),
                               ("0 < ldxb < n", [(15, Q), (16, Q), (17, n - 1)]), ("curv_eps < 0", [(18, -1.0)]),
                               ("curv_eps NaN", [(18, float("nan"))]), ("null HS", [(19, None)]), ("null HY", [(20, None)]),
                               ("ldh", [(21, n - 1)]), ("null HMETA", [(22, None)]), ("null GR", [(24, None)]),
                               ("ldgr", [(25, n - 1)]), ("null RSUM", [(26, None)]), ("ldrs", [(27, ldr - 1)]),
                               ("null USUM", [(28, None)]), ("ldus", [(29, 5)]), ("null DSUM", [(30, None)]), ("ldds", [(31, 4)]),
                               ("null XP", [(32, None)]), ("ldxp", [(33, n - 1)]), ("null SSUM", [(34, None)]),
                               ("ldss", [(35, lss - 1)]), ("mem 0", [(0, 0)]), ("mem 17", [(0, capi.LBFGS_MAX_MEM + 1)])])
    assert call(h, -1, *ok, None) == INV
    first = _but(ok, (3, None), (4, 0), (5, None), (6, 0), (28, None), (29, 0))   # the first iteration: no update, no USUM
    assert call(h, 1, *first, None) == NODEV
    assert call(h, 1, *_but(ok, (23, None)), None) == NODEV                       # F is optional
    assert call(h, 1, *_but(first, (0, 0)), None) == INV                          # (mem still bounds the direction)


def test_methods_refuse_bad_operands(p):
    torch = pytest.importorskip("torch")
    n = p.n
    host = lambda rows, cols, dt=torch.float64: torch.zeros((rows, cols), dtype=dt)
    with pytest.raises(TowrGpuError, match="expected a HIP device tensor"):
        p.lbfgs_direction_batch_device(host(2, n), host(6, n), host(6, n), torch.zeros(4, dtype=torch.int32), host(2, n), host(2, 5), 3)

    class OnDevice:
        def __init__(self, t):
            self.dtype, self.shape, self._t = t.dtype, t.shape, t
            self.device = type("D", (), {"type": "cuda", "index": -1})()
        def dim(self): return self._t.dim()
        def stride(self, i): return self._t.stride(i)
        def numel(self): return self._t.numel()
        def is_contiguous(self): return self._t.is_contiguous()
        def data_ptr(self): raise AssertionError("operand reached the C-ABI")
    dev = lambda rows, cols, dt=torch.float64: OnDevice(host(rows, cols, dt))
    meta = lambda k, dt=torch.int32: OnDevice(torch.zeros(k, dtype=dt))
    with pytest.raises(TowrGpuError, match="mem: "):
        p.lbfgs_direction_batch_device(dev(2, n), dev(6, n), dev(6, n), meta(4), dev(2, n), dev(2, 5), 17)
    with pytest.raises(TowrGpuError, match="HS: "):
        p.lbfgs_direction_batch_device(dev(2, n), dev(5, n), dev(6, n), meta(4), dev(2, n), dev(2, 5), 3)
    with pytest.raises(TowrGpuError, match="HS and HY"):
        p.lbfgs_direction_batch_device(dev(2, n), dev(6, n), dev(6, n + 1), meta(4), dev(2, n), dev(2, 5), 3)
    with pytest.raises(TowrGpuError, match="HMETA: dtype"):
        p.lbfgs_direction_batch_device(dev(2, n), dev(6, n), dev(6, n), meta(4, torch.int64), dev(2, n), dev(2, 5), 3)
    with pytest.raises(TowrGpuError, match="HMETA: expected"):
        p.lbfgs_direction_batch_device(dev(2, n), dev(6, n), dev(6, n), meta(3), dev(2, n), dev(2, 5), 3)
    with pytest.raises(TowrGpuError, match="SUM: "):
        p.lbfgs_direction_batch_device(dev(2, n), dev(6, n), dev(6, n), meta(4), dev(2, n), dev(2, 4), 3)
    with pytest.raises(TowrGpuError, match="SUM: "):
        p.lbfgs_update_batch_device(dev(2, n), dev(2, n), dev(2, n), dev(2, n), dev(6, n), dev(6, n), meta(4), dev(2, 5), 3)
    with pytest.raises(TowrGpuError, match="GRN: "):
        p.lbfgs_update_batch_device(dev(2, n), dev(2, n), dev(2, n), dev(2, n - 1), dev(6, n), dev(6, n), meta(4), dev(2, 6), 3)
    lss, ldr = 5 + p.desc.n_varsets, 4 + p.desc.n_constraints
    with pytest.raises(TowrGpuError, match="both or neither"):
        p.auglag_lbfgs_step_batch_device(dev(2, n), dev(2, n), dev(2, n), dev(2, lss), dev(2, ldr), dev(2, 5), dev(6, n), dev(6, n),
                                         meta(4), 3, XPREV=dev(2, n))
    with pytest.raises(TowrGpuError, match="USUM: "):
        p.auglag_lbfgs_step_batch_device(dev(2, n), dev(2, n), dev(2, n), dev(2, lss), dev(2, ldr), dev(2, 5), dev(6, n), dev(6, n),
                                         meta(4), 3, XPREV=dev(2, n), GRPREV=dev(2, n))
    with pytest.raises(TowrGpuError, match="DSUM: "):
        p.auglag_lbfgs_step_batch_device(dev(2, n), dev(2, n), dev(2, n), dev(2, lss), dev(2, ldr), dev(2, 4), dev(6, n), dev(6, n),
                                         meta(4), 3)
