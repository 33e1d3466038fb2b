"""Jacobian products, host side (no GPU): the pattern by column (jac_csc) is the transpose view of jac_csr on every
configuration; the device entry points refuse layout-only handles with TOWR_ERR_NO_DEVICE and bad arguments with
TOWR_ERR_INVALID; the Python methods refuse operands the C-ABI would read or write out of bounds."""
import ctypes as C

import numpy as np
import pytest

from tests.configs import config_descs
from towr2025_amd import TowrGpuProblem, _capi as capi
from towr2025_amd.problem import TowrGpuError

CONFIGS = config_descs()


@pytest.mark.parametrize("name", sorted(CONFIGS))
def test_csc_is_transpose_of_csr(name):
    p = TowrGpuProblem(CONFIGS[name], device=-1)
    rp, col = p.jac_csr()
    cp, row, idx = p.jac_csc()
    n, m, nnz = p.sizes()
    assert cp.shape == (n + 1,) and row.shape == (nnz,) and idx.shape == (nnz,)
    assert cp[0] == 0 and cp[n] == nnz and (np.diff(cp) >= 0).all()
    np.testing.assert_array_equal(np.sort(idx), np.arange(nnz))          # a permutation of the CSR positions
    col_of_q = np.repeat(np.arange(n), np.diff(cp))                      # the column each CSC entry sits in
    np.testing.assert_array_equal(col[idx], col_of_q)
    csr_row = np.repeat(np.arange(m), np.diff(rp))
    np.testing.assert_array_equal(row, csr_row[idx])
    inner = np.ones(nnz, dtype=bool)                                     # entries that are not the first of a column
    inner[cp[:-1][np.diff(cp) > 0]] = False
    assert (np.diff(row)[inner[1:]] > 0).all(), "rows do not ascend strictly inside a column"


def _fake(p):
    """Non-null pointers that must never be dereferenced (the calls under test fail before any launch)."""
    return C.c_void_p(4096)


def test_device_calls_refuse_layout_only_handle():
    p = TowrGpuProblem(CONFIGS["monoped_procedural"], device=-1)
    q, lib, h = _fake(p), p._lib, p._h
    n, m, nnz = p.sizes()
    calls = {
        "jac_vec": lambda: lib.towr_gpu_jac_vec_batch_device(h, 1, q, nnz, q, n, q, m, None),
        "jac_tvec": lambda: lib.towr_gpu_jac_tvec_batch_device(h, 1, q, nnz, q, m, q, n, 0, None),
        "eval_products": lambda: lib.towr_gpu_eval_products_batch_device(h, 1, q, n, q, m, q, m, q, n, 0, q, n, q, m, None),
    }
    for name, call in calls.items():
        assert call() == capi.TOWR_ERR_NO_DEVICE, name
        with pytest.raises(TowrGpuError, match=r"towr_gpu error -4"):
            p._check(call())
    assert lib.towr_gpu_set_products_chunk(h, 7) == capi.TOWR_OK      # the setter needs no device
    assert lib.towr_gpu_set_products_chunk(h, -1) == capi.TOWR_ERR_INVALID


def test_argument_errors_are_invalid_before_anything_runs():
    p = TowrGpuProblem(CONFIGS["monoped_procedural"], device=-1)
    q, lib, h, nul = _fake(p), p._lib, p._h, None
    n, m, nnz = p.sizes()
    INV = capi.TOWR_ERR_INVALID
    vec, tvec, fused = lib.towr_gpu_jac_vec_batch_device, lib.towr_gpu_jac_tvec_batch_device, lib.towr_gpu_eval_products_batch_device
    assert vec(h, 1, q, nnz - 1, q, n, q, m, None) == INV          # ldv < nnz
    assert vec(h, 1, q, nnz, q, n - 1, q, m, None) == INV          # ldp < n
    assert vec(h, 1, q, nnz, q, n, q, m - 1, None) == INV          # ldy < m
    assert vec(h, -1, q, nnz, q, n, q, m, None) == INV             # B < 0
    for args in ((nul, nnz, q, n, q, m), (q, nnz, nul, n, q, m), (q, nnz, q, n, nul, m)):
        assert vec(h, 1, *args, None) == INV                       # a null required pointer
    assert tvec(h, 1, q, nnz - 1, q, m, q, n, 0, None) == INV
    assert tvec(h, 1, q, nnz, q, m - 1, q, n, 0, None) == INV      # ldl < m
    assert tvec(h, 1, q, nnz, q, m, q, n - 1, 0, None) == INV      # ldz < n
    assert tvec(h, -1, q, nnz, q, m, q, n, 0, None) == INV
    for args in ((nul, nnz, q, m, q, n), (q, nnz, nul, m, q, n), (q, nnz, q, m, nul, n)):
        assert tvec(h, 1, *args, 0, None) == INV
    assert fused(h, 1, nul, n, q, m, q, m, q, n, 0, q, n, q, m, None) == INV       # null X
    assert fused(h, -1, q, n, q, m, q, m, q, n, 0, q, n, q, m, None) == INV
    assert fused(h, 1, q, n, q, m, nul, 0, q, n, 0, q, n, q, m, None) == INV       # Z without LAM
    assert fused(h, 1, q, n, q, m, q, m, q, n, 0, nul, 0, q, m, None) == INV       # Y without P
    assert fused(h, 1, q, n, q, m, q, m, nul, n, 0, q, n, q, m, None) == INV       # LAM without its output
    assert fused(h, 1, q, n, q, m, q, m - 1, q, n, 0, q, n, q, m, None) == INV     # ldl < m
    assert fused(h, 1, q, n, q, m, q, m, q, n - 1, 0, q, n, q, m, None) == INV     # ldz < n
    assert fused(h, 1, q, n, q, m, q, m, q, n, 0, q, n - 1, q, m, None) == INV     # ldp < n
    assert fused(h, 1, q, n, q, m, q, m, q, n, 0, q, n, q, m - 1, None) == INV     # ldy < m
    assert b"LAM" in lib.towr_gpu_last_error(h) or b"leading" in lib.towr_gpu_last_error(h)


def test_methods_refuse_bad_operands():
    torch = pytest.importorskip("torch")
    p = TowrGpuProblem(CONFIGS["monoped_procedural"], device=-1)
    n, m, nnz = p.sizes()
    host = lambda cols, dt=torch.float64: torch.zeros((2, cols), dtype=dt)
    V, P, Y, LAM, Z, X = host(nnz), host(n), host(m), host(m), host(n), host(n)
    with pytest.raises(TowrGpuError, match="expected a HIP device tensor"):
        p.jac_vec_batch_device(V, P, Y)
    with pytest.raises(TowrGpuError, match="expected a HIP device tensor"):
        p.jac_tvec_batch_device(V, LAM, Z)
    with pytest.raises(TowrGpuError, match="expected a HIP device tensor"):
        p.eval_products_batch_device(X, LAM=LAM, Z=Z)
    # Short rows and short leading dimensions. Without a GPU no tensor passes the device check, so these operands
    # report a host tensor's dtype, shape and strides as living on the handle's device; every method must raise
    # before it asks for their address.
    class OnDevice:
        def __init__(self, t):
            self.dtype, self.shape, self._t = t.dtype, t.shape, t
            self.device = type("D", (), {"type": "cuda", "index": -1})()
        def dim(self): return self._t.dim()
        def stride(self, i): return self._t.stride(i)
        def data_ptr(self): raise AssertionError("operand reached the C-ABI")
    dev = lambda cols: OnDevice(host(cols))
    overlapped = lambda cols: OnDevice(torch.as_strided(torch.zeros(cols + 1, dtype=torch.float64), (2, cols), (1, 1)))
    for bad, what in ((dev(nnz - 1), "needs >="), (overlapped(nnz), "leading dimension")):
        with pytest.raises(TowrGpuError, match=what):
            p.jac_vec_batch_device(bad, dev(n), dev(m))
        with pytest.raises(TowrGpuError, match=what):
            p.jac_tvec_batch_device(bad, dev(m), dev(n))
    for bad_cols, make in ((n - 1, dev), (n, overlapped)):
        with pytest.raises(TowrGpuError, match="P: "):
            p.jac_vec_batch_device(dev(nnz), make(bad_cols), dev(m))
        with pytest.raises(TowrGpuError, match="Z: "):
            p.jac_tvec_batch_device(dev(nnz), dev(m), make(bad_cols))
        with pytest.raises(TowrGpuError, match="Z: "):
            p.eval_products_batch_device(dev(n), LAM=dev(m), Z=make(bad_cols))
    with pytest.raises(TowrGpuError, match="Y: "):
        p.eval_products_batch_device(dev(n), P=dev(n), Y=dev(m - 1))
    f32 = lambda cols: OnDevice(host(cols, torch.float32))
    with pytest.raises(TowrGpuError, match="V: dtype"):
        p.jac_vec_batch_device(f32(nnz), dev(n), dev(m))
    with pytest.raises(TowrGpuError, match="LAM: dtype"):
        p.jac_tvec_batch_device(dev(nnz), f32(m), dev(n))
    with pytest.raises(TowrGpuError, match="Y: dtype"):
        p.eval_products_batch_device(dev(n), P=dev(n), Y=f32(m))
    with pytest.raises(TowrGpuError, match="LAM: .*rows"):
        p.jac_tvec_batch_device(dev(nnz), OnDevice(torch.zeros((1, m), dtype=torch.float64)), dev(n))
