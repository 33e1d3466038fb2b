"""The Jacobian products' tables and their host walks through the test-only emulation (tests/host_emu/emu.hip
emu_jp_tables_ex, emu_jac_products, emu_eval_ex, emu_gn_direction_ex): a helper of tests/test_jac_product_tables.py,
tests/test_gn_emu.py (CPU), tests/test_gpu_sweep_consumers.py and tests/test_gpu_sweep_gn.py (GPU); not a test."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np

from towr2025_amd import _capi as capi

HERE = os.path.dirname(os.path.abspath(__file__))
D = C.POINTER(C.c_double)


@functools.lru_cache(maxsize=None)
def lib():
    path = os.path.join(HERE, "host_emu", "build", "libemu.so")
    if not os.path.exists(path):
        subprocess.check_call(["make", "-s", "-C", os.path.join(HERE, "host_emu")])
    L = C.CDLL(path)
    L.emu_jp_tables_ex.argtypes = [C.POINTER(capi.ProblemDesc), C.c_int, C.POINTER(capi.SideData)] + [C.c_void_p] * 7
    L.emu_eval_ex.argtypes = [C.POINTER(capi.ProblemDesc), C.c_int, C.POINTER(capi.SideData), D, D, D, C.c_char_p, C.c_int]
    L.emu_gn_direction_ex.argtypes = ([C.POINTER(capi.ProblemDesc), C.c_int, C.POINTER(capi.SideData)] + [D] * 6 + [C.c_double] * 3 +
                                      [C.c_int, D, D])
    L.emu_jac_products.argtypes = [C.POINTER(capi.ProblemDesc)] + [D] * 7
    return L


def tables(desc, data=None):
    """build_jprod's tables of a description (`data`: its side data, [(kind, index, array)]): dict of jp_long, chunk (the
    chunk length), nnz, m, n, gn_block (towr_gn_direction_kernel's block), chunks (n_chunks, 6: rs0, rns, rnl, cs0, cns,
    cnl), rseg / cseg (segments, 4: out, q0, len, flags), cidx (n_chunks * chunk), empty_rows, row (nnz)."""
    L = lib()
    arr, keep = capi.side_data(data or [])
    nd = len(data or [])
    sizes = np.zeros(10, dtype=np.int64)
    assert L.emu_jp_tables_ex(C.byref(desc), nd, arr, sizes.ctypes.data, None, None, None, None, None, None) == 0
    nch, nr, nc, ne, jp_long, chunk, nnz, m, n, gn_block = (int(v) for v in sizes)
    t = dict(jp_long=jp_long, chunk=chunk, nnz=nnz, m=m, n=n, gn_block=gn_block,
             chunks=np.full((nch, 6), -1, dtype=np.int32), rseg=np.full((nr, 4), -1, dtype=np.int32),
             cseg=np.full((nc, 4), -1, dtype=np.int32), cidx=np.zeros(nch * chunk, dtype=np.uint16),
             empty_rows=np.full(ne, -1, dtype=np.int32), row=np.full(nnz, -1, dtype=np.int32))
    assert L.emu_jp_tables_ex(C.byref(desc), nd, arr, sizes.ctypes.data, *(t[k].ctypes.data for k in ("chunks", "rseg", "cseg", "cidx", "empty_rows", "row"))) == 0
    return t


def products(desc, V, P, LAM, Z0):
    """Y (B, m), Z (B, n), Za (B, n) of emu_jac_products for every row of V (B, nnz), P, Z0 (B, n), LAM (B, m); the
    outputs start as NaN."""
    L = lib()
    B, n, m = V.shape[0], P.shape[1], LAM.shape[1]
    Y, Z, Za = np.full((B, m), np.nan), np.full((B, n), np.nan), np.full((B, n), np.nan)
    for b in range(B):
        ops = [np.ascontiguousarray(a[b], dtype=np.float64) for a in (V, P, LAM, Z0)]
        assert L.emu_jac_products(C.byref(desc), *(a.ctypes.data_as(D) for a in ops), Y[b].ctypes.data_as(D), Z[b].ctypes.data_as(D),
                                  Za[b].ctypes.data_as(D)) == 0
    return Y, Z, Za


def evaluate(desc, x, m, nnz, data=None):
    """g (m) and the CSR values (nnz) of emu_eval_ex at x."""
    L = lib()
    arr, keep = capi.side_data(data or [])
    x = np.ascontiguousarray(x, dtype=np.float64)
    g, v = np.zeros(m), np.zeros(nnz)
    err = C.create_string_buffer(256)
    assert L.emu_eval_ex(C.byref(desc), len(data or []), arr, x.ctypes.data_as(D), g.ctypes.data_as(D), v.ctypes.data_as(D), err, 256) == 0, err.value
    return g, v


def gn_direction(desc, V, LAMP, GR, rho, mu, tol, ncg, X=None, XL=None, XU=None, data=None):
    """D (n) and SUM (6) of emu_gn_direction_ex, the host walk of towr_gn_direction_kernel, for one problem; X None:
    every column is free. The outputs start as NaN."""
    L = lib()
    arr, keep = capi.side_data(data or [])
    ops = [None if a is None else np.ascontiguousarray(a, dtype=np.float64) for a in (V, LAMP, GR, X, XL, XU)]
    assert (ops[3] is None) or (ops[4] is not None and ops[5] is not None)
    Dv, S = np.full(ops[2].size, np.nan), np.full(6, np.nan)
    rc = L.emu_gn_direction_ex(C.byref(desc), len(data or []), arr, *(None if a is None else a.ctypes.data_as(D) for a in ops),
                               float(rho), float(mu), float(tol), int(ncg), Dv.ctypes.data_as(D), S.ctypes.data_as(D))
    assert rc == 0, rc
    return Dv, S


class Host:
    """A host array where _check_products expects a device tensor."""

    def __init__(self, a):
        self.a = a

    def cpu(self):
        return self

    def numpy(self):
        return self.a
