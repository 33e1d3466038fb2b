"""The Jacobian products' tables and their host walk through the test-only emulation (tests/host_emu/emu.hip
emu_jp_tables, emu_jac_products): a helper of tests/test_jac_product_tables.py (CPU) and
tests/test_gpu_sweep_consumers.py (GPU); not a test."""
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
    L.emu_jp_tables.argtypes = [C.POINTER(capi.ProblemDesc)] + [C.c_void_p] * 7
    L.emu_jac_products.argtypes = [C.POINTER(capi.ProblemDesc)] + [D] * 7
    return L


def tables(desc):
    """build_jprod's tables of a description: dict of jp_long, chunk (the chunk length), nnz, m, n, chunks (n_chunks, 6:
    rs0, rns, rnl, cs0, cns, cnl), rseg / cseg (segments, 4: out, q0, len, flags), cidx (n_chunks * chunk), empty_rows,
    row (nnz)."""
    L = lib()
    sizes = np.zeros(9, dtype=np.int64)
    assert L.emu_jp_tables(C.byref(desc), sizes.ctypes.data, None, None, None, None, None, None) == 0
    nch, nr, nc, ne, jp_long, chunk, nnz, m, n = (int(v) for v in sizes)
    t = dict(jp_long=jp_long, chunk=chunk, nnz=nnz, m=m, n=n,
             chunks=np.full((nch, 6), -1, dtype=np.int32), rseg=np.full((nr, 4), -1, dtype=np.int32),
             cseg=np.full((nc, 4), -1, dtype=np.int32), cidx=np.zeros(nch * chunk, dtype=np.uint16),
             empty_rows=np.full(ne, -1, dtype=np.int32), row=np.full(nnz, -1, dtype=np.int32))
    assert L.emu_jp_tables(C.byref(desc), sizes.ctypes.data, *(t[k].ctypes.data for k in ("chunks", "rseg", "cseg", "cidx", "empty_rows", "row"))) == 0
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


class Host:
    """A host array where _check_products expects a device tensor."""

    def __init__(self, a):
        self.a = a

    def cpu(self):
        return self

    def numpy(self):
        return self.a
