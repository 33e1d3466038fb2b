"""The product kernels' tables (layout.hip build_jprod: chunks, row segments with their carry flags, by-column lists,
the long / short split at jp_long, the empty rows) on the CPU, for every shape of the seeded sweep and every parity
configuration, through the test-only host emulation and layout-only handles.

Invariants: what towr_jac_vec_kernel / towr_jac_tvec_kernel (jprod.hip) take for granted when they walk the tables.
Values: emu_jac_products is the host walk of the same tables in the kernels' order (tests/host_emu/emu.hip); on
standard-normal V, P, LAM and Z0 its Y, Z and accumulated Z are checked against the extended-precision reference under
the a-priori dot-product bound of tests/test_gpu_jac_products.py (tests/gpu_helpers.py _reference / _check_products,
which also ask +0.0 in empty rows, 0.0 in empty columns and untouched bits there under `accumulate`). The GPU's bits
are compared with this walk in tests/test_gpu_sweep_consumers.py."""
import numpy as np
import pytest

from tests import jp_emu
from tests.configs import config_descs
from tests.gpu_helpers import _check_products, _reference
from tests.shape_sweep import make
from towr2025_amd import TowrGpuProblem

CONFIGS = config_descs()
CASES = [f"seed_{s}" for s in range(200)] + sorted(CONFIGS)


def _desc(case):
    return make(int(case[5:]))[0].to_desc() if case.startswith("seed_") else CONFIGS[case]


def _ranges(start, length):
    """The concatenation of arange(start[i], start[i] + length[i])."""
    total = int(length.sum())
    first = np.repeat(start - np.concatenate(([0], np.cumsum(length)[:-1])), length)
    return first + np.arange(total)


@pytest.mark.parametrize("case", CASES)
def test_table_invariants(case):
    desc = _desc(case)
    p = TowrGpuProblem(desc, device=-1)
    t = jp_emu.tables(desc)
    rp, col = p.jac_csr()
    n, m, nnz = p.sizes()
    CH, LONG = t["chunk"], t["jp_long"]
    assert (t["n"], t["m"], t["nnz"]) == (n, m, nnz) and CH == 2048 and LONG >= 1
    csr_row = np.repeat(np.arange(m), np.diff(rp))
    np.testing.assert_array_equal(t["row"], csr_row, err_msg="jp_row")
    np.testing.assert_array_equal(t["empty_rows"], np.flatnonzero(np.diff(rp) == 0), err_msg="jp_empty_rows")
    nch = (nnz + CH - 1) // CH
    ch = t["chunks"].astype(np.int64)
    assert ch.shape[0] == nch and (ch[:, [1, 2, 4, 5]] >= 0).all()
    k0 = np.arange(nch, dtype=np.int64) * CH
    k1 = np.minimum(k0 + CH, nnz)
    for what, seg, s0, ns, nl in (("row", t["rseg"].astype(np.int64), ch[:, 0], ch[:, 1], ch[:, 2]),
                                  ("column", t["cseg"].astype(np.int64), ch[:, 3], ch[:, 4], ch[:, 5])):
        # the chunks' segment ranges follow each other and cover the segment table
        cnt = ns + nl
        np.testing.assert_array_equal(s0, np.concatenate(([0], np.cumsum(cnt)[:-1])), err_msg=f"{what} segments: first index per chunk")
        assert int(cnt.sum()) == seg.shape[0], f"{what} segments: table length"
        chunk_of = np.repeat(np.arange(nch), cnt)
        out, q0, ln, flags = seg.T
        assert (ln > 0).all(), f"{what} segments: an empty segment"
        # short segments first, then long ones, split exactly at jp_long
        is_long = np.arange(seg.shape[0]) - s0[chunk_of] >= ns[chunk_of]
        np.testing.assert_array_equal(is_long, ln >= LONG, err_msg=f"{what} segments: long exactly when len >= jp_long, short ones first")
        # an output has one segment per chunk at most (two would be summed by two lanes at once)
        assert np.unique(chunk_of * (max(n, m) + 1) + out).size == seg.shape[0], f"{what} segments: an output twice in a chunk"
        # the segments of a chunk tile its positions: every position in exactly one of them
        start = q0 + k0[chunk_of] if what == "row" else q0     # (a column segment's q0 is its index into jp_cidx)
        assert (start >= k0[chunk_of]).all() and (start + ln <= k1[chunk_of]).all(), f"{what} segments: outside the chunk"
        if what == "column":
            assert ((q0 & (CH - 1)) == q0 - k0[chunk_of]).all()
        cover = np.zeros(nnz + 1, dtype=np.int64)
        np.add.at(cover, start, 1)
        np.add.at(cover, start + ln, -1)
        assert (np.cumsum(cover)[:nnz] == 1).all(), f"{what} segments: a position in no segment or in two"
        pos = _ranges(start, ln)                               # positions, segment by segment
        owner = np.repeat(out, ln)
        if what == "row":
            np.testing.assert_array_equal(owner, csr_row[pos], err_msg="a row segment holds another row's entry")
            np.testing.assert_array_equal(flags & 1, (rp[out] < k0[chunk_of]).astype(np.int64), err_msg="flag bit 0: the row started in an earlier chunk")
            np.testing.assert_array_equal((flags >> 1) & 1, (rp[out + 1] > k1[chunk_of]).astype(np.int64), err_msg="flag bit 1: the row continues into the next chunk")
            assert (flags >> 2 == 0).all()
        else:
            assert (flags == 0).all()
            cidx = t["cidx"].astype(np.int64)
            for c in range(nch):                               # the by-column list is a permutation of the chunk's positions
                np.testing.assert_array_equal(np.sort(cidx[k0[c]:k1[c]]), np.arange(k1[c] - k0[c]), err_msg=f"chunk {c}: by-column list")
            entry = np.repeat(k0[chunk_of], ln) + cidx[pos]    # the CSR index behind every list position
            np.testing.assert_array_equal(owner, col[entry], err_msg="a column segment holds another column's entry")
            inner = np.ones(pos.size, dtype=bool)              # list positions that are not the first of their segment
            inner[np.cumsum(ln) - ln] = False
            assert (np.diff(csr_row[entry])[inner[1:]] > 0).all(), "rows do not ascend inside a column segment"


@pytest.mark.parametrize("case", CASES)
def test_emulated_products_within_bound(case):
    desc = _desc(case)
    p = TowrGpuProblem(desc, device=-1)
    rng = np.random.default_rng(20261020)
    V, P, LAM, Z0 = (rng.standard_normal((1, k)) for k in (p.nnz, p.n, p.m, p.n))
    Y, Z, Za = jp_emu.products(desc, V, P, LAM, Z0)
    assert np.isfinite(Y).all() and np.isfinite(Z).all() and np.isfinite(Za).all(), "an output not written, or summed over an entry not written"
    _check_products(case, p, jp_emu.Host(Y), jp_emu.Host(Z), jp_emu.Host(Za), Z0, _reference(p, V, P, LAM))
