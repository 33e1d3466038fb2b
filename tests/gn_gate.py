"""The gate of the Gauss-Newton direction's tests and the comparison of one problem's D / SUM with the references of
tests/gn_ref.py, importable without torch: shared by tests/test_gpu_gn.py, tests/test_gpu_sweep_gn.py (the device's
outputs) and tests/test_gn_emu.py (the host walk's). Not a test.

The gate is measured on the reference and never on what is checked: err against the long double reference
<= 8 max(e64, gamma_n scale), e64 = the larger error of two float64 evaluations of the reference with different
summation orders, scale = max |value| (of D: over its free columns), gamma_n of tests/test_gpu_lbfgs.py."""
import numpy as np

from tests import gn_ref as G
from tests.gpu_helpers import _np_bits
from tests.test_gpu_lbfgs import _gamma

LD = np.longdouble


def refs(P, V, LAMP, rho, GR, ncg, mu, tol, held):
    """(the long double reference, [the two float64 references]) of one problem."""
    a = (P, V, LAMP, rho, GR, ncg, mu, tol)
    return G.direction(*a, dtype=LD, held=held), [G.direction(*a, reverse=rev, held=held) for rev in (False, True)]


def gate(ld, f64, key, n):
    """(long double value, gate, e64 / scale) of D (key 'D', its free columns) or of a scalar."""
    v = np.asarray(ld[key], dtype=LD)
    sel = ld["free"] if key == "D" else ...
    e64 = max(float(np.max(np.abs(np.asarray(f[key]).astype(LD) - v)[sel], initial=0.0)) for f in f64)
    scale = float(np.max(np.abs(v)[sel], initial=0.0))   # (D: over its free columns — the held ones hold g, far larger)
    return v, 8 * max(e64, _gamma(n) * scale), e64 / scale if scale else 0.0


def check_values(tag, n, g, held, Dh, S, ld, f64):
    """D (n) and SUM (6) of one problem against the references: the held columns, steps, held count and stop code
    exactly, D == g when no step completed, the free columns of D and bb, rr, slope within the gate. Returns the largest
    err / gate."""
    assert np.array_equal(_np_bits(Dh[:n][held]), _np_bits(g[held])), f"{tag}: held columns"
    assert all((f["steps"], f["code"]) == (ld["steps"], ld["code"]) for f in f64), f"{tag}: the references disagree"
    assert (S[0], S[4], S[5]) == (ld["steps"], ld["nheld"], ld["code"]), f"{tag}: steps / held / code {S[:6]} vs {ld['steps'], ld['nheld'], ld['code']}"
    if ld["steps"] == 0:
        assert np.array_equal(_np_bits(Dh[:n]), _np_bits(g)), f"{tag}: no step completed, D must be GR"
    worst = 0.0
    for key, got in (("D", Dh[:n]), ("bb", S[1]), ("rr", S[2]), ("slope", S[3])):
        v, gt, _ = gate(ld, f64, key, n)
        sel = ld["free"] if key == "D" else ...
        err = float(np.max(np.abs(np.asarray(got).astype(LD) - v)[sel], initial=0.0))
        print(f"{tag}: {key} err {err:.3e} gate {gt:.3e}")
        assert err <= gt, f"{tag}: {key} err {err:.3e} gate {gt:.3e}"
        worst = max(worst, err / gt if gt > 0 else 0.0)
    return worst
