"""The batched L-BFGS kernels on the device (towr_gpu_lbfgs_update_batch_device, towr_gpu_lbfgs_direction_batch_device)
and the one-call iteration (towr_gpu_auglag_lbfgs_step_batch_device) against tests/lbfgs_ref.py, the numpy restatement
of the formulas in include/towr_gpu.h. Every case uses padded leading dimensions with NaN padding and NaN-filled
outputs and history. The shapes are those of tests/test_gpu_step.py, for its reasons; mem in {1, 3, 5}: the ring wraps
and is not a power of two.

Gates.
Update: s and y are single rounded subtractions: bit-equal to numpy. The slot, count, next and SUM[3..5] are exact.
SUM[0..2] are sums of n terms: |got - ref| <= 2 gamma_n sum |term| + 8 u sum |term| against the long double
reference (the bound tests/test_gpu_step.py derives). The whole history (padding included) is compared bit for bit
with a numpy mirror after every call, so a rejected problem's bytes and the padding are seen untouched. No decision
is a rounding tie: the reference has |sy - curv_eps yy| >= 1e-6 sum |s y| for every problem of every call.

Direction: the held columns of D, the pairs used and the held count are exact. The free columns of D, gamma, SUM[2]
and SUM[4] cannot be bounded a priori (the recursion's conditioning enters), so the gate is measured on the reference,
never on the kernel: per problem, err = max_j |D_j - D_ld_j| against the long double reference, scale = max_j
|D_ld_j|, e64 = the larger err of two float64 evaluations of the reference with different summation orders (numpy's
pairwise sum; the columns reversed); the kernel passes when err <= 8 max(e64, gamma_n scale). (The kernel's tree is a
third order of the same sums; 8 covers the tail over the problems tested.) For the scalars err, e64 and scale are the
same quantities of the scalar. The gate still refuses a wrong recursion: dropping any one used pair from the
reference moves D by more than 1000 gates (asserted on the CPU). No used / unused decision is a tie: every
|c_i| >= 1e-6 sum_free |s y| in the reference — the seeds below were chosen so that this holds (the assertion would
say otherwise). Largest err / gate seen on MI355X: 1.2e-3 (per case: DESIGN 4i)."""
import functools

import numpy as np
import pytest

from tests import lbfgs_ref as R
from tests.configs import config_descs, cost_descs
from tests.gpu_helpers import _dev, _formulation, _nan, _np_bits, _padded, _same_bits, _terrains, _vec
from towr2025_amd import TowrGpuProblem
from towr2025_amd import formulation as F

pytestmark = pytest.mark.gpu

U = 2.0 ** -53
LD = np.longdouble
CASES = [("monoped_procedural", 1), ("monoped_procedural", 3), ("anymal_trot_2p4s", 37), ("anymal_stairs_gaitopt", 3)]
MEMS = [1, 3, 5]
ITERS = 6


def _gamma(n):
    return n * U / (1 - n * U)


def _ints(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).to(_dev())


@functools.lru_cache(maxsize=None)
def _problem(name):
    """The handle of a configuration of tests/configs.py, or of shape N of the seeded sweep ("sweep_seed_N":
    tests/test_gpu_sweep_consumers.py), with its variable bounds."""
    if name.startswith("sweep_seed_"):
        from tests.shape_sweep import make
        f = make(int(name[len("sweep_seed_"):]))[0]
        f.params_.enable_stance_tracking = False   # (as gpu_helpers._formulation: no stance positions are given)
        vb = f.var_bounds_data()
        p = TowrGpuProblem(f.to_desc(), device=0, data=vb)
        return (p,) + p.variable_bounds() + (vb,)
    f, kw = _formulation(name)
    vb = f.var_bounds_data(**kw)
    p = TowrGpuProblem(config_descs()[name], device=0, data=vb)
    lo, up = p.variable_bounds()
    return p, lo, up, vb


class Quadratic:
    """Per problem b the convex quadratic 0.5 x^T A_b x - b_b^T x with A_b = M + diag(d_b), SPD and n by n: M = W^T W
    (rank 24, formed once and shared) and d_b the problem's own diagonal, in [0.5, 5] (1 + b % 3), so the problems'
    curvatures differ. Minimised at xs_b: grad = A_b (x - xs_b), b_b = A_b xs_b."""

    def __init__(self, B, n, seed):
        rng = np.random.default_rng(seed)
        W = rng.standard_normal((24, n)) / np.sqrt(24.0)
        self.M = W.T @ W
        self.d = np.exp(rng.uniform(np.log(0.5), np.log(5.0), (B, n))) * (1 + np.arange(B) % 3)[:, None]

    def mul(self, V):
        return self.d * V + V @ self.M

    def grad(self, X, XS):
        return self.mul(X) - self.mul(XS)


# ---- update ----------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _update_sequence(name, B, mem):
    """mem + 2 independent offers per problem on the quadratic. Offer t of problem b is, by (t + 2 b) % 5: 1 a
    negative-curvature pair (y negated), 3 a NaN in XN, else a plain pair; the last offer (problem 0's a plain pair) is
    made with curv_eps set between the problems' sy / yy (fewer than two plain pairs: above it), every other with
    curv_eps = 0."""
    p, _, _, _ = _problem(name)
    n = p.n
    quad = Quadratic(B, n, 77 + mem)
    rng = np.random.default_rng(1000 + 10 * B + mem)
    steps = []
    for t in range(mem + 2):
        X, S = rng.standard_normal((B, n)), 0.1 * rng.standard_normal((B, n))
        XN = X + S
        GR = quad.mul(X)
        GRN = quad.mul(XN)
        kind = (t + 2 * np.arange(B)) % 5
        if t == mem + 1:
            kind[0] = 0                                                 # (a plain pair for the curv_eps test to reject)
        GRN[kind == 1] = GR[kind == 1] - (GRN[kind == 1] - GR[kind == 1])
        XN[kind == 3, n // 3] = np.nan
        eps = 0.0
        if t == mem + 1:
            s, y = XN - X, GRN - GR
            ratio = np.sort([(s[b] @ y[b]) / (y[b] @ y[b]) for b in range(B) if kind[b] not in (1, 3)])
            eps = 2.0 * ratio[0] if len(ratio) == 1 else float(np.sqrt(ratio[len(ratio) // 2 - 1] * ratio[len(ratio) // 2]))
        steps.append((X, XN, GR, GRN, eps, kind))
    return p, steps


@pytest.mark.parametrize("mem", MEMS)
@pytest.mark.parametrize("name,B", CASES)
def test_update_against_numpy(name, B, mem):
    check_update(name, B, mem)


def check_update(name, B, mem):
    import torch
    p, steps = _update_sequence(name, B, mem)
    n = p.n
    ldh = n + 3
    HSd, HYd, METAd = _nan(B * mem, ldh), _nan(B * mem, ldh), _ints(np.zeros((B, 2)))
    HS, HY = HSd.cpu().numpy().reshape(B, mem, ldh), HYd.cpu().numpy().reshape(B, mem, ldh)   # the numpy mirror (NaN-filled)
    META = np.zeros((B, 2), dtype=np.int32)
    seen, worst, decisions = set(), 0.0, [[] for _ in range(B)]
    for t, (X, XN, GR, GRN, eps, kind) in enumerate(steps):
        ref = np.zeros((B, 6), dtype=LD)
        absterm = np.zeros((B, 3), dtype=LD)
        for b in range(B):
            before = META[b].copy()
            ref[b], abs_sy = R.update(X[b], XN[b], GR[b], GRN[b], eps, HS[b], HY[b], META[b], dtype=LD)
            with np.errstate(invalid="ignore"):
                s, y = (XN[b] - X[b]).astype(LD), (GRN[b] - GR[b]).astype(LD)
            absterm[b] = abs_sy, np.sum(s * s), np.sum(y * y)
            if np.isnan(ref[b, 0]):
                assert ref[b, 3] == 0.0
                seen.add("nan")
            else:                                                       # no decision is a rounding tie
                assert abs(ref[b, 0] - LD(eps) * ref[b, 2]) >= 1e-6 * abs_sy, f"offer {t} problem {b}: a tie"
                seen.add("accept" if ref[b, 3] else ("negative" if ref[b, 0] < 0 else "eps"))
            assert ref[b, 3] == 1.0 or (META[b] == before).all()
            decisions[b].append(int(ref[b, 3]))
        SUM = _nan(B, 6 + 2)
        p.lbfgs_update_batch_device(_padded(X, n + 1), _padded(XN, n + 7), _padded(GR, n + 2), _padded(GRN, n), HSd, HYd, METAd, SUM,
                                    mem, curv_eps=eps)
        torch.cuda.synchronize()
        S = SUM.cpu().numpy()
        assert np.isnan(S[:, 6:]).all(), "SUM written beyond 6"
        np.testing.assert_array_equal(S[:, 3:6], ref[:, 3:6].astype(np.float64), err_msg=f"offer {t}: accepted / count / slot")
        np.testing.assert_array_equal(METAd.cpu().numpy(), META, err_msg=f"offer {t}: HMETA")
        for dev, mirror, what in ((HSd, HS, "HS"), (HYd, HY, "HY")):   # bit for bit: the slot written, every other byte untouched
            np.testing.assert_array_equal(_np_bits(dev.cpu().numpy()), _np_bits(mirror.reshape(B * mem, ldh)), err_msg=f"offer {t}: {what}")
        fin = ~np.isnan(ref[:, :3].astype(np.float64))
        assert np.isnan(S[:, :3][~fin]).all(), "a NaN operand must make its sums NaN"
        err = np.abs(S[:, :3].astype(LD) - ref[:, :3])
        bound = (2 * _gamma(n) + 8 * U) * absterm
        assert (err[fin] <= bound[fin]).all(), f"offer {t}: SUM[0..2] outside 2 gamma_n sum |term| + 8 u sum |term|"
        worst = max(worst, float(np.max(err[fin] / bound[fin])))
    print(f"{name} B={B} mem={mem}: update sums |err|/bound {worst:.3f}; decisions {sorted(seen)}")
    assert {"accept", "negative"} <= seen and ("eps" in seen)
    if mem + 2 > 3 or B > 1:
        assert "nan" in seen
    if B > 1:                                                           # the rings diverged: the problems' accept sequences differ
        assert len({tuple(d) for d in decisions}) > 1


# ---- direction -------------------------------------------------------------------------------------------------------
def _step(x, d, alpha, lo, up):
    """The projected step of include/towr_gpu.h (as tests/test_gpu_step.py's reference)."""
    t = x - alpha * d
    t = np.where((lo > -1e19) & (t < lo), lo, t)
    return np.where((up < 1e19) & (t > up), up, t)


@functools.lru_cache(maxsize=None)
def _direction_case(name, B, mem):
    """The reference's own bound-projected L-BFGS loop on the quadratic, ITERS iterations from a start with box columns
    on either bound and inside: per iteration the operands (X, GR, the history before the direction) and the reference
    results in long double and in float64 with two summation orders. Two departures, so that the cases hold what the
    kernel must get right: after iteration 3's update the newest pair of the last problem has its y negated (a stale
    pair a caller left behind: c_i < 0, unused); after iteration 4's update problem 1 (when B > 1) has its HMETA
    zeroed (a reset, as after a change of lam or rho: count < mem next to wrapped rings)."""
    p, lo, up, _ = _problem(name)
    n = p.n
    rng = np.random.default_rng(4242 + 100 * B + mem)
    quad = Quadratic(B, n, 11 + mem)
    box = (lo > -1e19) & (up < 1e19) & (lo < up)
    fixed = lo == up
    x0 = p.initial_x()
    X = x0 + 0.05 * rng.standard_normal((B, n))
    XS = x0 + 0.3 * rng.standard_normal((B, n))
    w = np.where(box, up - lo, 0.0)
    XS[:, box] = (lo - w)[box] + rng.random((B, int(box.sum()))) * 3 * w[box]          # optima inside and beyond either side
    where = rng.integers(0, 3, (B, n))
    X = np.where(box & (where == 0), lo, np.where(box & (where == 1), up, X))
    X[:, box] = np.clip(X[:, box], lo[box], up[box])
    ldh = n + 3
    HS, HY = np.full((B, mem, ldh), np.nan), np.full((B, mem, ldh), np.nan)
    META = np.zeros((B, 2), dtype=np.int32)
    its, Xprev, Gprev = [], None, None
    accepted = np.zeros(B, dtype=int)
    for k in range(ITERS):
        GR = quad.grad(X, XS)
        if k > 0:
            for b in range(B):
                out, _ = R.update(Xprev[b], X[b], Gprev[b], GR[b], 0.0, HS[b], HY[b], META[b])
                accepted[b] += int(out[3])
                if k == 3 and b == B - 1 and out[3]:
                    HY[b, int(out[5]), :n] *= -1.0
            if k == 4 and B > 1:
                META[1] = 0
                accepted[1] = 0
        held = np.stack([R.held_mask(X[b], GR[b], lo, up) for b in range(B)])
        ld = [R.direction(GR[b], HS[b], HY[b], META[b], held[b], dtype=LD) for b in range(B)]
        f64 = [[R.direction(GR[b], HS[b], HY[b], META[b], held[b], reverse=rev) for b in range(B)] for rev in (False, True)]
        its.append(dict(X=X.copy(), GR=GR, HS=HS.copy(), HY=HY.copy(), META=META.copy(), held=held, ld=ld, f64=f64,
                        accepted=accepted.copy()))
        D = np.stack([f64[0][b]["D"] for b in range(B)])
        Xprev, Gprev = X, GR
        X = _step(X, D, 0.1 if k == 0 else 1.0, lo, up)
    return dict(p=p, lo=lo, up=up, box=box, fixed=fixed, its=its, ldh=ldh)


def _gates(it, b, key):
    """(long double value, gate) of D (key 'D') or of a scalar of problem b: 8 max(e64, gamma_n scale)."""
    v = it["ld"][b][key]
    free = it["ld"][b]["free"] if key == "D" else ...
    e64 = max(float(np.max(np.abs(it["f64"][o][b][key].astype(LD) - v)[free], initial=0.0)) for o in (0, 1))
    scale = float(np.max(np.abs(v), initial=0.0))
    return v, 8 * max(e64, _gamma(it["X"].shape[1]) * scale)


def _assert_direction_inputs(c, name, B, mem):
    """On the reference, on the CPU: what the cases must contain, no tie, and a gate that refuses a wrong recursion."""
    lo, up, box, fixed = c["lo"], c["up"], c["box"], c["fixed"]
    n = lo.shape[0]
    assert fixed.any()
    unused = wrapped = short = False
    low = high = inward = False
    for k, it in enumerate(c["its"]):
        for b in range(B):
            ld = it["ld"][b]
            x, g, held = it["X"][b], it["GR"][b], it["held"][b]
            assert held[fixed].all() and ld["nheld"] == held.sum()
            low |= bool((held & box & (x == lo)).any())
            high |= bool((held & box & (x == up)).any())
            inward |= bool((~held & box & ((x == lo) | (x == up))).any())
            for c_i, a_i in zip(ld["c"], ld["abs_c"]):
                assert abs(c_i) >= 1e-6 * a_i, f"iteration {k} problem {b}: a used / unused tie"
            unused |= len(ld["used"]) < len(ld["c"])
            assert all(f["used"] == ld["used"] for f in (it["f64"][0][b], it["f64"][1][b]))
            _, gate = _gates(it, b, "D")
            for i in ld["used"]:                                        # a recursion without pair i is far outside the gate
                wrong = R.direction(g, it["HS"][b], it["HY"][b], it["META"][b], held, dtype=LD, drop=i)["D"]
                assert float(np.max(np.abs(wrong - ld["D"]))) > 1000 * gate, f"iteration {k} problem {b}: dropping pair {i} passes"
        wrapped |= bool((it["accepted"] > mem).any())
        short |= bool((it["accepted"] > mem).any() and (it["META"][:, 0] < mem).any())
    assert unused, "no unused pair"
    if box.any():
        assert low and high and inward, "no held-at-lower / held-at-upper / free-on-a-bound column"
    if mem < ITERS - 1:
        assert wrapped
        assert short or B == 1, "no problem with count < mem next to a wrapped ring"
    assert n == c["p"].n


def _check_direction(tag, it, b_rows, D, SUM, n):
    """Device D (rows, >= n) and SUM (rows, >= 5) of the problems b_rows of iteration `it`; returns the largest err / gate."""
    Dh, S = D.cpu().numpy(), SUM.cpu().numpy()
    assert np.isnan(Dh[:, n:]).all() and np.isnan(S[:, 5:]).all(), f"{tag}: padding written"
    worst = 0.0
    for r, b in enumerate(b_rows):
        ld = it["ld"][b]
        held = ~ld["free"]
        np.testing.assert_array_equal(_np_bits(Dh[r, :n][held]), _np_bits(it["GR"][b][held]), err_msg=f"{tag} problem {b}: held columns")
        assert S[r, 0] == len(ld["used"]) and S[r, 3] == ld["nheld"], f"{tag} problem {b}: pairs used / held columns"
        if not ld["used"]:
            np.testing.assert_array_equal(_np_bits(Dh[r, :n]), _np_bits(it["GR"][b]), err_msg=f"{tag} problem {b}: no pair used, D must be GR")
            assert S[r, 1] == 1.0
        for key, got in (("D", Dh[r, :n]), ("gamma", S[r, 1]), ("slope", S[r, 2]), ("gg", S[r, 4])):
            v, gate = _gates(it, b, key)
            err = float(np.max(np.abs(np.asarray(got).astype(LD) - v)))
            assert err <= gate, f"{tag} problem {b}: {key} err {err:.3e} gate {gate:.3e}"
            worst = max(worst, err / gate if gate > 0 else 0.0)
    return worst


def _upload(c, it):
    B, mem, ldh = it["HS"].shape
    n = c["p"].n
    return (_padded(it["X"], n + 1), _padded(it["GR"], n + 7), _padded(it["HS"].reshape(B * mem, ldh), ldh),
            _padded(it["HY"].reshape(B * mem, ldh), ldh), _ints(it["META"]))


@pytest.mark.parametrize("mem", MEMS)
@pytest.mark.parametrize("name,B", CASES)
def test_direction_against_numpy(name, B, mem):
    check_direction(name, B, mem)


def check_direction(name, B, mem):
    import torch
    c = _direction_case(name, B, mem)
    _assert_direction_inputs(c, name, B, mem)
    p, n = c["p"], c["p"].n
    worst = 0.0
    for k, it in enumerate(c["its"]):
        Xd, Gd, HSd, HYd, Md = _upload(c, it)
        D, SUM = _nan(B, n + 5), _nan(B, 5 + 3)
        p.lbfgs_direction_batch_device(Gd, HSd, HYd, Md, D, SUM, mem, X=Xd)
        torch.cuda.synchronize()
        if k == 0:
            assert _same_bits(D[:, :n], Gd[:, :n]), "count == 0: D must equal GR bit for bit"
        worst = max(worst, _check_direction(f"{name} B={B} mem={mem} iteration {k}", it, range(B), D, SUM, n))
        assert np.array_equal(Md.cpu().numpy(), it["META"]) and np.isnan(Xd.cpu().numpy()[:, n:]).all()
    print(f"{name} B={B} mem={mem}: direction largest err / gate {worst:.2e}")


@pytest.mark.parametrize("name,B,mem", [("anymal_stairs_gaitopt", 3, 3), ("anymal_trot_2p4s", 37, 5)])
def test_bounds_sources_free_columns_and_garbage_meta(name, B, mem):
    import torch
    c = _direction_case(name, B, mem)
    p, n, lo, up = c["p"], c["p"].n, c["lo"], c["up"]
    it = c["its"][-1]
    Xd, Gd, HSd, HYd, Md = _upload(c, it)
    D0, S0 = _nan(B, n + 5), _nan(B, 8)
    p.lbfgs_direction_batch_device(Gd, HSd, HYd, Md, D0, S0, mem, X=Xd)
    for XL, XU in ((_vec(lo), _vec(up)),                                # the same bounds uploaded: shared, then per problem
                   (_padded(np.tile(lo, (B, 1)), n + 4), _padded(np.tile(up, (B, 1)), n + 4)),
                   (_vec(np.where(lo <= -1e20, -np.inf, lo)), _vec(np.where(up >= 1e20, np.inf, up)))):   # IEEE infinities
        D, S = _nan(B, n + 5), _nan(B, 8)
        p.lbfgs_direction_batch_device(Gd, HSd, HYd, Md, D, S, mem, X=Xd, XL=XL, XU=XU)
        torch.cuda.synchronize()
        assert _same_bits(D, D0) and _same_bits(S, S0), "uploaded bounds differ from the handle's"
    free_it = dict(it)                                                  # X = NULL: the all-free result
    free_it["ld"] = [R.direction(it["GR"][b], it["HS"][b], it["HY"][b], it["META"][b], None, dtype=LD) for b in range(B)]
    free_it["f64"] = [[R.direction(it["GR"][b], it["HS"][b], it["HY"][b], it["META"][b], None, reverse=rev) for b in range(B)]
                      for rev in (False, True)]
    D, S = _nan(B, n + 5), _nan(B, 8)
    p.lbfgs_direction_batch_device(Gd, HSd, HYd, Md, D, S, mem)
    torch.cuda.synchronize()
    assert (S.cpu().numpy()[:, 3] == 0).all() and not _same_bits(D, D0)
    w = _check_direction(f"{name} X = NULL", free_it, range(B), D, S, n)
    print(f"{name} B={B} mem={mem}: all columns free, largest err / gate {w:.2e}")
    bad = it["META"].copy()                                             # garbage {count, next}: an empty history
    rows = [0, B - 1] if B < 4 else [0, 5, 17, B - 1]
    for r, g in zip(rows, ([-7, 99], [mem + 1, 0], [1, mem], [2, -1])):
        bad[r] = g
    D, S = _nan(B, n + 5), _nan(B, 8)
    p.lbfgs_direction_batch_device(Gd, HSd, HYd, _ints(bad), D, S, mem, X=Xd)
    torch.cuda.synchronize()
    for r in set(rows):
        assert _same_bits(D[r, :n], Gd[r, :n]) and S[r, 0].item() == 0.0 and S[r, 1].item() == 1.0, "garbage HMETA must behave as an empty history"
    others = [b for b in range(B) if b not in rows]
    assert _same_bits(D[others], D0[others]) and _same_bits(S[others], S0[others])


@pytest.mark.parametrize("name,B,mem", [("monoped_procedural", 3, 3), ("anymal_trot_2p4s", 37, 5)])
def test_secant_equation_on_the_device(name, B, mem):
    """All columns free and the newest pair used: the direction of GR = y_newest is s_newest."""
    import torch
    c = _direction_case(name, B, mem)
    p, n = c["p"], c["p"].n
    it = c["its"][-1]
    newest = [(int(it["META"][b, 1]) - 1) % mem for b in range(B)]
    Y = np.stack([it["HY"][b, newest[b], :n] for b in range(B)])
    S = np.stack([it["HS"][b, newest[b], :n] for b in range(B)])
    sec = dict(it, GR=Y)
    sec["ld"] = [R.direction(Y[b], it["HS"][b], it["HY"][b], it["META"][b], dtype=LD) for b in range(B)]
    sec["f64"] = [[R.direction(Y[b], it["HS"][b], it["HY"][b], it["META"][b], reverse=rev) for b in range(B)] for rev in (False, True)]
    assert all(1 in d["used"] for d in sec["ld"]), "the newest pair must be used"
    _, _, HSd, HYd, Md = _upload(c, it)
    D, SUM = _nan(B, n + 5), _nan(B, 8)
    p.lbfgs_direction_batch_device(_padded(Y, n + 7), HSd, HYd, Md, D, SUM, mem)
    torch.cuda.synchronize()
    _check_direction(f"{name} secant", sec, range(B), D, SUM, n)
    Dh = D.cpu().numpy()[:, :n]
    worst = 0.0
    for b in range(B):
        e64 = max(float(np.max(np.abs(sec["f64"][o][b]["D"] - S[b]))) for o in (0, 1))
        gate = 8 * max(e64, _gamma(n) * float(np.max(np.abs(S[b]))))
        err = float(np.max(np.abs(Dh[b] - S[b])))
        assert err <= gate, f"{name} problem {b}: H y != s, err {err:.3e} gate {gate:.3e}"
        worst = max(worst, err / gate)
    print(f"{name} B={B} mem={mem}: secant largest err / gate {worst:.2e}")


# ---- determinism and NaN locality ------------------------------------------------------------------------------------
def _run_both(p, mem, Xd, Gd, XNd, GNd, HSd, HYd, Md, stream=None):
    """The update with (Xd -> XNd, Gd -> GNd) on a copy of the history, then the direction at (XNd, GNd): every output."""
    B, n = Xd.shape[0], p.n
    HS, HY, M = HSd.clone(), HYd.clone(), Md.clone()
    US, D, DS = _nan(B, 6), _nan(B, n + 5), _nan(B, 5)
    p.lbfgs_update_batch_device(Xd, XNd, Gd, GNd, HS, HY, M, US, mem, curv_eps=1e-10, stream=stream)
    p.lbfgs_direction_batch_device(GNd, HS, HY, M, D, DS, mem, X=XNd, stream=stream)
    return HS, HY, M, US, D, DS


def test_bits_do_not_depend_on_batch_position_stream_or_run():
    import torch
    B, mem = 37, 3
    c = _direction_case("anymal_trot_2p4s", B, mem)
    p, n, ldh = c["p"], c["p"].n, c["ldh"]
    a, z = c["its"][-2], c["its"][-1]                                   # the last pair of the loop, offered to the history before it
    Xd, Gd, HSd, HYd, Md = _upload(c, a)
    XNd, GNd = _padded(z["X"], n + 2), _padded(z["GR"], n + 1)
    base = _run_both(p, mem, Xd, Gd, XNd, GNd, HSd, HYd, Md)
    torch.cuda.synchronize()
    assert base[3][:, 3].sum().item() > B // 2 and (base[5][:, 0] > 0).any()
    rows = lambda t, idx: t.reshape(B, mem, ldh)[idx].reshape(-1, ldh).contiguous()

    def same(got, idx, what):
        for g, w, hist in zip(got, base, (True, True, False, False, False, False)):
            want = rows(w, idx) if hist else w[idx]
            assert torch.equal(g, want) if g.dtype == torch.int32 else _same_bits(g, want), what
    for b in (0, 17, 36):                                               # alone
        i = torch.tensor([b], device=_dev())
        got = _run_both(p, mem, Xd[b:b + 1], Gd[b:b + 1], XNd[b:b + 1], GNd[b:b + 1], rows(HSd, i), rows(HYd, i), Md[b:b + 1].contiguous())
        torch.cuda.synchronize()
        same(got, i, f"problem {b} alone differs from row {b} of B = {B}")
    perm = torch.roll(torch.arange(B, device=_dev()), 11)               # at another position in the batch
    got = _run_both(p, mem, Xd[perm].contiguous(), Gd[perm].contiguous(), XNd[perm].contiguous(), GNd[perm].contiguous(),
                    rows(HSd, perm), rows(HYd, perm), Md[perm].contiguous())
    torch.cuda.synchronize()
    same(got, perm, "a problem's bits depend on its position in the batch")
    every = torch.arange(B, device=_dev())
    s = torch.cuda.Stream(device=_dev())
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        got = _run_both(p, mem, Xd, Gd, XNd, GNd, HSd, HYd, Md, stream=s)
    s.synchronize()
    same(got, every, "another stream gives other bits")
    got = _run_both(p, mem, Xd, Gd, XNd, GNd, HSd, HYd, Md)
    torch.cuda.synchronize()
    same(got, every, "two runs give different bits")


@pytest.mark.parametrize("name,B,b,mem", [("anymal_trot_2p4s", 37, 11, 3), ("anymal_stairs_gaitopt", 3, 1, 5)])
def test_nan_gradient_stays_in_its_problem(name, B, b, mem):
    import torch
    c = _direction_case(name, B, mem)
    p, n = c["p"], c["p"].n
    it = c["its"][-1]
    Xd, Gd, HSd, HYd, Md = _upload(c, it)
    D0, S0 = _nan(B, n + 5), _nan(B, 8)
    p.lbfgs_direction_batch_device(Gd, HSd, HYd, Md, D0, S0, mem, X=Xd)
    free = it["ld"][b]["free"]
    j = int(np.flatnonzero(free)[len(np.flatnonzero(free)) // 2])
    assert it["ld"][b]["used"]
    Gn = Gd.clone()
    Gn[b, j] = float("nan")
    D, S = _nan(B, n + 5), _nan(B, 8)
    p.lbfgs_direction_batch_device(Gn, HSd, HYd, Md, D, S, mem, X=Xd)
    torch.cuda.synchronize()
    others = [r for r in range(B) if r != b]
    assert _same_bits(D[others], D0[others]) and _same_bits(S[others], S0[others]), "a NaN gradient reached another problem"
    Dh = D.cpu().numpy()[b, :n]
    assert np.isnan(Dh[free]).all(), "a NaN g_j on a free column makes the problem's free columns NaN"
    np.testing.assert_array_equal(_np_bits(Dh[~free]), _np_bits(it["GR"][b][~free]))
    Sh = S.cpu().numpy()[b]
    assert Sh[3] == it["ld"][b]["nheld"] and np.isnan(Sh[2]) and np.isnan(Sh[4]) and np.isnan(Sh[5:]).all()


def test_direction_keeps_the_kept_jacobian():
    B, mem = 37, 3
    c = _direction_case("anymal_trot_2p4s", B, mem)
    _, _, _, vb = _problem("anymal_trot_2p4s")
    p = TowrGpuProblem(config_descs()["anymal_trot_2p4s"], device=0, data=vb)
    n = p.n
    it = c["its"][-1]
    x = it["X"][1]
    v_ref = p.eval_jac_values(x)
    p.eval_g_keep_jac(x)
    Xd, Gd, HSd, HYd, Md = _upload(c, it)
    p.lbfgs_update_batch_device(Xd, Xd, Gd, Gd, HSd, HYd, Md, _nan(B, 6), mem)
    p.lbfgs_direction_batch_device(Gd, HSd, HYd, Md, _nan(B, n), _nan(B, 5), mem, X=Xd)
    v = p.eval_jac_values_kept(x)
    assert np.array_equal(v.view(np.int64), v_ref.view(np.int64))


# ---- the fused entry -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,B", [("anymal_all_costs", 5), ("anymal_stairs_gaitopt_costs", 3)])
def test_fused_entry_is_bit_identical_to_the_separate_calls(name, B):
    """Three consecutive iterations (the first without XPREV) of eval_cost_batch_device (GRAD = GR),
    eval_auglag_batch_device (accumulate), lbfgs_update_batch_device, lbfgs_direction_batch_device and
    step_batch_device against auglag_lbfgs_step_batch_device, at the automatic chunk and at chunks 1 and 2 (a ragged last
    chunk), with batch terrains set."""
    import torch
    gait = name == "anymal_stairs_gaitopt_costs"
    f = F.with_costs(F.anymal_trot(terrain=F.HeightMap.MakeTerrain(F.HeightMap.StairsID), optimize_timings=True) if gait else F.anymal_trot())
    f.params_.enable_stance_tracking = False
    desc = cost_descs()[name]
    assert bytes(f.to_desc()) == bytes(desc)
    p = TowrGpuProblem(desc, device=0, data=f.var_bounds_data())
    n, m, ns, nc, mem = p.n, p.m, desc.n_varsets, desc.n_constraints, 3
    rng = np.random.default_rng(7)
    p.set_batch_terrain(_terrains(name, B, rng))
    x0 = p.initial_x()
    lo, up = p.variable_bounds()                                        # a start inside the box: the steps are the directions'
    X0 = _padded(np.stack([np.clip(x0 + 0.05 * np.random.default_rng(500 + b).standard_normal(n), lo, up) for b in range(B)]), n + 1)
    Ld = _padded(rng.standard_normal((B, m)), m + 3)
    rho, eps = 10.0, 1e-12                                             # (these problems are stiff: sy / yy is about 9e-11)
    ldh = n + 2
    fvec = lambda: torch.full((B,), float("nan"), dtype=torch.float64, device=_dev())
    G0 = _nan(B, n)                                                     # step lengths that move x by a few 1e-3 at most in the first step
    p.eval_cost_batch_device(X0, fvec(), GRAD=G0)
    p.eval_auglag_batch_device(X0, _nan(B, 4 + nc), G0, LAM=Ld, rho=rho, accumulate=True)
    al = _vec(rng.uniform(1e-3, 5e-3, B) / np.abs(G0.cpu().numpy()).max(axis=1))

    def separate():
        HS, HY, M = _nan(B * mem, ldh), _nan(B * mem, ldh), _ints(np.zeros((B, 2)))
        X, Xprev, Gprev, out = X0, None, None, []
        for k in range(3):
            Fk, GR, RS, US, D, DS = fvec(), _nan(B, n + 3), _nan(B, 4 + nc + 3), _nan(B, 6 + 1), _nan(B, n + 4), _nan(B, 5 + 2)
            XP, SS = _nan(B, n + 5), _nan(B, 5 + ns + 3)
            p.eval_cost_batch_device(X, Fk, GRAD=GR)
            p.eval_auglag_batch_device(X, RS, GR, LAM=Ld, rho=rho, accumulate=True)
            if Xprev is not None:
                p.lbfgs_update_batch_device(Xprev, X, Gprev, GR, HS, HY, M, US, mem, curv_eps=eps)
            p.lbfgs_direction_batch_device(GR, HS, HY, M, D, DS, mem, X=X)
            p.step_batch_device(X, D, SS, XP=XP, alpha=al)
            torch.cuda.synchronize()
            out.append(dict(F=Fk, GR=GR, RS=RS, US=US, DS=DS, XP=XP, SS=SS, HS=HS.clone(), HY=HY.clone(), M=M.clone()))
            Xprev, Gprev, X = X, GR, XP
        return out

    def fused(with_f):
        HS, HY, M = _nan(B * mem, ldh), _nan(B * mem, ldh), _ints(np.zeros((B, 2)))
        X, Xprev, Gprev, out = X0, None, None, []
        for k in range(3):
            Fk, GR, RS, US, DS = fvec(), _nan(B, n + 3), _nan(B, 4 + nc + 3), _nan(B, 6 + 1), _nan(B, 5 + 2)
            XP, SS = _nan(B, n + 5), _nan(B, 5 + ns + 3)
            p.auglag_lbfgs_step_batch_device(X, GR, XP, SS, RS, DS, HS, HY, M, mem, XPREV=Xprev, GRPREV=Gprev,
                                             USUM=US if Xprev is not None else None, curv_eps=eps, LAM=Ld, rho=rho, alpha=al,
                                             F=Fk if with_f else None)
            torch.cuda.synchronize()
            out.append(dict(F=Fk, GR=GR, RS=RS, US=US, DS=DS, XP=XP, SS=SS, HS=HS.clone(), HY=HY.clone(), M=M.clone()))
            Xprev, Gprev, X = X, GR, XP
        return out

    want = separate()
    assert np.isnan(want[0]["US"].cpu().numpy()).all(), "no update in the first iteration: USUM is not written"
    assert np.isfinite(want[2]["GR"].cpu().numpy()[:, :n]).all() and np.isfinite(want[2]["XP"].cpu().numpy()[:, :n]).all()
    print(f"{name}: pairs accepted per problem {want[2]['M'].cpu().numpy()[:, 0].tolist()}, used {want[2]['DS'][:, 0].tolist()}")
    assert (want[2]["M"][:, 0] > 0).any() and (want[2]["DS"][:, 0] > 0).any(), "the history stayed empty: the comparison would show nothing"
    try:
        for chunk in (0, 1, 2):
            for with_f in (True, False):
                p.set_products_chunk(chunk)
                got = fused(with_f)
                for k in range(3):
                    for key in want[k]:
                        if key == "F" and not with_f:
                            continue
                        a, b = got[k][key], want[k][key]
                        eq = torch.equal(a, b) if a.dtype == torch.int32 else _same_bits(a, b)
                        assert eq, f"{name} chunk {chunk} iteration {k}: {key}"
    finally:
        p.set_products_chunk(0)


def test_fused_entry_keeps_the_kept_jacobian():
    B, mem = 37, 3
    c = _direction_case("anymal_trot_2p4s", B, mem)
    _, _, _, vb = _problem("anymal_trot_2p4s")
    desc = config_descs()["anymal_trot_2p4s"]
    p = TowrGpuProblem(desc, device=0, data=vb)
    n = p.n
    it = c["its"][-1]
    x = it["X"][1]
    v_ref = p.eval_jac_values(x)
    p.eval_g_keep_jac(x)
    Xd, _, HSd, HYd, Md = _upload(c, it)
    p.auglag_lbfgs_step_batch_device(Xd, _nan(B, n), _nan(B, n), _nan(B, 5 + desc.n_varsets), _nan(B, 4 + desc.n_constraints),
                                     _nan(B, 5), HSd, HYd, Md, mem, rho=2.0, alpha=1e-3)
    v = p.eval_jac_values_kept(x)
    assert np.array_equal(v.view(np.int64), v_ref.view(np.int64))
