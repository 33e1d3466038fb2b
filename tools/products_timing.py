"""Jacobian-product timings on the GPU box (tool, not product): per call, on one box in one session,
  (a) eval_batch_device (g + J) alone — the yardstick on that box;
  (b) jac_vec_batch_device; (c) jac_tvec_batch_device (overwrite);
  (d) eval_products_batch_device (g, J^T lam and J p) at the automatic chunk and at chunks of 128, 512 and B;
  (e) residual_batch_device (summary and lam+, the handle's bounds): rate = 8 (3 m + 4 + n_constraints) B / time, the
      bytes of G + LAM + LAMP + SUM, beside (f) a device-to-device torch copy moving the same bytes (half read, half
      written);
  (g) eval_auglag_batch_device (g and lam+ in scratch) beside the sum of its parts a + e + c from the same session;
  (h) step_batch_device (XP and the summary, the handle's bounds, scalar step length): rate = 8 (3 n + 5 + n_varsets)
      B / time, the bytes of X + D + XP + SUM, beside (i) a device-to-device torch copy moving the same bytes,
for ANYmal trot at B = 4096 and ANYmal stairs with phase-duration optimisation at B = 1024. Each product's achieved
rate is 8 (nnz + n + m) B / time, printed against the 8 TB/s peak. HIP events around windows of REPS calls after a
warm-up of every shape; the windows alternate between the variants and the median and the spread over ROUNDS are
printed. usage: python tools/products_timing.py [anymal|gait|all]"""
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from towr2025_amd import TowrGpuProblem, _capi as capi  # noqa: E402
from towr2025_amd import formulation as F  # noqa: E402

REPS = int(os.environ.get("REPS", "20"))
ROUNDS = int(os.environ.get("ROUNDS", "5"))
PEAK = 8.0e12


def batch_x(p, B, seed=20261019):
    """x0 + noise per variable (phase durations: +-3 % multiplicative), as bench.make_batch perturbs them."""
    rng = np.random.default_rng(seed)
    x0 = p.initial_x()
    sched = np.zeros(p.n, dtype=bool)
    for kind, _ee, c0, n in p.varset_info():
        if kind == capi.VAR_EE_SCHEDULE:
            sched[c0:c0 + n] = True
    X = x0 + 0.02 * rng.standard_normal((B, p.n))
    X[:, sched] = x0[sched] * (1.0 + 0.03 * rng.standard_normal((B, int(sched.sum()))))
    return X


def run(name, f, B):
    dev = torch.device("cuda", 0)
    f.params_.enable_stance_tracking = False   # the start / goal variable bounds (the step kernel's box)
    p = TowrGpuProblem(f.to_desc(), device=0, data=f.var_bounds_data())
    stream = torch.cuda.Stream(dev)
    torch.cuda.set_stream(stream)
    ld = lambda k: (k + 15) // 16 * 16
    X = torch.from_numpy(batch_x(p, B)).to(dev)
    G = torch.empty((B, ld(p.m)), dtype=torch.float64, device=dev)
    V = torch.empty((B, ld(p.nnz)), dtype=torch.float64, device=dev)
    P = torch.randn((B, ld(p.n)), dtype=torch.float64, device=dev)
    LAM = torch.randn((B, ld(p.m)), dtype=torch.float64, device=dev)
    Y, Z = torch.empty_like(LAM), torch.empty_like(P)
    ns = p.desc.n_constraints
    LAMP, SUM = torch.empty_like(LAM), torch.empty((B, ld(4 + ns)), dtype=torch.float64, device=dev)
    bytes_res = 8 * (3 * p.m + 4 + ns) * B
    src = torch.randn(bytes_res // 16, dtype=torch.float64, device=dev)
    dst = torch.empty_like(src)
    rho = 10.0
    nv = p.desc.n_varsets
    XP, SSUM = torch.empty_like(P), torch.empty((B, ld(5 + nv)), dtype=torch.float64, device=dev)
    Xs = torch.zeros_like(P)
    Xs[:, :p.n] = X
    bytes_step = 8 * (3 * p.n + 5 + nv) * B
    src_s = torch.randn(bytes_step // 16, dtype=torch.float64, device=dev)
    dst_s = torch.empty_like(src_s)

    def fused(chunk):
        def f():
            p.set_products_chunk(chunk)
            p.eval_products_batch_device(X, G=G, LAM=LAM, Z=Z, P=P, Y=Y, stream=stream)
        return f
    variants = [("a eval_batch_device", lambda: p.eval_batch_device(X, G, V, stream=stream)),
                ("b jac_vec", lambda: p.jac_vec_batch_device(V, P, Y, stream=stream)),
                ("c jac_tvec", lambda: p.jac_tvec_batch_device(V, LAM, Z, stream=stream)),
                ("d fused chunk auto", fused(0)), ("d fused chunk 128", fused(128)), ("d fused chunk 512", fused(512)),
                (f"d fused chunk B={B}", fused(B)),
                ("e residual", lambda: p.residual_batch_device(G, SUM, LAM=LAM, rho=rho, LAMP=LAMP, stream=stream)),
                ("f copy, same bytes", lambda: dst.copy_(src)),
                ("g auglag fused auto", lambda: (p.set_products_chunk(0),
                                                 p.eval_auglag_batch_device(X, SUM, Z, LAM=LAM, rho=rho, stream=stream))),
                ("h step", lambda: p.step_batch_device(Xs, P, SSUM, XP=XP, alpha=0.01, stream=stream)),
                ("i copy, step's bytes", lambda: dst_s.copy_(src_s))]
    for _, fn in variants:   # warm-up: every shape, the tables' upload, the scratch at its largest
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k, _ in variants}
    for _ in range(ROUNDS):
        for k, fn in variants:
            a, z = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(stream)
            for _ in range(REPS):
                fn()
            z.record(stream)
            torch.cuda.synchronize()
            times[k].append(a.elapsed_time(z) / REPS)
    bytes_prod = 8 * (p.nnz + p.n + p.m) * B
    print(f"{name}: B={B} n={p.n} m={p.m} nnz={p.nnz}  product bytes {bytes_prod / 1e9:.3f} GB, V {8 * p.nnz * B / 2**30:.2f} GiB", flush=True)
    for k, _ in variants:
        t = times[k]
        med = statistics.median(t)
        nbytes = bytes_prod if k[0] in "bc" else bytes_res if k[0] in "ef" else bytes_step if k[0] in "hi" else 0
        rate = f"  {nbytes / (med * 1e-3) / 1e12:.2f} TB/s = {100 * nbytes / (med * 1e-3) / PEAK:.0f} % of 8 TB/s" if nbytes else ""
        print(f"  {k:22s} {med:.4f} ms  (min {min(t):.4f} max {max(t):.4f}){rate}", flush=True)
    parts = sum(statistics.median(times[k]) for k in ("a eval_batch_device", "e residual", "c jac_tvec"))
    print(f"  residual bytes {bytes_res / 1e9:.3f} GB; auglag parts a + e + c {parts:.4f} ms, fused / parts "
          f"{statistics.median(times['g auglag fused auto']) / parts:.3f}", flush=True)
    p.set_products_chunk(0)


if __name__ == "__main__":
    which = sys.argv[1] if len(sys.argv) > 1 else "all"
    if which in ("anymal", "all"):
        run("anymal_trot", F.anymal_trot(), int(os.environ.get("B", "4096")))
    if which in ("gait", "all"):
        run("anymal_stairs_gaitopt", F.anymal_trot(terrain=F.HeightMap.MakeTerrain(F.HeightMap.StairsID), optimize_timings=True),
            int(os.environ.get("B_GAIT", "1024")))
