"""Solve-to-completion timings on the GPU box (tool, not product): towr_gpu_alsolve_solve_batch_device with and without
compaction, beside the hand-written iterate-and-poll loop it replaces, on one box in one session.

ANYmal trot (anymal_trot_2p4s, B default 1024) or the procedural monoped of the short-solve tests (B_MONOPED default
4096, whose starts freeze after 9 .. 100+ iterations), from the starts x0 + 0.05 randn(SEED + b), TOWR_SOLVE_GN_TILED with
wrows = B, SOLVE_PAR of the short-solve tests, damping MU (default 1e-6), at most MAX_ITERS iterations (default 120).
Per check_every K in KS (default 4,16), alternated within every round:
  (n) alsolve_solve(compact = 0);
  (c) alsolve_solve(compact = 1);
  (h) the hand loop: alsolve_gn_tiled_iterate(iters = K) through the C-ABI, the phase words copied to the host, repeated
      until no problem is active or MAX_ITERS is reached — what a caller wrote before the driver existed;
and on a batch of B copies of start 0, where every problem freezes in the same round and compaction has nothing to gain:
  (n1), (c1) as (n), (c).
A solve is timed by the host clock from a synchronised device to the return of the call (the driver synchronises before
it returns; the hand loop ends in a copy to the host); the state is restored and alsolve_init run before every solve,
outside the window. Printed: the median and the spread over ROUNDS per variant, iters_run, problem_iters, the phase counts,
the ratio of times beside the ratio of problem_iters, and whether compact = 1 and compact = 0 left the same bits in X.
Environment: FEASIBLE=1 gives the ANYmal goal the standing height -nominal_stance[0][2] (the default goal z = 0 has no
feasible point); STOP=1 runs the driver through towr_gpu_alsolve_solve_ex_batch_device with the stop rule's
example parameters (ACC_ETA 1e-6, ACC_OMEGA 1e-4, ACC_ITERS 15, INFEAS_KEEP 0.99, INFEAS_RHO 1e4) and leaves out the hand
loop, whose iterate entry has no rule; MAX_INNER overrides SOLVE_PAR's 200.
`stopcost`: the rule's own cost — one round of STOPCOST_ITERS (default 20) iterations on all B ANYmal problems (default
4096), compact = 0, with and without the rule, alternated, per iteration.
QUEUE=1: towr_gpu_alsolve_solve_queue_batch_device (queue_run below): N starts (N_MONOPED default 16384, N default 2048
for ANYmal) through B slots (B_MONOPED 4096, B 512) with K = the first of KS, beside N / B successive compact = 1 solves of B
and one compact = 1 solve of all N (ALL_AT_ONCE=0 leaves it out); STOP, FEASIBLE and MAX_ITERS as above.
PROBE=T: the probe stage (towr_gpu_alsolve_solve_probe_batch_device). Per K two more variants, alternated with
the others: (s) compact = 1 with shrink = PROBE_SHRINK (default 0.5) and no probes, (p) the same with T probes; the frozen
count of every variant is printed, so the gain of the finer ladder and of the probes can be told apart. ONLY=c,p runs only
the variants with those letters (n, c, h, s, p, n1, c1). `probecost` / `probecost_monoped`: the stage's own cost, as
`stopcost`: one round of STOPCOST_ITERS iterations on all B problems (B / B_MONOPED, default 4096), compact = 0,
shrink = PROBE_SHRINK, with and without PROBE (default 4) probes, alternated, per iteration.
LAZY=1: the lazy GN loop (towr_gpu_alsolve_solve_lazy_batch_device). Every compact = 1 variant (c, s, p) gets a
twin (cl, sl, pl) that runs the same solve through the lazy entry, alternated with the others; printed per pair: the ratio
of times and directions / problem_iters, the share of problem iterations whose direction was computed. The tool asserts
that a twin's report and persistent arrays (X, GR, LAM, RHO, SCAL, ISTATE, HS, HY, HMETA, D, ALPHA) are bit-equal to its
eager variant's.
usage: python tools/solve_timing.py [anymal|monoped|all|stopcost|probecost|probecost_monoped]"""
import ctypes as C
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from towr2025_amd import AlSolveState, TowrGpuProblem, _capi as capi, alsolve_params, alsolve_stop_params, gn_params  # noqa: E402
from towr2025_amd import formulation as F  # noqa: E402

ROUNDS = int(os.environ.get("ROUNDS", "3"))
MAX_ITERS = int(os.environ.get("MAX_ITERS", "120"))
KS = [int(k) for k in os.environ.get("KS", "4,16").split(",")]
MU = float(os.environ.get("MU", "1e-6"))
SEED = int(os.environ.get("SEED", "900"))
SOLVE_PAR = dict(mem=8, shrink=0.1, rho0=10.0, curv_eps=1e-14, max_inner=int(os.environ.get("MAX_INNER", "200")), alpha_min=1e-16)
FEASIBLE = os.environ.get("FEASIBLE", "0") == "1"
STOP = os.environ.get("STOP", "0") == "1"
PROBE = int(os.environ.get("PROBE", "0"))
PROBE_SHRINK = float(os.environ.get("PROBE_SHRINK", "0.5"))
ONLY = [v for v in os.environ.get("ONLY", "").split(",") if v]
LAZY = os.environ.get("LAZY", "0") == "1"
PERSISTENT = ("X", "GR", "LAM", "RHO", "SCAL", "ISTATE", "HS", "HY", "HMETA", "D", "ALPHA")


def stop_params():
    e = os.environ.get
    return alsolve_stop_params(acc_eta=float(e("ACC_ETA", "1e-6")), acc_omega=float(e("ACC_OMEGA", "1e-4")),
                               acc_iters=int(e("ACC_ITERS", "15")), infeas_keep=float(e("INFEAS_KEEP", "0.99")),
                               infeas_rho=float(e("INFEAS_RHO", "1e4")))


def anymal():
    f = F.anymal_trot(goal=(2.1, 0.0, -F.RobotModel(F.RobotModel.Anymal).kinematic_model.nominal_stance[0][2])) if FEASIBLE \
        else F.anymal_trot()
    f.params_.enable_stance_tracking = False
    return TowrGpuProblem(f.to_desc(), device=0, data=f.var_bounds_data())


def run(title, p, B):
    dev = torch.device("cuda", 0)
    stream = torch.cuda.Stream(dev)
    torch.cuda.set_stream(stream)
    n, mem = p.n, SOLVE_PAR["mem"]
    par, gn = alsolve_params(**SOLVE_PAR), gn_params(mu=MU)
    x0 = p.initial_x()
    starts = np.stack([x0 + 0.05 * np.random.default_rng(SEED + b).standard_normal(n) for b in range(B)])
    X0 = {"spread": torch.from_numpy(starts).to(dev), "same": torch.from_numpy(np.repeat(starts[:1], B, axis=0)).to(dev)}
    st = AlSolveState.allocate(p, B, mem)
    DC, GS = torch.zeros_like(st.X), torch.zeros((B, 8), dtype=torch.float64, device=dev)
    W = torch.empty((B, p.gn_tile_info()["ldw_min"]), dtype=torch.float64, device=dev)
    LOG = torch.zeros(8 + 2 * B, dtype=torch.int32, device=dev)
    sp = C.c_void_p(stream.cuda_stream)
    c = p._alsolve_state(st, par)

    def restart(which):
        st.X.copy_(X0[which])
        st.LAM.zero_()
        if LAZY:   # (the slots a solve does not write would keep the previous variant's pairs: compared below)
            st.HS.zero_()
            st.HY.zero_()
        p.alsolve_init(par, st, stream=stream)
        torch.cuda.synchronize()

    stop = stop_params() if STOP else None
    par_fine = alsolve_params(**{**SOLVE_PAR, "shrink": PROBE_SHRINK})
    PSUM = torch.zeros((B, 8), dtype=torch.float64, device=dev)

    VERDICT, NDIR = (torch.zeros(B, dtype=torch.int32, device=dev) for _ in range(2))

    def lazy_kw(lazy):   # (NDIR counts from zero in every solve; the memset is inside the window)
        if lazy:
            NDIR.zero_()
        return dict(lazy=True, VERDICT=VERDICT, NDIR=NDIR) if lazy else {}

    def probed(K, T, lazy=False):   # (T = 0: the finer ladder alone)
        return p.alsolve_solve(par_fine, st, method=capi.SOLVE_GN_TILED, gn=gn, DC=DC, GSUM=GS, W=W, wrows=B, max_iters=MAX_ITERS,
                               check_every=K, compact=True, LOG=LOG, stream=stream, stop=stop, probes=T or None,
                               PSUM=PSUM if T else None, **lazy_kw(lazy))

    def driver(K, compact, lazy=False):
        return p.alsolve_solve(par, st, method=capi.SOLVE_GN_TILED, gn=gn, DC=DC, GSUM=GS, W=W, wrows=B, max_iters=MAX_ITERS,
                               check_every=K, compact=compact, LOG=LOG, stream=stream, stop=stop, **lazy_kw(lazy))

    def hand(K):
        phases = st.ISTATE.view(B, 4)[:, 0]
        done, rounds = 0, 0
        while done < MAX_ITERS:
            k = min(K, MAX_ITERS - done)
            p._check(p._lib.towr_gpu_alsolve_gn_tiled_iterate_batch_device(
                p._h, B, k, C.byref(par), C.byref(c), C.byref(gn), C.c_void_p(DC.data_ptr()), C.c_void_p(GS.data_ptr()), GS.stride(0),
                C.c_void_p(W.data_ptr()), W.stride(0), B, None, None, 0, None, None, 0, sp))
            done, rounds = done + k, rounds + 1
            ph = phases.cpu()
            if not ((ph == 0) | (ph == 1)).any():
                break
        counts = [int((ph == v).sum()) for v in range(5)]
        return dict(rounds=rounds, iters_run=done, problem_iters=B * done, n_phase=counts + [B - sum(counts)])

    variants = []
    for K in KS:
        variants += [(f"n  K={K:<2d} compact=0", "spread", lambda K=K: driver(K, False)),
                     (f"c  K={K:<2d} compact=1", "spread", lambda K=K: driver(K, True))]
        if not STOP:
            variants += [(f"h  K={K:<2d} hand loop", "spread", lambda K=K: hand(K))]
        if PROBE:
            variants += [(f"s  K={K:<2d} compact=1 shrink={PROBE_SHRINK:g}", "spread", lambda K=K: probed(K, 0)),
                         (f"p  K={K:<2d} compact=1 shrink={PROBE_SHRINK:g} probes={PROBE}", "spread", lambda K=K: probed(K, PROBE))]
        if LAZY:
            variants += [(f"cl K={K:<2d} compact=1 lazy", "spread", lambda K=K: driver(K, True, True))]
            if PROBE:
                variants += [(f"sl K={K:<2d} compact=1 shrink={PROBE_SHRINK:g} lazy", "spread", lambda K=K: probed(K, 0, True)),
                             (f"pl K={K:<2d} compact=1 shrink={PROBE_SHRINK:g} probes={PROBE} lazy", "spread",
                              lambda K=K: probed(K, PROBE, True))]
    variants += [(f"n1 K={KS[0]:<2d} compact=0, one start", "same", lambda: driver(KS[0], False)),
                 (f"c1 K={KS[0]:<2d} compact=1, one start", "same", lambda: driver(KS[0], True))]
    if ONLY:
        variants = [v for v in variants if v[0].split()[0] in ONLY]
    # warm-up: every variant once (the tables' upload, the scratch, the page-locked HEAD); the bits of X kept per variant
    bits, reports, kept = {}, {}, {}
    for name, which, fn in variants:
        restart(which)
        reports[name] = fn()
        torch.cuda.synchronize()
        bits[name] = st.X.clone()
        if LAZY:
            kept[name] = {k: getattr(st, k).clone() for k in PERSISTENT}
    times = {name: [] for name, _, _ in variants}
    for _ in range(ROUNDS):
        for name, which, fn in variants:
            restart(which)
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            times[name].append(1e3 * (time.perf_counter() - t0))
    codes = torch.bincount(GS[:, 5].to(torch.int64).clamp(0, 3), minlength=4).tolist()
    print(f"{title}: B={B} n={p.n} m={p.m} nnz={p.nnz} mu={MU} max_iters={MAX_ITERS} max_inner={SOLVE_PAR['max_inner']} "
          f"rounds={ROUNDS} stop={'on' if STOP else 'off'}; direction codes 0..3 of "
          f"the last solve {codes}", flush=True)
    med = {}
    for name, _, _ in variants:
        t, r = times[name], reports[name]
        med[name] = statistics.median(t)
        print(f"  {name:32s} {med[name]:9.2f} ms  (min {min(t):.2f} max {max(t):.2f})  rounds {r['rounds']} iters_run {r['iters_run']} "
              f"problem_iters {r['problem_iters']} frozen {B - r['n_phase'][0] - r['n_phase'][1]} of {B} "
              f"phases 0..4,other {r['n_phase']}"
              + (f" acceptable {r['n_acceptable']} infeasible {r['n_infeasible']}" if STOP else ""), flush=True)
    if LAZY:
        for K in KS:
            for e in ("c", "s", "p"):
                a = next((v for v in times if v.startswith(f"{e}  K={K:<2d} ")), None)
                b = next((v for v in times if v.startswith(f"{e}l K={K:<2d} ")), None)
                if a is None or b is None:
                    continue
                ra, rb = reports[a], dict(reports[b])
                directions = rb.pop("directions")
                assert ra == rb, f"{b}: the report differs from the eager variant's: {rb} against {ra}"
                for k in PERSISTENT:
                    x, y = kept[a][k], kept[b][k]
                    same = torch.equal(x, y) if x.dtype == torch.int32 else torch.equal(x.view(torch.int64), y.view(torch.int64))
                    assert same, f"{b}: {k} differs from the eager variant's"
                print(f"  K={K}: time {e}l / {e} {med[b] / med[a]:.3f}; directions {directions} of problem_iters {rb['problem_iters']} = "
                      f"{directions / max(rb['problem_iters'], 1):.3f}; persistent arrays and report bit-equal: True", flush=True)
    if ONLY:                                   # (the ratios below need every variant)
        return
    for K in KS:
        nn, cc, hh = (f"{v}  K={K:<2d} {w}" for v, w in (("n", "compact=0"), ("c", "compact=1"), ("h", "hand loop")))
        if STOP:
            print(f"  K={K}: time c / n {med[cc] / med[nn]:.3f} vs problem_iters c / n "
                  f"{reports[cc]['problem_iters'] / max(reports[nn]['problem_iters'], 1):.3f}; X bit-equal c vs n: "
                  f"{torch.equal(bits[cc].view(torch.int64), bits[nn].view(torch.int64))}", flush=True)
            continue
        print(f"  K={K}: time c / n {med[cc] / med[nn]:.3f} vs problem_iters c / n "
              f"{reports[cc]['problem_iters'] / max(reports[nn]['problem_iters'], 1):.3f}; driver n / hand loop {med[nn] / med[hh]:.3f}; "
              f"X bit-equal c vs n: {torch.equal(bits[cc].view(torch.int64), bits[nn].view(torch.int64))}, n vs hand: "
              f"{torch.equal(bits[nn].view(torch.int64), bits[hh].view(torch.int64))}", flush=True)
    n1, c1 = (f"{v} K={KS[0]:<2d} compact={k}, one start" for v, k in (("n1", 0), ("c1", 1)))
    print(f"  one start: time c1 / n1 {med[c1] / med[n1]:.3f}; X bit-equal: "
          f"{torch.equal(bits[c1].view(torch.int64), bits[n1].view(torch.int64))}", flush=True)


def stop_cost(p, B):
    """One round of `iters` iterations on the whole batch with and without the rule, alternated."""
    dev = torch.device("cuda", 0)
    stream = torch.cuda.Stream(dev)
    torch.cuda.set_stream(stream)
    n, mem, iters = p.n, SOLVE_PAR["mem"], int(os.environ.get("STOPCOST_ITERS", "20"))
    par, gn, stop = alsolve_params(**SOLVE_PAR), gn_params(mu=MU), stop_params()
    x0 = p.initial_x()
    X0 = torch.from_numpy(np.stack([x0 + 0.05 * np.random.default_rng(SEED + b).standard_normal(n) for b in range(B)])).to(dev)
    st = AlSolveState.allocate(p, B, mem)
    DC, GS = torch.zeros_like(st.X), torch.zeros((B, 8), dtype=torch.float64, device=dev)
    W = torch.empty((B, p.gn_tile_info()["ldw_min"]), dtype=torch.float64, device=dev)
    LOG = torch.zeros(8 + 2 * B, dtype=torch.int32, device=dev)
    times = {"without": [], "with": []}
    for r in range(ROUNDS + 1):               # (round 0: warm-up)
        for name, s in (("without", None), ("with", stop)):
            st.X.copy_(X0)
            st.LAM.zero_()
            p.alsolve_init(par, st, stream=stream)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            p.alsolve_solve(par, st, method=capi.SOLVE_GN_TILED, gn=gn, DC=DC, GSUM=GS, W=W, wrows=B, max_iters=iters,
                            check_every=iters, compact=False, LOG=LOG, stream=stream, stop=s)
            torch.cuda.synchronize()
            if r:
                times[name].append(1e3 * (time.perf_counter() - t0) / iters)
    a, b = statistics.median(times["without"]), statistics.median(times["with"])
    print(f"stop rule's cost: anymal B={B}, one round of {iters} iterations, ms per iteration: without {a:.4f} "
          f"(min {min(times['without']):.4f} max {max(times['without']):.4f}), with {b:.4f} (min {min(times['with']):.4f} max "
          f"{max(times['with']):.4f}), difference {1e3 * (b - a):.1f} us", flush=True)


def probe_cost(title, p, B):
    """One round of `iters` iterations on the whole batch with and without the probe stage, alternated (stop_cost's shape)."""
    dev = torch.device("cuda", 0)
    stream = torch.cuda.Stream(dev)
    torch.cuda.set_stream(stream)
    n, mem, iters, T = p.n, SOLVE_PAR["mem"], int(os.environ.get("STOPCOST_ITERS", "20")), PROBE or 4
    par, gn = alsolve_params(**{**SOLVE_PAR, "shrink": PROBE_SHRINK}), gn_params(mu=MU)
    x0 = p.initial_x()
    X0 = torch.from_numpy(np.stack([x0 + 0.05 * np.random.default_rng(SEED + b).standard_normal(n) for b in range(B)])).to(dev)
    st = AlSolveState.allocate(p, B, mem)
    DC, GS = torch.zeros_like(st.X), torch.zeros((B, 8), dtype=torch.float64, device=dev)
    W = torch.empty((B, p.gn_tile_info()["ldw_min"]), dtype=torch.float64, device=dev)
    LOG = torch.zeros(8 + 2 * B, dtype=torch.int32, device=dev)
    PSUM = torch.zeros((B, 8), dtype=torch.float64, device=dev)
    times = {"without": [], "with": []}
    for r in range(ROUNDS + 1):               # (round 0: warm-up)
        for name, probes in (("without", None), ("with", T)):
            st.X.copy_(X0)
            st.LAM.zero_()
            p.alsolve_init(par, st, stream=stream)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            p.alsolve_solve(par, st, method=capi.SOLVE_GN_TILED, gn=gn, DC=DC, GSUM=GS, W=W, wrows=B, max_iters=iters,
                            check_every=iters, compact=False, LOG=LOG, stream=stream, probes=probes, PSUM=PSUM if probes else None)
            torch.cuda.synchronize()
            if r:
                times[name].append(1e3 * (time.perf_counter() - t0) / iters)
    a, b = statistics.median(times["without"]), statistics.median(times["with"])
    print(f"probe stage's cost: {title} B={B} T={T} shrink={PROBE_SHRINK:g}, one round of {iters} iterations, ms per iteration: "
          f"without {a:.4f} (min {min(times['without']):.4f} max {max(times['without']):.4f}), with {b:.4f} (min "
          f"{min(times['with']):.4f} max {max(times['with']):.4f}), ratio {b / a:.3f}", flush=True)


def queue_run(title, p, N, B, K):
    """QUEUE=1: N starts through B slots (q) beside what the solve entry can do in the same memory, N / B successive
    compact = 1 solves of B starts each (s), and beside one compact = 1 solve of all N where its state fits (a); and (q0, s0)
    a run of 2 K iterations on B starts, where nothing freezes, for the queue's overhead per round. Every window holds the
    whole job from the starts on the device to the results on the device: the copies in, alsolve_init, the solve, the copies
    out."""
    dev = torch.device("cuda", 0)
    stream = torch.cuda.Stream(dev)
    torch.cuda.set_stream(stream)
    n, m, mem = p.n, p.m, SOLVE_PAR["mem"]
    par, gn = alsolve_params(**SOLVE_PAR), gn_params(mu=MU)
    stop = stop_params() if STOP else None
    x0 = p.initial_x()
    X0 = torch.from_numpy(np.stack([x0 + 0.05 * np.random.default_rng(SEED + b).standard_normal(n) for b in range(N)])).to(dev)
    ldw = p.gn_tile_info()["ldw_min"]

    def slots(rows):
        st = AlSolveState.allocate(p, rows, mem)
        return dict(st=st, DC=torch.zeros_like(st.X), GS=torch.zeros((rows, 8), dtype=torch.float64, device=dev),
                    W=torch.empty((rows, ldw), dtype=torch.float64, device=dev),
                    LOG=torch.zeros(8 + 2 * rows, dtype=torch.int32, device=dev))

    def outputs():
        z = lambda *s: torch.zeros(s, dtype=torch.float64, device=dev)
        i = lambda k: torch.zeros(k, dtype=torch.int32, device=dev)
        return dict(X_OUT=z(N, n), LAM_OUT=z(N, m), RHO_OUT=z(N), SCAL_OUT=z(N, 8), ISTATE_OUT=i(4 * N), ITERS_OUT=i(N))

    sB = slots(B)
    out_q, out_s, out_a = outputs(), outputs(), outputs()
    book = dict(ID=torch.zeros(B, dtype=torch.int32, device=dev), AGE=torch.zeros(B, dtype=torch.int32, device=dev),
                KEY=torch.zeros(4 * B, dtype=torch.int32, device=dev))

    def queue(count=N, M=MAX_ITERS):
        r = p.alsolve_solve_queue(par, sB["st"], X0[:count], method=capi.SOLVE_GN_TILED, gn=gn, DC=sB["DC"], GSUM=sB["GS"], W=sB["W"],
                                  wrows=B, max_iters=M, check_every=K, LOG=sB["LOG"], stream=stream, stop=stop,
                                  out={k: t[:count * (4 if k == "ISTATE_OUT" else 1)] for k, t in out_q.items()}, **book)
        return {k: r[k] for k in ("rounds", "iters_run", "problem_iters", "n_phase")}

    def solve(s, lo, hi, out, M=MAX_ITERS):
        st = s["st"]
        st.X[:hi - lo].copy_(X0[lo:hi])
        st.LAM.zero_()
        p.alsolve_init(par, st, stream=stream)
        r = p.alsolve_solve(par, st, method=capi.SOLVE_GN_TILED, gn=gn, DC=s["DC"], GSUM=s["GS"], W=s["W"], wrows=st.B, max_iters=M,
                            check_every=K, compact=True, LOG=s["LOG"], stream=stream, stop=stop, ex=True)
        out["X_OUT"][lo:hi].copy_(st.X)
        out["LAM_OUT"][lo:hi].copy_(st.LAM)
        out["RHO_OUT"][lo:hi].copy_(st.RHO)
        out["SCAL_OUT"][lo:hi].copy_(st.SCAL)
        out["ISTATE_OUT"][4 * lo:4 * hi].copy_(st.ISTATE)
        return r

    def successive():
        tot = dict(rounds=0, iters_run=0, problem_iters=0, n_phase=[0] * 6)
        for lo in range(0, N, B):
            r = solve(sB, lo, lo + B, out_s)
            tot = dict(rounds=tot["rounds"] + r["rounds"], iters_run=tot["iters_run"] + r["iters_run"],
                       problem_iters=tot["problem_iters"] + r["problem_iters"],
                       n_phase=[a + b for a, b in zip(tot["n_phase"], r["n_phase"])])
        return tot

    assert N % B == 0, "N must be a multiple of B"
    variants = [(f"q  queue N={N} through B={B}", queue), (f"s  {N // B} solves of B={B}", successive)]
    if os.environ.get("ALL_AT_ONCE", "1") == "1":
        try:
            sN = slots(N)
            variants.append((f"a  one solve of N={N}", lambda: solve(sN, 0, N, out_a)))
        except RuntimeError as e:           # (the state of all N does not fit)
            print(f"  one solve of N={N}: not run ({str(e).splitlines()[0]})", flush=True)
    variants += [(f"q0 queue N=B={B}, {2 * K} iterations", lambda: queue(B, 2 * K)),
                 (f"s0 solve B={B}, {2 * K} iterations", lambda: solve(sB, 0, B, out_s, 2 * K))]
    reports, times = {}, {name: [] for name, _ in variants}
    same = None
    for name, fn in variants:               # warm-up: every variant once
        reports[name] = fn()
        torch.cuda.synchronize()
        if name == variants[1][0]:          # (before q0 / s0 write their rows of the outputs)
            same = all(torch.equal(out_q[k], out_s[k]) if out_q[k].dtype == torch.int32 else
                       torch.equal(out_q[k].view(torch.int64), out_s[k].view(torch.int64)) for k in out_s if k != "ITERS_OUT")
    for _ in range(ROUNDS):
        for name, fn in variants:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            times[name].append(1e3 * (time.perf_counter() - t0))
    print(f"{title} QUEUE: N={N} B={B} K={K} n={n} m={m} mu={MU} max_iters={MAX_ITERS} max_inner={SOLVE_PAR['max_inner']} "
          f"rounds={ROUNDS} stop={'on' if STOP else 'off'}", flush=True)
    med = {}
    for name, _ in variants:
        t, r = times[name], reports[name]
        med[name] = statistics.median(t)
        rows = B if name[0] in "qs" else N
        print(f"  {name:40s} {med[name]:9.2f} ms  (min {min(t):.2f} max {max(t):.2f})  rounds {r['rounds']} problem_iters "
              f"{r['problem_iters']} occupancy {r['problem_iters'] / max(r['rounds'] * K * rows, 1):.3f} phases 0..4,other {r['n_phase']}",
              flush=True)
    q, s = variants[0][0], variants[1][0]
    q0, s0 = variants[-2][0], variants[-1][0]
    print(f"  time q / s {med[q] / med[s]:.3f}" + (f", q / a {med[q] / med[variants[2][0]]:.3f}" if len(variants) == 5 else "")
          + f"; outputs bit-equal q vs s: {same}; nothing freezes: q0 - s0 = {1e3 * (med[q0] - med[s0]):.0f} us over "
          f"{reports[q0]['rounds']} rounds = {1e3 * (med[q0] - med[s0]) / max(reports[q0]['rounds'], 1):.0f} us per round", flush=True)


if __name__ == "__main__":
    which = sys.argv[1] if len(sys.argv) > 1 else "anymal"
    if os.environ.get("QUEUE", "0") == "1":
        K = KS[0]
        if which in ("monoped", "all"):
            f, vs, cs, goal, T = F.procedural_monoped()
            vb = f.var_bounds_data(varsets=vs, init_mode=capi.INIT_PROCEDURAL, ee_goal=goal, total_time=T)
            queue_run("monoped_procedural", TowrGpuProblem(F.procedural_desc(), device=0, data=vb),
                      int(os.environ.get("N_MONOPED", "16384")), int(os.environ.get("B_MONOPED", "4096")), K)
        if which in ("anymal", "all"):
            queue_run("anymal_trot_feasible" if FEASIBLE else "anymal_trot", anymal(), int(os.environ.get("N", "2048")),
                      int(os.environ.get("B", "512")), K)
        sys.exit(0)
    if which == "stopcost":
        stop_cost(anymal(), int(os.environ.get("B", "4096")))
    if which == "probecost":
        probe_cost("anymal_trot_feasible" if FEASIBLE else "anymal_trot", anymal(), int(os.environ.get("B", "4096")))
    if which == "probecost_monoped":
        f, vs, cs, goal, T = F.procedural_monoped()
        vb = f.var_bounds_data(varsets=vs, init_mode=capi.INIT_PROCEDURAL, ee_goal=goal, total_time=T)
        probe_cost("monoped_procedural", TowrGpuProblem(F.procedural_desc(), device=0, data=vb), int(os.environ.get("B_MONOPED", "4096")))
    if which in ("anymal", "all"):
        run("anymal_trot_feasible" if FEASIBLE else "anymal_trot", anymal(), int(os.environ.get("B", "1024")))
    if which in ("monoped", "all"):
        f, vs, cs, goal, T = F.procedural_monoped()
        vb = f.var_bounds_data(varsets=vs, init_mode=capi.INIT_PROCEDURAL, ee_goal=goal, total_time=T)
        run("monoped_procedural", TowrGpuProblem(F.procedural_desc(), device=0, data=vb), int(os.environ.get("B_MONOPED", "4096")))
