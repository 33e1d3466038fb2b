"""tests/compact_ref.py: the partition rule on every small phase pattern, the swap lists of a multi-round sequence, and
the monoped short solve through the reference driver with and without compaction."""
import itertools

import numpy as np

from tests import alsolve_ref as R
from tests import compact_ref as C
from tests import tile_chol_ref as TC
from tests.test_chol_ref import SOLVE_MU, SOLVE_SEEDS, _layout_handle
from tests.test_pgn_ref import SOLVE_PAR, _monoped

WORDS = (0, 1, 2, 3, 4, 7, -1)


def test_partition_on_every_small_pattern():
    """B = 0..6, every pattern of phase words from WORDS: after the swaps the prefix [0, na) is all active and the suffix
    all frozen, rows that were on their side did not move, the list applied twice is the identity, np <= B / 2, the pairs
    are ascending and the counts add up."""
    seen = 0
    for B in range(7):
        for pat in itertools.product(WORDS, repeat=B):
            head, pairs = C.partition(pat)
            head, fs, as_ = head.tolist(), pairs[:, 0].tolist(), pairs[:, 1].tolist()
            na = head[0]
            assert head[1] == len(fs) == len(as_) <= B // 2 and sum(head[2:]) == B and na == head[2] + head[3]
            assert head[7] == sum(w in (7, -1) for w in pat)
            assert fs == sorted(set(fs)) and as_ == sorted(set(as_))
            assert all(f < na for f in fs) and all(na <= a < B for a in as_)
            assert all(pat[f] not in (0, 1) for f in fs) and all(pat[a] in (0, 1) for a in as_), pat
            rows = list(range(B))
            C.swap_rows(rows, pairs)
            assert all(pat[r] in (0, 1) for r in rows[:na]) and all(pat[r] not in (0, 1) for r in rows[na:]), pat
            assert {r for r in range(B) if rows[r] != r} == set(fs + as_), pat   # (rows on their side did not move)
            C.swap_rows(rows, pairs)
            assert rows == list(range(B)), pat
            seen += 1
    assert seen == sum(len(WORDS) ** B for B in range(7))


def test_pairs_of_all_rounds_number_at_most_b_and_replay_restores():
    """Random freezing sequences through the driver's loop: a frozen row moves at most once, so the pairs of all rounds
    together number at most B (the LOG's room); the swaps in reverse restore the order (asserted inside solve), and
    problem_iters counts the rows of every round's batch."""
    rng = np.random.default_rng(20261021)
    for trial in range(200):
        B = int(rng.integers(0, 40))
        life = rng.integers(0, 30, size=B)   # iterations until the problem freezes
        states = [dict(ISTATE=np.array([0 if life[b] > 0 else 2, 0, 0, 0]), its=0, b=b) for b in range(B)]

        def it(st, k):
            for _ in range(k):
                st["its"] += 1
                if st["ISTATE"][0] < 2 and st["its"] >= life[st["b"]]:
                    st["ISTATE"][0] = int(rng.choice([2, 3, 4, 7, -1]))

        K = int(rng.integers(1, 6))
        rep = C.solve(states, it, max_iters=25, check_every=K, compact=True)
        assert sum(len(p) for p in rep["pairs"]) <= B
        assert sum(rep["n_phase"]) == B and rep["iters_run"] <= 25
        want = 0
        for r in range(rep["rounds"]):
            k = min(K, 25 - r * K)
            want += k * int(sum((life[b] > r * K) or (r == 0) for b in range(B)))
        assert rep["problem_iters"] == want, (trial, rep, life.tolist())


def _solve_monoped(compact, K=100, check_every=4):
    o, P, x0, lo, up, evaluate = _monoped()
    info = _layout_handle("monoped_procedural").gn_factor_info()
    gn = dict(mu=SOLVE_MU, pos=info["pos"], first=info["first"])
    par = R.params(**SOLVE_PAR)
    states = []
    for seed in SOLVE_SEEDS:
        st = R.new_state(o.n, o.m, par["mem"], x0 + 0.05 * np.random.default_rng(seed).standard_normal(o.n),
                         n_rsum=4 + o.desc.n_constraints, n_ssum=5 + o.desc.n_varsets)
        R.init(st, par, lo, up)
        states.append(st)
    last = {}

    def cached(x, lam, rho):   # (a frozen problem is evaluated at the same point in every iteration: XC = X)
        key = (x.tobytes(), lam.tobytes(), rho)
        if last.get("key") != key:
            last["key"], last["out"] = key, evaluate(x, lam, rho)
        return last["out"]

    rep = C.solve(states, lambda st, k: TC.iterate(st, par, gn, P, cached, lo, up, k), K, check_every, compact)
    return states, rep


def test_monoped_short_solve_with_and_without_compaction():
    """Seeds 900..905, SOLVE_PAR, mu = 1e-6, at most 100 iterations in rounds of 4: the persistent arrays of every problem
    are bit-equal with and without compaction, and compaction runs sum_b 4 ceil(done_b / 4) problem-iterations."""
    a, ra = _solve_monoped(True)
    b, rb = _solve_monoped(False)
    print(f"compact: {ra['rounds']} rounds, {ra['iters_run']} iterations, {ra['problem_iters']} problem-iterations; "
          f"plain: {rb['problem_iters']}; phases {ra['n_phase']}")
    assert ra["iters_run"] == rb["iters_run"] and ra["rounds"] == rb["rounds"] and ra["n_phase"] == rb["n_phase"]
    assert rb["problem_iters"] == len(SOLVE_SEEDS) * rb["iters_run"] and ra["problem_iters"] < rb["problem_iters"]
    for sa, sb in zip(a, b):
        for k in C.PERSISTENT:
            assert np.asarray(sa[k]).tobytes() == np.asarray(sb[k]).tobytes(), k
    assert sum(int(s["ISTATE"][0]) == R.CONVERGED for s in a) >= 5
