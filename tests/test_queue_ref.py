"""tests/queue_ref.py: the queue's bookkeeping on every small (N, B, K, M) with random freezing times, and the monoped's
six starts through two slots against the same six solved as one batch by tests/compact_ref.py."""
import numpy as np

from tests import alsolve_ref as R
from tests import compact_ref as C
from tests import queue_ref as Q
from tests import tile_chol_ref as TC
from tests.test_chol_ref import SOLVE_MU, SOLVE_SEEDS, _layout_handle
from tests.test_pgn_ref import SOLVE_PAR, _monoped

MONOPED_ITERS_OUT = [68, 12, 40, 32, 12, 12]     # 4 ceil(t / 4) of the freezing iterations 67 / 9 / 39 / 32 / 10 / 12


def test_retire_key():
    words = [0, 1, 2, 3, 4, 5, 6, 7, -1, -2 ** 31]
    for max_age in (0, 4, 5):
        for age in (0, 3, 4, 5, 8):
            key = Q.retire_key(words, [age] * len(words), max_age)
            want = [7 if w in (0, 1) and age >= max_age else w for w in words]
            assert key.tolist() == want, (max_age, age)


def test_bookkeeping_on_every_small_queue():
    """N = 0..6, B = 1..3, K in {1, 2}, M in {K, 3 K}, freezing times drawn per problem (some never freeze): every problem
    is retired exactly once with ITERS_OUT = min(K ceil(t / K), M), an expired problem keeps an active phase word, the two
    report identities hold, the live rows never exceed B and admission follows the queue."""
    rng = np.random.default_rng(20261021)
    seen = 0
    for N in range(7):
        for B in (1, 2, 3):
            for K in (1, 2):
                for M in (K, 3 * K):
                    for trial in range(6):
                        life = rng.integers(1, 3 * M + 2, size=N)          # the iteration at which problem i freezes
                        life[rng.random(N) < 0.3] = 10 ** 6                # never
                        words = rng.choice([2, 3, 4, 5, 6, 7, -1], size=N)

                        def admit(i):
                            return dict(ISTATE=np.array([0, 0, 0, 0]), its=0, i=i)

                        def it(st, k):
                            for _ in range(k):
                                st["its"] += 1
                                if "frozen_at" in st:
                                    continue                                  # (still evaluated to the round's end)
                                if st["its"] >= life[st["i"]]:
                                    st["ISTATE"][0], st["frozen_at"] = int(words[st["i"]]), st["its"]
                                else:
                                    st["ISTATE"][0] = 1                       # RESTART -> SEARCH: still active

                        rep = Q.solve_queue(N, B, admit, it, M, K)
                        what = (N, B, K, M, life.tolist())
                        assert all(s is not None for s in rep["states"]) and len(rep["states"]) == N, what
                        assert sorted(s["i"] for s in rep["states"]) == list(range(N)), what
                        for i, (st, its) in enumerate(zip(rep["states"], rep["iters"])):
                            assert st["i"] == i, what
                            assert its == min(K * -(-int(life[i]) // K), M) == st["its"], what
                            if life[i] > M:
                                assert int(st["ISTATE"][0]) in (0, 1), what      # expired: its word is still active
                            else:
                                assert int(st["ISTATE"][0]) == int(words[i]) and st["frozen_at"] == life[i], what
                        assert rep["problem_iters"] == sum(rep["iters"]), what
                        assert rep["rounds"] >= -(-rep["problem_iters"] // (B * K)), what
                        assert rep["iters_run"] == K * rep["rounds"] and rep["problem_iters"] == K * sum(rep["live"]), what
                        assert all(0 < b <= B for b in rep["live"]) and len(rep["live"]) == rep["rounds"], what
                        assert rep["admitted"] == list(range(N)), what
                        assert sum(rep["n_phase"]) == N, what
                        if N == 0:
                            assert rep["rounds"] == 0 and rep["problem_iters"] == 0
                        seen += 1
    assert seen == 7 * 3 * 2 * 2 * 6


def test_monoped_six_starts_through_two_slots(monkeypatch):
    """Seeds 900..905, SOLVE_PAR, mu = 1e-6 around tile_chol_ref.iterate: through B = 2 slots with K = 4, M = 100 the five
    output arrays of every problem are bit-equal to compact_ref.solve's on the six as one batch, and ITERS_OUT is
    68 / 12 / 40 / 32 / 12 / 12. Evaluations and directions are pure functions of their operands and are shared between
    the two runs through a memo on the operands' bytes."""
    o, P, x0, lo, up, evaluate = _monoped()
    info = _layout_handle("monoped_procedural").gn_factor_info()
    gn = dict(mu=SOLVE_MU, pos=info["pos"], first=info["first"])
    par = R.params(**SOLVE_PAR)
    memo_e, memo_d = {}, {}
    direction = TC.direction

    def evaluate_memo(x, lam, rho):
        key = (x.tobytes(), lam.tobytes(), float(rho))
        if key not in memo_e:
            memo_e[key] = evaluate(x, lam, rho)
        return memo_e[key]

    def direction_memo(P_, vals, lamp, rho, g, mu, pos, first, held=None, dtype=np.float64, **kw):
        assert not kw and P_ is P
        key = (np.asarray(vals).tobytes(), np.asarray(lamp).tobytes(), float(rho), np.asarray(g).tobytes(), float(mu),
               None if held is None else np.asarray(held).tobytes(), np.dtype(dtype).str)
        if key not in memo_d:
            memo_d[key] = direction(P_, vals, lamp, rho, g, mu, pos, first, held, dtype)
        return memo_d[key]

    monkeypatch.setattr(TC, "direction", direction_memo)

    def admit(i):
        st = R.new_state(o.n, o.m, par["mem"], x0 + 0.05 * np.random.default_rng(SOLVE_SEEDS[i]).standard_normal(o.n),
                         n_rsum=4 + o.desc.n_constraints, n_ssum=5 + o.desc.n_varsets)
        R.init(st, par, lo, up)
        return st

    it = lambda st, k: TC.iterate(st, par, gn, P, evaluate_memo, lo, up, k)
    N = len(SOLVE_SEEDS)
    rep = Q.solve_queue(N, 2, admit, it, 100, 4)
    evals = len(memo_e)
    batch = [admit(i) for i in range(N)]
    ref = C.solve(batch, it, 100, 4, True)
    print(f"queue: {rep['rounds']} rounds, {rep['problem_iters']} problem-iterations, ITERS_OUT {rep['iters']}; "
          f"batch: {ref['rounds']} rounds, {ref['problem_iters']}; {evals} evaluations, {len(memo_e) - evals} more for the batch")
    assert rep["iters"] == MONOPED_ITERS_OUT
    for i, (a, b) in enumerate(zip(rep["states"], batch)):
        for k in Q.OUTPUTS:
            assert np.asarray(a[k]).tobytes() == np.asarray(b[k]).tobytes(), (i, k)
    assert rep["n_phase"] == ref["n_phase"] and rep["n_phase"][R.CONVERGED] == 6
    assert rep["problem_iters"] == sum(rep["iters"]) == ref["problem_iters"]
    assert rep["rounds"] >= -(-rep["problem_iters"] // (2 * 4)) and max(rep["live"]) <= 2
    assert rep["admitted"] == list(range(N))
