"""numpy restatement of the queued solve (include/towr_gpu.h, towr_gpu_alsolve_solve_queue_batch_device): N problems
through B slots around a per-problem reference iteration, in the style of tests/compact_ref.py, whose partition and row
swap it reuses. A slot holds a per-problem state (a dict with ISTATE[0] the phase), the problem's index and its age."""
import numpy as np

from tests.compact_ref import partition, swap_rows

EXPIRED = 7          # the retire key of an active row that has run out of budget
OUTPUTS = ("X", "LAM", "RHO", "SCAL", "ISTATE")


def retire_key(phases, ages, max_age):
    """KEY per row: 7 where the phase word is 0 or 1 and the age has reached max_age, else the phase word."""
    p = np.asarray(phases, dtype=np.int64)
    a = np.asarray(ages, dtype=np.int64)
    return np.where(((p == 0) | (p == 1)) & (a >= max_age), EXPIRED, p)


def solve_queue(N, B, admit, iterate_one, max_iters, check_every):
    """The driver's rounds. admit(i) returns problem i's state as the admission leaves it (copied in and initialised);
    iterate_one(state, k) runs k iterations on one problem. Returns dict(rounds, iters_run, problem_iters, n_phase,
    states (per problem, as retired), iters (ITERS_OUT), admitted (the order of admission), live (rows per round))."""
    K, M = int(check_every), int(max_iters)
    if K < 1 or M < 1 or M % K:
        raise ValueError("max_iters must be a positive multiple of check_every")
    if N > 0 and B < 1:
        raise ValueError("N problems need B >= 1 slots")
    slots, ids, ages = [], [], []
    states, iters = [None] * N, [None] * N
    admitted, live = [], []
    rounds = problem_iters = nxt = 0
    while True:
        c = min(B - len(slots), N - nxt)
        for i in range(nxt, nxt + c):
            slots.append(admit(i))
            ids.append(i)
            ages.append(0)
            admitted.append(i)
        nxt += c
        bcur = len(slots)
        if bcur == 0:
            break
        for st in slots:
            iterate_one(st, K)
        ages = [a + K for a in ages]
        key = retire_key([int(st["ISTATE"][0]) for st in slots], ages, M)
        head, pairs = partition(key)
        for rows in (slots, ids, ages):
            swap_rows(rows, pairs)
        rounds, problem_iters = rounds + 1, problem_iters + bcur * K
        live.append(bcur)
        na = int(head[0])
        for r in range(na, bcur):
            assert states[ids[r]] is None, "a problem was retired twice"
            states[ids[r]], iters[ids[r]] = slots[r], ages[r]
        del slots[na:], ids[na:], ages[na:]
    phases = np.array([int(st["ISTATE"][0]) for st in states], dtype=np.int64)
    counts = [int((phases == k).sum()) for k in range(5)]
    return dict(rounds=rounds, iters_run=K * rounds, problem_iters=problem_iters, n_phase=counts + [N - sum(counts)],
                states=states, iters=iters, admitted=admitted, live=live)
