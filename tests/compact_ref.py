"""numpy restatement of the compacting solve (include/towr_gpu.h): the partition plan of a batch by its phase words
(towr_gpu_alsolve_partition_batch_device), the row swap, and the solve driver's rounds
(towr_gpu_alsolve_solve_batch_device) around a per-problem reference iteration (tests/alsolve_ref.py's states, e.g.
tests/tile_chol_ref.iterate), with and without compaction. A batch is a list of per-problem states."""
import numpy as np

PERSISTENT = ("X", "GR", "LAM", "RHO", "SCAL", "ISTATE", "HS", "HY", "HMETA", "D", "ALPHA")


def active(phases):
    p = np.asarray(phases, dtype=np.int64)
    return (p == 0) | (p == 1)


def partition(phases):
    """(HEAD (8), PAIRS (np, 2)): na, np, the rows with phase 0..4 and with any other word; pair i = (the i-th frozen row
    of [0, na), the i-th active row of [na, B)), both ascending."""
    p = np.asarray(phases, dtype=np.int64)
    act = active(p)
    na = int(act.sum())
    f = np.flatnonzero(~act[:na])
    a = na + np.flatnonzero(act[na:])
    assert len(f) == len(a)
    counts = [int((p == k).sum()) for k in range(5)]
    head = np.array([na, len(f)] + counts + [len(p) - sum(counts)], dtype=np.int32)
    return head, np.stack([f, a], axis=1).astype(np.int32).reshape(-1, 2)


def swap_rows(rows, pairs):
    """Exchanges rows[f], rows[a] for every pair, in place (a list, or the first axis of an array)."""
    for f, a in np.asarray(pairs).reshape(-1, 2):
        if isinstance(rows, np.ndarray):
            rows[[f, a]] = rows[[a, f]]
        else:
            rows[f], rows[a] = rows[a], rows[f]
    return rows


def solve(states, iterate_one, max_iters, check_every, compact):
    """The driver's loop on a list of per-problem states (dicts with ISTATE[0] the phase); iterate_one(state, k) runs k
    iterations on one problem. The list is permuted between the rounds (compact) and put back by the swaps in reverse.
    Returns dict(rounds, iters_run, problem_iters, n_phase, pairs: the pairs of every round)."""
    B = len(states)
    order = list(states)
    log, rounds, iters_run, problem_iters, bcur = [], 0, 0, 0, B
    while iters_run < max_iters and bcur > 0:
        k = min(check_every, max_iters - iters_run)
        for st in order[:bcur]:
            iterate_one(st, k)
        head, pairs = partition([int(st["ISTATE"][0]) for st in order[:bcur]])
        rounds, iters_run, problem_iters = rounds + 1, iters_run + k, problem_iters + bcur * k
        if compact:
            swap_rows(order, pairs)
            log.append(pairs)
            bcur = int(head[0])
        if head[0] == 0:
            break
    for pairs in reversed(log):
        swap_rows(order, pairs)
    assert all(a is b for a, b in zip(order, states)), "the replay did not restore the order"
    head, _ = partition([int(st["ISTATE"][0]) for st in states])
    return dict(rounds=rounds, iters_run=iters_run, problem_iters=problem_iters, n_phase=head[2:].tolist(), pairs=log)
