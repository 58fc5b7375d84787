"""CPU restatement of ppgs_amd.alignment.recognize for the tests (tests/test_recognize_host.py,
tests/test_gpu_recognize.py): a float64 Viterbi over any number of states with the documented tie rule (staying beats
switching, the lowest predecessor beats a higher one, the lowest end state wins), a brute-force enumerator over every
label sequence for tiny cases, and the float64 cost of a given path.

e is (T, K): e[t, q] the emission of state q at frame t.  A is (K, K): A[p, q] the weight of going from p to q.
initial and final are (K,).  Entries are finite or -inf."""
import itertools

import numpy as np


def viterbi(e, A, initial, final, dtype=np.float64):
    """(total, labels): the best path's weight and its (T,) int64 labels; (-inf, None) if no path exists.  `dtype` is
    the arithmetic: float64 is the reference, float32 restates the device's own additions."""
    e, A = np.asarray(e, dtype=dtype), np.asarray(A, dtype=dtype)
    initial, final = np.asarray(initial, dtype=dtype), np.asarray(final, dtype=dtype)
    frames, states = e.shape
    assert A.shape == (states, states) and initial.shape == final.shape == (states,) and frames >= 1
    origin = np.zeros((frames, states), dtype=np.int64)
    d = e[0] + initial
    index = np.arange(states)
    with np.errstate(invalid='ignore'):
        for t in range(1, frames):
            c = d[:, None] + A                                  # c[p, q]
            best = c.max(axis=0)
            # staying wherever it is among the best, else the lowest of the best (argmax takes the first)
            origin[t] = np.where(c[index, index] == best, index, c.argmax(axis=0))
            d = e[t] + best
        f = d + final
    last = 0
    for q in range(1, states):
        if f[q] > f[last]:
            last = q
    if not f[last] > -np.inf:
        return -np.inf, None
    labels = np.empty(frames, dtype=np.int64)
    labels[frames - 1] = last
    for t in range(frames - 1, 0, -1):
        labels[t - 1] = origin[t, labels[t]]
    return float(f[last]), labels


def rescore(labels, e, A, initial, final):
    """The float64 weight of the path `labels`, added in frame order; -inf if the model forbids it."""
    e, A = np.asarray(e, dtype=np.float64), np.asarray(A, dtype=np.float64)
    labels = [int(q) for q in labels]
    assert len(labels) == e.shape[0] and all(0 <= q < e.shape[1] for q in labels)
    total = e[0, labels[0]] + float(initial[labels[0]])
    for t in range(1, len(labels)):
        total = e[t, labels[t]] + (total + A[labels[t - 1], labels[t]])
    return float(total + float(final[labels[-1]]))


def brute_force(e, A, initial, final):
    """(total, labels) by enumerating all K^T label sequences: the largest weight, and among equal weights the path
    the tie rule picks -- the lowest end state, then, walking backwards, the same state if staying is optimal and
    else the lowest predecessor.  (-inf, None) if every path weighs -inf.  Exact for integer-valued inputs."""
    e = np.asarray(e, dtype=np.float64)
    frames, states = e.shape
    chosen = None
    for labels in itertools.product(range(states), repeat=frames):
        total = rescore(labels, e, A, initial, final)
        if not total > -np.inf:
            continue
        order = [labels[-1]]
        for t in range(frames - 1, 0, -1):
            order.append(0 if labels[t - 1] == labels[t] else 1 + labels[t - 1])
        key = (-total, tuple(order))
        if chosen is None or key < chosen[0]:
            chosen = (key, labels)
    if chosen is None:
        return -np.inf, None
    return -chosen[0][0], np.asarray(chosen[1], dtype=np.int64)


def runs(labels):
    """(phonemes, starts) int64 of a label row: the runs' labels and their first frames, starts[R] = T."""
    labels = np.asarray(labels, dtype=np.int64)
    opens = np.concatenate([[True], labels[1:] != labels[:-1]])
    starts = np.concatenate([np.nonzero(opens)[0], [len(labels)]])
    return labels[opens], starts


def expand(phonemes, starts):
    """The label row of runs: the inverse of `runs`."""
    return np.repeat(np.asarray(phonemes, dtype=np.int64), np.diff(np.asarray(starts, dtype=np.int64)))
