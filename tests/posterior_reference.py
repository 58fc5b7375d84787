"""CPU restatement of ppgs_amd.alignment.posterior for the tests (tests/test_posterior_host.py,
tests/test_gpu_posterior.py): the forward-backward recurrences over arc lists in float64 (the reference), the same in
float32 with the device's shifts (a restatement of the device arithmetic), and a brute-force enumerator that sums exp of
every path's weight for tiny graphs.

A graph is viterbi_reference's `Lists`; e is (T, S), e[t, n] the emission of STATE n at frame t.  Weights are finite or
-inf.  Parallel arcs and arcs n -> n each count as a path of their own."""
import numpy as np

import viterbi_reference

lists = viterbi_reference.lists
emissions = viterbi_reference.emissions


def prepared(ppg):
    """The prepared log-posteriors (T, 40) float32 of a (40, T) PPG, as the device computes them: logf of the value
    clamped to [1e-8, 1 - 1e-8] in float32.  (numpy's float32 log is correctly rounded or within an ulp of the device's;
    the tests' bounds carry that rounding as the emission's.)"""
    p = np.asarray(ppg, dtype=np.float32).T
    return np.log(np.minimum(np.maximum(p, np.float32(1e-8)), np.float32(1.) - np.float32(1e-8)))


def arcs(g):
    """(source, target, weight) arrays of every arc of `g`, in in-list order."""
    source = [s for into in g.into for s, _ in into]
    target = [n for n, into in enumerate(g.into) for _ in into]
    weight = [w for into in g.into for _, w in into]
    return np.asarray(source, dtype=np.int64), np.asarray(target, dtype=np.int64), np.asarray(weight, dtype=np.float64)


def _lse_into(count, own, candidates, where, dtype):
    """Per state n: LSE(own[n], candidates[i] for where[i] == n), LSE of -inf alone = -inf, in `dtype`."""
    top = own.copy()
    np.maximum.at(top, where, candidates)
    safe = np.where(np.isneginf(top), dtype(0), top)
    with np.errstate(invalid='ignore'):
        total = np.exp(own - safe)
        np.add.at(total, where, np.exp(candidates - safe[where]))
    with np.errstate(divide='ignore'):
        return (top + np.log(total)).astype(dtype)


def _lse(values, dtype=np.float64):
    top = values.max()
    if np.isneginf(top):
        return dtype(-np.inf)
    return dtype(top + np.log(np.exp(values - top).sum(dtype=dtype)))


def forward_backward(e, g, dtype=np.float64):
    """(total, gamma (T, S), post (40, T)) by the recurrences, vectorised per frame.  In float64 this is the reference.
    In float32 it restates the device: a row is kept less the maxima of the rows before it (frame t+1 takes the maximum
    of row t off after its LSE), the maxima are added up in float64, beta the same way, and gamma is normalised per frame.
    total is a float (-inf without a path, gamma and post then None)."""
    e = np.asarray(e, dtype=dtype)
    frames, count = e.shape
    assert count == len(g.into) and frames >= 1
    source, target, weight = arcs(g)
    weight = weight.astype(dtype)
    stay, initial, final = (np.asarray(v, dtype=dtype) for v in (g.stay, g.initial, g.final))
    shifted = dtype is not np.float64
    a = np.empty((frames, count), dtype=dtype)
    a[0] = e[0] + initial
    shift = 0.
    for t in range(1, frames):
        before = a[t - 1].max() if shifted else dtype(0)
        if np.isneginf(a[t - 1].max()):
            return -np.inf, None, None
        shift += float(before)
        step = _lse_into(count, a[t - 1] + stay, a[t - 1][source] + weight, target, dtype)
        a[t] = e[t] + (step - before)
    end = _lse(a[frames - 1] + final, dtype)
    if np.isneginf(end):
        return -np.inf, None, None
    total = shift + float(end)
    gamma = np.empty((frames, count), dtype=dtype)
    b = final.copy()
    for t in range(frames - 1, -1, -1):
        if t < frames - 1:
            before = b.max() if shifted else dtype(0)
            inner = e[t + 1] + b
            b = _lse_into(count, inner + stay, inner[target] + weight, source, dtype) - before
        both = a[t] + b
        z = both.max()
        terms = np.exp(both - z)
        gamma[t] = terms / terms.sum(dtype=dtype)
    post = np.zeros((40, frames), dtype=dtype)
    np.add.at(post, (np.asarray(g.sym)[None, :].repeat(frames, 0), np.arange(frames)[:, None].repeat(count, 1)), gamma)
    return total, gamma, post


def brute_force(e, g):
    """(total, gamma (T, S)) by enumerating every path: a state at frame 0, then per frame either staying or one of
    the in-arcs of the state entered, parallel arcs and arcs n -> n as choices of their own; the sum of exp(weight).
    (-inf, None) if every path weighs -inf."""
    e = np.asarray(e, dtype=np.float64)
    frames, count = e.shape
    out_of = [[] for _ in range(count)]                        # (target, ordinal) per source; staying is ordinal 0
    for n in range(count):
        out_of[n].append((n, 0))
        for j, (source, _) in enumerate(g.into[n]):
            out_of[source].append((n, j + 1))
    mass = np.zeros((frames, count))
    whole = 0.

    def walk(states, ordinals):
        nonlocal whole
        if len(states) == frames:
            weight = viterbi_reference.rescore(states, ordinals, e, g)
            if weight > -np.inf:
                whole += np.exp(weight)
                mass[np.arange(frames), states] += np.exp(weight)
            return
        for target, ordinal in out_of[states[-1]]:
            walk(states + [target], ordinals + [ordinal])
    for first in range(count):
        walk([first], [0])
    if whole == 0.:
        return -np.inf, None
    return float(np.log(whole)), mass / whole
