"""CPU restatement of ppgs_amd.alignment.viterbi for the tests (tests/test_viterbi_host.py, tests/test_gpu_viterbi.py):
the recurrence over arc lists in float64 (the reference) or float32 (the device's own additions) with the documented
tie rule (staying wins, then the arc listed first, the lowest end state) and run rule (a run opens at frame 0 and
wherever the path takes an arc, also an arc n -> n), a brute-force enumerator over every path for tiny graphs, and the
float64 cost of a given path.

A graph here is `Lists`: stay, initial and final (S,) float64, `into[n]` the ordered list of (source, weight) into state
n, and sym (S,) the phonemes.  e is (T, S): e[t, n] the emission of STATE n at frame t (`emissions` makes it from the
prepared log-posteriors).  Weights are finite or -inf."""
import collections
import itertools

import numpy as np

Lists = collections.namedtuple('Lists', ['sym', 'stay', 'into', 'initial', 'final'])


def lists(graph):
    """`Lists` of a ppgs_amd.alignment.Graph."""
    offsets = graph.offsets.tolist()
    sources, weights = graph.sources.tolist(), graph.weights.double().tolist()
    into = [list(zip(sources[a:b], weights[a:b])) for a, b in zip(offsets, offsets[1:])]
    return Lists(np.asarray(graph.phonemes.tolist(), dtype=np.int64), graph.stay.double().numpy(), into,
                 graph.initial.double().numpy(), graph.final.double().numpy())


def emissions(logp, sym):
    """e (T, S) from logp (T, 40): column sym[n] for state n."""
    return np.asarray(logp)[:, np.asarray(sym, dtype=np.int64)]


def viterbi(e, g, dtype=np.float64):
    """(total, states, ordinals): the best path's weight, its (T,) int64 states and its (T,) int64 ordinals (0 where
    the path stays, j + 1 where it takes in-arc j; ordinals[0] = 0); (-inf, None, None) if no path exists."""
    e = np.asarray(e, dtype=dtype)
    frames, count = e.shape
    assert count == len(g.into) and frames >= 1
    stay, initial, final = (np.asarray(v, dtype=dtype) for v in (g.stay, g.initial, g.final))
    origin = np.zeros((frames, count), dtype=np.int64)
    d = e[0] + initial
    for t in range(1, frames):
        now = np.empty(count, dtype=dtype)
        for n in range(count):
            best, chosen = d[n] + stay[n], 0
            for j, (source, weight) in enumerate(g.into[n]):
                c = d[source] + dtype(weight)
                if c > best:
                    best, chosen = c, j + 1
            now[n] = e[t, n] + best
            origin[t, n] = chosen
        d = now
    f = d + final
    last = 0
    for n in range(1, count):
        if f[n] > f[last]:
            last = n
    if not f[last] > -np.inf:
        return -np.inf, None, None
    states, ordinals = np.empty(frames, dtype=np.int64), np.zeros(frames, dtype=np.int64)
    states[frames - 1] = last
    for t in range(frames - 1, 0, -1):
        n = states[t]
        ordinals[t] = origin[t, n]
        states[t - 1] = n if ordinals[t] == 0 else g.into[n][ordinals[t] - 1][0]
    return float(f[last]), states, ordinals


def rescore(states, ordinals, e, g):
    """The float64 weight of a path given by its states and ordinals, added in frame order."""
    e = np.asarray(e, dtype=np.float64)
    total = e[0, states[0]] + float(g.initial[states[0]])
    for t in range(1, len(states)):
        n = int(states[t])
        if ordinals[t] == 0:
            assert states[t - 1] == n
            step = float(g.stay[n])
        else:
            source, step = g.into[n][int(ordinals[t]) - 1]
            assert source == states[t - 1]
        total = e[t, n] + (total + step)
    return float(total + float(g.final[states[-1]]))


def brute_force(e, g):
    """(total, states, ordinals) by enumerating every path: a state at frame 0, then per frame either staying or one of
    the in-arcs of the state entered.  The largest weight, and among equal weights the path the tie rule picks: the
    lowest end state, then, walking backwards, the lowest ordinal.  (-inf, None, None) if every path weighs -inf.
    Exact for integer-valued inputs."""
    e = np.asarray(e, dtype=np.float64)
    frames, count = e.shape
    out_of = [[] for _ in range(count)]                        # (target, ordinal) per source; staying is ordinal 0
    for n in range(count):
        out_of[n].append((n, 0))
        for j, (source, _) in enumerate(g.into[n]):
            out_of[source].append((n, j + 1))
    chosen = None

    def walk(states, ordinals):
        nonlocal chosen
        if len(states) == frames:
            total = rescore(states, ordinals, e, g)
            if total > -np.inf:
                key = (-total, (states[-1],) + tuple(reversed(ordinals[1:])))
                if chosen is None or key < chosen[0]:
                    chosen = (key, list(states), list(ordinals))
            return
        for target, ordinal in out_of[states[-1]]:
            walk(states + [target], ordinals + [ordinal])
    for first in range(count):
        walk([first], [0])
    if chosen is None:
        return -np.inf, None, None
    return -chosen[0][0], np.asarray(chosen[1], dtype=np.int64), np.asarray(chosen[2], dtype=np.int64)


def runs(states, ordinals):
    """(run states, starts) int64 of a path: a run opens at frame 0 and wherever the ordinal is not 0; starts[R] = T."""
    states, ordinals = np.asarray(states, dtype=np.int64), np.asarray(ordinals, dtype=np.int64)
    opens = ordinals != 0
    opens[0] = True
    return states[opens], np.concatenate([np.nonzero(opens)[0], [len(states)]])


def best_rescore(run_states, starts, e, g):
    """The float64 weight of the path with these runs, each entered through the heaviest arc from the run before it;
    None if some run cannot follow the one before it (no such arc) or the runs do not cover the frames."""
    run_states, starts = [int(n) for n in run_states], [int(t) for t in starts]
    frames = e.shape[0]
    if len(starts) != len(run_states) + 1 or starts[0] != 0 or starts[-1] != frames or len(run_states) < 1:
        return None
    if any(b <= a for a, b in zip(starts, starts[1:])) or not all(0 <= n < len(g.into) for n in run_states):
        return None
    states, ordinals = np.empty(frames, dtype=np.int64), np.zeros(frames, dtype=np.int64)
    for r, n in enumerate(run_states):
        states[starts[r]:starts[r + 1]] = n
        if r:
            entering = [(weight, -j) for j, (source, weight) in enumerate(g.into[n]) if source == run_states[r - 1]]
            if not entering:
                return None
            ordinals[starts[r]] = 1 - max(entering)[1]
    return rescore(states, ordinals, e, g)
