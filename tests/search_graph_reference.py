"""CPU restatement of ppgs_amd.alignment.search_graph for the tests (tests/test_search_graph_host.py,
tests/test_gpu_search_graph.py): the programme over a graph with a free start at every frame and a free end, every
state carrying the begin of its partial match, in float64 (the reference) or float32 (the device's own additions); the
curve per end frame with the lowest final state on ties; the float64 optimum inside given spans; brute force over
every (begin, end, state sequence) for tiny cases; and three mutants of the programme that the tests must catch.

A graph here is viterbi_reference.Lists; r is (T, S): r[t, n] the emission of STATE n at frame t, the log-likelihood
ratio against the frame's best phoneme (`emissions`)."""
import itertools

import numpy as np

import search_reference as S
import viterbi_reference as V

lists = V.lists
log_posteriors = S.log_posteriors
MUTANTS = ('fresh_first', 'not_strict', 'highest_final')


def emissions(logp, sym, dtype=np.float64):
    """r (T, S): logp[t, sym[n]] - max_q logp[t, q], one subtraction in `dtype`."""
    logp = np.asarray(logp).astype(dtype)
    return logp[:, np.asarray(sym, dtype=np.int64)] - logp.max(axis=1)[:, None]


def padded(g):
    """The in-arc lists as (S, 1 + most) arrays: column 0 is staying (the state itself), then the arcs in list order,
    padded with source 0 and weight -inf, which is never better."""
    count = len(g.into)
    most = max([len(into) for into in g.into] + [0])
    source = np.zeros((count, 1 + most), dtype=np.int64)
    weight = np.full((count, 1 + most), -np.inf)
    source[:, 0] = np.arange(count)
    weight[:, 0] = np.asarray(g.stay, dtype=np.float64)
    for n, into in enumerate(g.into):
        for j, (p, w) in enumerate(into):
            source[n, 1 + j], weight[n, 1 + j] = p, w
    return source, weight


def programme(r, g, dtype=np.float64, mutant=None):
    """The curve of r (T, S) under graph g: (curve_total `dtype`, curve_begin int64, curve_state int64, curve_mass
    float64), each (T,).  curve_state is the final state taken (-1 where the total is -inf) and curve_mass the sum of
    |emission| and |weight| along the path taken, the A of the tests' error bound.  Candidates in the documented order:
    staying, the arcs as listed, the fresh start last, each only if strictly better (the first of the largest); on
    ties the lowest final state.  `mutant` breaks one of these rules (MUTANTS)."""
    assert mutant is None or mutant in MUTANTS
    r = np.asarray(r).astype(dtype)
    frames, count = r.shape
    source, weight = padded(g)
    weight = weight.astype(dtype)
    initial, final = np.asarray(g.initial).astype(dtype), np.asarray(g.final).astype(dtype)
    rows = np.arange(count)
    with np.errstate(invalid='ignore'):
        heavy = np.where(np.isinf(weight), 0., np.abs(weight.astype(np.float64)))
        fresh_mass = np.where(np.isinf(initial), 0., np.abs(initial.astype(np.float64)))
        final_mass = np.where(np.isinf(final), 0., np.abs(final.astype(np.float64)))
    d = np.full(count, -np.inf, dtype=dtype)
    b = np.full(count, -1, dtype=np.int64)
    mass = np.zeros(count)
    curve_total = np.full(frames, -np.inf, dtype=dtype)
    curve_begin = np.full(frames, -1, dtype=np.int64)
    curve_state = np.full(frames, -1, dtype=np.int64)
    curve_mass = np.zeros(frames)
    for t in range(frames):
        candidates = d[source] + weight                                  # one addition per candidate
        if mutant == 'fresh_first':                                      # the fresh start in front of staying
            candidates = np.concatenate([initial[:, None], candidates], axis=1)
        if mutant == 'not_strict':                                       # >= : the LAST of the largest
            taken = candidates.shape[1] - 1 - np.argmax(candidates[:, ::-1], axis=1)
        else:
            taken = np.argmax(candidates, axis=1)                        # strict >: the first of the largest
        best = candidates[rows, taken]
        if mutant == 'fresh_first':
            start = taken == 0
            taken = np.maximum(taken - 1, 0)
        else:
            start = initial >= best if mutant == 'not_strict' else initial > best
            best = np.where(start, initial, best)
        via = source[rows, taken]
        mass = np.where(start, fresh_mass, mass[via] + heavy[rows, taken]) + np.abs(r[t].astype(np.float64))
        b = np.where(start, t, b[via])
        d = r[t] + best
        f = d + final
        if mutant == 'highest_final':
            last = count - 1 - int(np.argmax(f[::-1]))
        else:
            last = int(np.argmax(f))                                     # the lowest state of equal values
        curve_total[t] = f[last]
        if f[last] > -np.inf:
            curve_begin[t], curve_state[t], curve_mass[t] = b[last], last, mass[last] + final_mass[last]
    return curve_total, curve_begin, curve_state, curve_mass


def spans(r, g, begins):
    """(T,) float64: for every end frame t with begins[t] >= 0 the weight of the best path that begins at frame
    begins[t] (with its state's `initial`), covers every frame up to t and ends there (with `final`): what `viterbi`
    maximises on that span.  NaN where begins[t] < 0.  The distinct begins advance together, one pinned programme
    each."""
    r = np.asarray(r, dtype=np.float64)
    frames, count = r.shape
    begins = np.asarray(begins, dtype=np.int64)
    source, weight = padded(g)
    initial, final = np.asarray(g.initial, dtype=np.float64), np.asarray(g.final, dtype=np.float64)
    out = np.full(frames, np.nan)
    firsts = np.unique(begins[begins >= 0])
    if firsts.size == 0:
        return out
    row_of = {int(first): k for k, first in enumerate(firsts)}
    ends_of = {}
    for t in np.nonzero(begins >= 0)[0]:
        ends_of.setdefault(int(t - begins[t]), []).append(int(t))
    d = r[firsts] + initial                                              # (rows, S): frame `first` of every row
    for j in range(max(ends_of) + 1):
        if j:
            at = np.minimum(firsts + j, frames - 1)                      # (rows past the end run along, unread)
            d = r[at] + (d[:, source] + weight).max(axis=2)
        for t in ends_of.get(j, ()):
            out[t] = (d[row_of[int(begins[t])]] + final).max()
    return out


def brute_force(r, g):
    """Per end frame t: (the largest weight over every begin and every state sequence that starts with `initial` at
    its begin, moves by staying or along an arc, and ends with `final` at t; the set of begins of the paths that reach
    it).  (-inf, empty) where no path ends.  Added in frame order; exact for integer-valued inputs."""
    r = np.asarray(r, dtype=np.float64)
    frames, count = r.shape
    step = np.full((count, count), -np.inf)                              # the best single move p -> n
    for n in range(count):
        step[n, n] = max(step[n, n], float(g.stay[n]))
        for p, w in g.into[n]:
            step[p, n] = max(step[p, n], w)
    out = []
    for t in range(frames):
        best, firsts = -np.inf, set()
        for first in range(t + 1):
            for states in itertools.product(range(count), repeat=t - first + 1):
                total = float(g.initial[states[0]])
                for k, n in enumerate(states):
                    if k:
                        total = total + step[states[k - 1], n]
                    total = r[first + k, n] + total
                total = total + float(g.final[states[-1]])
                if total > best:
                    best, firsts = total, {first}
                elif total == best and total > -np.inf:
                    firsts.add(first)
        out.append((best, firsts))
    return out
