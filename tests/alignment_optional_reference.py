"""CPU restatement of forced alignment with optional phonemes for the tests (tests/test_alignment_optional_host.py,
tests/test_gpu_alignment_optional.py): the float64 programme with the documented recurrence and tie order (stay beats
advance beats skip), its own trace-back, scores on given segments through tests/alignment_reference.py, and a
brute-force enumerator over every (subset of optional phonemes left out x segmentation of the rest) for tiny cases."""
import itertools

import numpy as np

import alignment_reference as R


def legal(optional, frames):
    """The three conditions on a transcript: no two adjacent optional phonemes, a mandatory one, the mandatory ones
    fit the frames."""
    optional = [bool(v) for v in optional]
    mandatory = optional.count(False)
    return not any(a and b for a, b in zip(optional, optional[1:])) and 1 <= mandatory <= frames


def programme(e, optional):
    """(total, starts) of the float64 programme over e (T, N) with optional (N,) flags; starts is (N + 1,) int64,
    non-decreasing, with starts[n] == starts[n + 1] exactly for the phonemes left out."""
    e = np.asarray(e, dtype=np.float64)
    frames, count = e.shape
    optional = np.asarray(optional).astype(bool)
    assert optional.shape == (count,) and legal(optional, frames)
    may = np.concatenate([[False], optional[:-1]])            # may[n]: a path may come to n from n - 2, over n - 1
    best = np.full(count, -np.inf)
    direction = np.zeros((frames, count), dtype=np.int8)
    # frame 0 from the virtual origin: state -1 holds 0, every real state -inf
    best[0] = e[0, 0]
    direction[0, 0] = 1
    if count > 1 and optional[0]:
        best[1] = e[0, 1]
        direction[0, 1] = 2
    for t in range(1, frames):
        stay = best
        advance = np.concatenate([[-np.inf], best[:-1]])
        skip = np.where(may, np.concatenate([[-np.inf, -np.inf], best[:-2]])[:count], -np.inf)
        chosen, way = stay.copy(), np.zeros(count, dtype=np.int8)
        better = advance > chosen                             # strictly: stay beats advance
        chosen, way = np.where(better, advance, chosen), np.where(better, 1, way)
        better = skip > chosen                                # strictly: stay and advance beat skip
        chosen, way = np.where(better, skip, chosen), np.where(better, 2, way)
        best = e[t] + chosen
        direction[t] = way
    end = count - 1
    if optional[count - 1] and best[count - 2] > best[count - 1]:
        end = count - 2
    starts = np.full(count + 1, -1, dtype=np.int64)
    starts[count] = frames
    if end == count - 2:
        starts[count - 1] = frames
    n = end
    for t in range(frames - 1, 0, -1):
        if direction[t, n] == 1:
            starts[n] = t
            n -= 1
        elif direction[t, n] == 2:
            starts[n] = starts[n - 1] = t
            n -= 2
    assert n in (0, 1) and (n == 0 or optional[0])
    if n == 1:
        starts[1] = 0
    starts[0] = 0
    assert (starts >= 0).all()
    return float(best[end]), starts


def path_total(e, starts):
    """The sum of e along the segmentation, added in frame order (empty segments add nothing)."""
    return R.path_total(e, starts)


def brute_force(e, optional):
    """(total, every optimal starts) by enumeration: every subset of the optional phonemes left out, every monotone
    segmentation of the kept ones, each path's sum added in frame order.  The optima come as a set of tuples."""
    e = np.asarray(e, dtype=np.float64)
    frames, count = e.shape
    free = [n for n in range(count) if optional[n]]
    top, optima = -np.inf, set()
    for size in range(len(free) + 1):
        for dropped in itertools.combinations(free, size):
            kept = [n for n in range(count) if n not in dropped]
            if not 1 <= len(kept) <= frames:
                continue
            for cuts in itertools.combinations(range(1, frames), len(kept) - 1):
                edges = (0,) + cuts + (frames,)
                starts = np.empty(count + 1, dtype=np.int64)
                starts[count] = frames
                at = len(kept)
                for n in range(count - 1, -1, -1):            # a left-out phoneme starts where the next one does
                    if n in dropped:
                        starts[n] = starts[n + 1]
                    else:
                        at -= 1
                        starts[n] = edges[at]
                        assert starts[n + 1] == edges[at + 1]
                value = path_total(e, starts)
                if value > top:
                    top, optima = value, {tuple(starts.tolist())}
                elif value == top:
                    optima.add(tuple(starts.tolist()))
    return top, optima


def scores(logp, phonemes, starts):
    """(score, gop) float64 (N,) each on the given segments, NaN for the empty ones."""
    starts = np.asarray(starts)
    score, gop = np.full(len(phonemes), np.nan), np.full(len(phonemes), np.nan)
    for n in np.flatnonzero(np.diff(starts) > 0):             # alignment_reference.scores on each present phoneme
        one_score, one_gop = R.scores(logp, [phonemes[n]], [starts[n], starts[n + 1]])
        score[n], gop[n] = one_score[0], one_gop[0]
    return score, gop


def check_starts(starts, frames, optional):
    """A valid segmentation with optional phonemes: N + 1 non-decreasing frames from 0 to T, empty segments only for
    optional phonemes.  Returns the flags of the phonemes left out."""
    starts = np.asarray(starts)
    count = len(optional)
    assert starts.shape == (count + 1,), starts.shape
    assert starts[0] == 0 and starts[count] == frames
    steps = np.diff(starts)
    assert (steps >= 0).all()
    dropped = steps == 0
    assert not (dropped & ~np.asarray(optional).astype(bool)).any()
    return dropped
