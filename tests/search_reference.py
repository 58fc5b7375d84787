"""CPU restatement of ppgs_amd.alignment.search for the tests (tests/test_search_host.py, tests/test_gpu_search.py):
float64 emissions (the log-likelihood ratio against the frame's best phoneme, from the oracle-style clamp), the float64
programme with a free start at every frame that carries the begin of every partial match, the picker, a vectorised
re-scoring of given spans, and brute force over every (begin, end, segmentation) for tiny cases."""
import itertools

import numpy as np

import alignment_reference as A

log_posteriors = A.log_posteriors
random_ppg = A.random_ppg
random_phonemes = A.random_phonemes


def emissions(logp, phonemes):
    """(T, N) float64: r[t, n] = logp[t, phonemes[n]] - max_q logp[t, q]: <= 0, exactly 0 at the frame's maximum."""
    return logp[:, np.asarray(phonemes, dtype=np.int64)] - logp.max(axis=1)[:, None]


def programme(r):
    """The curve of r (..., T, N): (curve_total float64, curve_begin int64), each (..., T); leading axes are
    independent problems that share the loop over frames."""
    r = np.asarray(r, dtype=np.float64)
    lead, (frames, count) = r.shape[:-2], r.shape[-2:]
    best = np.full(lead + (count,), -np.inf)
    begin = np.full(lead + (count,), -1, dtype=np.int64)
    curve_total = np.full(lead + (frames,), -np.inf)
    curve_begin = np.full(lead + (frames,), -1, dtype=np.int64)
    origin = np.zeros(lead + (1,))
    for t in range(frames):
        below = np.concatenate([origin, best[..., :-1]], axis=-1)        # the origin: 0, beginning here, at every frame
        source = np.concatenate([np.full(lead + (1,), t, dtype=np.int64), begin[..., :-1]], axis=-1)
        advance = below > best                                           # a tie stays
        best = r[..., t, :] + np.where(advance, below, best)
        begin = np.where(advance, source, begin)
        curve_total[..., t] = best[..., -1]
        curve_begin[..., t] = begin[..., -1]
    return curve_total, curve_begin


def brute_force(r):
    """The curve of r (T, N) by enumerating, per end frame, every begin and every monotone segmentation: the largest
    sum (added in frame order), and among equal sums the last phoneme starts earliest, then the one before it, ...,
    then the earliest begin."""
    r = np.asarray(r, dtype=np.float64)
    frames, count = r.shape
    curve_total = np.full(frames, -np.inf)
    curve_begin = np.full(frames, -1, dtype=np.int64)
    for t in range(count - 1, frames):
        chosen = None
        for first in range(0, t - count + 2):
            for cuts in itertools.combinations(range(first + 1, t + 1), count - 1):
                starts = (first,) + cuts
                total = A.path_total(r[:t + 1], starts + (t + 1,))
                key = (-total, tuple(reversed(starts)))
                if chosen is None or key < chosen:
                    chosen = key
        curve_total[t], curve_begin[t] = -chosen[0], chosen[1][-1]
    return curve_total, curve_begin


def means(curve_total, curve_begin, dtype):
    """mean[t] = curve_total[t] / (t - curve_begin[t] + 1) as one division in `dtype`; where no match ends, -inf."""
    curve_begin = np.asarray(curve_begin, dtype=np.int64)
    time = np.arange(curve_begin.shape[0])
    length = np.where(curve_begin >= 0, time - curve_begin + 1, 1).astype(dtype)
    return np.where(curve_begin >= 0, np.asarray(curve_total).astype(dtype) / length, dtype(-np.inf)).astype(dtype)


def pick(curve_total, curve_begin, count, top, threshold=-np.inf, dtype=np.float32):
    """The hits of one curve as a list of (begin, end, total, mean), best first: numpy over the end frames."""
    curve_begin = np.asarray(curve_begin, dtype=np.int64)
    time = np.arange(curve_begin.shape[0])
    mean = means(curve_total, curve_begin, dtype)
    alive = (time >= count - 1) & (curve_begin >= 0)
    hits = []
    for _ in range(top):
        if not alive.any():
            break
        best = mean[alive].max()
        if best < threshold:
            break
        at = int(time[alive & (mean == best)].max())                     # ties: the largest end frame
        hits.append((int(curve_begin[at]), at + 1, dtype(curve_total[at]), mean[at]))
        alive &= ~((curve_begin < at + 1) & (time >= curve_begin[at]))    # spans that meet frames begin .. at
    return hits


def pick_by_the_letter(curve_total, curve_begin, count, top, threshold=-np.inf, dtype=np.float32):
    """`pick` restated word for word from the definition: candidates tested against every hit taken so far."""
    mean = means(curve_total, curve_begin, dtype)
    hits = []
    for _ in range(top):
        chosen = None
        for t in range(count - 1, len(curve_begin)):
            first = int(curve_begin[t])
            if first < 0 or any(first < end and begin < t + 1 for begin, end, _, _ in hits):
                continue
            if chosen is None or (mean[t], t) > (mean[chosen], chosen):
                chosen = t
        if chosen is None or mean[chosen] < threshold:
            break
        hits.append((int(curve_begin[chosen]), chosen + 1, dtype(curve_total[chosen]), mean[chosen]))
    return hits


def rescore(r, curve_begin):
    """(T,) float64: for every end frame t with curve_begin[t] >= 0 the best sum over the segmentations of frames
    curve_begin[t] .. t alone (the first phoneme starts at curve_begin[t], the last ends at t); NaN elsewhere.  All
    begins advance together: after j steps row b holds the programme pinned to a start at frame b, at frame b + j."""
    r = np.asarray(r, dtype=np.float64)
    frames, count = r.shape
    curve_begin = np.asarray(curve_begin, dtype=np.int64)
    time = np.arange(frames)
    span = np.where(curve_begin >= 0, time - curve_begin + 1, 0)
    out = np.full(frames, np.nan)
    best = np.full((frames, count), -np.inf)
    best[:, 0] = r[:, 0]
    for j in range(int(span.max())):
        if j:
            best = best[:frames - j]
            below = np.concatenate([np.full((frames - j, 1), -np.inf), best[:, :-1]], axis=1)
            best = r[j:] + np.maximum(best, below)
        ends = np.nonzero(span == j + 1)[0]
        out[ends] = best[curve_begin[ends], count - 1]
    return out
