"""CPU restatement of ppgs_amd.alignment for the tests (tests/test_alignment_host.py, tests/test_gpu_alignment.py):
float64 emissions from the oracle-style clamp, a float64 programme with the documented tie rule (advance only if
strictly better) vectorised over the phonemes per frame, its own trace-back, scores and GOP, and a brute-force
enumerator over every monotone segmentation for tiny cases."""
import itertools

import numpy as np
import torch


def log_posteriors(ppg):
    """(40, T) -> (T, 40) float64: the log of the PPG clamped as oracle.distance clamps it (in fp32, so the clamped
    value is exactly what an fp32 implementation sees)."""
    clamped = ppg.float().clamp(1e-8, 1 - 1e-8)
    return np.log(clamped.double().numpy()).T.copy()


def emissions(logp, phonemes):
    """(T, N) float64: e[t, n] = logp[t, phonemes[n]]."""
    return logp[:, np.asarray(phonemes, dtype=np.int64)]


def programme(e):
    """(total, starts) of the float64 programme over e (T, N); starts is (N + 1,) int64."""
    e = np.asarray(e, dtype=np.float64)
    frames, count = e.shape
    assert 1 <= count <= frames
    best = np.full(count, -np.inf)
    best[0] = e[0, 0]
    advanced = np.zeros((frames, count), dtype=bool)
    for t in range(1, frames):
        below = np.concatenate([[-np.inf], best[:-1]])
        advance = below > best                              # a tie stays
        best = e[t] + np.where(advance, below, best)
        advanced[t] = advance
    starts = np.zeros(count + 1, dtype=np.int64)
    starts[count] = frames
    n = count - 1
    for t in range(frames - 1, 0, -1):
        if advanced[t, n]:
            starts[n] = t
            n -= 1
    assert n == 0
    return float(best[count - 1]), starts


def path_total(e, starts):
    """The sum of e along the segmentation, added in frame order."""
    e = np.asarray(e, dtype=np.float64)
    total = 0.
    for n in range(e.shape[1]):
        for t in range(int(starts[n]), int(starts[n + 1])):
            total += e[t, n]
    return total


def brute_force(e):
    """(total, starts) by enumerating every monotone segmentation: the largest sum, and among equal sums the one
    the tie rule picks -- the trace-back stays wherever staying is optimal, so the last phoneme starts as early as
    it can, then the one before it, and so on."""
    e = np.asarray(e, dtype=np.float64)
    frames, count = e.shape
    chosen = None
    for cuts in itertools.combinations(range(1, frames), count - 1):
        starts = (0,) + cuts + (frames,)
        key = (-path_total(e, starts), tuple(reversed(cuts)))
        if chosen is None or key < chosen[0]:
            chosen = (key, starts)
    return -chosen[0][0], np.asarray(chosen[1], dtype=np.int64)


def scores(logp, phonemes, starts):
    """(score, gop) float64 (N,) each, on the given segments."""
    e = emissions(logp, phonemes)
    top = logp.max(axis=1)
    score, gop = np.empty(len(phonemes)), np.empty(len(phonemes))
    for n in range(len(phonemes)):
        a, b = int(starts[n]), int(starts[n + 1])
        score[n] = e[a:b, n].mean()
        gop[n] = (e[a:b, n] - top[a:b]).mean()
    return score, gop


def check_starts(starts, frames, count):
    """A valid segmentation: N + 1 strictly increasing frames from 0 to T."""
    starts = np.asarray(starts)
    assert starts.shape == (count + 1,), starts.shape
    assert starts[0] == 0 and starts[count] == frames
    assert (np.diff(starts) >= 1).all()


def decode(ppg):
    """(phonemes, starts) int64 from torch.argmax + torch.unique_consecutive on the CPU; starts is (runs + 1,)."""
    labels = ppg.argmax(dim=0)
    phonemes, counts = torch.unique_consecutive(labels, return_counts=True)
    starts = torch.cat([torch.zeros(1, dtype=torch.int64), counts.cumsum(0)])
    return phonemes.numpy(), starts.numpy()


def random_ppg(frames, scale, generator):
    return torch.softmax(scale * torch.randn(40, frames, generator=generator), dim=0)


def random_phonemes(count, generator):
    return torch.randint(0, 40, (count,), generator=generator).tolist()
