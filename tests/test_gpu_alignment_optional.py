"""Forced alignment with optional phonemes on the GPU (ppg_align_optional) against the float64 programme
of tests/alignment_optional_reference.py, which tests/test_alignment_optional_host.py holds against brute force.

The bounds are those of tests/test_gpu_alignment.py and are derived there, not measured: one logf within 1 ulp, then T
same-sign fp32 additions in frame order, and a maximum over paths (now also over the subsets of phonemes left out) of
values each within the bound: |total - ref| <= (T + 2) * 2^-23 * |ref|.  A left-out phoneme adds no term.  Scores and
GOP are the same sums over a present phoneme's own frames, plus an absolute 4e-6.  Boundaries are compared by cost,
never by identity, except where the input decides them: exact ties, or a margin orders of magnitude above the bound."""
import itertools

import numpy as np
import pytest
import torch

import ppgs_amd
from ppgs_amd import alignment, engine as E

import alignment_optional_reference as OR
import alignment_reference as R

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -23

# the (T, N) shapes of tests/test_gpu_alignment.py
PLAIN_CASES = [(1, 1), (300, 1), (64, 64), (65, 65), (63, 63), (64, 63), (200, 65), (700, 255), (700, 256), (700, 257),
               (4096, 37), (4096, 1024), (1024, 1024), (31, 31), (32, 31), (32, 32), (33, 32), (33, 33), (129, 64),
               (300, 256), (300, 257)]


def strip(count):
    return 1 if count <= 64 else 4 if count <= 256 else 16


def flags_for(count, pattern):
    """The optional flags of a transcript of `count` phonemes.
    'even' / 'odd': every second phoneme, from phoneme 0 / 1 (so opt[0] or, by the parity of N, opt[N-1] is set).
    'edges': around the boundaries between the lanes' strips of S states, alternately the last state of a strip
    (n = S-1 mod S) and the first of the next (n = 0 mod S), so that skips and the values they take cross lanes both
    ways; opt[0] and opt[N-1] as well where their neighbours allow."""
    flags = [False] * count
    if pattern in ('even', 'odd'):
        for n in range(0 if pattern == 'even' else 1, count, 2):
            flags[n] = True
    else:
        size = strip(count)
        for lane in range(1, -(-count // size)):
            n = lane * size - 1 if lane % 2 == 0 else lane * size
            if size == 1:
                n = 2 * lane                                   # every state is both: every second one
            if n < count:
                flags[n] = True
        for n in (0, count - 1):
            if not any(flags[max(n - 1, 0):n + 2]):
                flags[n] = True
    return flags


# (T, N, pattern).  T around the 32-frame staging chunk and the 64-frame trace-back refill; N = 64 / 65 and 256 / 257
# (the strip lengths change there) with optional phonemes at the strips' edges; T equal to the number of mandatory
# phonemes, so that every optional one must be left out; N > T; the limits once.
CASES = [(31, 21, 'even'), (32, 21, 'odd'), (33, 64, 'even'), (63, 65, 'edges'), (64, 65, 'even'), (65, 64, 'edges'),
         (129, 64, 'edges'), (200, 65, 'edges'), (300, 256, 'edges'), (300, 257, 'edges'),
         (32, 64, 'even'), (32, 64, 'odd'), (128, 256, 'odd'), (129, 257, 'even'), (31, 61, 'even'), (3, 7, 'even'),
         (1, 3, 'even'), (700, 256, 'even'), (700, 257, 'odd'), (4096, 1024, 'even')]


def test_the_cases_are_the_places_the_kernel_can_go_wrong():
    for frames, count, pattern in CASES:
        assert OR.legal(flags_for(count, pattern), frames), (frames, count, pattern)
    assert {t for t, _, _ in CASES} >= {31, 32, 33, 63, 64, 65} and {n for _, n, _ in CASES} >= {64, 65, 256, 257}
    for count in (65, 256, 257):
        flags, size = flags_for(count, 'edges'), strip(count)
        assert any(f and n % size == size - 1 for n, f in enumerate(flags))
        assert any(f and n % size == 0 and n > 0 for n, f in enumerate(flags))
    assert any(flags_for(n, p)[0] for _, n, p in CASES) and any(flags_for(n, p)[-1] for _, n, p in CASES)
    assert any(flags_for(n, p).count(False) == t for t, n, p in CASES) and any(n > t for t, n, _ in CASES)


@pytest.mark.parametrize('frames,count', PLAIN_CASES)
def test_no_optional_phoneme_is_the_plain_alignment_bit_for_bit(frames, count):
    generator = torch.Generator().manual_seed(1000 * frames + count)
    ppg = R.random_ppg(frames, 3., generator).cuda()
    phonemes = R.random_phonemes(count, generator)
    plain = alignment.forced(ppg, phonemes)
    got = alignment.forced(ppg, phonemes, optional=[False] * count)
    assert torch.equal(got.starts, plain.starts) and torch.equal(got.phonemes, plain.phonemes)
    for a, b in ((got.total, plain.total), (got.score, plain.score), (got.gop, plain.gop)):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    assert alignment.forced(ppg, phonemes, optional=torch.zeros(count, dtype=torch.bool), gop=False).gop is None


def check_against_reference(ppg, phonemes, flags, label):
    """One utterance on the device against the float64 programme; returns the relative error of the total and the
    number of phonemes the device left out."""
    frames, count = ppg.shape[1], len(phonemes)
    logp = R.log_posteriors(ppg)
    e = R.emissions(logp, phonemes)
    ref_total, _ = OR.programme(e, flags)
    got = alignment.forced(ppg.cuda(), phonemes, optional=flags)
    assert got.starts.dtype == torch.int32 and got.starts.is_cuda and got.phonemes.tolist() == list(phonemes)
    starts, total = got.starts.cpu().numpy(), float(got.total)
    dropped = OR.check_starts(starts, frames, flags)
    bound = (frames + 2) * EPS * abs(ref_total)
    error = abs(total - ref_total)
    print(f'optional alignment {label}: total {total:.6f} reference {ref_total:.6f} relative error '
          f'{error / max(abs(ref_total), 1e-30):.3e} (bound {(frames + 2) * EPS:.3e}), {int(dropped.sum())} of '
          f'{sum(flags)} optional phonemes left out')
    assert error <= bound, label
    assert OR.path_total(e, starts) >= ref_total - 2 * bound, label
    ref_score, ref_gop = OR.scores(logp, phonemes, starts)
    lengths = np.diff(starts)
    score, gop = got.score.cpu().numpy().astype(np.float64), got.gop.cpu().numpy().astype(np.float64)
    assert score.shape == gop.shape == (count,)
    # left-out phonemes are NaN in both, and nothing else is
    assert (np.isnan(score) == dropped).all() and (np.isnan(gop) == dropped).all(), label
    assert (np.isnan(ref_score) == dropped).all() and (np.isnan(ref_gop) == dropped).all(), label
    kept = ~dropped
    slack_score = np.abs(score - ref_score) - (4e-6 + (lengths + 2) * EPS * np.abs(ref_score))
    slack_gop = np.abs(gop - ref_gop) - (4e-6 + (lengths + 2) * EPS * np.abs(ref_gop))
    print(f'optional alignment {label}: score error {np.abs(score - ref_score)[kept].max():.3e}, gop error '
          f'{np.abs(gop - ref_gop)[kept].max():.3e}; closest to their bounds {slack_score[kept].max():.3e} '
          f'{slack_gop[kept].max():.3e} (<= 0 passes)')
    assert slack_score[kept].max() <= 0 and slack_gop[kept].max() <= 0, label
    assert (gop[kept] <= 0).all(), label
    return error / max(abs(ref_total), 1e-30), int(dropped.sum())


@pytest.mark.parametrize('frames,count,pattern', CASES)
def test_optimum_scores_and_gop_against_float64_programme(frames, count, pattern):
    generator = torch.Generator().manual_seed(1000 * frames + count)
    flags = flags_for(count, pattern)
    worst = 0.
    for scale in (1., 3., 8.):
        ppg = R.random_ppg(frames, scale, generator)
        phonemes = R.random_phonemes(count, generator)
        error, dropped = check_against_reference(ppg, phonemes, flags,
                                                 f'T={frames} N={count} {pattern} scale={scale}')
        worst = max(worst, error)
        if flags.count(False) == frames:
            assert dropped == sum(flags)                       # no frame to spare: every optional phoneme is left out
    print(f'optional alignment T={frames} N={count} {pattern}: largest relative error of total {worst:.3e}')


@pytest.mark.parametrize('frames,count,pattern', [(5, 3, 'odd'), (5, 3, 'even'), (40, 64, 'even'), (70, 65, 'edges'),
                                                  (150, 256, 'odd'), (300, 257, 'edges'), (128, 256, 'odd'),
                                                  (300, 1, 'odd')])
def test_a_uniform_ppg_is_decided_by_the_tie_rule_alone(frames, count, pattern):
    """Every emission is the same number, so every path into a cell has the same sum, in fp32 as in float64: stay beats
    advance beats skip, and the float64 programme's boundaries are the device's, exactly."""
    flags = flags_for(count, pattern)
    ppg = torch.full((40, frames), 1 / 40)
    generator = torch.Generator().manual_seed(frames + count)
    phonemes = R.random_phonemes(count, generator)
    _, starts = OR.programme(R.emissions(R.log_posteriors(ppg), phonemes), flags)
    got = alignment.forced(ppg.cuda(), phonemes, optional=flags)
    assert got.starts.tolist() == starts.tolist()
    value = float(np.log(np.float32(1 / 40)))
    assert abs(float(got.total) - frames * value) <= (frames + 2) * EPS * frames * abs(value)
    dropped = np.diff(starts) == 0
    assert (torch.isnan(got.score).cpu().numpy() == dropped).all()
    assert bool((got.gop[torch.from_numpy(~dropped).cuda()] == 0).all())
    if (frames, count, pattern) == (5, 3, 'odd'):
        assert starts.tolist() == [0, 1, 1, 5]                 # the last state is entered as early as it can be


def spoken(words, pauses, generator, low=1, high=7, lean=0.):
    """A PPG on which `words` (lists of phoneme indices) are said with a pause of pauses[i] frames before word i and
    pauses[-1] after the last (0: no pause): the intended label leads every frame's logits by 10.  Returns the PPG,
    the transcript (phonemes as indices, optional, word_of), the starts of that transcript and the frame labels.
    With `lean` the first half of a pause leans to the phoneme before it and the second half to the one after it."""
    names, optional, word_of = alignment.transcript(words, silence=True)
    index = [ppgs_amd.PHONEME_TO_INDEX_MAPPING[name] for name in names]
    durations, at = [], 0
    for n, word in enumerate(word_of):
        if word < 0:
            durations.append(pauses[at])
            at += 1
        else:
            durations.append(int(torch.randint(low, high, (1,), generator=generator)))
    starts = [0] + np.cumsum(durations).tolist()
    labels = torch.repeat_interleave(torch.tensor(index), torch.tensor(durations))
    frames = labels.shape[0]
    logits = torch.randn(40, frames, generator=generator)
    logits[labels, torch.arange(frames)] += 10.
    if lean:
        for n, word in enumerate(word_of):
            if word < 0 and durations[n]:
                middle = (starts[n] + starts[n + 1] + 1) // 2
                if n > 0:
                    logits[index[n - 1], starts[n]:(middle if n + 1 < len(index) else starts[n + 1])] += lean
                if n + 1 < len(index):
                    logits[index[n + 1], (middle if n > 0 else starts[n]):starts[n + 1]] += lean
    return torch.softmax(logits, dim=0), index, optional, word_of, starts, labels


def margin_of(ppg, labels):
    logp = torch.from_numpy(R.log_posteriors(ppg))
    frames = ppg.shape[1]
    target = logp[torch.arange(frames), labels]
    others = logp.clone()
    others[torch.arange(frames), labels] = -np.inf
    return float((target - others.max(dim=1).values).min())


def test_exact_paths_where_the_margin_allows_it():
    generator = torch.Generator().manual_seed(7)
    # 90 words of 1 .. 4 phonemes (none of them <silent>, no phoneme twice in a row): 91 optional pauses, some made
    words, last = [], 39
    for _ in range(90):
        word = []
        for _ in range(int(torch.randint(1, 5, (1,), generator=generator))):
            last = (last + 1 + int(torch.randint(0, 37, (1,), generator=generator))) % 39
            word.append(last)
        words.append(word)
    pauses = [int(v) for v in torch.randint(0, 4, (91,), generator=generator)]
    pauses[0], pauses[1], pauses[-1] = 0, 2, 0                 # a start in state 1 and an end in state N - 2
    ppg, index, optional, word_of, starts, labels = spoken(words, pauses, generator)
    frames, count = ppg.shape[1], len(index)
    assert all(a != b for a, b in zip(index, index[1:])) and count > 256 and 0 in pauses[1:-1]
    margin = margin_of(ppg, labels)
    print(f'optional alignment exact paths: T = {frames}, N = {count}, smallest margin {margin:.3f}')
    assert margin >= 1.0                                                   # a condition on the input
    got = alignment.forced(ppg.cuda(), index, optional=optional)
    assert got.starts.tolist() == starts
    dropped = torch.tensor(np.diff(starts) == 0)
    assert dropped.tolist() == [word < 0 and pauses[word_of[:n].count(-1)] == 0 for n, word in enumerate(word_of)]
    assert torch.equal(torch.isnan(got.gop).cpu(), dropped) and torch.equal(torch.isnan(got.score).cpu(), dropped)
    assert bool((got.gop.cpu()[~dropped] == 0).all()) and bool((got.score.cpu()[~dropped] < 0).all())
    expanded = alignment.frame_labels(got.starts, got.phonemes, frames)
    assert torch.equal(expanded.cpu().long(), ppg.argmax(0)) and torch.equal(expanded.cpu().long(), labels)
    # the other way round: the first and the last pause are made
    pauses[0], pauses[-1] = 3, 1
    ppg, index, optional, word_of, starts, labels = spoken(words, pauses, generator)
    assert margin_of(ppg, labels) >= 1.0
    got = alignment.forced(ppg.cuda(), index, optional=optional)
    assert got.starts.tolist() == starts and starts[1] == 3 and starts[-2] == starts[-1] - 1
    assert bool((got.gop.cpu()[torch.tensor(np.diff(starts) > 0)] == 0).all())


@pytest.mark.parametrize('frames,count,free', [(40, 9, (0, 4, 8)), (7, 9, (0, 2, 4, 8)), (90, 70, (0, 43, 64, 69)),
                                               (300, 260, (15, 32, 240, 259)), (150, 257, ()), (64, 6, (1, 3, 5))])
def test_total_is_the_best_plain_total_over_the_subsets_left_out_bit_for_bit(frames, count, free):
    """Both are the maximum over the same paths of the same fp32 sums added in frame order, and rounding is monotone."""
    generator = torch.Generator().manual_seed(100 * frames + count)
    if not free:                                                           # N > T: as many optional ones as it takes
        free = tuple(range(0, count, 2))
    flags = [n in free for n in range(count)]
    phonemes = R.random_phonemes(count, generator)
    subsets = [s for k in range(len(free) + 1) for s in itertools.combinations(free, k)] if len(free) <= 4 else [free]
    kept = [[p for n, p in enumerate(phonemes) if n not in subset] for subset in subsets]
    kept = [sequence for sequence in kept if 1 <= len(sequence) <= frames]
    for scale in (1., 3., 8.):
        ppg = R.random_ppg(frames, scale, generator).cuda()
        got = alignment.forced(ppg, phonemes, optional=flags)
        plain = alignment.forced(ppg[None].expand(len(kept), -1, -1), kept, [frames] * len(kept))
        best = plain.total.max()
        print(f'optional alignment T={frames} N={count} scale={scale}: total {float(got.total):.6f}, best of '
              f'{len(kept)} plain alignments {float(best):.6f}')
        if len(free) <= 4:
            assert torch.equal(got.total.view(torch.int32), best.view(torch.int32))
        else:                                                  # (the one subset that fits is a lower bound only)
            assert float(got.total) >= float(best)


def ragged_batch():
    """33 items, padded with NaN and -1; items 5, 11, 17, 23 and 29 cannot be aligned, each in its own way."""
    generator = torch.Generator().manual_seed(33)
    lengths = torch.randint(1, 301, (33,), generator=generator).tolist()
    counts = [int(torch.randint(1, 301, (1,), generator=generator)) for _ in lengths]
    lengths[0], counts[0], lengths[1], counts[1], lengths[2], counts[2] = 1, 1, 300, 300, 300, 1
    lengths[3], counts[3] = 150, 300
    ppg = torch.full((33, 40, 300), float('nan'))
    table = torch.full((33, max(counts)), -1, dtype=torch.int64)
    flags = torch.full((33, max(counts)), -1, dtype=torch.int64)
    for b in range(33):
        ppg[b, :, :lengths[b]] = R.random_ppg(lengths[b], 3., generator)
        table[b, :counts[b]] = torch.tensor(R.random_phonemes(counts[b], generator))
        row = flags_for(counts[b], ('even', 'odd', 'edges')[b % 3])
        while row.count(False) > lengths[b]:                   # more mandatory phonemes than frames: a shorter transcript
            counts[b] = max(1, counts[b] // 2)
            row = flags_for(counts[b], 'odd')
        if row.count(False) < 1:
            row = [False] * counts[b]
        flags[b, :counts[b]] = torch.tensor(row, dtype=torch.int64)
        table[b, counts[b]:], flags[b, counts[b]:] = -1, -1
    impossible = (5, 11, 17, 23, 29)
    lengths[5], counts[5] = 200, 100
    flags[5, :100] = 0
    flags[5, 40:42] = 1                                        # two adjacent optional phonemes
    table[5, :100] = torch.tensor(R.random_phonemes(100, generator))
    lengths[11], counts[11] = 50, 1
    flags[11, 0], table[11, 0] = 1, 3                          # no mandatory phoneme
    lengths[17], counts[17] = 10, 31
    flags[17, :31] = torch.tensor(flags_for(31, 'even'), dtype=torch.int64)     # 15 mandatory phonemes, 10 frames
    table[17, :31] = 7
    lengths[23], counts[23] = 80, 20
    flags[23, :20], table[23, :20] = 0, 4
    table[23, 19] = 40                                         # a phoneme index outside 0 .. 39
    lengths[29], counts[29] = 301, 5                           # T beyond the padded frames
    flags[29, :5], table[29, :5] = 0, 9
    for b in impossible:
        ppg[b, :, :min(lengths[b], 300)] = R.random_ppg(min(lengths[b], 300), 3., generator)
    return ppg, table, flags, lengths, counts, impossible


def test_batch_equals_singles_also_from_two_streams():
    ppg, table, flags, lengths, counts, impossible = ragged_batch()
    device = ppg.cuda()
    assert any(c > t for b, (t, c) in enumerate(zip(lengths, counts)) if b not in impossible)
    singles = {}
    for b in range(33):
        if b not in impossible:
            singles[b] = alignment.forced(device[b, :, :lengths[b]], table[b, :counts[b]],
                                          optional=flags[b, :counts[b]])
            assert bool(torch.isfinite(singles[b].total))
            OR.check_starts(singles[b].starts.cpu().numpy(), lengths[b], flags[b, :counts[b]].tolist())

    def check(result, low=0):
        total, starts, score, gop = result
        for b in range(low, low + total.shape[0]):
            at = b - low
            if b in impossible:                                # total = NaN, the rest as it was: zeros
                assert bool(torch.isnan(total[at])), b
                assert not starts[at].any() and not score[at].any() and not gop[at].any(), b
                continue
            one, n = singles[b], counts[b]
            assert torch.equal(total[at].view(torch.int32), one.total.view(torch.int32)), b
            assert torch.equal(starts[at, :n + 1], one.starts), b
            assert torch.equal(score[at, :n].view(torch.int32), one.score.view(torch.int32)), b
            assert torch.equal(gop[at, :n].view(torch.int32), one.gop.view(torch.int32)), b
            assert not starts[at, n + 1:].any() and not score[at, n:].any(), b

    check(E.align_items(device, lengths, table, counts, optional=flags))
    # the items that can be aligned, through the module: lists and tables
    fine = [b for b in range(33) if b not in impossible]
    batch = alignment.forced(device[fine], table[fine], [lengths[b] for b in fine], [counts[b] for b in fine],
                             optional=flags[fine])
    as_lists = alignment.forced(device[fine], [table[b, :counts[b]].tolist() for b in fine], [lengths[b] for b in fine],
                                optional=[flags[b, :counts[b]].bool().tolist() for b in fine])
    for at, b in enumerate(fine):
        for result in (batch, as_lists):
            assert torch.equal(result.starts[at], singles[b].starts), b
            assert torch.equal(result.total[at], singles[b].total), b
            assert torch.equal(result.gop[at].view(torch.int32), singles[b].gop.view(torch.int32)), b
    # the two halves from two streams at once
    torch.cuda.synchronize()
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    halves = [(0, 16), (16, 33)]
    results = [[], []]
    for _ in range(3):
        for side, (low, high) in enumerate(halves):
            with torch.cuda.stream(streams[side]):
                results[side].append(E.align_items(device[low:high], lengths[low:high], table[low:high],
                                                   counts[low:high], optional=flags[low:high]))
    torch.cuda.synchronize()
    for side, (low, _) in enumerate(halves):
        for result in results[side]:
            check(result, low)


def raw_optional(ppg, lengths, table, flags, counts, workspace, want_gop=True, frames=None, items=None, most=None,
                 size=None, offset=0):
    """ppg_align_optional through ctypes with the caller's workspace; outputs start as sentinels:
    (rc, total, starts, score, gop)."""
    lib = E.library()
    both = torch.tensor([lengths, counts], dtype=torch.int32).cuda()
    total = torch.full((ppg.shape[0],), -7., device='cuda')
    starts = torch.full((ppg.shape[0], table.shape[1] + 1), -7, dtype=torch.int32, device='cuda')
    score = torch.full((ppg.shape[0], table.shape[1]), -7., device='cuda')
    gop = torch.full((ppg.shape[0], table.shape[1]), -7., device='cuda')
    torch.cuda.synchronize()
    rc = lib.ppg_align_optional(
        0, ppg.data_ptr(), ppg.shape[2] if frames is None else frames, ppg.shape[0] if items is None else items,
        both[0].data_ptr(), table.data_ptr(), flags.data_ptr(), table.shape[1] if most is None else most,
        both[1].data_ptr(), total.data_ptr(), starts.data_ptr(), score.data_ptr(),
        gop.data_ptr() if want_gop else None, workspace.data_ptr() + offset,
        workspace.numel() - offset if size is None else size, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return rc, total, starts, score, gop


def small_problem():
    generator = torch.Generator().manual_seed(12)
    ppg = torch.stack([R.random_ppg(100, 3., generator), R.random_ppg(100, 8., generator)]).cuda().contiguous()
    table = torch.randint(0, 40, (2, 70), generator=generator, dtype=torch.int32).cuda()
    flags = torch.tensor([flags_for(70, 'edges'), flags_for(70, 'even')], dtype=torch.int32).cuda()
    return ppg, table, flags, [100, 83], [70, 5]


def test_poisoned_workspace_gives_the_same_bits():
    generator = torch.Generator().manual_seed(4)
    size = E.library().ppg_align_optional_workspace_bytes
    workspace = torch.zeros(size(1, 4096, 1024), dtype=torch.uint8, device='cuda')
    large = R.random_ppg(4096, 3., generator)[None].cuda().contiguous()
    large_table = torch.randint(0, 40, (1, 1024), generator=generator, dtype=torch.int32).cuda()
    large_flags = torch.tensor([flags_for(1024, 'edges')], dtype=torch.int32).cuda()
    rc, total, _, _, _ = raw_optional(large, [4096], large_table, large_flags, [1024], workspace)
    assert rc == 0 and bool(torch.isfinite(total).all())
    ppg, table, flags, lengths, counts = small_problem()
    assert size(2, 100, 70) <= workspace.numel()
    reused = raw_optional(ppg, lengths, table, flags, counts, workspace)
    fresh = raw_optional(ppg, lengths, table, flags, counts,
                         torch.zeros(size(2, 100, 70), dtype=torch.uint8, device='cuda'))
    poisoned = raw_optional(ppg, lengths, table, flags, counts,
                            torch.full((size(2, 100, 70),), 255, dtype=torch.uint8, device='cuda'))
    assert reused[0] == fresh[0] == poisoned[0] == 0
    for a, b, c in zip(reused[1:], fresh[1:], poisoned[1:]):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))
        assert torch.equal(a.view(torch.int32), c.view(torch.int32))
    through_module = alignment.forced(ppg, table, lengths, counts, optional=flags)
    assert torch.equal(through_module.total, fresh[1])
    assert torch.equal(through_module.starts[1], fresh[2][1, :6])
    assert torch.equal(through_module.gop[0].view(torch.int32), fresh[4][0].view(torch.int32))
    assert bool((fresh[2][1, 6:] == -7).all()) and bool((fresh[3][1, 5:] == -7).all())      # the rest is left alone
    without = raw_optional(ppg, lengths, table, flags, counts, workspace, want_gop=False)
    assert without[0] == 0 and torch.equal(without[3].view(torch.int32), fresh[3].view(torch.int32))
    assert bool((without[4] == -7).all())


def test_error_paths_launch_nothing_and_impossible_items_give_nan():
    lib = E.library()
    ppg, table, flags, lengths, counts = small_problem()
    need = lib.ppg_align_optional_workspace_bytes(2, 100, 70)
    workspace = torch.zeros(need + 64, dtype=torch.uint8, device='cuda')
    assert workspace.data_ptr() % 16 == 0
    refused = [
        raw_optional(ppg, lengths, table, flags, counts, workspace, size=need - 1),            # workspace too small
        raw_optional(ppg, lengths, table, flags, counts, workspace, size=lib.ppg_align_workspace_bytes(2, 100, 70)),
        raw_optional(ppg, lengths, table, flags, counts, workspace, offset=8),                 # misaligned
        raw_optional(ppg, lengths, table, flags, counts, workspace, frames=E.ALIGN_MAX_FRAMES + 1, size=1 << 40),
        raw_optional(ppg, lengths, table, flags, counts, workspace, most=E.ALIGN_MAX_PHONEMES + 1, size=1 << 40),
        raw_optional(ppg, lengths, table, flags, counts, workspace, items=E.ALIGN_MAX_ITEMS + 1, size=1 << 50),
        raw_optional(ppg, lengths, table, flags, counts, workspace, items=0),
    ]
    for rc, total, starts, score, gop in refused:
        assert rc == -1 and lib.ppg_last_error()
        assert bool((total == -7).all()) and bool((starts == -7).all()) and bool((score == -7).all())
        assert bool((gop == -7).all())
    assert not workspace.any()                                                             # nothing was launched
    # impossible device-side items: total = NaN, starts untouched, the neighbours unharmed.  Pointers stay in range.
    good = raw_optional(ppg, lengths, table, flags, counts, workspace)
    assert good[0] == 0 and bool(torch.isfinite(good[1]).all())
    high, negative, adjacent, every, many = table.clone(), table.clone(), flags.clone(), flags.clone(), flags.clone()
    high[0, 3], negative[1, 4] = 40, -1
    adjacent[0, 30:32] = 1
    every[1, :5] = torch.tensor([1, 0, 1, 0, 1], dtype=torch.int32)                        # (legal: two mandatory ones)
    many[0, :70] = 0
    cases = (
        ([100, 83], [0, 5], table, flags, 0),                  # N < 1
        ([100, 83], [70, -3], table, flags, 1),
        ([100, 83], [71, 5], table, flags, 0),                 # N beyond the table
        ([0, 83], [70, 5], table, flags, 0),                   # T outside [1, frames]
        ([100, 101], [70, 5], table, flags, 1),
        ([100, 83], [70, 5], high, flags, 0),                  # a phoneme index outside 0 .. 39
        ([100, 83], [70, 5], negative, flags, 1),
        ([100, 83], [70, 5], table, adjacent, 0),              # two adjacent optional phonemes
        ([100, 83], [70, 1], table, every, 1),                 # no mandatory phoneme: the only one is optional
        ([100, 1], [70, 5], table, every, 1),                  # two mandatory phonemes, one frame
        ([69, 83], [70, 5], table, many, 0))                   # 70 mandatory phonemes, 69 frames
    for bad_lengths, bad_counts, bad_table, bad_flags, item in cases:
        rc, total, starts, score, gop = raw_optional(ppg, bad_lengths, bad_table, bad_flags, bad_counts, workspace)
        other = 1 - item
        assert rc == 0 and bool(torch.isnan(total[item])), (bad_lengths, bad_counts)
        assert bool((starts[item] == -7).all()) and bool((score[item] == -7).all()) and bool((gop[item] == -7).all())
        # (every case leaves the neighbour's own lengths, phonemes and flags as they are in `good`)
        assert torch.equal(total[other], good[1][other]) and torch.equal(starts[other], good[2][other])
        assert torch.equal(score[other].view(torch.int32), good[3][other].view(torch.int32))
        assert torch.equal(gop[other].view(torch.int32), good[4][other].view(torch.int32))
    # N > T is legal where the mandatory phonemes fit: item 1 with 5 phonemes, 2 of them mandatory, on 2 frames
    rc, total, starts, score, _ = raw_optional(ppg, [100, 2], table, every, [70, 5], workspace)
    assert rc == 0 and bool(torch.isfinite(total).all()) and starts[1, :6].tolist() == [0, 0, 1, 1, 2, 2]
    assert torch.isnan(score[1, :5]).tolist() == [True, False, True, False, True]
    # an index outside 0 .. 39 or adjacent flags past the item's own N are padding: never read
    rc, total, starts, _, _ = raw_optional(ppg, [100, 83], high, adjacent, [3, 5], workspace)
    assert rc == 0 and bool(torch.isfinite(total).all()) and starts[0, :4].tolist()[::3] == [0, 100]


def test_pauses_between_words_as_a_speaker_makes_them():
    generator = torch.Generator().manual_seed(21)
    words = [['hh', 'ah', 'l', 'ow'], ['w', 'er', 'l', 'd'], ['ae', 'n', 'd'], ['g', 'uh', 'd'], ['b', 'ay']]
    pauses = [6, 0, 9, 0, 4, 0]                                # before the first word, between words, after the last
    indices = [[ppgs_amd.PHONEME_TO_INDEX_MAPPING[name] for name in word] for word in words]
    ppg, index, optional, word_of, starts, labels = spoken(indices, pauses, generator, low=3, high=9, lean=5.)
    assert margin_of(ppg, labels) >= 1.0
    names, flags, again = alignment.transcript(words, silence=True)
    assert [ppgs_amd.PHONEME_TO_INDEX_MAPPING[name] for name in names] == index and again == word_of
    device = ppg.cuda()
    got = alignment.forced(device, names, optional=flags)
    assert got.starts.tolist() == starts                                   # the boundaries are exact
    of_words = torch.tensor([word >= 0 for word in word_of])
    assert bool((got.gop.cpu()[of_words] == 0).all())                      # every word phoneme is the argmax of its frames
    made = [n for n, word in enumerate(word_of) if word < 0 and starts[n] < starts[n + 1]]
    assert [n for n in range(len(names)) if starts[n] == starts[n + 1]] == [5, 14, 21]
    assert bool(torch.isnan(got.gop[[5, 14, 21]]).all()) and bool((got.gop[made] == 0).all())
    listed = alignment.word_segments(got, word_of)
    assert [w[0] for w in listed] == [0, 1, 2, 3, 4] and all(w[3] == 0. for w in listed)
    assert listed[0][1:3] == (starts[1] * 160 / 16000, starts[5] * 160 / 16000) and starts[1] == 6
    assert listed[1][2] == starts[10] * 160 / 16000 and listed[2][1] == starts[11] * 160 / 16000     # 9 frames apart
    # the plain alignment of the words alone has nowhere to put the pauses but into the phonemes beside them
    flat = [name for word in words for name in word]
    plain = alignment.forced(device, flat)
    ours = got.gop.cpu()[of_words]
    beside = [0, 7, 8, 13, 14]        # 'hh' after the first pause; 'd' | 'ae' and 'd' | 'b' around the two inside
    print(f'optional alignment, pauses: plain gop beside the pauses {plain.gop.cpu()[beside].tolist()}, total '
          f'{float(plain.total):.3f} against {float(got.total):.3f}')
    assert bool((plain.gop.cpu()[beside] < ours[beside]).all())
    assert float(plain.total) < float(got.total)
