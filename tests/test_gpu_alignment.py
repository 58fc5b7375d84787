"""ppgs_amd.alignment on the GPU against the CPU restatement of tests/alignment_reference.py (float64 emissions from
the oracle-style clamp, a float64 programme with the same tie rule).

The bound on a total is derived, not measured: a clamped input is exact and logf is within 1 ulp, so every emission
is within 2^-23 relative; sequential fp32 summation of T same-sign terms adds (T - 1) * 2^-24 relative; and the
maximum over paths of values each within the bound is within the bound: (T + 2) * 2^-23 * |total|.  A phoneme's
score and GOP are the same sums over its own frames, plus an absolute 4e-6 for the two logf values of magnitude up
to 18.5 that a GOP term subtracts.  Boundaries are compared by cost, never by identity, except where the input's own
margin is orders of magnitude above that bound."""
import numpy as np
import pytest
import torch

import ppgs_amd
from ppgs_amd import alignment, engine as E

import alignment_reference as R

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -23

# (T, N): pure diagonals, every strip length (N <= 64: 1 state per lane, <= 256: 4, above: 16) and its edges, the
# 32-frame staging chunk and the 64-frame trace-back refill and their edges, and the limits
CASES = [(1, 1), (300, 1), (64, 64), (65, 65), (63, 63), (64, 63), (200, 65), (700, 255), (700, 256), (700, 257),
         (4096, 37), (4096, 1024), (1024, 1024), (31, 31), (32, 31), (32, 32), (33, 32), (33, 33), (129, 64),
         (300, 256), (300, 257)]


def check_against_reference(ppg, phonemes, label):
    """One utterance on the device against the float64 programme; returns the relative error of the total."""
    frames, count = ppg.shape[1], len(phonemes)
    logp = R.log_posteriors(ppg)
    e = R.emissions(logp, phonemes)
    ref_total, _ = R.programme(e)
    got = alignment.forced(ppg.cuda(), phonemes)
    assert got.starts.dtype == torch.int32 and got.starts.is_cuda and got.phonemes.tolist() == list(phonemes)
    starts, total = got.starts.cpu().numpy(), float(got.total)
    R.check_starts(starts, frames, count)
    bound = (frames + 2) * EPS * abs(ref_total)
    error = abs(total - ref_total)
    print(f'alignment {label}: total {total:.6f} reference {ref_total:.6f} relative error '
          f'{error / max(abs(ref_total), 1e-30):.3e} (bound {(frames + 2) * EPS:.3e})')
    assert error <= bound, label
    assert R.path_total(e, starts) >= ref_total - 2 * bound, label
    ref_score, ref_gop = R.scores(logp, phonemes, starts)
    lengths = np.diff(starts)
    score, gop = got.score.cpu().numpy().astype(np.float64), got.gop.cpu().numpy().astype(np.float64)
    assert score.shape == gop.shape == (count,)
    worst_score = (np.abs(score - ref_score) - (4e-6 + (lengths + 2) * EPS * np.abs(ref_score))).max()
    worst_gop = (np.abs(gop - ref_gop) - (4e-6 + (lengths + 2) * EPS * np.abs(ref_gop))).max()
    print(f'alignment {label}: score error {np.abs(score - ref_score).max():.3e}, gop error '
          f'{np.abs(gop - ref_gop).max():.3e}; closest to their bounds {worst_score:.3e} {worst_gop:.3e} (<= 0 passes)')
    assert worst_score <= 0 and worst_gop <= 0, label
    assert (gop <= 0).all(), label
    return error / max(abs(ref_total), 1e-30)


@pytest.mark.parametrize('frames,count', CASES)
def test_optimum_scores_and_gop_against_float64_programme(frames, count):
    generator = torch.Generator().manual_seed(1000 * frames + count)
    worst = 0.
    for scale in (1., 3., 8.):
        ppg = R.random_ppg(frames, scale, generator)
        phonemes = R.random_phonemes(count, generator)
        worst = max(worst, check_against_reference(ppg, phonemes, f'T={frames} N={count} scale={scale}'))
    print(f'alignment T={frames} N={count}: largest relative error of total {worst:.3e}')


def test_optimum_on_the_reference_fixture(golden):
    ppg = torch.from_numpy(golden('g9_postops')['x'])
    assert ppg.shape == (40, 57)
    generator = torch.Generator().manual_seed(57)
    check_against_reference(ppg, R.random_phonemes(9, generator), 'fixture T=57 N=9')
    free, _ = R.decode(ppg)
    check_against_reference(ppg, free.tolist(), f'fixture T=57 on its own decode N={len(free)}')


def known_segmentation():
    generator = torch.Generator().manual_seed(7)
    count = 200
    phonemes = (7 * torch.arange(count)) % 40
    durations = torch.randint(1, 7, (count,), generator=generator)
    labels = torch.repeat_interleave(phonemes, durations)
    frames = labels.shape[0]
    logits = torch.randn(40, frames, generator=generator)
    logits[labels, torch.arange(frames)] += 10.
    starts = torch.cat([torch.zeros(1, dtype=torch.int64), durations.cumsum(0)])
    return torch.softmax(logits, dim=0), phonemes, starts, labels


def test_exact_boundaries_where_the_margin_allows_it():
    ppg, phonemes, starts, labels = known_segmentation()
    frames = ppg.shape[1]
    logp = torch.from_numpy(R.log_posteriors(ppg))                         # (T, 40)
    target = logp[torch.arange(frames), labels]
    others = logp.clone()
    others[torch.arange(frames), labels] = -np.inf
    margin = float((target - others.max(dim=1).values).min())
    print(f'alignment exact boundaries: T = {frames}, smallest margin of the target log-posterior {margin:.3f}')
    assert margin >= 1.0                                                   # a condition on the input
    device = ppg.cuda()
    got = alignment.forced(device, phonemes)
    assert got.starts.tolist() == starts.tolist()
    assert bool((got.gop == 0).all()) and bool((got.score < 0).all())
    assert torch.equal(got.score, alignment.forced(device, phonemes, gop=False).score)
    assert alignment.forced(device, phonemes, gop=False).gop is None
    free = alignment.decode(device)
    assert free.phonemes.dtype == torch.int32 and free.phonemes.is_cuda
    assert free.phonemes.tolist() == phonemes.tolist() and free.starts.tolist() == starts.tolist()
    again = alignment.forced(device, free.phonemes)
    assert torch.equal(again.starts, free.starts) and torch.equal(again.total, got.total)
    by_name = alignment.forced(device, [ppgs_amd.PHONEMES[p] for p in phonemes.tolist()])
    assert torch.equal(by_name.starts, got.starts) and torch.equal(by_name.score, got.score)
    expanded = alignment.frame_labels(got.starts, got.phonemes, frames)
    assert expanded.is_cuda and torch.equal(expanded.cpu().long(), ppg.argmax(0))
    listed = alignment.segments(got)
    assert len(listed) == 200 and listed[0][0] == 'aa' and listed[-1][2] == frames * 160 / 16000
    # CPU tensors are moved to the device, half precision is promoted, as in the other post-ops
    assert torch.equal(alignment.forced(ppg, phonemes).starts, got.starts)
    half = alignment.forced(device.half(), phonemes)
    assert half.total.dtype == torch.float32
    assert torch.equal(half.total, alignment.forced(device.half().float(), phonemes).total)


def tied_ppg(frames, generator):
    """A PPG with exact ties (rows 5 and 17 equal and largest), all-equal frames, and clear frames, in thirds."""
    ppg = R.random_ppg(frames, 3., generator)
    third = frames // 3
    ppg[5, :third] = ppg[17, :third] = 2.
    ppg[:, third:2 * third] = 1 / 40
    return ppg


def test_decode_equals_argmax_and_unique_consecutive(golden):
    generator = torch.Generator().manual_seed(3)
    inputs = [('fixture', torch.from_numpy(golden('g9_postops')['x']))]
    for frames in (1, 63, 64, 65, 4096):
        inputs.append((f'random T={frames}', R.random_ppg(frames, 3., generator)))
        inputs.append((f'ties T={frames}', tied_ppg(frames, generator)))
        single = R.random_ppg(frames, 1., generator)
        single[23] = 2.
        inputs.append((f'single run T={frames}', single))
        inputs.append((f'all equal T={frames}', torch.full((40, frames), 1 / 40)))
        slow = R.random_ppg(-(-frames // 7), 3., generator).repeat_interleave(7, dim=1)[:, :frames]
        inputs.append((f'runs of 7 T={frames}', slow))
    for label, ppg in inputs:
        phonemes, starts = R.decode(ppg)
        got = alignment.decode(ppg.cuda())
        assert got.phonemes.tolist() == phonemes.tolist(), label
        assert got.starts.tolist() == starts.tolist(), label
    assert alignment.decode(inputs[-2][1].cuda()).phonemes.tolist() == [0]
    # a ragged batch, padded with NaN, equals its singles
    lengths = [4096, 1, 64, 65, 777]
    batch = torch.full((5, 40, 4096), float('nan'))
    for b, length in enumerate(lengths):
        batch[b, :, :length] = tied_ppg(length, generator) if b % 2 else R.random_ppg(length, 3., generator)
    got = alignment.decode(batch.cuda(), lengths)
    for b, length in enumerate(lengths):
        phonemes, starts = R.decode(batch[b, :, :length])
        assert got.phonemes[b].tolist() == phonemes.tolist() and got.starts[b].tolist() == starts.tolist(), b


def ragged_batch():
    generator = torch.Generator().manual_seed(33)
    lengths = torch.randint(1, 301, (33,), generator=generator).tolist()
    counts = [int(torch.randint(1, length + 1, (1,), generator=generator)) for length in lengths]
    lengths[0], counts[0], lengths[1], counts[1], lengths[2], counts[2] = 1, 1, 300, 300, 300, 1
    ppg = torch.full((33, 40, 300), float('nan'))
    table = torch.full((33, max(counts)), -1, dtype=torch.int64)
    for b in range(33):
        ppg[b, :, :lengths[b]] = R.random_ppg(lengths[b], 3., generator)
        table[b, :counts[b]] = torch.tensor(R.random_phonemes(counts[b], generator))
    return ppg, table, lengths, counts


def equal_alignments(batch, singles, offset=0):
    for b, one in enumerate(singles):
        at = b - offset
        if not 0 <= at < len(batch.starts):
            continue
        assert torch.equal(batch.starts[at], one.starts) and torch.equal(batch.phonemes[at], one.phonemes), b
        assert torch.equal(batch.total[at], one.total), b
        assert torch.equal(batch.score[at], one.score) and torch.equal(batch.gop[at], one.gop), b


def test_batch_equals_singles_also_from_two_streams():
    ppg, table, lengths, counts = ragged_batch()
    device = ppg.cuda()
    batch = alignment.forced(device, table, lengths, counts)
    assert batch.total.shape == (33,) and bool(torch.isfinite(batch.total).all())
    singles = [alignment.forced(device[b, :, :lengths[b]], table[b, :counts[b]]) for b in range(33)]
    equal_alignments(batch, singles)
    for b in (0, 1, 2, 17):
        R.check_starts(batch.starts[b].cpu().numpy(), lengths[b], counts[b])
    as_lists = alignment.forced(device, [table[b, :counts[b]].tolist() for b in range(33)], lengths)
    equal_alignments(as_lists, singles)
    # the two halves from two streams at once
    torch.cuda.synchronize()
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    halves = [(0, 16), (16, 33)]
    results = [[], []]
    for _ in range(3):
        for side, (low, high) in enumerate(halves):
            with torch.cuda.stream(streams[side]):
                results[side].append(alignment.forced(device[low:high], table[low:high], lengths[low:high],
                                                      counts[low:high]))
    torch.cuda.synchronize()
    for side, (low, _) in enumerate(halves):
        for result in results[side]:
            equal_alignments(result, singles, offset=low)


def raw_align(ppg, lengths, table, counts, workspace, want_gop=True, frames=None, items=None, most=None, size=None,
              offset=0):
    """ppg_align through ctypes with the caller's workspace; outputs start as sentinels: (rc, total, starts, score, gop)."""
    lib = E.library()
    both = torch.tensor([lengths, counts], dtype=torch.int32).cuda()
    total = torch.full((ppg.shape[0],), -7., device='cuda')
    starts = torch.full((ppg.shape[0], table.shape[1] + 1), -7, dtype=torch.int32, device='cuda')
    score = torch.full((ppg.shape[0], table.shape[1]), -7., device='cuda')
    gop = torch.full((ppg.shape[0], table.shape[1]), -7., device='cuda')
    torch.cuda.synchronize()
    rc = lib.ppg_align(
        0, ppg.data_ptr(), ppg.shape[2] if frames is None else frames, ppg.shape[0] if items is None else items,
        both[0].data_ptr(), table.data_ptr(), table.shape[1] if most is None else most, both[1].data_ptr(),
        total.data_ptr(), starts.data_ptr(), score.data_ptr(), gop.data_ptr() if want_gop else None,
        workspace.data_ptr() + offset, workspace.numel() - offset if size is None else size,
        torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return rc, total, starts, score, gop


def small_problem():
    generator = torch.Generator().manual_seed(12)
    ppg = torch.stack([R.random_ppg(100, 3., generator), R.random_ppg(100, 8., generator)]).cuda().contiguous()
    table = torch.randint(0, 40, (2, 70), generator=generator, dtype=torch.int32).cuda()
    return ppg, table, [100, 83], [70, 5]


def test_poisoned_workspace_gives_the_same_bits():
    generator = torch.Generator().manual_seed(4)
    size = E.library().ppg_align_workspace_bytes
    workspace = torch.zeros(size(1, 4096, 1024), dtype=torch.uint8, device='cuda')
    large = R.random_ppg(4096, 3., generator)[None].cuda().contiguous()
    large_table = torch.randint(0, 40, (1, 1024), generator=generator, dtype=torch.int32).cuda()
    rc, total, _, _, _ = raw_align(large, [4096], large_table, [1024], workspace)
    assert rc == 0 and bool(torch.isfinite(total).all())
    ppg, table, lengths, counts = small_problem()
    assert size(2, 100, 70) <= workspace.numel()
    reused = raw_align(ppg, lengths, table, counts, workspace)
    fresh = raw_align(ppg, lengths, table, counts, torch.zeros(size(2, 100, 70), dtype=torch.uint8, device='cuda'))
    poisoned = raw_align(ppg, lengths, table, counts, torch.full((size(2, 100, 70),), 255, dtype=torch.uint8,
                                                                   device='cuda'))
    assert reused[0] == fresh[0] == poisoned[0] == 0
    for a, b, c in zip(reused[1:], fresh[1:], poisoned[1:]):
        assert torch.equal(a, b) and torch.equal(a.view(torch.int32), c.view(torch.int32))
    through_module = alignment.forced(ppg, table, lengths, counts)
    assert torch.equal(through_module.total, fresh[1])
    assert torch.equal(through_module.starts[1], fresh[2][1, :6]) and torch.equal(through_module.gop[0], fresh[4][0])
    assert bool((fresh[2][1, 6:] == -7).all()) and bool((fresh[3][1, 5:] == -7).all())      # the rest is left alone
    without = raw_align(ppg, lengths, table, counts, workspace, want_gop=False)
    assert without[0] == 0 and torch.equal(without[3], fresh[3]) and bool((without[4] == -7).all())


def test_error_paths_launch_nothing_and_impossible_items_give_nan():
    lib = E.library()
    ppg, table, lengths, counts = small_problem()
    need = lib.ppg_align_workspace_bytes(2, 100, 70)
    workspace = torch.zeros(need + 64, dtype=torch.uint8, device='cuda')
    assert workspace.data_ptr() % 16 == 0
    refused = [
        raw_align(ppg, lengths, table, counts, workspace, size=need - 1),                  # workspace too small
        raw_align(ppg, lengths, table, counts, workspace, offset=8),                       # misaligned
        raw_align(ppg, lengths, table, counts, workspace, frames=E.ALIGN_MAX_FRAMES + 1, size=1 << 40),
        raw_align(ppg, lengths, table, counts, workspace, most=E.ALIGN_MAX_PHONEMES + 1, size=1 << 40),
        raw_align(ppg, lengths, table, counts, workspace, items=E.ALIGN_MAX_ITEMS + 1, size=1 << 50),
        raw_align(ppg, lengths, table, counts, workspace, items=0),
    ]
    for rc, total, starts, score, gop in refused:
        assert rc == -1 and lib.ppg_last_error()
        assert bool((total == -7).all()) and bool((starts == -7).all()) and bool((score == -7).all())
        assert bool((gop == -7).all())
    assert not workspace.any()                                                             # nothing was launched
    runs = torch.full((2,), -7, dtype=torch.int32, device='cuda')
    out = torch.full((2, 101), -7, dtype=torch.int32, device='cuda')
    both = torch.tensor(lengths, dtype=torch.int32).cuda()
    torch.cuda.synchronize()
    for frames, items in ((E.ALIGN_MAX_FRAMES + 1, 2), (100, E.ALIGN_MAX_ITEMS + 1), (0, 2)):
        assert lib.ppg_decode(0, ppg.data_ptr(), frames, items, both.data_ptr(), out.data_ptr(), out.data_ptr(),
                              runs.data_ptr(), None) == -1
    assert lib.ppg_decode(0, ppg.data_ptr(), 100, 2, both.data_ptr(), None, out.data_ptr(), runs.data_ptr(), None) == -1
    torch.cuda.synchronize()
    assert bool((runs == -7).all()) and bool((out == -7).all())
    # impossible device-side lengths: total = NaN, starts untouched, the neighbours unharmed.  Pointers stay in range.
    good = raw_align(ppg, lengths, table, counts, workspace)
    assert good[0] == 0
    high, negative = table.clone(), table.clone()
    high[0, 3], negative[1, 4] = 40, -1
    for bad_lengths, bad_counts, bad_table, item in (
            ([100, 4], [70, 5], table, 1),                     # N > T
            ([100, 83], [0, 5], table, 0),                     # N < 1
            ([100, 83], [70, -3], table, 1),
            ([100, 83], [71, 5], table, 0),                    # N beyond the table
            ([0, 83], [70, 5], table, 0),                      # T outside [1, frames]
            ([100, 101], [70, 5], table, 1),
            ([100, 83], [70, 5], high, 0),                     # a phoneme index outside 0 .. 39
            ([100, 83], [70, 5], negative, 1)):
        rc, total, starts, score, gop = raw_align(ppg, bad_lengths, bad_table, bad_counts, workspace)
        other = 1 - item
        assert rc == 0 and bool(torch.isnan(total[item])), (bad_lengths, bad_counts)
        assert bool((starts[item] == -7).all()) and bool((score[item] == -7).all()) and bool((gop[item] == -7).all())
        assert torch.equal(total[other], good[1][other]) and torch.equal(starts[other], good[2][other])
        assert torch.equal(score[other], good[3][other]) and torch.equal(gop[other], good[4][other])
    # an index outside 0 .. 39 past the item's own N is padding: never read
    rc, total, starts, _, _ = raw_align(ppg, [100, 83], high, [3, 5], workspace)
    assert rc == 0 and bool(torch.isfinite(total).all()) and starts[0, :4].tolist()[::3] == [0, 100]
    # the decode's counterpart: a length outside [1, frames] gives no runs and nothing else
    bad = torch.tensor([0, 101], dtype=torch.int32).cuda()
    labels = torch.full((2, 100), -7, dtype=torch.int32, device='cuda')
    torch.cuda.synchronize()
    assert lib.ppg_decode(0, ppg.data_ptr(), 100, 2, bad.data_ptr(), labels.data_ptr(), out.data_ptr(),
                          runs.data_ptr(), torch.cuda.current_stream().cuda_stream) == 0
    torch.cuda.synchronize()
    assert runs.tolist() == [0, 0] and bool((labels == -7).all()) and bool((out == -7).all())
