"""ppgs_amd.alignment.search on the GPU against the CPU restatement of tests/search_reference.py (float64 emissions from
the oracle-style clamp, a float64 programme with the same tie rule, the picker in numpy).

The bound on a curve value is derived, not measured.  An emission is the difference of two logf values, each within
1 ulp of a magnitude <= 18.43 (1.9e-6), rounded once (0.95e-6): within 5e-6 absolute.  L sequential same-sign
additions add L * 2^-24 relative, and a maximum of bounded values is bounded: with L the longer of the device's and
the reference's span,  |curve_total - ref| <= L * 5e-6 + (L + 2) * 2^-23 * |ref|.  Spans are compared by cost, never
by identity: the device's own span, re-scored in float64 with the best segmentation inside it, must be within twice
the bound of the reference optimum.  The picker is compared bit for bit, on the device's own curve."""
import math

import numpy as np
import pytest
import torch

import ppgs_amd
from ppgs_amd import alignment, engine as E

import alignment_reference as R
import search_reference as S

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -23

# (T, N): one frame, pure diagonals, both strip lengths (N <= 64: 1 state per lane, above: 4) and their edges, the
# 32-frame staging chunk and the picker's 64 lanes and their edges, past the limit of `forced`, and a long recording
CASES = [(1, 1), (5, 5), (64, 64), (65, 65), (200, 65), (300, 256), (700, 255), (31, 3), (32, 3), (33, 3), (63, 3),
         (64, 3), (65, 3), (4097, 7), (70000, 5)]


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.view(torch.int32), b.view(torch.int32))


@pytest.mark.parametrize('frames,count', CASES)
def test_curve_against_float64_programme(frames, count):
    generator = torch.Generator().manual_seed(1000 * frames + count)
    scales = (1., 3., 8.)
    ppgs = [R.random_ppg(frames, scale, generator) for scale in scales]
    queries = [R.random_phonemes(count, generator) for _ in scales]
    emissions = [S.emissions(S.log_posteriors(ppg), query) for ppg, query in zip(ppgs, queries)]
    ref_totals, ref_begins = S.programme(np.stack(emissions))            # the three scales share the loop over frames
    time = np.arange(frames)
    worst = 0.
    for k, scale in enumerate(scales):
        label = f'T={frames} N={count} scale={scale}'
        got = alignment.search(ppgs[k].cuda(), queries[k], curve=True)
        assert got.curve[0].shape == got.curve[1].shape == (frames,) and got.curve[0].is_cuda
        assert got.curve[0].dtype == torch.float32 and got.curve[1].dtype == torch.int32
        total, begin = got.curve[0].cpu().numpy().astype(np.float64), got.curve[1].cpu().numpy().astype(np.int64)
        ref_total, ref_begin = ref_totals[k], ref_begins[k]
        # before a match can end: exactly -inf and -1
        assert np.isneginf(total[:count - 1]).all() and (begin[:count - 1] == -1).all(), label
        total, begin, ref_total, ref_begin = total[count - 1:], begin[count - 1:], ref_total[count - 1:], ref_begin[count - 1:]
        ends = time[count - 1:]
        assert np.isfinite(total).all() and (total <= 0).all(), label
        assert (begin >= 0).all() and (begin <= ends - count + 1).all(), label               # room for every phoneme
        longest = np.maximum(ends - begin, ends - ref_begin) + 1
        bound = longest * 5e-6 + (longest + 2) * EPS * np.abs(ref_total)
        error = np.abs(total - ref_total)
        relative = float((error / np.maximum(np.abs(ref_total), 1e-30)).max())
        print(f'search {label}: largest relative error {relative:.3e}, largest error / bound '
              f'{float((error / bound).max()):.3e}, longest span {int(longest.max())}')
        worst = max(worst, relative)
        assert (error <= bound).all(), label
        full = np.concatenate([np.full(count - 1, -1, dtype=np.int64), begin])
        rescored = S.rescore(emissions[k], full)[count - 1:]
        print(f'search {label}: the device spans re-scored lie at most '
              f'{float(((ref_total - rescored) / bound).max()):.3e} bounds below the optimum (2 allowed)')
        assert (rescored >= ref_total - 2 * bound).all(), label
        assert (rescored <= ref_total + 1e-9 * np.abs(ref_total) + 1e-12).all(), label        # the optimum is one
    print(f'search T={frames} N={count}: largest relative error of a curve value {worst:.3e}')


def device_curve_and_hits(ppg, query, top, threshold=None):
    got = alignment.search(ppg, query, top=top, threshold=threshold, curve=True)
    return got, got.curve[0].cpu().numpy(), got.curve[1].cpu().numpy()


def check_picker(got, total, begin, count, top, threshold, label):
    """The hits of the device against the numpy picker on the device's own curve, bit for bit."""
    hits = S.pick(total, begin, count, top, -np.inf if threshold is None else threshold, np.float32)
    assert got.begin.shape == got.end.shape == got.total.shape == got.mean.shape == (top,), label
    assert got.begin.dtype == got.end.dtype == got.count.dtype == torch.int32 and got.count.dim() == 0
    assert int(got.count) == len(hits), (label, int(got.count), len(hits))
    taken = len(hits)
    assert got.begin[:taken].tolist() == [h[0] for h in hits] and got.end[:taken].tolist() == [h[1] for h in hits], label
    expected_total = torch.tensor([h[2] for h in hits], dtype=torch.float32)
    expected_mean = torch.tensor([h[3] for h in hits], dtype=torch.float32)
    assert same_bits(got.total[:taken].cpu(), expected_total) and same_bits(got.mean[:taken].cpu(), expected_mean), label
    # the tail
    assert bool((got.begin[taken:] == -1).all()) and bool((got.end[taken:] == -1).all()), label
    assert bool(torch.isnan(got.total[taken:]).all()) and bool(torch.isnan(got.mean[taken:]).all()), label
    spans = sorted(zip(got.begin[:taken].tolist(), got.end[:taken].tolist()))
    assert all(0 <= b < e for b, e in spans) and all(a[1] <= b[0] for a, b in zip(spans, spans[1:])), label
    return taken


@pytest.mark.parametrize('frames,count', [(5, 5), (64, 3), (65, 3), (300, 7), (700, 65), (4097, 7), (20000, 2)])
def test_picker_bitwise_on_the_device_curve(frames, count):
    generator = torch.Generator().manual_seed(77 * frames + count)
    ppg = R.random_ppg(frames, 3., generator).cuda()
    query = R.random_phonemes(count, generator)
    whole = None
    for top in (1, 3, 64):
        got, total, begin = device_curve_and_hits(ppg, query, top)
        taken = check_picker(got, total, begin, count, top, None, f'T={frames} N={count} top={top}')
        assert taken >= min(top, 1)
        whole = got
        without = alignment.search(ppg, query, top=top)
        assert without.curve is None and same_bits(without.mean, got.mean) and torch.equal(without.begin, got.begin)
    means = whole.mean[:int(whole.count)].cpu().numpy()
    print(f'search picker T={frames} N={count}: {len(means)} hits of 64, means {means[0]:.4f} .. {means[-1]:.4f}')
    # a threshold that cuts the list short: between two of the means taken (at one of them: it is still a hit)
    if len(means) >= 3 and means[1] > means[-1]:
        cut = float(means[1])
        got, total, begin = device_curve_and_hits(ppg, query, 64, cut)
        taken = check_picker(got, total, begin, count, 64, cut, f'T={frames} N={count} threshold={cut}')
        assert 2 <= taken < len(means) and float(got.mean[taken - 1]) >= cut
    # a threshold above every mean
    for cut in (float(np.nextafter(means[0], np.float32(np.inf))), 0.5, math.inf):
        got, total, begin = device_curve_and_hits(ppg, query, 3, cut)
        assert check_picker(got, total, begin, count, 3, cut, f'T={frames} N={count} threshold={cut}') == 0
        assert int(got.count) == 0 and bool(torch.isnan(got.mean).all()) and bool((got.end == -1).all())


def planted():
    """A PPG by the recipe of test_gpu_alignment.known_segmentation (target logit +10) in which the query stands at
    three known places; the frames between carry labels that are neither the query's first nor its last phoneme."""
    generator = torch.Generator().manual_seed(19)
    query = [3, 11, 22, 11, 30]
    others = [p for p in range(40) if p not in (query[0], query[-1])]

    def filler(frames):
        picks = torch.randint(0, len(others), (frames,), generator=generator).tolist()
        return [others[p] for p in picks]
    labels, places = [], []
    for gap in (23, 40, 17, 31):
        labels += filler(gap)
        if len(places) < 3:
            durations = torch.randint(1, 7, (len(query),), generator=generator).tolist()
            starts = [len(labels)]
            for phoneme, duration in zip(query, durations):
                labels += [phoneme] * duration
                starts.append(len(labels))
            places.append(starts)
    labels = torch.tensor(labels)
    frames = labels.shape[0]
    logits = torch.randn(40, frames, generator=generator)
    logits[labels, torch.arange(frames)] += 10.
    return torch.softmax(logits, dim=0), query, places, labels


def test_planted_occurrences_are_found_exactly():
    ppg, query, places, labels = planted()
    frames = ppg.shape[1]
    logp = torch.from_numpy(S.log_posteriors(ppg))
    target = logp[torch.arange(frames), labels]
    others = logp.clone()
    others[torch.arange(frames), labels] = -np.inf
    margin = float((target - others.max(dim=1).values).min())
    print(f'search planted: T = {frames}, smallest margin of the target log-posterior {margin:.3f}')
    assert margin >= 1.0                                                   # a condition on the input
    device = ppg.cuda()
    got = alignment.search(device, query, top=3)
    assert int(got.count) == 3
    # all three are perfect, so they tie in the mean and come by decreasing end frame
    expected = sorted(((starts[0], starts[-1]) for starts in places), key=lambda span: -span[1])
    assert list(zip(got.begin.tolist(), got.end.tolist())) == expected
    assert bool((got.total == 0).all()) and bool((got.mean == 0).all())
    four = alignment.search(device, query, top=4)
    assert int(four.count) == 4 and torch.equal(four.begin[:3], got.begin) and torch.equal(four.end[:3], got.end)
    assert float(four.mean[3]) < 0 and float(four.total[3]) < 0 and int(four.end[3]) - int(four.begin[3]) >= len(query)
    assert all(int(four.end[3]) <= b or e <= int(four.begin[3]) for b, e in expected)
    by_name = alignment.search(device, [ppgs_amd.PHONEMES[p] for p in query], top=3)
    assert torch.equal(by_name.begin, got.begin) and torch.equal(by_name.end, got.end)
    assert alignment.search(device, query, top=4, threshold=-1e-3).count.item() == 3
    # the phoneme boundaries inside a hit: forced alignment of the slice
    by_begin = {starts[0]: starts for starts in places}
    for b, e in zip(got.begin.tolist(), got.end.tolist()):
        inside = alignment.forced(device[:, b:e], query)
        assert [b + s for s in inside.starts.tolist()] == by_begin[b]
        assert bool((inside.gop == 0).all())
    listed = alignment.hit_segments(got)
    assert listed == [(b * 160 / 16000, e * 160 / 16000, 0., 0.) for b, e in expected]
    # CPU tensors are moved to the device, half precision is promoted, as in the other post-ops
    assert torch.equal(alignment.search(ppg, query, top=3).begin, got.begin)
    half = alignment.search(device.half(), query, top=3)
    assert half.total.dtype == torch.float32 and same_bits(half.mean, alignment.search(device.half().float(), query, top=3).mean)


@pytest.mark.parametrize('frames,count', [(300, 1), (300, 5), (257, 40), (300, 65), (120, 100)])
def test_top_hit_ties_to_forced_alignment_of_its_span(frames, count):
    generator = torch.Generator().manual_seed(5000 + frames + count)
    for scale in (1., 3., 8.):
        ppg = R.random_ppg(frames, scale, generator).cuda()
        query = R.random_phonemes(count, generator)
        hit = alignment.search(ppg, query)
        assert int(hit.count) == 1 and hit.begin.shape == (1,)
        b, e = int(hit.begin[0]), int(hit.end[0])
        assert 0 <= b and b + count <= e <= frames
        inside = alignment.forced(ppg[:, b:e], query)
        lengths = np.diff(inside.starts.cpu().numpy()).astype(np.float64)
        through_forced = float((inside.gop.cpu().numpy().astype(np.float64) * lengths).sum())
        total = float(hit.total[0])
        bound = (e - b) * 5e-6 + (e - b + 2) * EPS * abs(total)
        print(f'search T={frames} N={count} scale={scale}: span [{b}, {e}) total {total:.6f}, through forced '
              f'{through_forced:.6f}, difference / bound {abs(total - through_forced) / bound:.3e}')
        assert abs(total - through_forced) <= bound


def ragged():
    """3 recordings (NaN padding) and 5 queries (-1 padding); query 3 is longer than the shortest recording."""
    generator = torch.Generator().manual_seed(41)
    lengths, counts = [150, 9, 97], [4, 1, 70, 12, 7]
    ppg = torch.full((3, 40, 150), float('nan'))
    for b, length in enumerate(lengths):
        ppg[b, :, :length] = R.random_ppg(length, 3., generator)
    queries = [R.random_phonemes(count, generator) for count in counts]
    return ppg, lengths, queries, counts


def test_batch_equals_singles_also_from_two_streams():
    ppg, lengths, queries, counts = ragged()
    device = ppg.cuda()
    top = 3
    batch = alignment.search(device, queries, lengths, top=top, curve=True)
    assert batch.begin.shape == (3, 5, top) and batch.count.shape == (3, 5) and batch.curve[0].shape == (3, 5, 150)
    assert [q.tolist() for q in batch.phonemes] == queries
    singles = {(b, q): alignment.search(device[b, :, :lengths[b]], queries[q], top=top, curve=True)
               for b in range(3) for q in range(5)}

    def equal(result, offset=0, rows=range(3)):
        for b in rows:
            for q in range(5):
                one, at = singles[b, q], b - offset
                assert torch.equal(result.begin[at, q], one.begin) and torch.equal(result.end[at, q], one.end), (b, q)
                assert same_bits(result.total[at, q], one.total) and same_bits(result.mean[at, q], one.mean), (b, q)
                assert torch.equal(result.count[at, q], one.count), (b, q)
                for whole, own in zip(result.curve, one.curve):
                    assert same_bits(whole[at, q, :lengths[b]], own), (b, q)
                assert bool(torch.isneginf(result.curve[0][at, q, lengths[b]:]).all())
                assert bool((result.curve[1][at, q, lengths[b]:] == -1).all())
    equal(batch)
    counted = batch.count.cpu()
    assert counted[1, 2].item() == 0 and counted[1, 3].item() == 0          # 9 frames: no room for 70 or 12 phonemes
    counted[1, 2] = counted[1, 3] = 1
    assert bool((counted >= 1).all()) and bool((counted <= top).all())     # every other pair has a hit
    counted = batch.count.cpu()
    assert bool(torch.isneginf(batch.curve[0][1, 3, :9]).all()) and bool((batch.curve[1][1, 3] == -1).all())
    assert bool((batch.begin[1, 3] == -1).all()) and bool(torch.isnan(batch.mean[1, 3]).all())
    # drops: one recording keeps the Q axis, one sequence keeps the B axis
    row = alignment.search(device[0], queries, top=top)
    assert row.begin.shape == (5, top) and row.count.shape == (5,) and torch.equal(row.begin, batch.begin[0])
    column = alignment.search(device, queries[0], lengths, top=top)
    assert column.begin.shape == (3, top) and column.count.shape == (3,) and torch.equal(column.end, batch.end[:, 0])
    assert column.phonemes.tolist() == queries[0]
    nested = alignment.hit_segments(batch)
    assert len(nested) == 3 and len(nested[1]) == 5 and [len(hits) for hits in nested[1]] == counted[1].tolist()
    # the first two recordings and the last from two streams at once
    torch.cuda.synchronize()
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    halves = [(0, 2), (2, 3)]
    results = [[], []]
    for _ in range(3):
        for side, (low, high) in enumerate(halves):
            with torch.cuda.stream(streams[side]):
                results[side].append(alignment.search(device[low:high], queries, lengths[low:high], top=top, curve=True))
    torch.cuda.synchronize()
    for side, (low, high) in enumerate(halves):
        for result in results[side]:
            equal(result, offset=low, rows=range(low, high))


def test_a_batch_split_over_several_calls_equals_one_call(monkeypatch):
    ppg, lengths, queries, counts = ragged()
    device = ppg.cuda()
    whole = alignment.search(device, queries, lengths, top=2, curve=True)
    # a budget that holds one recording and two queries per call: queries in groups, through temporaries
    monkeypatch.setattr(E, 'SEARCH_WORKSPACE_BYTES', 150 * (176 + 2 * 8) + 1024)
    split = alignment.search(device, queries, lengths, top=2, curve=True)
    for a, b in zip(whole[1:6] + whole.curve, split[1:6] + split.curve):
        assert same_bits(a, b)
    # ... and one that holds two recordings and all five queries: recordings in groups, straight into the outputs
    monkeypatch.setattr(E, 'SEARCH_WORKSPACE_BYTES', 2 * 150 * (176 + 5 * 8) + 2048)
    split = alignment.search(device, queries, lengths, top=2, curve=True)
    for a, b in zip(whole[1:6] + whole.curve, split[1:6] + split.curve):
        assert same_bits(a, b)


def raw_search(ppg, lengths, table, counts, workspace, top=3, threshold=-math.inf, want_curve=True, frames=None,
               items=None, queries=None, most=None, size=None, offset=0, curve_begin=True):
    """ppg_search through ctypes with the caller's workspace; outputs start as sentinels:
    (rc, begin, end, total, mean, count, curve_total, curve_begin)."""
    lib = E.library()
    both = torch.tensor(lengths, dtype=torch.int32).cuda(), torch.tensor(counts, dtype=torch.int32).cuda()
    shape = (ppg.shape[0], table.shape[0], top if 1 <= top <= 64 else 1)
    begin = torch.full(shape, -7, dtype=torch.int32, device='cuda')
    end = torch.full(shape, -7, dtype=torch.int32, device='cuda')
    total = torch.full(shape, -7., device='cuda')
    mean = torch.full(shape, -7., device='cuda')
    count = torch.full(shape[:2], -7, dtype=torch.int32, device='cuda')
    curve_shape = (ppg.shape[0], table.shape[0], ppg.shape[2])
    curves = torch.full(curve_shape, -7., device='cuda'), torch.full(curve_shape, -7, dtype=torch.int32, device='cuda')
    torch.cuda.synchronize()
    rc = lib.ppg_search(
        0, ppg.data_ptr(), ppg.shape[2] if frames is None else frames, ppg.shape[0] if items is None else items,
        both[0].data_ptr(), table.data_ptr(), table.shape[1] if most is None else most,
        table.shape[0] if queries is None else queries, both[1].data_ptr(), top, threshold, begin.data_ptr(),
        end.data_ptr(), total.data_ptr(), mean.data_ptr(), count.data_ptr(),
        curves[0].data_ptr() if want_curve else None, curves[1].data_ptr() if want_curve and curve_begin else None,
        workspace.data_ptr() + offset, workspace.numel() - offset if size is None else size,
        torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return (rc, begin, end, total, mean, count) + curves


def small_problem():
    ppg, lengths, queries, counts = ragged()
    table = torch.full((5, 70), -1, dtype=torch.int32)
    for q, query in enumerate(queries):
        table[q, :len(query)] = torch.tensor(query)
    return ppg.cuda().contiguous(), lengths, table.cuda(), counts


def test_poisoned_workspace_gives_the_same_bits():
    generator = torch.Generator().manual_seed(4)
    size = E.library().ppg_search_workspace_bytes
    workspace = torch.zeros(size(1, 5000, 8), dtype=torch.uint8, device='cuda')
    large = R.random_ppg(5000, 3., generator)[None].cuda().contiguous()
    large_table = torch.randint(0, 40, (8, 100), generator=generator, dtype=torch.int32).cuda()
    first = raw_search(large, [5000], large_table, [100] * 8, workspace)
    assert first[0] == 0 and bool((first[5] == 3).all())
    ppg, lengths, table, counts = small_problem()
    need = size(3, 150, 5)
    assert need <= workspace.numel()
    reused = raw_search(ppg, lengths, table, counts, workspace)
    fresh = raw_search(ppg, lengths, table, counts, torch.zeros(need, dtype=torch.uint8, device='cuda'))
    poisoned = raw_search(ppg, lengths, table, counts, torch.full((need,), 255, dtype=torch.uint8, device='cuda'))
    assert reused[0] == fresh[0] == poisoned[0] == 0
    for a, b, c in zip(reused[1:], fresh[1:], poisoned[1:]):
        assert same_bits(a, b) and same_bits(a, c)
    through_module = alignment.search(ppg, [table[q, :n] for q, n in enumerate(counts)], lengths, top=3, curve=True)
    assert same_bits(through_module.mean, fresh[4]) and torch.equal(through_module.count, fresh[5])
    # the curve past a recording's own length is left alone
    assert bool((fresh[6][1, :, 9:] == -7).all()) and bool((fresh[7][2, :, 97:] == -7).all())
    assert same_bits(through_module.curve[0][1, :, :9], fresh[6][1, :, :9])
    without = raw_search(ppg, lengths, table, counts, workspace, want_curve=False)
    assert without[0] == 0 and same_bits(without[4], fresh[4]) and bool((without[6] == -7).all())
    assert bool((without[7] == -7).all())


def test_error_paths_launch_nothing_and_impossible_pairs_give_minus_one():
    lib = E.library()
    ppg, lengths, table, counts = small_problem()
    need = lib.ppg_search_workspace_bytes(3, 150, 5)
    workspace = torch.zeros(need + 64, dtype=torch.uint8, device='cuda')
    assert workspace.data_ptr() % 16 == 0
    refused = [
        raw_search(ppg, lengths, table, counts, workspace, size=need - 1),                 # workspace too small
        raw_search(ppg, lengths, table, counts, workspace, offset=8),                      # misaligned
        raw_search(ppg, lengths, table, counts, workspace, frames=E.SEARCH_MAX_FRAMES + 1, size=1 << 40),
        raw_search(ppg, lengths, table, counts, workspace, most=E.SEARCH_MAX_PHONEMES + 1, size=1 << 40),
        raw_search(ppg, lengths, table, counts, workspace, items=E.SEARCH_MAX_ITEMS + 1, size=1 << 50),
        raw_search(ppg, lengths, table, counts, workspace, queries=E.SEARCH_MAX_QUERIES + 1, size=1 << 50),
        raw_search(ppg, lengths, table, counts, workspace, items=0),
        raw_search(ppg, lengths, table, counts, workspace, queries=0),
        raw_search(ppg, lengths, table, counts, workspace, top=0),
        raw_search(ppg, lengths, table, counts, workspace, top=E.SEARCH_MAX_HITS + 1),
        raw_search(ppg, lengths, table, counts, workspace, threshold=math.nan),
        raw_search(ppg, lengths, table, counts, workspace, curve_begin=False),             # one curve without the other
    ]
    for result in refused:
        assert result[0] == -1 and lib.ppg_last_error()
        for out in result[1:]:
            assert bool((out == -7).all())
    assert not workspace.any()                                                             # nothing was launched
    # impossible device-side pairs: count = -1, every other output untouched, the neighbours unharmed
    good = raw_search(ppg, lengths, table, counts, workspace)
    assert good[0] == 0 and bool((good[5] >= 0).all())
    high, negative = table.clone(), table.clone()
    high[2, 69], negative[0, 0] = 40, -1
    for bad_lengths, bad_counts, bad_table, where in (
            (lengths, [4, 0, 70, 12, 7], table, (slice(None), 1)),          # N = 0
            (lengths, [4, 1, 70, -2, 7], table, (slice(None), 3)),
            (lengths, [4, 1, 71, 12, 7], table, (slice(None), 2)),          # N beyond the table
            ([150, 0, 97], counts, table, (1, slice(None))),                # T = 0
            ([150, 9, 151], counts, table, (2, slice(None))),               # T beyond the padded frames
            ([-5, 9, 97], counts, table, (0, slice(None))),
            (lengths, counts, high, (slice(None), 2)),                      # a phoneme index outside 0 .. 39
            (lengths, counts, negative, (slice(None), 0))):
        result = raw_search(ppg, bad_lengths, bad_table, bad_counts, workspace)
        assert result[0] == 0
        struck = torch.zeros((3, 5), dtype=torch.bool, device='cuda')
        struck[where] = True
        assert bool((result[5][struck] == -1).all()), (bad_lengths, bad_counts)
        for out, fine in zip(result[1:], good[1:]):
            if out is not result[5]:
                assert bool((out[struck] == -7).all()), (bad_lengths, bad_counts)
            assert same_bits(out[~struck], fine[~struck]), (bad_lengths, bad_counts)
    # an index outside 0 .. 39 past a query's own N is padding: never read
    result = raw_search(ppg, lengths, high, [4, 1, 69, 12, 7], workspace)
    assert result[0] == 0 and bool((result[5] >= 0).all())


def test_the_reference_fixture_finds_its_own_decode(golden):
    ppg = torch.from_numpy(golden('g9_postops')['x'])
    assert ppg.shape == (40, 57)
    phonemes, starts = R.decode(ppg)
    assert len(phonemes) >= 6
    query = phonemes[2:6].tolist()
    got = alignment.search(ppg.cuda(), query, top=2, curve=True)
    print(f'search fixture: query {query} decoded at [{starts[2]}, {starts[6]}), hits '
          f'{list(zip(got.begin.tolist(), got.end.tolist(), got.mean.tolist()))}')
    assert int(got.count) >= 1 and float(got.mean[0]) == 0. and float(got.total[0]) == 0.
    assert (int(got.begin[0]), int(got.end[0])) == (int(starts[2]), int(starts[6]))
    check_picker(got, got.curve[0].cpu().numpy(), got.curve[1].cpu().numpy(), 4, 2, None, 'fixture')
