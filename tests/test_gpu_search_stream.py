"""ppgs_amd.alignment.SearchStream on the GPU.  Nothing here has a tolerance: the curve of the pushed frames is compared
bit for bit with alignment.search(..., curve=True) over the whole recording, whatever the pushes, and the events with
the reference detector (tests/search_stream_reference.py: the rule word for word, numpy float32 division) run on the
device's own curve, with the push that gives each one out."""
import ctypes
import math

import numpy as np
import pytest
import torch

from ppgs_amd import alignment, engine as E
from ppgs_amd import weights as W

import alignment_reference as R
import search_stream_reference as L

pytestmark = pytest.mark.gpu

FRAMES = 200
PATTERNS = {'uneven': [1, 31, 32, 33, 1, 64, 38], 'ones': [1] * FRAMES, 'whole': [FRAMES]}
SCALES = (1., 3., 8.)


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.view(torch.int32), b.view(torch.int32))


def feed(spotter, ppg, pushes, lengths=None):
    """Push ppg (..., 40, T) in pieces of `pushes` frames: the list of Hits, one per push (nothing is read back)."""
    out, at = [], 0
    for frames in pushes:
        out.append(spotter.push(ppg[..., at:at + frames]))
        at += frames
    assert at == ppg.shape[-1]
    return out


def events_of(hits):
    """The events of one pair's Hits (no B and no Q axis) as the reference lists them, sentinels checked."""
    count = int(hits.count)
    cap = hits.begin.shape[0]
    assert 0 <= count <= cap, (count, cap)
    begin, end = hits.begin.tolist(), hits.end.tolist()
    total, mean = hits.total.cpu().numpy(), hits.mean.cpu().numpy()
    assert begin[count:] == [-1] * (cap - count) and end[count:] == [-1] * (cap - count)
    assert np.isnan(total[count:]).all() and np.isnan(mean[count:]).all()
    return [(begin[h], end[h], total[h], mean[h]) for h in range(count)]


def to_host(hits):
    """Hits with its result tensors on the host: one copy each, however many pairs."""
    return hits._replace(begin=hits.begin.cpu(), end=hits.end.cpu(), total=hits.total.cpu(), mean=hits.mean.cpu(),
                         count=hits.count.cpu(), curve=None)


def identical(got, expected):
    """Two event lists: begin and end exact, total and mean the same bits."""
    return len(got) == len(expected) and all(
        a[:2] == b[:2] and np.float32(a[2]).tobytes() == np.float32(b[2]).tobytes() and
        np.float32(a[3]).tobytes() == np.float32(b[3]).tobytes() for a, b in zip(got, expected))


_recordings = {}


def recordings():
    """The three recordings of FRAMES frames (one per softmax scale) on the device, made once: (3, 40, FRAMES)."""
    if 'ppg' not in _recordings:
        generator = torch.Generator().manual_seed(20240)
        _recordings['ppg'] = torch.stack([R.random_ppg(FRAMES, scale, generator) for scale in SCALES]).cuda()
    return _recordings['ppg']


@pytest.mark.parametrize('count', [1, 3, 64, 65, 255, 256])
def test_curve_equals_the_whole_recording_search_bit_for_bit(count):
    ppg = recordings()
    generator = torch.Generator().manual_seed(count)
    query = R.random_phonemes(count, generator)
    for k, scale in enumerate(SCALES):
        whole = alignment.search(ppg[k], query, curve=True).curve          # the reference, once per recording
        assert bool(torch.isneginf(whole[0][:count - 1]).all()) and bool(torch.isfinite(whole[0][count - 1:]).all())
        for name, pushes in PATTERNS.items():
            spotter = alignment.SearchStream(query, -math.inf, curve=True)
            pieces = feed(spotter, ppg[k], pushes)
            assert spotter.position == [FRAMES]
            assert all(piece.curve[0].shape == (frames,) for piece, frames in zip(pieces, pushes))
            total = torch.cat([piece.curve[0] for piece in pieces])
            begin = torch.cat([piece.curve[1] for piece in pieces])
            assert total.dtype == torch.float32 and begin.dtype == torch.int32 and total.is_cuda
            assert same_bits(total, whole[0]) and torch.equal(begin, whole[1]), (count, scale, name)


def test_curve_with_absolute_begins_past_the_limit_of_forced():
    generator = torch.Generator().manual_seed(4200)
    ppg = R.random_ppg(4200, 3., generator).cuda()
    query = R.random_phonemes(7, generator)
    whole = alignment.search(ppg, query, curve=True).curve
    spotter = alignment.SearchStream(query, -1., curve=True)
    pieces = feed(spotter, ppg, [500] * 8 + [200])
    assert same_bits(torch.cat([piece.curve[0] for piece in pieces]), whole[0])
    assert torch.equal(torch.cat([piece.curve[1] for piece in pieces]), whole[1])
    assert int(whole[1].max()) > 4096 and spotter.position == [4200]


def detector_queries():
    """Five queries for the three recordings: lengths 1 and 3, one on each side of the strip threshold, and the first
    runs of the peaked recording's own decode (a query that is really there)."""
    generator = torch.Generator().manual_seed(5)
    said = R.decode(recordings()[2].cpu())[0][1:5].tolist()
    return [R.random_phonemes(1, generator), R.random_phonemes(3, generator), said, R.random_phonemes(64, generator),
            R.random_phonemes(65, generator)]


@pytest.mark.parametrize('patience', [0, 1, 7, 25])
def test_events_equal_the_reference_detector_on_the_device_curve(patience):
    ppg = recordings()
    queries = detector_queries()
    whole = alignment.search(ppg, queries, curve=True).curve               # (3, 5, FRAMES) twice
    totals, begins = whole[0].cpu().numpy(), whole[1].cpu().numpy()
    emitted = 0
    for threshold in (-math.inf, -1., -0.3):
        lists = {}
        for name, pushes in PATTERNS.items():
            spotter = alignment.SearchStream(queries, threshold, patience=patience, batch=3, curve=True)
            pieces = feed(spotter, ppg, pushes)
            pieces.append(spotter.flush())
            assert pieces[0].begin.shape == (3, 5, pushes[0] // 1 + 2) and pieces[-1].begin.shape == (3, 5, 1)
            assert same_bits(torch.cat([piece.curve[0] for piece in pieces[:-1]], dim=2), whole[0])
            pieces = [to_host(piece) for piece in pieces]
            for b in range(3):
                for q in range(5):
                    expected = L.detect(totals[b, q], begins[b, q], threshold, patience, pushes)
                    got = [events_of(alignment.Hits(None, piece.begin[b, q], piece.end[b, q], piece.total[b, q],
                                                    piece.mean[b, q], piece.count[b, q], None)) for piece in pieces]
                    assert len(got) == len(expected)
                    for index, (mine, theirs) in enumerate(zip(got, expected)):
                        assert identical(mine, theirs), (threshold, name, b, q, index, mine, theirs)
                    lists.setdefault((b, q), []).append(L.flat(got))
                    emitted += len(L.flat(got))
        for (b, q), (first, second, third) in lists.items():                # the same events whatever the pushes
            assert identical(first, second) and identical(first, third), (threshold, b, q)
    print(f'search stream patience={patience}: {emitted} events compared')
    assert emitted > 100


@pytest.mark.parametrize('pushes', [[16] * 11, [1, 31, 32, 33, 1, 64, 14], [176], [1] * 176])
def test_planted_occurrences_come_out_exactly_and_on_time(pushes):
    ppg, query, places, _ = L.planted()
    spans = [(starts[0], starts[-1]) for starts in places]
    assert spans == [(23, 49), (89, 107), (124, 145)] and ppg.shape[1] == sum(pushes) == 176
    patience = 5
    spotter = alignment.SearchStream(query, -1e-3, patience=patience)
    pieces = feed(spotter, ppg.cuda(), pushes)
    assert pieces[0].curve is None
    got = [events_of(piece) for piece in pieces]
    assert [(b, e) for b, e, _, _ in L.flat(got)] == spans                  # in time order
    assert all(total == 0 and mean == 0 for _, _, total, mean in L.flat(got))
    # each one leaves in the push that holds frame end - 1 + patience + 1 (the next occurrence qualifies later)
    edges = np.cumsum(pushes)
    due = [[] for _ in pushes]
    for b, e in spans:
        due[int(np.searchsorted(edges, e - 1 + patience + 1, side='right'))].append((b, e))
    assert [[(hit[0], hit[1]) for hit in events] for events in got] == due
    last = spotter.flush()
    assert int(last.count) == 0 and events_of(last) == []
    assert alignment.hit_segments(pieces[-1]) == [(b * 160 / 16000, e * 160 / 16000, 0., 0.) for b, e, _, _ in got[-1]]


def ragged():
    """3 recordings and 5 queries; the pushes are ragged, with steps a stream sits out; stream 1 receives 9 frames in
    all, fewer than queries 2 and 3 have phonemes.  (ppg (3, 40, 150) NaN past each length, totals, queries, schedule:
    the lengths of every push.)"""
    generator = torch.Generator().manual_seed(41)
    totals, counts = [150, 9, 97], [4, 1, 70, 12, 7]
    ppg = torch.full((3, 40, 150), float('nan'))
    for b, length in enumerate(totals):
        ppg[b, :, :length] = R.random_ppg(length, 3., generator)
    queries = [R.random_phonemes(count, generator) for count in counts]
    schedule = [[16, 3, 0], [1, 0, 33], [64, 5, 31], [0, 0, 0], [37, 1, 32], [32, 0, 1]]
    assert [sum(step[b] for step in schedule) for b in range(3)] == totals
    return ppg, totals, queries, schedule


def run_schedule(spotter, ppg, schedule, rows, reset_before=None, reset_row=None):
    """Feed rows `rows` of `ppg` to a batched spotter by `schedule`, padded with NaN: the Hits per step.  Before step
    `reset_before`, stream `reset_row` of the spotter is reset (its frames go on from where they were)."""
    at = [0] * len(rows)
    out = []
    for index, step in enumerate(schedule):
        if index == reset_before and reset_row is not None:
            spotter.reset(item=reset_row)
        lengths = [step[b] for b in rows]
        block = torch.full((len(rows), 40, max(max(lengths), 1)), float('nan'))
        for k, b in enumerate(rows):
            block[k, :, :lengths[k]] = ppg[b, :, at[k]:at[k] + lengths[k]]
            at[k] += lengths[k]
        out.append(spotter.push(block.cuda(), lengths))
    return out


def run_single(ppg, query, schedule, b, threshold, patience, reset_before=None):
    """One (stream, query) pair by itself over the same steps: the Hits per step (empty pushes included)."""
    spotter = alignment.SearchStream(query, threshold, patience=patience, curve=True)
    at, out = 0, []
    for index, step in enumerate(schedule):
        if index == reset_before:
            spotter.reset()
        out.append(spotter.push(ppg[b, :, at:at + step[b]].cuda()))
        at += step[b]
    return spotter, out


def equal_to_singles(steps, singles, schedule, rows, label):
    for index, (step, lengths) in enumerate(zip(steps, schedule)):
        for k, b in enumerate(rows):
            for q in range(5):
                one = singles[b, q][index]
                mine = alignment.Hits(None, step.begin[k, q], step.end[k, q], step.total[k, q], step.mean[k, q],
                                      step.count[k, q], None)
                assert identical(events_of(mine), events_of(one) if lengths[b] else []), (label, index, b, q)
                assert same_bits(step.curve[0][k, q, :lengths[b]], one.curve[0]), (label, index, b, q)
                assert torch.equal(step.curve[1][k, q, :lengths[b]], one.curve[1]), (label, index, b, q)
                assert bool(torch.isneginf(step.curve[0][k, q, lengths[b]:]).all())
                assert bool((step.curve[1][k, q, lengths[b]:] == -1).all())


def test_batch_equals_single_pairs_also_from_two_streams_and_across_a_reset():
    ppg, totals, queries, schedule = ragged()
    threshold, patience = -3., 4
    singles = {}
    for b in range(3):
        for q in range(5):
            spotter, singles[b, q] = run_single(ppg, queries[q], schedule, b, threshold, patience)
            assert spotter.position == [totals[b]]
    events = sum(int(step.count) for steps in singles.values() for step in steps)
    assert events >= 10                                                    # there is something to compare
    batch = alignment.SearchStream(queries, threshold, patience=patience, batch=3, curve=True)
    steps = run_schedule(batch, ppg, schedule, range(3))
    assert batch.position == totals and [q.tolist() for q in steps[0].phonemes] == queries
    assert steps[0].begin.shape == (3, 5, 16 // 1 + 2) and steps[0].count.shape == (3, 5)
    assert steps[3].begin.shape == (3, 5, 1 // 1 + 2) and bool((steps[3].count == 0).all())      # everyone sat out
    equal_to_singles(steps, singles, schedule, range(3), 'batch')
    # stream 1 never has room for 70 or 12 phonemes: a curve of -inf / -1 and no event, flush included
    assert all(bool(torch.isneginf(step.curve[0][1, 2:4]).all()) and bool((step.count[1, 2:4] == 0).all())
               for step in steps)
    last = batch.flush()
    assert last.count.shape == (3, 5) and bool((last.count[1, 2:4] == 0).all())
    for b in range(3):
        for q in range(5):
            one = alignment.SearchStream(queries[q], threshold, patience=patience)
            feed(one, ppg[b, :, :totals[b]].cuda(), [totals[b]])
            assert identical(events_of(alignment.Hits(None, last.begin[b, q], last.end[b, q], last.total[b, q],
                                                      last.mean[b, q], last.count[b, q], None)),
                             events_of(one.flush())), (b, q)
    assert bool((batch.flush().count == 0).all())                          # nothing is pending twice
    # the first two streams and the last from two HIP streams at once
    torch.cuda.synchronize()
    sides = [torch.cuda.Stream(), torch.cuda.Stream()]
    halves = [[0, 1], [2]]
    results = [[], []]
    for _ in range(3):
        spotters = [alignment.SearchStream(queries, threshold, patience=patience, batch=len(rows), curve=True)
                    for rows in halves]
        both = [[], []]
        at = [[0] * len(rows) for rows in halves]
        for step in schedule:
            for side, rows in enumerate(halves):
                with torch.cuda.stream(sides[side]):
                    lengths = [step[b] for b in rows]
                    block = torch.full((len(rows), 40, max(max(lengths), 1)), float('nan'))
                    for k, b in enumerate(rows):
                        block[k, :, :lengths[k]] = ppg[b, :, at[side][k]:at[side][k] + lengths[k]]
                        at[side][k] += lengths[k]
                    both[side].append(spotters[side].push(block.cuda(), lengths))
        for side in range(2):
            results[side].append(both[side])
    torch.cuda.synchronize()
    for side, rows in enumerate(halves):
        for result in results[side]:
            equal_to_singles(result, singles, schedule, rows, f'side {side}')
    # reset(item=1) before step 2 affects stream 1 only
    again = {(1, q): run_single(ppg, queries[q], schedule, 1, threshold, patience, reset_before=2)[1] for q in range(5)}
    assert any(not same_bits(again[1, q][2].curve[0], singles[1, q][2].curve[0]) for q in range(5))
    mixed = {key: again.get(key, value) for key, value in singles.items()}
    batch = alignment.SearchStream(queries, threshold, patience=patience, batch=3, curve=True)
    steps = run_schedule(batch, ppg, schedule, range(3), reset_before=2, reset_row=1)
    assert batch.position == [150, 6, 97]
    equal_to_singles(steps, mixed, schedule, range(3), 'reset')


# ---- through the raw binding ----

def layout(streams, queries, most):
    """Byte offsets of the four blocks of a state (include/ppgs_amd.h) and the states per pair."""
    def up(value):
        return (value + 255) // 256 * 256
    states = 64 if most <= 64 else 256
    pairs = streams * queries
    positions, detectors = 0, up(streams * 4)
    totals = detectors + up(pairs * 32)
    begins = totals + up(pairs * states * 4)
    assert begins + up(pairs * states * 4) == E.library().ppg_search_stream_state_bytes(streams, queries, most)
    return positions, detectors, totals, begins, states


def raw_reset(state, streams, queries, most, which=None):
    rc = E.library().ppg_search_stream_reset(0, state.data_ptr(), streams, queries, most,
                                             which.data_ptr() if which is not None else None,
                                             torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return rc


def raw_push(state, ppg, lengths, table, counts, workspace, threshold=-math.inf, patience=3, cap=None, slots=None,
             want_curve=True, curve_begin=True, frames=None, streams=None, queries=None, most=None, size=None,
             offset=0, state_offset=0):
    """ppg_search_stream_push through ctypes; outputs start as sentinels (-7) and have `slots` >= cap slots per pair:
    (rc, begin, end, total, mean, count, curve_total, curve_begin)."""
    lib = E.library()
    both = torch.tensor(lengths, dtype=torch.int32).cuda(), torch.tensor(counts, dtype=torch.int32).cuda()
    cap = ppg.shape[2] + 2 if cap is None else cap
    slots = max(cap, 1) if slots is None else slots
    shape = (ppg.shape[0], table.shape[0], slots)
    begin = torch.full(shape, -7, dtype=torch.int32, device='cuda')
    end = torch.full(shape, -7, dtype=torch.int32, device='cuda')
    total = torch.full(shape, -7., device='cuda')
    mean = torch.full(shape, -7., device='cuda')
    count = torch.full(shape[:2], -7, dtype=torch.int32, device='cuda')
    curve_shape = (ppg.shape[0], table.shape[0], ppg.shape[2])
    curves = torch.full(curve_shape, -7., device='cuda'), torch.full(curve_shape, -7, dtype=torch.int32, device='cuda')
    torch.cuda.synchronize()
    rc = lib.ppg_search_stream_push(
        0, state.data_ptr() + state_offset, ppg.data_ptr(), ppg.shape[2] if frames is None else frames,
        ppg.shape[0] if streams is None else streams, both[0].data_ptr(), table.data_ptr(),
        table.shape[1] if most is None else most, table.shape[0] if queries is None else queries, both[1].data_ptr(),
        threshold, patience, cap, begin.data_ptr(), end.data_ptr(), total.data_ptr(), mean.data_ptr(), count.data_ptr(),
        curves[0].data_ptr() if want_curve else None, curves[1].data_ptr() if want_curve and curve_begin else None,
        workspace.data_ptr() + offset, workspace.numel() - offset if size is None else size,
        torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return (rc, begin, end, total, mean, count) + curves


def small_problem():
    """3 streams x 5 queries in a table of 70 columns (-1 padding), one push of 40 frames with lengths 40, 9, 33."""
    generator = torch.Generator().manual_seed(77)
    counts = [4, 1, 70, 12, 7]
    table = torch.full((5, 70), -1, dtype=torch.int32)
    for q, count in enumerate(counts):
        table[q, :count] = torch.tensor(R.random_phonemes(count, generator))
    lengths = [40, 9, 33]
    ppg = torch.full((3, 40, 40), float('nan'))
    for b, length in enumerate(lengths):
        ppg[b, :, :length] = R.random_ppg(length, 3., generator)
    return ppg.cuda().contiguous(), lengths, table.cuda(), counts


def test_poisoned_state_and_workspace_give_the_same_bits():
    lib = E.library()
    ppg, lengths, table, counts = small_problem()
    state_bytes, need = lib.ppg_search_stream_state_bytes(3, 5, 70), lib.ppg_search_stream_workspace_bytes(3, 40, 5)
    runs = []
    for fill in (0, 255):
        state = torch.full((state_bytes,), fill, dtype=torch.uint8, device='cuda')
        workspace = torch.full((need,), fill, dtype=torch.uint8, device='cuda')
        assert raw_reset(state, 3, 5, 70) == 0
        first = raw_push(state, ppg, lengths, table, counts, workspace)
        second = raw_push(state, ppg, [33, 0, 20], table, counts, workspace)        # (other frames of the same block)
        assert first[0] == second[0] == 0 and bool((first[5] >= 0).all()) and bool((second[5] >= 0).all())
        # of the state, the four blocks: the bytes that pad each to a multiple of 256 belong to nobody
        positions, detectors, totals, begins, states = layout(3, 5, 70)
        blocks = tuple(state[at:at + size] for at, size in ((positions, 12), (detectors, 15 * 32),
                                                             (totals, 15 * states * 4), (begins, 15 * states * 4)))
        runs.append(first[1:] + second[1:] + blocks + (state,))
    for a, b in zip(runs[0][:-1], runs[1][:-1]):
        assert torch.equal(a.view(torch.uint8), b.view(torch.uint8))
    positions = runs[0][-1][:12].view(torch.int32).tolist()
    assert positions == [73, 9, 53]
    # the curve past a stream's own length is left alone, and so are all the outputs of a stream that sat out but count
    first = runs[0]
    assert bool((first[5][1, :, 9:] == -7).all()) and bool((first[6][2, :, 33:] == -7).all())
    assert bool((first[7 + 4][1] == 0).all()) and bool((first[7 + 5][1] == -7).all())
    assert bool((first[7 + 0][1] == -1).all()) and bool(torch.isnan(first[7 + 3][1]).all())
    # through the module: the same bits
    spotter = alignment.SearchStream([table[q, :n] for q, n in enumerate(counts)], -math.inf, patience=3, batch=3,
                                     curve=True)
    through = spotter.push(ppg, lengths)
    assert through.begin.shape == (3, 5, 42) and torch.equal(through.count, first[4])
    assert same_bits(through.mean, first[3]) and torch.equal(through.begin, first[0])
    assert same_bits(through.curve[0][0], first[5][0])


def test_overflow_counts_every_event_and_writes_cap_slots():
    lib = E.library()
    generator = torch.Generator().manual_seed(3)
    ppg = R.random_ppg(64, 1., generator)[None].cuda().contiguous()
    table = torch.tensor([[17]], dtype=torch.int32).cuda()
    results = []
    for cap in (64, 3, 1):
        state = torch.zeros(lib.ppg_search_stream_state_bytes(1, 1, 1), dtype=torch.uint8, device='cuda')
        workspace = torch.zeros(lib.ppg_search_stream_workspace_bytes(1, 64, 1), dtype=torch.uint8, device='cuda')
        assert raw_reset(state, 1, 1, 1) == 0
        results.append(raw_push(state, ppg, [64], table, [1], workspace, patience=0, cap=cap, slots=64) + (state,))
    whole, three, one = results
    count = int(whole[5])
    expected = L.detect(whole[6][0, 0].cpu().numpy(), whole[7][0, 0].cpu().numpy(), -math.inf, 0, flush=False)[0]
    print(f'search stream overflow: {count} events in 64 frames')
    assert count == len(expected) and 10 <= count <= 64
    for result, cap in ((three, 3), (one, 1)):
        assert result[0] == 0 and int(result[5]) == count > cap             # as snprintf: what it would have taken
        for out, full in zip(result[1:5], whole[1:5]):
            assert torch.equal(out[0, 0, :cap].view(torch.int32), full[0, 0, :cap].view(torch.int32))
            assert bool((out[0, 0, cap:] == -7).all())                      # the slots behind stay untouched
        assert torch.equal(result[-1], whole[-1])                           # the state does not depend on cap
    assert bool((whole[1][0, 0, count:] == -1).all()) and bool(torch.isnan(whole[4][0, 0, count:]).all())


def test_error_paths_launch_nothing_and_impossible_pairs_give_minus_one():
    lib = E.library()
    ppg, lengths, table, counts = small_problem()
    positions, detectors, totals, begins, states = layout(3, 5, 70)
    state_bytes, need = lib.ppg_search_stream_state_bytes(3, 5, 70), lib.ppg_search_stream_workspace_bytes(3, 40, 5)
    workspace = torch.zeros(need + 64, dtype=torch.uint8, device='cuda')
    state = torch.zeros(state_bytes + 64, dtype=torch.uint8, device='cuda')
    assert workspace.data_ptr() % 16 == 0 and state.data_ptr() % 16 == 0
    assert raw_reset(state, 3, 5, 70) == 0
    assert raw_push(state, ppg, [7, 7, 7], table, counts, workspace)[0] == 0        # a state with a history
    workspace.zero_()
    before = state.clone()
    refused = [
        raw_push(state, ppg, lengths, table, counts, workspace, size=need - 1),                 # workspace too small
        raw_push(state, ppg, lengths, table, counts, workspace, offset=8),                      # misaligned
        raw_push(state, ppg, lengths, table, counts, workspace, state_offset=8),
        raw_push(state, ppg, lengths, table, counts, workspace, frames=E.SEARCH_MAX_FRAMES + 1, size=1 << 40),
        raw_push(state, ppg, lengths, table, counts, workspace, frames=0),
        raw_push(state, ppg, lengths, table, counts, workspace, most=E.SEARCH_MAX_PHONEMES + 1),
        raw_push(state, ppg, lengths, table, counts, workspace, streams=E.SEARCH_MAX_ITEMS + 1, size=1 << 50),
        raw_push(state, ppg, lengths, table, counts, workspace, queries=E.SEARCH_MAX_QUERIES + 1),
        raw_push(state, ppg, lengths, table, counts, workspace, streams=0),
        raw_push(state, ppg, lengths, table, counts, workspace, queries=0),
        raw_push(state, ppg, lengths, table, counts, workspace, cap=0, slots=1),
        raw_push(state, ppg, lengths, table, counts, workspace, cap=-1, slots=1),
        raw_push(state, ppg, lengths, table, counts, workspace, patience=-1),
        raw_push(state, ppg, lengths, table, counts, workspace, threshold=math.nan),
        raw_push(state, ppg, lengths, table, counts, workspace, curve_begin=False),             # one curve pointer only
    ]
    for result in refused:
        assert result[0] == -1 and lib.ppg_last_error()
        for out in result[1:]:
            assert bool((out == -7).all())
    assert not workspace.any() and torch.equal(state, before)                                  # nothing was launched
    dummy = ctypes.c_void_p(state.data_ptr())
    assert lib.ppg_search_stream_flush(0, dummy, 3, 5, 70, None, None, dummy, dummy, dummy, dummy, None) == -1
    assert lib.ppg_search_stream_reset(0, ctypes.c_void_p(state.data_ptr() + 8), 3, 5, 70, None, None) == -1
    torch.cuda.synchronize()
    assert torch.equal(state, before)

    # impossible device-side pairs: count = -1, every other output and the pair's state untouched, the others unharmed
    def pair_state(buffer, b, q):
        pair = b * 5 + q
        return torch.cat([buffer[detectors + pair * 32:detectors + (pair + 1) * 32],
                          buffer[totals + pair * states * 4:totals + (pair + 1) * states * 4],
                          buffer[begins + pair * states * 4:begins + (pair + 1) * states * 4]])
    good_state = before.clone()
    good = raw_push(good_state, ppg, lengths, table, counts, workspace)
    assert good[0] == 0 and bool((good[5] >= 0).all())
    assert good_state[:12].view(torch.int32).tolist() == [47, 16, 40]
    high, negative = table.clone(), table.clone()
    high[2, 69], negative[0, 0] = 40, -1
    late = before.clone()
    late[4:8] = torch.tensor([2 ** 31 - 1 - 8], dtype=torch.int32).view(torch.uint8).cuda()       # stream 1: 8 frames left
    for start, bad_lengths, bad_counts, bad_table, where, stays in (
            (before, lengths, [4, 0, 70, 12, 7], table, (slice(None), 1), ()),          # N = 0
            (before, lengths, [4, 1, 70, -2, 7], table, (slice(None), 3), ()),
            (before, lengths, [4, 1, 71, 12, 7], table, (slice(None), 2), ()),          # N beyond the table
            (before, [40, -1, 33], counts, table, (1, slice(None)), (1,)),              # a length outside [0, frames]
            (before, [40, 9, 41], counts, table, (2, slice(None)), (2,)),
            (before, lengths, counts, high, (slice(None), 2), ()),                      # a phoneme index outside 0 .. 39
            (before, lengths, counts, negative, (slice(None), 0), ()),
            (late, lengths, counts, table, (1, slice(None)), (1,))):                    # the position would pass 2^31 - 1
        own = start.clone()
        result = raw_push(own, ppg, bad_lengths, bad_table, bad_counts, workspace)
        assert result[0] == 0
        struck = torch.zeros((3, 5), dtype=torch.bool, device='cuda')
        struck[where] = True
        assert bool((result[5][struck] == -1).all()), (bad_lengths, bad_counts)
        for out, fine in zip(result[1:], good[1:]):
            if out is not result[5]:
                assert bool((out[struck] == -7).all()), (bad_lengths, bad_counts)
            if start is before:
                assert torch.equal(out[~struck].view(torch.int32), fine[~struck].view(torch.int32)), (bad_lengths, bad_counts)
        now, was, fine = own[:12].view(torch.int32).tolist(), start[:12].view(torch.int32).tolist(), [47, 16, 40]
        assert now == [was[b] if b in stays else fine[b] for b in range(3)], (bad_lengths, bad_counts)
        for b in range(3):
            for q in range(5):
                if bool(struck[b, q]):
                    assert torch.equal(pair_state(own, b, q), pair_state(start, b, q)), (b, q)
                elif start is before:
                    assert torch.equal(pair_state(own, b, q), pair_state(good_state, b, q)), (b, q)
    # 8 frames left are 8 frames left: the last frame a stream can take is 2^31 - 2
    own = late.clone()
    result = raw_push(own, ppg, [40, 8, 33], table, counts, workspace)
    assert result[0] == 0 and bool((result[5] >= 0).all())
    assert own[:12].view(torch.int32).tolist() == [47, 2 ** 31 - 1, 40]
    begin = result[7][1, 1, :8]                                             # one phoneme: a fresh start at most frames
    assert bool((begin >= 0).all()) and bool((begin <= 2 ** 31 - 2).all()) and int(begin.max()) >= 2 ** 31 - 1 - 8
    ends = result[2][1, 1, :int(result[5][1, 1])]
    assert bool((ends > 0).all()) and bool((ends <= 2 ** 31 - 1).all())
    # an index outside 0 .. 39 past a query's own N is padding: never read
    own = before.clone()
    result = raw_push(own, ppg, lengths, high, [4, 1, 69, 12, 7], workspace)
    assert result[0] == 0 and bool((result[5] >= 0).all())


def test_audio_stream_into_search_stream():
    generator = torch.Generator().manual_seed(9)
    engine = E.Engine(W.seeded_state_dict(seed=1234), 0, 'fp32', True)
    audio = 0.1 * torch.randn(32000 + 77, generator=generator)
    query = [5, 17, 5]
    source, spotter = engine.audio_stream(500), alignment.SearchStream(query, -2., curve=True)
    pieces, hits, received = [], [], 0
    sizes = [1000, 100, 2561, 0, 77, 4111, 159, 8000, 50, 3000]
    index = 0
    while received < audio.shape[0]:
        n = min(sizes[index % len(sizes)], audio.shape[0] - received)
        index += 1
        piece = source.push(audio[received:received + n].cuda(), flush=received + n == audio.shape[0])
        received += n
        assert piece.shape[0] == 40
        pieces.append(piece.clone())
        hits.append(spotter.push(piece))                                   # the pieces of no frames too
        assert hits[-1].curve[0].shape == (piece.shape[1],) and hits[-1].begin.dim() == 1
    ppg = torch.cat(pieces, dim=1)
    assert ppg.shape[1] == 200 and any(piece.shape[1] == 0 for piece in pieces) and spotter.position == [200]
    whole = alignment.search(ppg, query, curve=True).curve
    assert same_bits(torch.cat([hit.curve[0] for hit in hits]), whole[0])
    assert torch.equal(torch.cat([hit.curve[1] for hit in hits]), whole[1])
    pushes = [piece.shape[1] for piece in pieces]
    expected = L.detect(whole[0].cpu().numpy(), whole[1].cpu().numpy(), -2., 25, pushes)
    got = [events_of(hit) for hit in hits] + [events_of(spotter.flush())]
    assert all(identical(mine, theirs) for mine, theirs in zip(got, expected)) and len(got) == len(expected)
