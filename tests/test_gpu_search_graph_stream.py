"""ppgs_amd.alignment.SearchGraphStream on the GPU.  Nothing here has a tolerance: the curve of the pushed frames is
compared bit for bit with alignment.search_graph(..., curve=True) over the whole recording, whatever the pushes; on a
chain every output is compared bit for bit with SearchStream's; and the events are compared with the reference detector
(tests/search_stream_reference.py: the rule word for word, numpy float32 division) run on the device's own curve, with
the push that gives each one out.  The push patterns 1, 31, 32, 33 put the end of a push on either side of the staging
chunk and, being odd and even, leave the last D in either half of the kernel's double buffer."""
import ctypes
import math

import numpy as np
import pytest
import torch

import ppgs_amd
from ppgs_amd import alignment, engine as E
from ppgs_amd import weights as W

import alignment_reference as R
import search_stream_reference as L
import test_gpu_search_graph as G                                       # graphs, `said`, `pack`
import test_gpu_search_stream as P                                      # pushes, events, the ragged schedule

pytestmark = pytest.mark.gpu

FRAMES = P.FRAMES
PATTERNS = P.PATTERNS
INF = math.inf
QUIET = G.QUIET
GRAPH_ARGUMENTS = ('state_begin', 'phonemes', 'stay', 'initial', 'final', 'arc_begin', 'sources', 'weights')
same_bits, feed, events_of, to_host, identical = P.same_bits, P.feed, P.events_of, P.to_host, P.identical


def chain(count, seed=0):
    return alignment.chain_graph(R.random_phonemes(count, torch.Generator().manual_seed(1000 * seed + count)))


def curve_graphs():
    generator = torch.Generator().manual_seed(23)
    words = [[['iy', 'dh', 'er'], ['ay', 'dh', 'er']], [['w', 'ey'], ['w', 'eh', 'y']], [['t', 'uw'], ['t', 'ah']]]
    graphs = {f'chain {count}': chain(count) for count in (1, 5, 64, 65, 255, 256)}
    graphs['phrase'] = alignment.phrase_graph(words)[0]                  # 3 words x 2 variants, pauses between
    graphs['weighted'] = G.random_graph(9, generator)                    # weights in [-2, 0], self-arcs, parallel arcs
    graphs['S=65 wide'] = G.random_graph(65, generator, wide=(40, 64))   # arcs beyond the registers, four states a lane
    graphs['S=64 wide'] = G.random_graph(64, generator, wide=(0, 33, 63))    # ... and one state a lane
    graphs['S=256 wide'] = G.random_graph(256, generator, wide=(5, 70, 71, 72, 130, 131, 200, 255))
    return graphs


GRAPHS = curve_graphs()


@pytest.mark.parametrize('name', list(GRAPHS))
def test_curve_equals_the_whole_recording_search_bit_for_bit(name):
    graph = GRAPHS[name]
    if 'wide' in name:
        degrees = (graph.offsets[1:] - graph.offsets[:-1]).tolist()
        assert sum(1 for degree in degrees if degree > 6) >= 2, name
    ppg = P.recordings()[:2]                                             # softmax scales 1 and 3, side by side
    whole = alignment.search_graph(ppg, graph, curve=True).curve         # the reference, once
    if name not in ('chain 255', 'chain 256'):                           # (longer than the recording: -inf throughout)
        assert bool(torch.isfinite(whole[0][:, FRAMES - 1]).all()), name
    for pattern, pushes in PATTERNS.items():
        spotter = alignment.SearchGraphStream(graph, -INF, batch=2, curve=True)
        pieces = feed(spotter, ppg, pushes)
        assert spotter.position == [FRAMES, FRAMES]
        assert all(piece.curve[0].shape == (2, frames) for piece, frames in zip(pieces, pushes))
        total = torch.cat([piece.curve[0] for piece in pieces], dim=1)
        begin = torch.cat([piece.curve[1] for piece in pieces], dim=1)
        assert total.dtype == torch.float32 and begin.dtype == torch.int32 and total.is_cuda
        assert same_bits(total, whole[0]) and torch.equal(begin, whole[1]), (name, pattern)
    one = alignment.SearchGraphStream(graph, -INF, curve=True)           # and one stream by itself
    pieces = feed(one, ppg[1], PATTERNS['uneven'])
    assert same_bits(torch.cat([piece.curve[0] for piece in pieces]), whole[0][1])
    assert torch.equal(torch.cat([piece.curve[1] for piece in pieces]), whole[1][1])


@pytest.mark.parametrize('count', [3, 64, 65])
def test_on_a_chain_every_output_is_that_of_the_chain_stream(count):
    ppg = P.recordings()
    query = R.random_phonemes(count, torch.Generator().manual_seed(count))
    fields = ('begin', 'end', 'total', 'mean', 'count')
    emitted = 0
    for threshold, patience in ((-INF, 0), (-2., 7)):
        for pattern in ('uneven', 'ones'):
            ours = alignment.SearchGraphStream(alignment.chain_graph(query), threshold, patience=patience, batch=3,
                                               curve=True)
            theirs = alignment.SearchStream(query, threshold, patience=patience, batch=3, curve=True)
            mine, other = feed(ours, ppg, PATTERNS[pattern]), feed(theirs, ppg, PATTERNS[pattern])
            mine.append(ours.flush())
            other.append(theirs.flush())
            for index, (a, b) in enumerate(zip(mine, other)):
                for field in fields:
                    assert same_bits(getattr(a, field), getattr(b, field)), (count, threshold, pattern, index, field)
                if a.curve is not None:
                    assert same_bits(a.curve[0], b.curve[0]) and torch.equal(a.curve[1], b.curve[1]), (pattern, index)
                emitted += int(a.count.sum())
            assert mine[0].begin.shape == (3, PATTERNS[pattern][0] // count + 2) and mine[-1].begin.shape == (3, 1)
    assert emitted >= 6, emitted              # (at -inf every stream has a candidate as soon as the chain fits)


def test_curve_with_absolute_begins_past_4096():
    generator = torch.Generator().manual_seed(4200)
    ppg = R.random_ppg(4200, 3., generator).cuda()
    graph = GRAPHS['phrase']
    whole = alignment.search_graph(ppg, graph, curve=True).curve
    spotter = alignment.SearchGraphStream(graph, -1., curve=True)
    pieces = feed(spotter, ppg, [500] * 8 + [200])
    assert same_bits(torch.cat([piece.curve[0] for piece in pieces]), whole[0])
    assert torch.equal(torch.cat([piece.curve[1] for piece in pieces]), whole[1])
    assert int(whole[1].max()) > 4096 and spotter.position == [4200]


def detector_graphs():
    generator = torch.Generator().manual_seed(5)
    return [G.random_graph(5, generator), G.random_graph(64, generator), G.random_graph(65, generator, wide=(7,)),
            G.random_graph(200, generator, wide=(100, 101))]


def pair_hits(piece, b, q):
    return alignment.GraphHits(piece.begin[b, q], piece.end[b, q], piece.total[b, q], piece.mean[b, q],
                               piece.count[b, q], None)


@pytest.mark.parametrize('patience', [0, 1, 7, 25])
def test_events_equal_the_reference_detector_on_the_device_curve(patience):
    ppg = P.recordings()
    graphs = detector_graphs()
    whole = alignment.search_graph(ppg, graphs, curve=True).curve        # (3, 4, FRAMES) twice
    totals, begins = whole[0].cpu().numpy(), whole[1].cpu().numpy()
    shortest = min(alignment.shortest_match(graph) for graph in graphs)
    emitted = 0
    for threshold in (-INF, -1., -0.3):
        lists = {}
        for name, pushes in PATTERNS.items():
            spotter = alignment.SearchGraphStream(graphs, threshold, patience=patience, batch=3, curve=True)
            pieces = feed(spotter, ppg, pushes)
            pieces.append(spotter.flush())
            assert pieces[0].begin.shape == (3, 4, pushes[0] // shortest + 2) and pieces[-1].begin.shape == (3, 4, 1)
            assert same_bits(torch.cat([piece.curve[0] for piece in pieces[:-1]], dim=2), whole[0])
            pieces = [to_host(piece) for piece in pieces]
            for b in range(3):
                for q in range(4):
                    expected = L.detect(totals[b, q], begins[b, q], threshold, patience, pushes)
                    got = [events_of(pair_hits(piece, b, q)) for piece in pieces]
                    assert len(got) == len(expected)
                    for index, (mine, theirs) in enumerate(zip(got, expected)):
                        assert identical(mine, theirs), (threshold, name, b, q, index, mine, theirs)
                    lists.setdefault((b, q), []).append(L.flat(got))
                    emitted += len(L.flat(got))
        for (b, q), (first, second, third) in lists.items():              # the same events whatever the pushes
            assert identical(first, second) and identical(first, third), (threshold, b, q)
    print(f'search graph stream patience={patience}: {emitted} events compared')
    assert emitted > 100


def planted_problems():
    """(graph, targets, spans): the planted variants and the planted optional pause of tests/test_gpu_search_graph.py."""
    names = ppgs_amd.PHONEMES
    first, second = [names.index(p) for p in ('iy', 'dh', 'er')], [names.index(p) for p in ('ay', 'dh', 'er')]
    filler = names.index('m')
    targets = [filler] * 10 + [p for p in first for _ in range(3)] + [filler] * 10
    targets += [p for p in second for _ in range(3)] + [filler] * 10
    variants = (alignment.phrase_graph([[first, second]])[0], targets, [(10, 19), (29, 38)])
    one, two = [names.index(p) for p in ('w', 'ey')], [names.index(p) for p in ('t', 'uw')]
    word = [p for p in one for _ in range(2)], [p for p in two for _ in range(2)]
    targets = [filler] * 7 + word[0] + [QUIET] * 5 + word[1] + [filler] * 9 + word[0] + word[1] + [filler] * 6
    pause = (alignment.phrase_graph([[one], [two]])[0], targets, [(7, 20), (29, 37)])
    return {'variants': variants, 'pause': pause}


@pytest.mark.parametrize('which', ['variants', 'pause'])
def test_planted_variants_and_a_planted_pause_come_out_exactly_and_on_time(which):
    graph, targets, spans = planted_problems()[which]
    ppg = G.said(targets).cuda()
    frames, patience = len(targets), 5
    for pushes in ([16] * (frames // 16) + [frames % 16], [1, 31, frames - 32], [frames], [1] * frames):
        spotter = alignment.SearchGraphStream(graph, -1e-3, patience=patience)
        pieces = feed(spotter, ppg, pushes)
        assert pieces[0].curve is None
        got = [events_of(piece) for piece in pieces] + [events_of(spotter.flush())]
        assert [(b, e) for b, e, _, _ in L.flat(got)] == spans, (which, pushes)     # in time order
        assert all(total == 0 and mean == 0 for _, _, total, mean in L.flat(got))
        # each one leaves in the push that holds frame end - 1 + patience + 1 (past the last frame: in the flush)
        edges = np.cumsum(pushes)
        due = [[] for _ in range(len(pushes) + 1)]
        for b, e in spans:
            due[int(np.searchsorted(edges, e - 1 + patience + 1, side='right'))].append((b, e))
        assert [[(hit[0], hit[1]) for hit in events] for events in got] == due, (which, pushes)
        assert due[-1] == []
        assert alignment.hit_segments(pieces[-1]) == [(b * 160 / 16000, e * 160 / 16000, 0., 0.)
                                                      for b, e, _, _ in got[-2]]


def ragged_graphs():
    """Five graphs for the ragged schedule of tests/test_gpu_search_stream.py; stream 1 receives 9 frames in all, fewer
    than the chain of 70 and the chain of 12 have states."""
    generator = torch.Generator().manual_seed(41)
    return [G.random_graph(4, generator), alignment.chain_graph([7]), chain(70), chain(12),
            G.random_graph(66, generator, wide=(9,))]


def run_single(ppg, graph, schedule, b, threshold, patience, reset_before=None):
    """One (stream, graph) pair by itself over the same steps: the GraphHits per step (empty pushes included)."""
    spotter = alignment.SearchGraphStream(graph, threshold, patience=patience, curve=True)
    at, out = 0, []
    for index, step in enumerate(schedule):
        if index == reset_before:
            spotter.reset()
        out.append(spotter.push(ppg[b, :, at:at + step[b]].cuda()))
        at += step[b]
    return spotter, out


def test_batch_equals_single_pairs_also_from_two_streams_and_across_a_reset():
    ppg, totals, _, schedule = P.ragged()
    graphs = ragged_graphs()
    threshold, patience = -3., 4
    singles = {}
    for b in range(3):
        for q in range(5):
            spotter, singles[b, q] = run_single(ppg, graphs[q], schedule, b, threshold, patience)
            assert spotter.position == [totals[b]]
    events = sum(int(step.count) for steps in singles.values() for step in steps)
    assert events >= 5                                                     # there is something to compare
    batch = alignment.SearchGraphStream(graphs, threshold, patience=patience, batch=3, curve=True)
    steps = P.run_schedule(batch, ppg, schedule, range(3))
    assert batch.position == totals
    assert steps[0].begin.shape == (3, 5, 16 // 1 + 2) and steps[0].count.shape == (3, 5)
    assert steps[3].begin.shape == (3, 5, 1 // 1 + 2) and bool((steps[3].count == 0).all())      # everyone sat out
    P.equal_to_singles(steps, singles, schedule, range(3), 'batch')
    # stream 1 never has room for 70 or 12 states: a curve of -inf / -1 and no event, flush included
    assert all(bool(torch.isneginf(step.curve[0][1, 2:4]).all()) and bool((step.count[1, 2:4] == 0).all())
               for step in steps)
    last = batch.flush()
    assert last.count.shape == (3, 5) and bool((last.count[1, 2:4] == 0).all())
    for b in range(3):
        for q in range(5):
            one = alignment.SearchGraphStream(graphs[q], threshold, patience=patience)
            feed(one, ppg[b, :, :totals[b]].cuda(), [totals[b]])
            assert identical(events_of(pair_hits(last, b, q)), events_of(one.flush())), (b, q)
    assert bool((batch.flush().count == 0).all())                          # nothing is pending twice
    # the first two streams and the last from two HIP streams at once
    torch.cuda.synchronize()
    sides = [torch.cuda.Stream(), torch.cuda.Stream()]
    halves = [[0, 1], [2]]
    results = [[], []]
    for _ in range(3):
        spotters = [alignment.SearchGraphStream(graphs, threshold, patience=patience, batch=len(rows), curve=True)
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
            P.equal_to_singles(result, singles, schedule, rows, f'side {side}')
    # reset(item=1) before step 2 affects stream 1 only
    again = {(1, q): run_single(ppg, graphs[q], schedule, 1, threshold, patience, reset_before=2)[1] for q in range(5)}
    assert any(not same_bits(again[1, q][2].curve[0], singles[1, q][2].curve[0]) for q in range(5))
    mixed = {key: again.get(key, value) for key, value in singles.items()}
    batch = alignment.SearchGraphStream(graphs, threshold, patience=patience, batch=3, curve=True)
    steps = P.run_schedule(batch, ppg, schedule, range(3), reset_before=2, reset_row=1)
    assert batch.position == [150, 6, 97]
    P.equal_to_singles(steps, mixed, schedule, range(3), 'reset')


# ---- through the raw binding ----

def layout(streams, graphs, most):
    """Byte offsets of the five blocks of a state (include/ppgs_amd.h) and the words of a pair's row."""
    def up(value):
        return (value + 255) // 256 * 256
    row = 64 if most <= 64 else 256
    pairs = streams * graphs
    positions, verdict = 0, up(streams * 4)
    detectors = verdict + up(graphs * 4)
    totals = detectors + up(pairs * 32)
    begins = totals + up(pairs * row * 4)
    assert begins + up(pairs * row * 4) == E.library().ppg_search_graph_stream_state_bytes(streams, graphs, most)
    return positions, verdict, detectors, totals, begins, row


class Packed:
    """Packed host lists (G.pack) on the device, with the host integers of the raw entries."""

    def __init__(self, arrays, max_states=None):
        self.graphs = len(arrays['state_begin']) - 1
        self.n_states, self.n_arcs = len(arrays['phonemes']), len(arrays['sources'])
        counts = np.diff(arrays['state_begin'])
        self.max_states = int(counts.max()) if max_states is None else max_states
        kinds = dict(state_begin=torch.int32, arc_begin=torch.int32, phonemes=torch.int32, sources=torch.int32)
        self.tensors = {name: torch.tensor(arrays[name], dtype=kinds.get(name, torch.float32)).cuda()
                        for name in GRAPH_ARGUMENTS}

    def pointers(self):
        return [self.tensors[name].data_ptr() if self.tensors[name].numel() else None for name in GRAPH_ARGUMENTS]


def raw_open(state, streams, packed, state_offset=0, **changes):
    a = dict(streams=streams, graphs=packed.graphs, n_states=packed.n_states, n_arcs=packed.n_arcs,
             max_states=packed.max_states)
    a.update(changes)
    rc = E.library().ppg_search_graph_stream_open(
        0, state.data_ptr() + state_offset, a['streams'], a['graphs'], a['n_states'], a['n_arcs'], a['max_states'],
        *packed.pointers(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return rc


def raw_push(state, ppg, lengths, packed, workspace, threshold=-INF, patience=3, cap=None, slots=None, want_curve=True,
             curve_begin=True, size=None, offset=0, state_offset=0, **changes):
    """ppg_search_graph_stream_push through ctypes; outputs start as sentinels (-7) and have `slots` >= cap slots per
    pair: (rc, begin, end, total, mean, count, curve_total, curve_begin)."""
    lengths = torch.tensor(lengths, dtype=torch.int32).cuda()
    cap = ppg.shape[2] + 2 if cap is None else cap
    slots = max(cap, 1) if slots is None else slots
    shape = (ppg.shape[0], packed.graphs, slots)
    begin = torch.full(shape, -7, dtype=torch.int32, device='cuda')
    end = torch.full(shape, -7, dtype=torch.int32, device='cuda')
    total = torch.full(shape, -7., device='cuda')
    mean = torch.full(shape, -7., device='cuda')
    count = torch.full(shape[:2], -7, dtype=torch.int32, device='cuda')
    curve_shape = (ppg.shape[0], packed.graphs, ppg.shape[2])
    curves = torch.full(curve_shape, -7., device='cuda'), torch.full(curve_shape, -7, dtype=torch.int32, device='cuda')
    a = dict(frames=ppg.shape[2], streams=ppg.shape[0], graphs=packed.graphs, n_states=packed.n_states,
             n_arcs=packed.n_arcs, max_states=packed.max_states)
    a.update(changes)
    torch.cuda.synchronize()
    rc = E.library().ppg_search_graph_stream_push(
        0, state.data_ptr() + state_offset, ppg.data_ptr(), a['frames'], a['streams'], lengths.data_ptr(), a['graphs'],
        a['n_states'], a['n_arcs'], a['max_states'], *packed.pointers(), threshold, patience, cap, begin.data_ptr(),
        end.data_ptr(), total.data_ptr(), mean.data_ptr(), count.data_ptr(),
        curves[0].data_ptr() if want_curve else None, curves[1].data_ptr() if want_curve and curve_begin else None,
        workspace.data_ptr() + offset, workspace.numel() - offset if size is None else size,
        torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return (rc, begin, end, total, mean, count) + curves


def small_problem():
    """3 streams x 4 graphs of 4, 1, 70 and 12 states (rows of 256 words), one push of 40 frames with lengths 40, 9,
    33."""
    generator = torch.Generator().manual_seed(77)
    graphs = [G.random_graph(4, generator), alignment.chain_graph([7]), G.random_graph(70, generator, wide=(20,)),
              chain(12)]
    lengths = [40, 9, 33]
    ppg = torch.full((3, 40, 40), float('nan'))
    for b, length in enumerate(lengths):
        ppg[b, :, :length] = R.random_ppg(length, 3., generator)
    return ppg.cuda().contiguous(), lengths, graphs


def test_poisoned_state_and_workspace_give_the_same_bits():
    lib = E.library()
    ppg, lengths, graphs = small_problem()
    packed = Packed(G.pack(graphs))
    assert packed.max_states == 70
    state_bytes = lib.ppg_search_graph_stream_state_bytes(3, 4, 70)
    need = lib.ppg_search_graph_stream_workspace_bytes(3, 40, 4)
    runs = []
    for fill in (0, 255):
        state = torch.full((state_bytes,), fill, dtype=torch.uint8, device='cuda')
        workspace = torch.full((need,), fill, dtype=torch.uint8, device='cuda')
        assert raw_open(state, 3, packed) == 0
        positions, verdict, detectors, totals, begins, row = layout(3, 4, 70)
        sizes = ((positions, 12), (verdict, 16), (detectors, 12 * 32), (totals, 12 * row * 4), (begins, 12 * row * 4))
        opened = tuple(state[at:at + size].clone() for at, size in sizes)
        first = raw_push(state, ppg, lengths, packed, workspace)
        second = raw_push(state, ppg, [33, 0, 20], packed, workspace)               # (other frames of the same block)
        assert first[0] == second[0] == 0 and bool((first[5] >= 0).all()) and bool((second[5] >= 0).all())
        # of the state, the five blocks: the bytes that pad each to a multiple of 256 belong to nobody
        blocks = tuple(state[at:at + size] for at, size in sizes)
        runs.append(opened + first[1:] + second[1:] + blocks + (state,))
    for a, b in zip(runs[0][:-1], runs[1][:-1]):
        assert torch.equal(a.view(torch.uint8), b.view(torch.uint8))
    opened = runs[0][:5]
    assert opened[0].view(torch.int32).tolist() == [0, 0, 0] and opened[1].view(torch.int32).tolist() == [1, 1, 1, 1]
    assert opened[2].view(torch.int32).view(12, 8).tolist() == [[0, -1, 0, 0, 0, 0, 0, 0]] * 12
    assert bool(torch.isneginf(opened[3].view(torch.float32)).all()) and bool((opened[4].view(torch.int32) == -1).all())
    assert runs[0][-1][:12].view(torch.int32).tolist() == [73, 9, 53]
    # the curve past a stream's own length is left alone, and so are all the outputs of a stream that sat out but count
    first, second = runs[0][5:12], runs[0][12:19]
    assert bool((first[5][1, :, 9:] == -7).all()) and bool((first[6][2, :, 33:] == -7).all())
    assert bool((second[4][1] == 0).all()) and bool((second[5][1] == -7).all())
    assert bool((second[0][1] == -1).all()) and bool(torch.isnan(second[3][1]).all())
    # through the module: the same bits
    spotter = alignment.SearchGraphStream(graphs, -INF, patience=3, batch=3, curve=True)
    through = spotter.push(ppg, lengths)
    assert through.begin.shape == (3, 4, 42) and torch.equal(through.count, first[4])
    assert same_bits(through.mean, first[3]) and torch.equal(through.begin, first[0])
    assert same_bits(through.curve[0][0], first[5][0])


def test_overflow_counts_every_event_and_writes_cap_slots():
    lib = E.library()
    generator = torch.Generator().manual_seed(3)
    ppg = R.random_ppg(64, 1., generator)[None].cuda().contiguous()
    packed = Packed(G.pack([alignment.chain_graph([17])]))
    results = []
    for cap in (64, 3, 1):
        state = torch.zeros(lib.ppg_search_graph_stream_state_bytes(1, 1, 1), dtype=torch.uint8, device='cuda')
        workspace = torch.zeros(lib.ppg_search_graph_stream_workspace_bytes(1, 64, 1), dtype=torch.uint8, device='cuda')
        assert raw_open(state, 1, packed) == 0
        results.append(raw_push(state, ppg, [64], packed, workspace, patience=0, cap=cap, slots=64) + (state,))
    whole, three, one = results
    count = int(whole[5])
    expected = L.detect(whole[6][0, 0].cpu().numpy(), whole[7][0, 0].cpu().numpy(), -INF, 0, flush=False)[0]
    print(f'search graph stream overflow: {count} events in 64 frames')
    assert count == len(expected) and 10 <= count <= 64
    for result, cap in ((three, 3), (one, 1)):
        assert result[0] == 0 and int(result[5]) == count > cap             # as snprintf: what it would have taken
        for out, full in zip(result[1:5], whole[1:5]):
            assert torch.equal(out[0, 0, :cap].view(torch.int32), full[0, 0, :cap].view(torch.int32))
            assert bool((out[0, 0, cap:] == -7).all())                      # the slots behind stay untouched
        assert torch.equal(result[-1], whole[-1])                           # the state does not depend on cap
    assert bool((whole[1][0, 0, count:] == -1).all()) and bool(torch.isnan(whole[4][0, 0, count:]).all())


def pair_state(buffer, geometry, graphs, b, q):
    _, _, detectors, totals, begins, row = geometry
    pair = b * graphs + q
    return torch.cat([buffer[detectors + pair * 32:detectors + (pair + 1) * 32],
                      buffer[totals + pair * row * 4:totals + (pair + 1) * row * 4],
                      buffer[begins + pair * row * 4:begins + (pair + 1) * row * 4]])


def test_refused_pairs_give_minus_one_and_leave_the_state_and_the_neighbours_alone():
    lib = E.library()
    generator = torch.Generator().manual_seed(3)
    ppg = torch.stack([R.random_ppg(50, 3., generator) for _ in range(3)]).cuda().contiguous()
    good = alignment.chain_graph([3, 3, 17, 4])
    other = G.random_graph(6, generator)
    wide = alignment.chain_graph([n % 40 for n in range(257)])
    fine = G.pack([good, other, good])
    first_arc = fine['arc_begin'][4]
    need = lib.ppg_search_graph_stream_workspace_bytes(3, 50, 3)
    workspace = torch.zeros(need, dtype=torch.uint8, device='cuda')

    def run(arrays, lengths, warm=(7, 7, 7), max_states=None):
        """open, a first push that gives every pair a history, then the push in question: (its result, the state
        before it, the state after it, the geometry)."""
        packed = Packed(arrays, max_states)
        geometry = layout(3, packed.graphs, packed.max_states)
        state = torch.zeros(lib.ppg_search_graph_stream_state_bytes(3, packed.graphs, packed.max_states),
                            dtype=torch.uint8, device='cuda')
        assert raw_open(state, 3, packed) == 0
        assert raw_push(state, ppg, list(warm), packed, workspace)[0] == 0
        before = state.clone()
        result = raw_push(state, ppg, lengths, packed, workspace)
        assert result[0] == 0
        return result, before, state, geometry

    def check(result, before, after, geometry, struck, reference, stays=()):
        ours, theirs = result, reference[0]
        assert bool((ours[5][struck] == -1).all())
        for out, fine_out in zip(ours[1:], theirs[1:]):
            if out is not ours[5]:
                assert bool((out[struck] == -7).all())
            assert torch.equal(out[~struck].view(torch.int32), fine_out[~struck].view(torch.int32))
        now, was, moved = (buffer[:12].view(torch.int32).tolist() for buffer in (after, before, reference[2]))
        assert now == [was[b] if b in stays else moved[b] for b in range(3)]
        for b in range(3):
            for q in range(3):
                if bool(struck[b, q]):
                    assert torch.equal(pair_state(after, geometry, 3, b, q), pair_state(before, geometry, 3, b, q)), (b, q)
                else:
                    assert torch.equal(pair_state(after, geometry, 3, b, q),
                                       pair_state(reference[2], reference[3], 3, b, q)), (b, q)

    reference = run(fine, [50, 41, 50])
    assert bool((reference[0][5] >= 0).all()) and reference[2][:12].view(torch.int32).tolist() == [57, 48, 57]
    column = torch.zeros((3, 3), dtype=torch.bool, device='cuda')
    column[:, 1] = True
    # graphs refused at open: graph 1 of three is broken, graphs 0 and 2 are the good chain
    for label, name, index, value in (('a source out of range', 'sources', first_arc, 6),
                                      ('a negative source', 'sources', first_arc, -1),
                                      ('a NaN weight', 'weights', first_arc, math.nan)):
        arrays = {key: list(values) for key, values in fine.items()}
        arrays[name][index] = value
        result, before, after, geometry = run(arrays, [50, 41, 50])
        assert before[geometry[1]:geometry[1] + 12].view(torch.int32).tolist() == [1, 0, 1], label
        check(result, before, after, geometry, column, reference)
    # a graph of 257 states beside the chain: the check at open passes it (max_states allows it), every push refuses it
    reference_wide = run(G.pack([good, other, good]), [50, 41, 50], max_states=257)
    result, before, after, geometry = run(G.pack([good, wide, good]), [50, 41, 50])
    assert geometry[5] == 256 and before[geometry[1]:geometry[1] + 12].view(torch.int32).tolist() == [1, 1, 1]
    check(result, before, after, geometry, column, reference_wide)
    # a length of frames + 1, and a negative one: the stream's position stays
    rows = torch.zeros((3, 3), dtype=torch.bool, device='cuda')
    rows[0] = rows[2] = True
    result, before, after, geometry = run(fine, [-1, 41, 51])
    check(result, before, after, geometry, rows, reference, stays=(0, 2))


def test_a_stream_at_the_position_limit_takes_what_is_left_and_refuses_more():
    lib = E.library()
    generator = torch.Generator().manual_seed(8)
    ppg = torch.stack([R.random_ppg(16, 3., generator) for _ in range(2)]).cuda().contiguous()
    packed = Packed(G.pack([alignment.chain_graph([7]), chain(3)]))
    workspace = torch.zeros(lib.ppg_search_graph_stream_workspace_bytes(2, 16, 2), dtype=torch.uint8, device='cuda')
    state = torch.zeros(lib.ppg_search_graph_stream_state_bytes(2, 2, 3), dtype=torch.uint8, device='cuda')
    assert raw_open(state, 2, packed) == 0
    assert raw_push(state, ppg, [5, 5], packed, workspace)[0] == 0
    state[4:8] = torch.tensor([2 ** 31 - 9], dtype=torch.int32).view(torch.uint8).cuda()      # stream 1: 8 frames left
    late = state.clone()
    result = raw_push(state, ppg, [16, 9], packed, workspace)
    assert result[0] == 0 and result[5].tolist()[1] == [-1, -1] and bool((result[5][0] >= 0).all())
    assert state[:8].view(torch.int32).tolist() == [21, 2 ** 31 - 9]
    assert torch.equal(state[256:], late[256:]) is False                                      # stream 0 moved on
    geometry = layout(2, 2, 3)
    for q in range(2):
        assert torch.equal(pair_state(state, geometry, 2, 1, q), pair_state(late, geometry, 2, 1, q))
    for out in result[1:5] + result[6:]:
        assert bool((out[1] == -7).all())
    result = raw_push(state, ppg, [0, 8], packed, workspace)
    assert result[0] == 0 and bool((result[5] >= 0).all())
    assert state[:8].view(torch.int32).tolist() == [21, 2 ** 31 - 1]
    begin = result[7][1, 0, :8]                                             # one state: a fresh start at most frames
    assert bool((begin >= 0).all()) and bool((begin <= 2 ** 31 - 2).all()) and int(begin.max()) >= 2 ** 31 - 9
    ends = result[2][1, 0, :int(result[5][1, 0])]
    assert bool((ends > 0).all()) and bool((ends <= 2 ** 31 - 1).all())
    assert raw_push(state, ppg, [0, 1], packed, workspace)[5].tolist()[1] == [-1, -1]           # nothing is left


def test_error_paths_launch_nothing():
    lib = E.library()
    ppg, lengths, graphs = small_problem()
    packed = Packed(G.pack(graphs))
    state_bytes = lib.ppg_search_graph_stream_state_bytes(3, 4, 70)
    need = lib.ppg_search_graph_stream_workspace_bytes(3, 40, 4)
    workspace = torch.zeros(need + 64, dtype=torch.uint8, device='cuda')
    state = torch.zeros(state_bytes + 64, dtype=torch.uint8, device='cuda')
    assert workspace.data_ptr() % 16 == 0 and state.data_ptr() % 16 == 0
    assert raw_open(state, 3, packed) == 0
    assert raw_push(state, ppg, [7, 7, 7], packed, workspace)[0] == 0                # a state with a history
    workspace.zero_()
    before = state.clone()
    refused = [
        raw_push(state, ppg, lengths, packed, workspace, size=need - 1),                        # workspace too small
        raw_push(state, ppg, lengths, packed, workspace, offset=8),                             # misaligned
        raw_push(state, ppg, lengths, packed, workspace, state_offset=8),
        raw_push(state, ppg, lengths, packed, workspace, frames=E.SEARCH_MAX_FRAMES + 1, size=1 << 40),
        raw_push(state, ppg, lengths, packed, workspace, frames=0),
        raw_push(state, ppg, lengths, packed, workspace, streams=E.SEARCH_MAX_ITEMS + 1, size=1 << 50),
        raw_push(state, ppg, lengths, packed, workspace, graphs=E.SEARCH_GRAPH_MAX_GRAPHS + 1),
        raw_push(state, ppg, lengths, packed, workspace, streams=0),
        raw_push(state, ppg, lengths, packed, workspace, graphs=0),
        raw_push(state, ppg, lengths, packed, workspace, max_states=0),
        raw_push(state, ppg, lengths, packed, workspace, max_states=E.VITERBI_MAX_STATES + 1),
        raw_push(state, ppg, lengths, packed, workspace, n_states=3),                           # fewer than graphs
        raw_push(state, ppg, lengths, packed, workspace, n_states=4 * 70 + 1),
        raw_push(state, ppg, lengths, packed, workspace, n_arcs=-1),
        raw_push(state, ppg, lengths, packed, workspace, n_arcs=4 * E.VITERBI_MAX_ARCS + 1),
        raw_push(state, ppg, lengths, packed, workspace, cap=0, slots=1),
        raw_push(state, ppg, lengths, packed, workspace, cap=-1, slots=1),
        raw_push(state, ppg, lengths, packed, workspace, patience=-1),
        raw_push(state, ppg, lengths, packed, workspace, threshold=math.nan),
        raw_push(state, ppg, lengths, packed, workspace, curve_begin=False),                    # one curve pointer only
    ]
    for index, result in enumerate(refused):
        assert result[0] == -1 and lib.ppg_last_error(), index
        for out in result[1:]:
            assert bool((out == -7).all()), index
    assert not workspace.any() and torch.equal(state, before)                                  # nothing was launched
    dummy = ctypes.c_void_p(state.data_ptr())
    stream = torch.cuda.current_stream().cuda_stream
    assert lib.ppg_search_graph_stream_flush(0, dummy, 3, 4, 70, None, None, dummy, dummy, dummy, dummy, stream) == -1
    assert lib.ppg_search_graph_stream_flush(0, dummy, 3, 0, 70, None, dummy, dummy, dummy, dummy, dummy, stream) == -1
    assert lib.ppg_search_graph_stream_reset(0, ctypes.c_void_p(state.data_ptr() + 8), 3, 4, 70, None, stream) == -1
    assert lib.ppg_search_graph_stream_reset(0, dummy, 3, 4, E.VITERBI_MAX_STATES + 1, None, stream) == -1
    for changes in (dict(state_offset=8), dict(streams=0), dict(graphs=0), dict(max_states=0), dict(n_states=3),
                    dict(n_states=4 * 70 + 1), dict(n_arcs=-1), dict(max_states=E.VITERBI_MAX_STATES + 1)):
        assert raw_open(state, changes.pop('streams', 3), packed, **changes) == -1, changes
    torch.cuda.synchronize()
    assert torch.equal(state, before)


def test_audio_stream_into_search_graph_stream():
    generator = torch.Generator().manual_seed(9)
    engine = E.Engine(W.seeded_state_dict(seed=1234), 0, 'fp32', True)
    audio = 0.1 * torch.randn(32000 + 77, generator=generator)
    graph = alignment.phrase_graph([[[5, 17], [5, 9, 17]], [[5]]])[0]
    source, spotter = engine.audio_stream(500), alignment.SearchGraphStream(graph, -2., curve=True)
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
    whole = alignment.search_graph(ppg, graph, curve=True).curve
    assert same_bits(torch.cat([hit.curve[0] for hit in hits]), whole[0])
    assert torch.equal(torch.cat([hit.curve[1] for hit in hits]), whole[1])
    pushes = [piece.shape[1] for piece in pieces]
    expected = L.detect(whole[0].cpu().numpy(), whole[1].cpu().numpy(), -2., 25, pushes)
    got = [events_of(hit) for hit in hits] + [events_of(spotter.flush())]
    assert all(identical(mine, theirs) for mine, theirs in zip(got, expected)) and len(got) == len(expected)
