"""ppgs_amd.alignment.ViterbiStream on the GPU.  Nothing here has a tolerance: where no commit can be forced the runs of
all pushes and of the flush are compared bit for bit with alignment.viterbi over the whole recording, whatever the
pushes; under model_graph every output with RecognizeStream's; forced commits on graphs with the reference stream
(tests/viterbi_stream_reference.py: DESIGN 4.18 word for word in numpy float32) run on the device's own prepared
frames."""
import math

import numpy as np
import pytest
import torch

from ppgs_amd import alignment, engine as E

import alignment_reference as R
import viterbi_reference as V
import viterbi_stream_reference as L
import viterbi_stream_cases as C

pytestmark = pytest.mark.gpu

FRAMES = 200
PATTERNS = {'uneven': [1, 31, 32, 33, 1, 64, 38], 'ones': [1] * FRAMES, 'whole': [FRAMES]}
FIELDS = ('states', 'phonemes', 'begin', 'end', 'score', 'gop')


def bits(tensor):
    return tensor.contiguous().view(torch.int32)


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(bits(a), bits(b))


def feed(stream, ppg, pushes):
    """Push ppg (..., 40, T) in pieces of `pushes` frames: the list of run tuples, one per push (nothing is read)."""
    out, at = [], 0
    for frames in pushes:
        out.append(stream.push(ppg[..., at:at + frames]))
        at += frames
    assert at == ppg.shape[-1]
    return out


def gathered(pieces, fields=FIELDS):
    """The runs of a list of run tuples of a batch of streams (tensors (B, cap)), per stream: a dict of host int32
    arrays (the floats as their bits), concatenated over the pieces; the slots at or past count checked to be -1 / NaN.  One
    copy to the host per field."""
    counts = torch.stack([piece.count for piece in pieces]).cpu().numpy()            # (P, B)
    caps = [piece.phonemes.shape[1] for piece in pieces]
    host = {}
    for name in fields:
        tensors = [getattr(piece, name) for piece in pieces]
        if tensors[0] is None:
            continue
        host[name] = bits(torch.cat(tensors, dim=1)).cpu().numpy()
    out = []
    for b in range(counts.shape[1]):
        parts, at = {name: [] for name in host}, 0
        for index, cap in enumerate(caps):
            count = int(counts[index, b])
            assert 0 <= count <= cap, (index, b, count, cap)
            for name, array in host.items():
                parts[name].append(array[b, at:at + count])
                rest = array[b, at + count:at + cap]
                if name in ('score', 'gop'):
                    assert np.isnan(rest.view(np.float32)).all(), (name, index, b)
                else:
                    assert (rest == -1).all(), (name, index, b)
            at += cap
        out.append({name: np.concatenate(parts[name]) for name in parts})
    return out


def single(runs):
    """The run tuple of one stream as that of a batch of one."""
    return type(runs)(*[None if value is None else value[None] for value in runs])


def expected_of(path):
    """What the concatenated runs must be, from a Path of the whole recording."""
    starts = path.starts.cpu().numpy()
    return {'states': path.states.cpu().numpy(), 'phonemes': path.phonemes.cpu().numpy(), 'begin': starts[:-1],
            'end': starts[1:], 'score': bits(path.score).cpu().numpy(), 'gop': bits(path.gop).cpu().numpy()}


def equal_runs(got, expected):
    return all(got[name].shape == expected[name].shape and (got[name] == expected[name]).all() for name in expected)


def host_runs(runs):
    """A reference run list in the form of `gathered`."""
    return {'states': np.array([run[0] for run in runs], dtype=np.int32),
            'phonemes': np.array([run[1] for run in runs], dtype=np.int32),
            'begin': np.array([run[2] for run in runs], dtype=np.int32),
            'end': np.array([run[3] for run in runs], dtype=np.int32),
            'score': np.array([run[4] for run in runs], dtype=np.float32).view(np.int32),
            'gop': np.array([run[5] for run in runs], dtype=np.float32).view(np.int32)}


def device_frames(ppg):
    """logp (T, 40) and top (T,) float32 as the device prepares them: the score of a one-frame utterance aligned to
    phoneme q is logp[t, q] exactly (a sum of one term over 1.f)."""
    frames = ppg.shape[1]
    x = ppg.t().repeat_interleave(40, dim=0)[:, :, None].contiguous()               # item t * 40 + q: frame t
    table = torch.arange(40, dtype=torch.int32).repeat(frames)[:, None].cuda()
    _, _, score, _ = E.align_items(x, [1] * (40 * frames), table, [1] * (40 * frames))
    logp = score.reshape(frames, 40).cpu().numpy()
    return logp, logp.max(axis=1)


# ---- 1. (I1): without force the runs are those of viterbi, bit for bit ----

def test_without_force_the_runs_are_those_of_viterbi_bit_for_bit():
    names, graphs, ppgs = C.first_cases()
    count = len(graphs)
    ppg = torch.stack(ppgs).cuda()
    assert ppg.shape == (count, 40, FRAMES)
    whole = alignment.viterbi(ppg, graphs)                                           # the reference, once
    expected = [expected_of(alignment.Path(*[field[b] for field in whole])) for b in range(count)]
    # (300 states have no path through 200 frames: that stream gives no runs and a total of -inf, as viterbi does)
    assert [len(item['states']) >= 1 for item in expected] == [label != 'chain 300' for label in names]
    for name, pushes in PATTERNS.items():
        stream = alignment.ViterbiStream(graphs, window=1024, max_lag=1023, batch=count)
        pieces = feed(stream, ppg, pushes)
        assert stream.position == [FRAMES] * count
        assert all(piece.states.shape == (count, 1023 + size) and piece.total is None and piece.forced is None
                   for piece, size in zip(pieces, pushes))
        early = torch.stack([piece.count for piece in pieces]).sum(dim=0).tolist()
        last = stream.flush()
        assert last.states.shape == (count, 1024) and stream.position == [0] * count
        got = gathered(pieces + [last])
        assert last.forced.tolist() == [0] * count, name
        assert same_bits(last.total, whole.total), name
        for b in range(count):
            if names[b] == 'chain 300':                                              # (I1) asks for a path: here the
                assert len(got[b]['states']) <= 1 and (got[b]['end'] <= 1).all()     # open run of frame 0 is closed
                continue
            assert equal_runs(got[b], expected[b]), (name, names[b])
        # not vacuous: the loop and the 700-state graph give runs out before the flush, the chains cannot
        for b, label in enumerate(names):
            if label in C.EARLY:
                assert early[b] >= 1, (name, label)
            if label.startswith('chain'):
                assert early[b] == 0, (name, label)
        # after the flush the streams start again at frame 0 with their graphs
        again = feed(stream, ppg[:, :, :60], [60]) + [stream.flush()]
        short = alignment.viterbi(ppg[:, :, :60], graphs)
        assert same_bits(again[-1].total, short.total), name
        got = gathered(again)
        for b in range(count):
            path = expected_of(alignment.Path(*[field[b] for field in short]))
            assert len(path['states']) == 0 or equal_runs(got[b], path), (name, names[b])


# ---- 2. the ring wraps and nothing is forced ----

@pytest.mark.parametrize('kind', ['loop', 'model'])
def test_ring_wraps_and_nothing_is_forced(kind):
    graph, ppg = C.wrap_case(kind)
    ppg = ppg.cuda()
    frames = ppg.shape[1]
    assert frames >= 2 * C.WRAP_WINDOW + 1
    whole = alignment.viterbi(ppg, graph)
    expected = expected_of(whole)
    assert len(expected['states']) > 10
    for pushes in ([1] * frames, [7] * (frames // 7) + [frames % 7], [32] * (frames // 32) + [frames % 32], [frames]):
        stream = alignment.ViterbiStream(graph, window=C.WRAP_WINDOW, max_lag=C.WRAP_LAG)
        pieces = feed(stream, ppg, pushes)
        assert all(piece.states.shape == (C.WRAP_LAG + size,) for piece, size in zip(pieces, pushes))
        last = stream.flush()
        assert int(last.forced) == 0, (kind, pushes[0])                              # from the device
        assert same_bits(last.total, whole.total)
        got = gathered([single(piece) for piece in pieces + [last]])[0]
        assert equal_runs(got, expected), (kind, pushes[0])


# ---- 3. (I2): under model_graph every output is RecognizeStream's ----

@pytest.mark.parametrize('max_lag', [0, 1, 7, 32])
def test_under_model_graph_every_output_is_that_of_the_live_recogniser(max_lag):
    generator = torch.Generator().manual_seed(300)
    ppg = R.random_ppg(300, 1., generator).cuda()
    forced = 0
    for keywords in (dict(transitions=alignment.switch_penalty(4.)), C.random_model(7)):
        graph = alignment.model_graph(**keywords)
        for pushes in ([7] * 42 + [6], [1, 31, 32 - max_lag, 33 - max_lag, 1, 57 - max_lag, 38, 43, 0, 57 - max_lag, 7,
                                       2 * max_lag]):
            pushes = pushes + [300 - sum(pushes)]
            assert min(pushes) >= 0
            theirs = alignment.RecognizeStream(window=64, max_lag=max_lag, **keywords)
            mine = alignment.ViterbiStream(graph, window=64, max_lag=max_lag)
            for a, b in zip(feed(theirs, ppg, pushes) + [theirs.flush()], feed(mine, ppg, pushes) + [mine.flush()]):
                assert torch.equal(b.states, b.phonemes)                             # state q carries phoneme q
                for name in alignment.Runs._fields:
                    x, y = getattr(a, name), getattr(b, name)
                    assert (x is None) == (y is None) and (x is None or same_bits(x, y)), (max_lag, pushes[0], name)
            forced += int(b.forced)
    assert forced > 0 or max_lag == 32


# ---- 4. forced commits on graphs: the reference on the device's own frames ----

@pytest.mark.parametrize('max_lag', [0, 1, 7])
def test_forced_commits_equal_the_reference_on_the_device_frames(max_lag):
    for label, graph, ppg in C.forced_cases():
        ppg = ppg.cuda()
        frames = ppg.shape[1]
        logp, top = device_frames(ppg)
        rest = frames - 195
        for pushes in ([7] * (frames // 7) + [frames % 7],
                       [1, 31, 32, 33, 1, 40, 0, 57] + [50] * (rest // 50) + [rest % 50]):
            reference = L.Stream(V.lists(graph), max_lag=max_lag, window=64, dtype=np.float32)
            theirs = L.feed(reference, logp, top, pushes)
            assert all(runs is not None for runs in theirs)
            final_runs, total, forced = reference.flush()
            stream = alignment.ViterbiStream(graph, window=64, max_lag=max_lag)
            pieces = feed(stream, ppg, pushes)
            last = stream.flush()
            counts = [int(piece.count) for piece in pieces + [last]]
            assert counts == [len(runs) for runs in theirs + [final_runs]], (label, max_lag, pushes[0])
            got = gathered([single(piece) for piece in pieces + [last]])[0]
            assert equal_runs(got, host_runs(L.flat(theirs) + final_runs)), (label, max_lag, pushes[0])
            assert int(last.forced) == forced and np.float32(total).tobytes() == last.total.cpu().numpy().tobytes()
            assert forced > 0, (label, forced)                                       # the forced step did run
            if label.startswith('chain'):
                # a complete left-to-right alignment although nothing commits naturally
                assert float(last.total) > -math.inf
                assert got['states'].tolist() == list(range(graph.phonemes.shape[0]))
                assert got['begin'][0] == 0 and got['end'][-1] == frames
                assert (got['begin'][1:] == got['end'][:-1]).all()


# ---- 5. (I3): a batch equals its single streams ----

def push_ragged(stream, ppg, steps, begin=None):
    """Push (3, 40, T) raggedly with NaN padding: the list of run tuples."""
    at, out = list(begin or [0, 0, 0]), []
    for lengths in steps:
        block = torch.full((3, 40, 40), math.nan, device='cuda')
        for b, size in enumerate(lengths):
            block[b, :, :size] = ppg[b, :, at[b]:at[b] + size]
            at[b] += size
        out.append(stream.push(block, lengths))
    return out


def test_ragged_batch_equals_single_streams_also_from_two_hip_streams_and_across_a_reset():
    graphs, ppg = C.ragged_case()
    ppg = ppg.cuda()
    steps = [[40, 0, 17], [1, 40, 33], [39, 25, 0], [40, 24, 40], [30, 1, 30]]         # 150, 90 and 120 frames
    keywords = dict(window=128, max_lag=20)

    def alone(b, low, cuts):
        one = alignment.ViterbiStream(graphs[b], **keywords)
        pieces = [one.push(ppg[b, :, low + sum(cuts[:k]):low + sum(cuts[:k + 1])]) for k in range(len(cuts))]
        last = one.flush()
        return gathered([single(piece) for piece in pieces + [last]])[0], last
    singles, totals, forced = [], [], []
    for b in range(3):
        runs, last = alone(b, 0, [step[b] for step in steps])
        singles.append(runs)
        totals.append(bits(last.total).item())
        forced.append(int(last.forced))
    assert sum(forced) > 0                                                           # the chains are forced
    batch = alignment.ViterbiStream(graphs, batch=3, **keywords)
    pieces = push_ragged(batch, ppg, steps)
    assert batch.position == [150, 90, 120]
    last = batch.flush()
    got = gathered(pieces + [last])
    for b in range(3):
        assert equal_runs(got[b], singles[b]), b
    assert bits(last.total).tolist() == totals and last.forced.tolist() == forced
    # two HIP streams at once, each with its own object
    side = [torch.cuda.Stream(), torch.cuda.Stream()]
    objects = [alignment.ViterbiStream(graphs, batch=3, **keywords) for _ in side]
    results = []
    torch.cuda.synchronize()
    for own, queue in zip(objects, side):
        with torch.cuda.stream(queue):
            results.append(push_ragged(own, ppg, steps) + [own.flush()])
    torch.cuda.synchronize()
    for result in results:
        other = gathered(result)
        assert all(equal_runs(other[b], singles[b]) for b in range(3))
        assert bits(result[-1].total).tolist() == totals and result[-1].forced.tolist() == forced
    # reset(item=1) in the middle: stream 1 starts again, the others go on
    batch = alignment.ViterbiStream(graphs, batch=3, **keywords)
    first = push_ragged(batch, ppg, steps[:2])
    batch.reset(item=1)
    assert batch.position == [41, 0, 50]
    rest = push_ragged(batch, ppg, steps[2:], begin=[41, 40, 50])
    last = batch.flush()
    got = gathered(first + rest + [last])
    assert equal_runs(got[0], singles[0]) and equal_runs(got[2], singles[2])
    expected, _ = alone(1, 40, [25, 24, 1])
    assert equal_runs(gathered(rest + [last])[1], expected)
    # flush(item): the others keep their state
    batch = alignment.ViterbiStream(graphs, batch=3, **keywords)
    first = push_ragged(batch, ppg, steps[:2])
    only = batch.flush(item=2)
    assert only.count[:2].tolist() == [0, 0] and only.forced[:2].tolist() == [-1, -1]
    assert bool(torch.isnan(only.total[:2]).all()) and batch.position == [41, 40, 0]
    rest = push_ragged(batch, ppg, [[step[0], step[1], 0] for step in steps[2:]], begin=[41, 40, 120])
    got = gathered(first + rest + [batch.flush()])
    assert equal_runs(got[0], singles[0]) and equal_runs(got[1], singles[1])


# ---- 6. the library's entries: poison, cap, refusals ----

def packed_of(graphs, device='cuda'):
    """engine.PackedGraphs of a list of Graphs on the device, as ViterbiStream packs them."""
    several = len(graphs) > 1
    stream = alignment.ViterbiStream(graphs if several else graphs[0], batch=len(graphs) if several else None)
    return E.PackedGraphs(*[value.to(device).contiguous() if torch.is_tensor(value) else value
                            for value in stream._graphs])


def graph_arguments(packed):
    return (packed.graphs, packed.states, packed.arcs, packed.max_states, packed.state_begin.data_ptr(),
            packed.phonemes.data_ptr(), packed.stay.data_ptr(), packed.initial.data_ptr(), packed.final.data_ptr(),
            packed.arc_begin.data_ptr(), packed.sources.data_ptr() if packed.arcs else None,
            packed.weights.data_ptr() if packed.arcs else None)


def raw_outputs(streams, slots):
    return [torch.full((streams, slots), -7, dtype=torch.int32, device='cuda') for _ in range(4)] + \
           [torch.full((streams, slots), -7., dtype=torch.float32, device='cuda') for _ in range(2)] + \
           [torch.full((streams,), -7, dtype=torch.int32, device='cuda')]


def raw_open(state, streams, window, packed, which=None, changes=()):
    arguments = dict(streams=streams, window=window)
    arguments.update(dict(changes))
    which = None if which is None else torch.tensor(which, dtype=torch.int32).cuda()
    with torch.cuda.device(0):
        rc = E.library().ppg_viterbi_stream_open(
            0, state.data_ptr(), arguments['streams'], arguments['window'], *graph_arguments(packed),
            None if which is None else which.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return rc


def raw_push(state, window, ppg, lengths, packed, workspace, max_lag=8, cap=None, slots=None, changes=()):
    """ppg_viterbi_stream_push with outputs prefilled with -7: (rc, states, phonemes, begin, end, score, gop, count)."""
    cap = max_lag + ppg.shape[2] if cap is None else cap
    outputs = raw_outputs(ppg.shape[0], slots or max(cap, 1))
    lengths = torch.tensor(lengths, dtype=torch.int32).cuda()
    a = dict(state=state.data_ptr(), streams=ppg.shape[0], window=window, frames=ppg.shape[2], max_lag=max_lag,
             cap=cap, workspace=workspace.data_ptr(), size=workspace.numel(), graphs=graph_arguments(packed))
    a.update(dict(changes))
    with torch.cuda.device(0):
        rc = E.library().ppg_viterbi_stream_push(
            0, a['state'], a['streams'], a['window'], ppg.data_ptr(), a['frames'], lengths.data_ptr(), *a['graphs'],
            a['max_lag'], a['cap'], *[out.data_ptr() for out in outputs], a['workspace'], a['size'],
            torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return (rc,) + tuple(outputs)


def raw_flush(state, streams, window, packed, cap, changes=()):
    outputs = raw_outputs(streams, max(cap, 1))
    total = torch.full((streams,), -7., dtype=torch.float32, device='cuda')
    forced = torch.full((streams,), -7, dtype=torch.int32, device='cuda')
    a = dict(state=state.data_ptr(), streams=streams, window=window, cap=cap, graphs=graph_arguments(packed))
    a.update(dict(changes))
    with torch.cuda.device(0):
        rc = E.library().ppg_viterbi_stream_flush(
            0, a['state'], a['streams'], a['window'], *a['graphs'], None, a['cap'],
            *[out.data_ptr() for out in outputs], total.data_ptr(), forced.data_ptr(),
            torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return (rc,) + tuple(outputs) + (total, forced)


def state_of(streams, window, packed, fill):
    size = E.library().ppg_viterbi_stream_state_bytes(streams, window, packed.max_states)
    assert size > 0
    return torch.full((size,), fill, dtype=torch.uint8, device='cuda')


def workspace_of(streams, frames, fill=0):
    return torch.full((E.library().ppg_viterbi_stream_workspace_bytes(streams, frames),), fill, dtype=torch.uint8,
                      device='cuda')


def heads_of(state, streams):
    return state[:streams * 32].view(torch.int32).reshape(streams, 8).cpu()


def test_poisoned_state_and_workspace_give_the_same_bits():
    graphs, ppg = C.ragged_case()
    ppg = ppg[:, :, :40].cuda().contiguous()
    packed = packed_of(graphs)
    runs = []
    for fill in (0x00, 0xFF):
        state, workspace = state_of(3, 64, packed, fill), workspace_of(3, 40, fill)
        assert raw_open(state, 3, 64, packed, [0, 1, 2]) == 0
        assert heads_of(state, 3).tolist() == [[0, 0, 0, -1, 0, 0, 0, g] for g in range(3)]
        out = raw_push(state, 64, ppg, [40, 40, 40], packed, workspace)
        assert out[0] == 0
        last = raw_flush(state, 3, 64, packed, 9)
        assert last[0] == 0
        runs.append([bits(value).clone() for value in out[1:] + last[1:]])
    assert all(torch.equal(a, b) for a, b in zip(*runs))
    assert (runs[0][6] >= 0).all() and (runs[0][-1] >= 0).all()                      # the push's counts; forced


def test_a_small_cap_counts_the_runs_and_writes_cap_slots():
    graph, ppg = C.wrap_case('loop')
    ppg = ppg[None, :, :64].cuda().contiguous()
    packed = packed_of([graph])
    workspace = workspace_of(1, 64)
    results = []
    for cap in (72, 2):
        state = state_of(1, 128, packed, 0xFF)
        assert raw_open(state, 1, 128, packed) == 0
        out = raw_push(state, 128, ppg, [64], packed, workspace, max_lag=8, cap=cap, slots=72)
        assert out[0] == 0
        results.append((out, state.clone()))
    (full, state_full), (small, state_small) = results
    count = int(full[7])
    assert count > 2 and int(small[7]) == count                                      # count > cap: the push overflowed
    for a, b in zip(full[1:7], small[1:7]):
        assert torch.equal(bits(a)[0, :2], bits(b)[0, :2])
        assert (bits(b)[0, 2:] == bits(torch.full_like(b, -7))[0, 2:]).all()         # exactly cap slots written
    assert torch.equal(state_full, state_small)                                      # the state does not depend on cap


def test_impossible_pushes_get_minus_one_and_keep_their_state():
    graphs, ppg = C.ragged_case()
    ppg = ppg.cuda()
    packed = packed_of(graphs)
    state, workspace = state_of(3, 64, packed, 0xFF), workspace_of(3, 64)
    assert raw_open(state, 3, 64, packed, [0, 1, 2]) == 0
    # max_lag 63: the chains commit nothing, so 40 + 40 frames overfill the window of streams 0 and 2
    first = raw_push(state, 64, ppg[:, :, :40].contiguous(), [40, 40, 40], packed, workspace, max_lag=63)
    assert first[0] == 0 and (first[7] >= 0).all()
    before = state.clone()
    heads = heads_of(state, 3)
    assert heads[:, 0].tolist() == [40, 40, 40]
    open_frames = (heads[:, 0] - heads[:, 1]).tolist()
    second = raw_push(state, 64, ppg[:, :, 40:80].contiguous(), [40, 41, -1], packed, workspace, max_lag=63)
    assert second[0] == 0
    assert open_frames[0] + 40 > 64                                                  # the condition on the input
    assert second[7].tolist() == [-1, -1, -1]    # an overfull window, a length past the frames, a negative length
    assert torch.equal(state, before)
    assert all((bits(out) == bits(torch.full_like(out, -7))).all() for out in second[1:7])
    # position 2^31 - 9 taking 9 frames
    words = state[:32].view(torch.int32)
    words[0] = words[1] = 2 ** 31 - 9
    before = state.clone()
    third = raw_push(state, 64, ppg[:, :, :9].contiguous(), [9, 0, 0], packed, workspace, max_lag=63)
    assert third[0] == 0 and third[7].tolist()[0] == -1 and torch.equal(state, before)
    eight = raw_push(state, 64, ppg[:, :, :8].contiguous(), [8, 0, 0], packed, workspace, max_lag=63)
    assert eight[0] == 0 and eight[7].tolist()[0] >= 0 and heads_of(state, 3)[0, 0] == 2 ** 31 - 1


def test_refused_graphs_answer_minus_one_and_leave_the_stream_beside_them_alone():
    good, ppg = C.wrap_case('loop')
    ppg = ppg[:, :48].cuda()
    block = torch.stack([ppg, ppg]).contiguous()
    reference = alignment.ViterbiStream(good, window=64, max_lag=8)
    expected = gathered([single(reference.push(ppg)), single(reference.flush())])[0]
    small = alignment.graph([1, 2, 3], [(0, 1, 0.), (1, 2, 0.)])
    for label, damage in C.DAMAGE.items():
        packed = packed_of([small, good])
        packed = damage(packed)
        which = [0, 1] if label != 'which_graph out of range' else [2, 1]
        state, workspace = state_of(2, 64, packed, 0xFF), workspace_of(2, 48)
        assert raw_open(state, 2, 64, packed, which) == 0
        assert heads_of(state, 2)[:, 7].tolist() == [-1, 1], label
        before = state.clone()
        out = raw_push(state, 64, block, [48, 48], packed, workspace)
        assert out[0] == 0 and out[7].tolist()[0] == -1 and out[7].tolist()[1] >= 0, label
        size = state.numel()                                                         # stream 0's blocks are untouched
        assert torch.equal(state[:32], before[:32]), label
        last = raw_flush(state, 2, 64, packed, 9)
        assert last[0] == 0 and last[7].tolist()[0] == 0 and int(last[9][0]) == -1, label
        assert math.isnan(float(last[8][0])), label
        assert heads_of(state, 2)[0].tolist() == [0, 0, 0, -1, 0, 0, 0, -1], label
        names = ('states', 'phonemes', 'begin', 'end', 'score', 'gop')
        beside = {}
        for index, name in enumerate(names):
            parts = []
            for result in (out, last):
                count = int(result[7][1])
                parts.append(bits(result[1 + index])[1, :count].cpu().numpy())
            beside[name] = np.concatenate(parts)
        assert equal_runs(beside, expected), label
        assert size == state.numel()


def test_einval_paths_leave_outputs_and_state_alone():
    graph, ppg = C.wrap_case('loop')
    block = ppg[None, :, :16].cuda().contiguous()
    packed = packed_of([graph])
    state, workspace = state_of(1, 64, packed, 0xFF), workspace_of(1, 16)
    assert raw_open(state, 1, 64, packed) == 0
    before = state.clone()
    graphs = graph_arguments(packed)
    bad = [dict(streams=0), dict(window=96), dict(window=32), dict(frames=0), dict(max_lag=64), dict(max_lag=-1),
           dict(cap=0), dict(size=workspace.numel() - 1), dict(state=state.data_ptr() + 8),
           dict(workspace=workspace.data_ptr() + 8), dict(graphs=(2,) + graphs[1:]), dict(graphs=(0,) + graphs[1:]),
           dict(graphs=graphs[:3] + (0,) + graphs[4:]), dict(graphs=graphs[:3] + (1025,) + graphs[4:]),
           dict(graphs=graphs[:4] + (None,) + graphs[5:]), dict(graphs=graphs[:10] + (None, None)),
           dict(graphs=graphs[:1] + (0,) + graphs[2:])]
    for changes in bad:
        out = raw_push(state, 64, block, [16], packed, workspace, changes=changes)
        assert out[0] == -1, changes
        assert all((bits(value) == bits(torch.full_like(value, -7))).all() for value in out[1:]), changes
        assert torch.equal(state, before), changes
    for changes in (dict(streams=0), dict(window=100), dict(cap=0), dict(state=state.data_ptr() + 8),
                    dict(graphs=(2,) + graphs[1:]), dict(graphs=graphs[:3] + (0,) + graphs[4:])):
        out = raw_flush(state, 1, 64, packed, 9, changes=changes)
        assert out[0] == -1, changes
        assert all((bits(value) == bits(torch.full_like(value, -7))).all() for value in out[1:]), changes
        assert torch.equal(state, before), changes
    assert raw_open(state, 1, 64, packed, changes=dict(streams=0)) == -1
    assert raw_open(state, 1, 64, packed, changes=dict(window=65)) == -1
    assert torch.equal(state, before)


def test_no_state_may_begin_gives_no_runs_and_a_total_of_minus_infinity():
    graph = alignment.chain_graph([3, 4, 5])
    dead = alignment.Graph(*[value if name != 'initial' else torch.full((3,), -math.inf)
                             for name, value in zip(alignment.Graph._fields, graph)])
    stream = alignment.ViterbiStream(dead, window=64, max_lag=4)
    ppg = R.random_ppg(30, 3., torch.Generator().manual_seed(5)).cuda()
    pieces = feed(stream, ppg, [10, 20])
    last = stream.flush()
    assert [int(piece.count) for piece in pieces] == [0, 0] and int(last.count) == 0
    assert float(last.total) == -math.inf and int(last.forced) == 0


# ---- 7. end to end: audio through the engine's stream into a word loop ----

def test_audio_stream_into_a_word_loop_equals_viterbi_of_the_whole():
    from ppgs_amd import weights as W
    engine = E.Engine(W.seeded_state_dict(seed=1234), 0, 'fp32', True)               # causal: it has audio streams
    generator = torch.Generator().manual_seed(77)
    audio = (0.1 * torch.randn(32000, generator=generator)).cuda()                   # 2 s
    graph, _ = C.wrap_loop()
    stream = alignment.ViterbiStream(graph, window=1024)
    source = engine.audio_stream(500)
    pieces, ppgs, at = [], [], 0
    sizes = (1600, 0, 7001, 399, 16000, 1, 6999)
    for index, size in enumerate(sizes):
        out = source.push(audio[at:at + size], flush=index == len(sizes) - 1)
        at += size
        assert out.shape[0] == 40
        ppgs.append(out)
        pieces.append(stream.push(out))
    assert at == 32000 and any(ppg.shape[1] == 0 for ppg in ppgs)                    # empty pieces included
    whole = torch.cat(ppgs, dim=1)
    assert whole.shape == (40, 200)
    last = stream.flush()
    path = alignment.viterbi(whole, graph)
    assert int(last.forced) == 0 and same_bits(last.total, path.total)
    got = gathered([single(piece) for piece in pieces + [last]])[0]
    assert len(got['states']) >= 1 and equal_runs(got, expected_of(path))
