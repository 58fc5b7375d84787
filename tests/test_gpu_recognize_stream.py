"""ppgs_amd.alignment.RecognizeStream on the GPU.  Nothing here has a tolerance: where no commit can be forced the
runs of all pushes and of the flush are compared bit for bit with alignment.recognize over the whole recording,
whatever the pushes; forced commits with the reference stream (tests/recognize_stream_reference.py: DESIGN 4.16 word
for word in numpy float32) run on the device's own prepared frames."""
import ctypes
import math

import numpy as np
import pytest
import torch

from ppgs_amd import alignment, engine as E
from ppgs_amd import weights as W

import alignment_reference as R
import recognize_stream_reference as L

pytestmark = pytest.mark.gpu

FRAMES = 200
PATTERNS = {'uneven': [1, 31, 32, 33, 1, 64, 38], 'ones': [1] * FRAMES, 'whole': [FRAMES]}
SCALES = (1., 3., 8.)
FIELDS = ('phonemes', 'begin', 'end', 'score', 'gop')


def bits(tensor):
    return tensor.contiguous().view(torch.int32)


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(bits(a), bits(b))


def feed(stream, ppg, pushes):
    """Push ppg (..., 40, T) in pieces of `pushes` frames: the list of Runs, one per push (nothing is read back)."""
    out, at = [], 0
    for frames in pushes:
        out.append(stream.push(ppg[..., at:at + frames]))
        at += frames
    assert at == ppg.shape[-1]
    return out


def gathered(pieces):
    """The runs of a list of Runs of a batch of streams (tensors (B, cap)), per stream: a dict of host int32 arrays
    (the floats as their bits), concatenated over the pieces; the slots at or past count checked to be -1 / NaN.  One
    copy to the host per field."""
    counts = torch.stack([piece.count for piece in pieces]).cpu().numpy()            # (P, B)
    caps = [piece.phonemes.shape[1] for piece in pieces]
    host = {}
    for name in FIELDS:
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
    """A Runs of one stream as a Runs of a batch of one."""
    return alignment.Runs(*[None if value is None else value[None] for value in runs])


def expected_of(said):
    """What the concatenated runs must be, from a Recognition of the whole recording."""
    starts = said.starts.cpu().numpy()
    return {'phonemes': said.phonemes.cpu().numpy(), 'begin': starts[:-1], 'end': starts[1:],
            'score': bits(said.score).cpu().numpy(), 'gop': bits(said.gop).cpu().numpy()}


def equal_runs(got, expected):
    return all(got[name].shape == expected[name].shape and (got[name] == expected[name]).all() for name in expected)


_recordings = {}


def recordings():
    """The three recordings of FRAMES frames (one per softmax scale) on the device, made once: (3, 40, FRAMES)."""
    if 'ppg' not in _recordings:
        generator = torch.Generator().manual_seed(20416)
        _recordings['ppg'] = torch.stack([R.random_ppg(FRAMES, scale, generator) for scale in SCALES]).cuda()
    return _recordings['ppg']


def random_model(seed):
    """transitions, initial, final with -inf entries that leave a path."""
    generator = torch.Generator().manual_seed(seed)
    A = -5. * torch.rand(40, 40, generator=generator)
    A[torch.rand(40, 40, generator=generator) < 0.3] = -math.inf
    A.fill_diagonal_(-0.25)
    initial, final = -2. * torch.rand(40, generator=generator), -2. * torch.rand(40, generator=generator)
    initial[torch.rand(40, generator=generator) < 0.3] = -math.inf
    final[torch.rand(40, generator=generator) < 0.3] = -math.inf
    return {'transitions': A, 'initial': initial, 'final': final}


MODELS = {'penalty 0': {'penalty': 0.}, 'penalty 1': {'penalty': 1.}, 'penalty 4': {'penalty': 4.},
          'random': random_model(7)}


@pytest.mark.parametrize('model', list(MODELS))
def test_without_force_the_runs_are_those_of_recognize_bit_for_bit(model):
    ppg = recordings()
    keywords = MODELS[model]
    whole = alignment.recognize(ppg, **keywords)                                     # the reference, once
    expected = [expected_of(alignment.Recognition(*[field[b] for field in whole])) for b in range(3)]
    assert all(len(item['phonemes']) >= 1 for item in expected)
    for name, pushes in PATTERNS.items():
        stream = alignment.RecognizeStream(window=1024, max_lag=512, batch=3, **keywords)
        pieces = feed(stream, ppg, pushes)
        assert stream.position == [FRAMES] * 3
        assert all(piece.phonemes.shape == (3, 512 + size) and piece.total is None and piece.forced is None
                   for piece, size in zip(pieces, pushes))
        last = stream.flush()
        assert last.phonemes.shape == (3, 513) and stream.position == [0, 0, 0]
        got = gathered(pieces + [last])
        assert last.forced.tolist() == [0, 0, 0], (model, name)
        assert same_bits(last.total, whole.total), (model, name)
        for b in range(3):
            assert equal_runs(got[b], expected[b]), (model, name, b)
        # after the flush the stream starts again at frame 0
        again = feed(stream, ppg[:, :, :40], [40]) + [stream.flush()]
        short = alignment.recognize(ppg[:, :, :40], **keywords)
        assert same_bits(again[-1].total, short.total)
        assert equal_runs(gathered(again)[1], expected_of(alignment.Recognition(*[field[1] for field in short])))


@pytest.mark.parametrize('scale', L.WRAP_SCALES)
def test_ring_wraps_and_nothing_is_forced(scale):
    ppg = L.wrap_ppg(scale).cuda()
    for penalty in L.WRAP_PENALTIES:
        whole = alignment.recognize(ppg, penalty=penalty)
        expected = expected_of(whole)
        for pushes in ([1] * L.WRAP_FRAMES, [7] * 42 + [6], [32] * 9 + [12], [L.WRAP_FRAMES]):
            stream = alignment.RecognizeStream(penalty=penalty, window=L.WRAP_WINDOW, max_lag=L.WRAP_LAG)
            pieces = feed(stream, ppg, pushes)
            assert all(piece.phonemes.shape == (L.WRAP_LAG + size,) for piece, size in zip(pieces, pushes))
            last = stream.flush()
            assert int(last.forced) == 0, (scale, penalty, pushes[0])              # from the device
            assert same_bits(last.total, whole.total)
            got = gathered([single(piece) for piece in pieces + [last]])[0]
            assert equal_runs(got, expected), (scale, penalty, pushes[0])


def device_frames(ppg):
    """e (T, 40) and top (T,) float32 as the device prepares them: the score of a one-frame utterance aligned to
    phoneme q is e[t, q] exactly (a sum of one term over 1.f)."""
    frames = ppg.shape[1]
    x = ppg.t().repeat_interleave(40, dim=0)[:, :, None].contiguous()               # item t * 40 + q: frame t
    table = torch.arange(40, dtype=torch.int32).repeat(frames)[:, None].cuda()
    _, _, score, _ = E.align_items(x, [1] * (40 * frames), table, [1] * (40 * frames))
    e = score.reshape(frames, 40).cpu().numpy()
    return e, e.max(axis=1)


def host_runs(runs):
    """A reference run list in the form of `gathered`."""
    return {'phonemes': np.array([run[0] for run in runs], dtype=np.int32),
            'begin': np.array([run[1] for run in runs], dtype=np.int32),
            'end': np.array([run[2] for run in runs], dtype=np.int32),
            'score': np.array([run[3] for run in runs], dtype=np.float32).view(np.int32),
            'gop': np.array([run[4] for run in runs], dtype=np.float32).view(np.int32)}


@pytest.mark.parametrize('max_lag', [0, 1, 7])
def test_forced_commits_equal_the_reference_on_the_device_frames(max_lag):
    generator = torch.Generator().manual_seed(300)
    ppg = R.random_ppg(300, 1., generator).cuda()
    e, top = device_frames(ppg)
    forced_frames = 0
    for pushes in ([7] * 42 + [6], [1, 31, 32, 33, 1, 57, 38, 43, 0, 57, 7]):
        reference = L.Stream(L.switch(4.), None, max_lag=max_lag, window=64, dtype=np.float32)
        theirs = L.feed(reference, e, top, pushes)
        final_runs, total, forced = reference.flush()
        stream = alignment.RecognizeStream(penalty=4., window=64, max_lag=max_lag)
        pieces = feed(stream, ppg, pushes)
        last = stream.flush()
        counts = [int(piece.count) for piece in pieces + [last]]
        assert counts == [len(runs) for runs in theirs + [final_runs]], (max_lag, pushes[0])
        got = gathered([single(piece) for piece in pieces + [last]])[0]
        assert equal_runs(got, host_runs(L.flat(theirs) + final_runs)), (max_lag, pushes[0])
        assert int(last.forced) == forced and np.float32(total).tobytes() == last.total.cpu().numpy().tobytes()
        forced_frames += forced
    assert forced_frames > 100                                                       # the forced step did run


def ragged():
    """3 streams of 150, 90 and 120 frames in 5 steps of at most 40 frames: the lengths per step (a stream sits out)."""
    return [[40, 0, 17], [1, 40, 33], [39, 25, 0], [40, 24, 40], [30, 1, 30]]


def push_ragged(stream, ppg, steps, begin=None):
    """Push (3, 40, T) raggedly with NaN padding: the list of Runs."""
    at, out = list(begin or [0, 0, 0]), []
    for lengths in steps:
        block = torch.full((3, 40, 40), math.nan, device='cuda')
        for b, size in enumerate(lengths):
            block[b, :, :size] = ppg[b, :, at[b]:at[b] + size]
            at[b] += size
        out.append(stream.push(block, lengths))
    return out


def test_ragged_batch_equals_single_streams_also_from_two_hip_streams_and_across_a_reset():
    generator = torch.Generator().manual_seed(44)
    ppg = torch.stack([R.random_ppg(150, scale, generator) for scale in (1., 3., 8.)]).cuda()
    steps = ragged()
    keywords = dict(penalty=1., window=128, max_lag=20)
    singles = []
    for b in range(3):
        one = alignment.RecognizeStream(**keywords)
        pieces = [one.push(ppg[b, :, sum(step[b] for step in steps[:k]):sum(step[b] for step in steps[:k + 1])])
                  for k in range(len(steps))]
        singles.append(gathered([single(piece) for piece in pieces + [one.flush()]])[0])
    batch = alignment.RecognizeStream(batch=3, **keywords)
    pieces = push_ragged(batch, ppg, steps)
    assert batch.position == [150, 90, 120]
    last = batch.flush()
    got = gathered(pieces + [last])
    for b in range(3):
        assert equal_runs(got[b], singles[b]), b
    totals, forced = bits(last.total).clone(), last.forced.clone()
    # two HIP streams at once, each with its own object
    side = [torch.cuda.Stream(), torch.cuda.Stream()]
    objects = [alignment.RecognizeStream(batch=3, **keywords) for _ in side]
    results = []
    torch.cuda.synchronize()
    for own, queue in zip(objects, side):
        with torch.cuda.stream(queue):
            results.append(push_ragged(own, ppg, steps) + [own.flush()])
    torch.cuda.synchronize()
    for result in results:
        other = gathered(result)
        assert all(equal_runs(other[b], singles[b]) for b in range(3))
        assert torch.equal(bits(result[-1].total), totals) and torch.equal(result[-1].forced, forced)
    # reset(item=1) in the middle: stream 1 starts again, the others go on
    batch = alignment.RecognizeStream(batch=3, **keywords)
    first = push_ragged(batch, ppg, steps[:2])
    batch.reset(item=1)
    assert batch.position == [41, 0, 50]
    rest = push_ragged(batch, ppg, steps[2:], begin=[41, 40, 50])
    last = batch.flush()
    got = gathered(first + rest + [last])
    assert equal_runs(got[0], singles[0]) and equal_runs(got[2], singles[2])
    alone = alignment.RecognizeStream(**keywords)
    alone_pieces = [alone.push(ppg[1, :, 40:65]), alone.push(ppg[1, :, 65:89]), alone.push(ppg[1, :, 89:90])]
    expected = gathered([single(piece) for piece in alone_pieces + [alone.flush()]])[0]
    after = gathered(rest + [last])[1]
    assert equal_runs(after, expected)
    # flush(item): the others keep their state
    batch = alignment.RecognizeStream(batch=3, **keywords)
    push_ragged(batch, ppg, steps[:2])
    only = batch.flush(item=2)
    assert only.count[:2].tolist() == [0, 0] and only.forced[:2].tolist() == [-1, -1]
    assert bool(torch.isnan(only.total[:2]).all()) and batch.position == [41, 40, 0]


def raw_outputs(streams, slots):
    return [torch.full((streams, slots), -7, dtype=torch.int32, device='cuda') for _ in range(3)] + \
           [torch.full((streams, slots), -7., dtype=torch.float32, device='cuda') for _ in range(2)] + \
           [torch.full((streams,), -7, dtype=torch.int32, device='cuda')]


def raw_push(state, window, ppg, lengths, transitions, workspace, max_lag=8, cap=None, slots=None, frames=None,
             streams=None, size=None, offset=0, state_offset=0, initial=None):
    """ppg_recognize_stream_push with outputs prefilled with -7: (rc, phonemes, begin, end, score, gop, count)."""
    frames = ppg.shape[2] if frames is None else frames
    streams = ppg.shape[0] if streams is None else streams
    cap = max_lag + ppg.shape[2] if cap is None else cap
    outputs = raw_outputs(ppg.shape[0], slots or max(cap, 1))
    lengths = torch.tensor(lengths, dtype=torch.int32).cuda()
    with torch.cuda.device(0):
        rc = E.library().ppg_recognize_stream_push(
            0, state.data_ptr() + state_offset, streams, window, ppg.data_ptr(), frames, lengths.data_ptr(),
            transitions.data_ptr(), None if initial is None else initial.data_ptr(), max_lag, cap,
            *[out.data_ptr() for out in outputs], workspace.data_ptr() + offset,
            workspace.numel() if size is None else size, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return (rc,) + tuple(outputs)


def raw_reset(state, streams, window):
    with torch.cuda.device(0):
        return E.library().ppg_recognize_stream_reset(0, state.data_ptr(), streams, window, None,
                                                      torch.cuda.current_stream().cuda_stream)


def raw_flush(state, streams, window, cap):
    outputs = raw_outputs(streams, cap)
    total = torch.full((streams,), -7., dtype=torch.float32, device='cuda')
    forced = torch.full((streams,), -7, dtype=torch.int32, device='cuda')
    with torch.cuda.device(0):
        rc = E.library().ppg_recognize_stream_flush(
            0, state.data_ptr(), streams, window, None, None, cap, *[out.data_ptr() for out in outputs],
            total.data_ptr(), forced.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return (rc,) + tuple(outputs) + (total, forced)


def layout(streams, window):
    """Byte offsets of the six blocks of a state: heads, D, ancestors, back-pointers, prepared frames, labels."""
    def up(value):
        return (value + 255) // 256 * 256
    heads, slots = 0, streams * window
    d = up(streams * 32)
    ancestors = d + up(streams * 256)
    back = ancestors + up(streams * 256)
    kept = back + up(slots * 64)
    labels = kept + up(slots * 176)
    assert labels + up(slots * 4) == E.library().ppg_recognize_stream_state_bytes(streams, window)
    return heads, d, ancestors, back, kept, labels


def heads_of(state, streams):
    return state[:streams * 32].view(torch.int32).reshape(streams, 8).cpu()


def test_poisoned_state_and_workspace_give_the_same_bits():
    lib = E.library()
    generator = torch.Generator().manual_seed(45)
    ppg = torch.stack([R.random_ppg(40, scale, generator) for scale in (1., 3., 8.)]).cuda().contiguous()
    transitions = alignment.switch_penalty(1.).cuda()
    runs = []
    for fill in (0, 255):
        state = torch.full((lib.ppg_recognize_stream_state_bytes(3, 64),), fill, dtype=torch.uint8, device='cuda')
        workspace = torch.full((lib.ppg_recognize_stream_workspace_bytes(3, 40),), fill, dtype=torch.uint8,
                               device='cuda')
        assert raw_reset(state, 3, 64) == 0
        first = raw_push(state, 64, ppg, [40, 9, 33], transitions, workspace)
        second = raw_push(state, 64, ppg, [13, 0, 20], transitions, workspace)      # (other frames of the same block)
        last = raw_flush(state, 3, 64, 9)
        assert first[0] == second[0] == last[0] == 0
        assert bool((first[6] >= 0).all()) and bool((second[6] >= 0).all()) and bool((last[6] >= 1).all())
        runs.append(first[1:] + second[1:] + last[1:] + (heads_of(state, 3),
                                                         state[layout(3, 64)[1]:layout(3, 64)[1] + 768].cpu(),
                                                         state[layout(3, 64)[2]:layout(3, 64)[2] + 768].cpu()))
    for a, b in zip(*runs):
        assert torch.equal(bits(a), bits(b))
    assert runs[0][-3][:, :5].tolist() == [[0, 0, 0, -1, 0]] * 3                      # the flush has reset the heads
    assert bool(torch.isneginf(runs[0][-2].view(torch.float32)).all())
    assert runs[0][-1].view(torch.int32).tolist() == list(range(64)) * 3


def test_overflow_counts_every_run_and_writes_cap_slots():
    lib = E.library()
    generator = torch.Generator().manual_seed(3)
    ppg = R.random_ppg(48, 1., generator)[None].cuda().contiguous()
    transitions = alignment.switch_penalty(0.).cuda()                                # the argmax: a run per frame or so
    results = []
    for cap in (56, 3, 1):
        state = torch.zeros(lib.ppg_recognize_stream_state_bytes(1, 64), dtype=torch.uint8, device='cuda')
        workspace = torch.zeros(lib.ppg_recognize_stream_workspace_bytes(1, 48), dtype=torch.uint8, device='cuda')
        assert raw_reset(state, 1, 64) == 0
        results.append(raw_push(state, 64, ppg, [48], transitions, workspace, cap=cap, slots=56) + (state,))
    whole, three, one = results
    count = int(whole[6])
    print(f'recognize stream overflow: {count} runs closed in 48 frames')
    assert whole[0] == 0 and 10 <= count <= 48
    for result, cap in ((three, 3), (one, 1)):
        assert result[0] == 0 and int(result[6]) == count > cap                      # as snprintf: what it would have taken
        for out, full in zip(result[1:6], whole[1:6]):
            assert torch.equal(bits(out[0, :cap]), bits(full[0, :cap]))
            assert bool((out[0, cap:] == -7).all())                                  # the slots behind stay untouched
        assert torch.equal(result[-1], whole[-1])                                    # the state does not depend on cap
    assert bool((whole[1][0, count:] == -1).all()) and bool(torch.isnan(whole[4][0, count:]).all())


def test_error_paths_launch_nothing_and_impossible_streams_give_minus_one():
    lib = E.library()
    generator = torch.Generator().manual_seed(46)
    ppg = torch.stack([R.random_ppg(40, scale, generator) for scale in (1., 3., 8.)]).cuda().contiguous()
    transitions = alignment.switch_penalty(1.).cuda()
    lengths = [40, 9, 33]
    need = lib.ppg_recognize_stream_workspace_bytes(3, 40)
    workspace = torch.zeros(need + 64, dtype=torch.uint8, device='cuda')
    state = torch.zeros(lib.ppg_recognize_stream_state_bytes(3, 64) + 64, dtype=torch.uint8, device='cuda')
    assert workspace.data_ptr() % 16 == 0 and state.data_ptr() % 16 == 0
    assert raw_reset(state, 3, 64) == 0
    assert raw_push(state, 64, ppg, [7, 7, 7], transitions, workspace)[0] == 0      # a state with a history
    workspace.zero_()
    before = state.clone()
    odd = transitions.reshape(-1).view(torch.uint8)[2:]                        # (a pointer off the 4-byte grid)
    refused = [
        raw_push(state, 64, ppg, lengths, transitions, workspace, size=need - 1),    # workspace too small
        raw_push(state, 64, ppg, lengths, transitions, workspace, offset=8),         # misaligned
        raw_push(state, 64, ppg, lengths, transitions, workspace, state_offset=8),
        raw_push(state, 64, ppg, lengths, transitions, workspace, frames=E.RECOGNIZE_MAX_FRAMES + 1, size=1 << 40),
        raw_push(state, 64, ppg, lengths, transitions, workspace, frames=0),
        raw_push(state, 64, ppg, lengths, transitions, workspace, streams=E.RECOGNIZE_STREAM_MAX_STREAMS + 1,
                 size=1 << 50),
        raw_push(state, 64, ppg, lengths, transitions, workspace, streams=0),
        raw_push(state, 32, ppg, lengths, transitions, workspace),                   # a bad window
        raw_push(state, 96, ppg, lengths, transitions, workspace),
        raw_push(state, 65536 + 64, ppg, lengths, transitions, workspace),
        raw_push(state, 64, ppg, lengths, transitions, workspace, cap=0, slots=1),
        raw_push(state, 64, ppg, lengths, transitions, workspace, cap=-1, slots=1),
        raw_push(state, 64, ppg, lengths, transitions, workspace, max_lag=-1, cap=40),
        raw_push(state, 64, ppg, lengths, transitions, workspace, max_lag=64, cap=40),
        raw_push(state, 64, ppg, lengths, odd, workspace),
    ]
    for result in refused:
        assert result[0] == -1 and lib.ppg_last_error()
        for out in result[1:]:
            assert bool((out == -7).all())
    assert not workspace.any() and torch.equal(state, before)                        # nothing was launched
    dummy = ctypes.c_void_p(state.data_ptr())
    assert lib.ppg_recognize_stream_flush(0, dummy, 3, 64, None, None, 9, None, dummy, dummy, dummy, None, dummy, dummy,
                                          dummy, None) == -1
    assert lib.ppg_recognize_stream_reset(0, ctypes.c_void_p(state.data_ptr() + 8), 3, 64, None, None) == -1
    torch.cuda.synchronize()
    assert torch.equal(state, before)

    # impossible streams: count = -1, every other output and the stream's state untouched, the others unharmed
    heads, d, ancestors, back, kept, labels = layout(3, 64)

    def stream_state(buffer, b):
        return torch.cat([buffer[b * 32:(b + 1) * 32], buffer[d + b * 256:d + (b + 1) * 256],
                          buffer[ancestors + b * 256:ancestors + (b + 1) * 256],
                          buffer[back + b * 4096:back + (b + 1) * 4096],
                          buffer[kept + b * 64 * 176:kept + (b + 1) * 64 * 176],
                          buffer[labels + b * 256:labels + (b + 1) * 256]])
    good_state = before.clone()
    good = raw_push(good_state, 64, ppg, lengths, transitions, workspace)
    assert good[0] == 0 and bool((good[6] >= 0).all())
    assert heads_of(good_state, 3)[:, 0].tolist() == [47, 16, 40]
    for bad_lengths, where in (([40, -1, 33], 1), ([40, 9, 41], 2), ([2 ** 31 - 1, 9, 33], 0)):
        own = before.clone()
        result = raw_push(own, 64, ppg, bad_lengths, transitions, workspace)
        assert result[0] == 0 and result[6].tolist()[where] == -1, bad_lengths
        for out, fine in zip(result[1:6], good[1:6]):
            assert bool((out[where] == -7).all()), bad_lengths
        for b in range(3):
            if b == where:
                assert torch.equal(stream_state(own, b), stream_state(before, b)), (bad_lengths, b)
            else:
                assert torch.equal(stream_state(own, b), stream_state(good_state, b)), (bad_lengths, b)
                assert all(torch.equal(bits(out[b]), bits(fine[b])) for out, fine in zip(result[1:], good[1:]))
    # an overfull window through the raw entry: 64 frames are in and none may go (no state is alive, so none is final)
    dead = torch.full((40,), -math.inf, device='cuda')
    full = torch.zeros_like(state)
    assert raw_reset(full, 3, 64) == 0
    block = torch.rand(3, 40, 64, device='cuda').softmax(1).contiguous()
    big = torch.zeros(lib.ppg_recognize_stream_workspace_bytes(3, 64), dtype=torch.uint8, device='cuda')
    result = raw_push(full, 64, block, [64, 63, 0], transitions, big, initial=dead)
    assert result[0] == 0 and result[6].tolist() == [0, 0, 0]
    assert heads_of(full, 3)[:, :2].tolist() == [[64, 0], [63, 0], [0, 0]]
    kept_full = full.clone()
    result = raw_push(full, 64, block, [1, 1, 64], transitions, big, initial=dead)
    assert result[0] == 0 and result[6].tolist() == [-1, 0, 0]
    assert torch.equal(stream_state(full, 0), stream_state(kept_full, 0))
    assert heads_of(full, 3)[:, :2].tolist() == [[64, 0], [64, 0], [64, 0]]
    result = raw_push(full, 64, block, [1, 1, 1], transitions, big, initial=dead)
    assert result[6].tolist() == [-1, -1, -1]
    last = raw_flush(full, 3, 64, 4)
    assert last[0] == 0 and last[6].tolist() == [0, 0, 0] and bool(torch.isneginf(last[7]).all())
    assert last[8].tolist() == [0, 0, 0]
    # position 2^31 - 9: 8 frames are 8 frames left, 9 are one too many.  D = 0 for the 40 states: a stream in mid-flight
    late = torch.zeros_like(state)
    assert raw_reset(late, 3, 64) == 0
    words = late[:32].view(torch.int32)
    words[0] = words[1] = 2 ** 31 - 9
    late[d:d + 160].view(torch.float32).zero_()
    for frames, fine in ((9, False), (8, True)):
        own = late.clone()
        result = raw_push(own, 64, ppg, [frames, 0, 0], transitions, workspace)
        assert result[0] == 0
        if not fine:
            assert result[6].tolist() == [-1, 0, 0] and torch.equal(stream_state(own, 0), stream_state(late, 0))
            continue
        count = int(result[6][0])
        assert count >= 0 and heads_of(own, 3)[0, 0] == 2 ** 31 - 1
        last = raw_flush(own, 3, 64, 16)
        total = count + int(last[6][0])
        ends = torch.cat([result[3][0, :count], last[3][0, :int(last[6][0])]])
        begins = torch.cat([result[2][0, :count], last[2][0, :int(last[6][0])]])
        assert total >= 1 and int(begins[0]) == 2 ** 31 - 9 and int(ends[-1]) == 2 ** 31 - 1
        assert torch.equal(begins[1:], ends[:-1]) and bool((ends > begins).all())
        assert bool(torch.isfinite(last[7][0])) and bool(torch.isfinite(last[4][0, :int(last[6][0])]).all())


def test_no_path_gives_no_runs_and_a_total_of_minus_infinity():
    ppg = recordings()
    dead = torch.full((40,), -math.inf)
    stream = alignment.RecognizeStream(penalty=1., initial=dead, batch=3)
    pieces = feed(stream, ppg, PATTERNS['uneven'])
    last = stream.flush()
    assert all(piece.count.tolist() == [0, 0, 0] for piece in pieces) and last.count.tolist() == [0, 0, 0]
    assert bool(torch.isneginf(last.total).all()) and last.forced.tolist() == [0, 0, 0]
    assert all(len(item['phonemes']) == 0 for item in gathered(pieces + [last]))
    assert alignment.run_segments(last) == [[], [], []]


def test_audio_stream_into_recognize_stream():
    generator = torch.Generator().manual_seed(9)
    engine = E.Engine(W.seeded_state_dict(seed=1234), 0, 'fp32', True)
    audio = 0.1 * torch.randn(32000 + 77, generator=generator)
    source, said = engine.audio_stream(500), alignment.RecognizeStream(penalty=0.5, window=1024)
    pieces, runs, received = [], [], 0
    sizes = [1000, 100, 2561, 0, 77, 4111, 159, 8000, 50, 3000]
    index = 0
    while received < audio.shape[0]:
        n = min(sizes[index % len(sizes)], audio.shape[0] - received)
        index += 1
        piece = source.push(audio[received:received + n].cuda(), flush=received + n == audio.shape[0])
        received += n
        pieces.append(piece.clone())
        runs.append(said.push(piece))                                      # the pieces of no frames too
        assert runs[-1].phonemes.shape == (512 + piece.shape[1] if piece.shape[1] else 0,)
    ppg = torch.cat(pieces, dim=1)
    assert ppg.shape[1] == 200 and any(piece.shape[1] == 0 for piece in pieces) and said.position == [200]
    whole = alignment.recognize(ppg, penalty=0.5)
    last = said.flush()
    assert int(last.forced) == 0 and same_bits(last.total, whole.total)
    assert equal_runs(gathered([single(piece) for piece in runs + [last]])[0], expected_of(whole))
    listed = [segment for piece in runs + [last] for segment in alignment.run_segments(piece)]
    assert [segment[:3] for segment in listed] == [segment[:3] for segment in alignment.segments(whole)]
