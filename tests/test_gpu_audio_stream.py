"""Streaming from raw audio on the GPU: the incremental mel frontend (engine.FrontendStream,
ppg_frontend_stream_*) and the audio-in streams built on it (Engine.audio_stream / batched_audio_stream /
long_audio_stream).

* the streamed mel frames are the batch frontend's, bit for bit, whatever the pieces;
* against the reference they meet the frontend criterion of test_gpu_parity.py (<= 1 fp16 ulp, >= 99.5 % equal);
* the audio-in streams equal the feature-in streams fed the batch frontend's mel in the same frame pieces, bit for
  bit, and the oracle's causal forward within test_gpu_parity.py's TOL.
"""
import numpy as np
import pytest
import torch

from oracle import ppg_oracle as O
from ppgs_amd import engine as E
from ppgs_amd import weights as W

pytestmark = pytest.mark.gpu

TOL = {'fp32': 1e-4, 'bf16': 4e-3, 'fp16': 1e-3}         # test_gpu_parity.py's file-wide tolerances
PIECES = [1, 159, 160, 161, 592, 0, 2560, 10007, 433, 77, 1600, 3]


def ulp_diff(a, b):
    return np.abs(a.view(np.int16).astype(np.int32) - b.view(np.int16).astype(np.int32))


def recording(samples, seed, batch=1):
    generator = torch.Generator().manual_seed(seed)
    return 0.1 * torch.randn(batch, samples, generator=generator)


_engines = {}


def eng(precision='fp32', causal=True, cin=80):
    key = (precision, causal, cin)
    if key not in _engines:
        state = W.seeded_state_dict(seed=1234, input_channels=cin)
        _engines[key] = (E.Engine(state, 0, precision, causal), state)
    return _engines[key]


def stream_one(audio, pieces, flush_with_samples, stream=None):
    """audio (samples,) on the GPU pushed in `pieces` (cycled) -> (mel (80, T), [(received, frames per push)])"""
    total = audio.shape[0]
    stream = stream or E.FrontendStream(1, max(pieces), 0)
    out, received, emitted, index = [], 0, 0, 0
    while True:
        n = min(pieces[index % len(pieces)], total - received)
        index += 1
        last = received + n == total
        flush = last and flush_with_samples
        mel, frames = stream.push(audio[None, received:received + n], flush=flush)
        received += n
        assert frames == [E.audio_stream_frames(received, flush) - emitted], (received, frames)
        assert mel.shape == (1, 80, frames[0])
        assert stream.received == [received]
        emitted += frames[0]
        assert stream.emitted == [emitted]
        out.append(mel[0])
        if last:
            break
    if not flush_with_samples:
        mel, frames = stream.push(None, flush=True)
        assert frames == [total // 160 - emitted]
        out.append(mel[0, :, :frames[0]])
    return torch.cat(out, dim=1)


@pytest.mark.parametrize('samples', [160 * 37 + 59, 160 * 149, 4000, 80003])
@pytest.mark.parametrize('flush_with_samples', [True, False])
def test_streamed_mel_equals_batch_frontend_bit_for_bit(samples, flush_with_samples):
    audio = recording(samples, seed=5 + samples % 7).cuda()
    _, whole = E.frontend(audio)
    pieces = PIECES if flush_with_samples else PIECES[::-1]
    mel = stream_one(audio[0], pieces, flush_with_samples)
    torch.cuda.synchronize()
    assert mel.shape == whole[0].shape == (80, samples // 160)
    assert np.array_equal(mel.cpu().numpy().view(np.int16), whole[0].cpu().numpy().view(np.int16))


def ragged_schedule(totals, n_max, seed):
    """Per push: (counts, flushes) -- items receive different counts, some sit out, each is flushed in the push
    that brings its last samples (every third item: in a later push that brings none)."""
    rng = np.random.default_rng(seed)
    batch = len(totals)
    received, done, steps = [0] * batch, [False] * batch, []
    while not all(done):
        counts, flushes = [0] * batch, [False] * batch
        for b in range(batch):
            if done[b]:
                continue
            if received[b] == totals[b]:                       # (the late flush)
                flushes[b], done[b] = True, True
                continue
            if rng.random() < 0.2:
                continue                                       # sits this push out
            counts[b] = int(min(rng.choice([1, 159, 160, 161, 592, 1000, n_max]), totals[b] - received[b]))
            received[b] += counts[b]
            if received[b] == totals[b] and b % 3:
                flushes[b], done[b] = True, True
        steps.append((counts, flushes))
    return steps


def test_streamed_mel_batch_of_64_ragged_equals_batch_frontend():
    batch, n_max = 64, 2560
    rng = np.random.default_rng(3)
    totals = [int(v) for v in rng.integers(2000, 24000, size=batch)]
    totals[0], totals[1], totals[2] = 433, 160 * 37 + 59, 160 * 64
    audio = recording(max(totals), seed=9, batch=batch).cuda()
    stream = E.FrontendStream(batch, n_max, 0)
    received, emitted = [0] * batch, [0] * batch
    got = [[] for _ in range(batch)]
    for counts, flushes in ragged_schedule(totals, n_max, seed=4):
        chunk = torch.zeros(batch, n_max, device='cuda')
        for b in range(batch):
            chunk[b, :counts[b]] = audio[b, received[b]:received[b] + counts[b]]
        mel, frames = stream.push(chunk, counts, flushes)
        for b in range(batch):
            received[b] += counts[b]
            expect = E.audio_stream_frames(received[b], flushes[b]) - emitted[b] if counts[b] or flushes[b] else 0
            assert frames[b] == expect, (b, received[b], frames[b])
            emitted[b] += frames[b]
            got[b].append(mel[b, :, :frames[b]])
            assert not mel[b, :, frames[b]:].any()
        assert mel.shape == (batch, 80, max(frames))
    torch.cuda.synchronize()
    for b in range(batch):
        _, whole = E.frontend(audio[b:b + 1, :totals[b]])
        mine = torch.cat(got[b], dim=1)
        assert mine.shape == whole[0].shape
        assert np.array_equal(mine.cpu().numpy().view(np.int16), whole[0].cpu().numpy().view(np.int16)), b


def test_streamed_mel_against_the_reference(golden):
    g = golden('g1_frontend')
    audio = torch.from_numpy(np.asarray(g['audio'])).float()
    audio = audio[:, 0] if audio.dim() == 3 else audio
    for b in range(audio.shape[0]):
        mel = stream_one(audio[b].cuda(), [700, 161, 2560, 33], True).cpu().numpy()
        d = ulp_diff(mel, g['mel16'][b])
        print('g1_frontend item', b, 'max ulp', d.max(), 'equal', (d == 0).mean())
        assert d.max() <= 1 and (d == 0).mean() >= 0.995
    for samples in (160 * 37 + 59, 160 * 149, 4000, 80003):
        audio = recording(samples, seed=5 + samples % 7)
        ref = O.mel_from_audios(audio[:, None]).numpy()[0]
        mel = stream_one(audio[0].cuda(), PIECES, True).cpu().numpy()
        d = ulp_diff(mel, ref)
        print(samples, 'samples: max ulp', d.max(), 'equal', (d == 0).mean())
        assert d.max() <= 1 and (d == 0).mean() >= 0.995


def frame_pieces(sample_pieces, total):
    """the frame counts audio pushes of `sample_pieces` (cycled, the last one flushing) turn into"""
    received, emitted, index, out = 0, 0, 0, []
    while received < total:
        n = min(sample_pieces[index % len(sample_pieces)], total - received)
        index += 1
        received += n
        frames = E.audio_stream_frames(received, received == total)
        out.append((n, frames - emitted))
        emitted = frames
    return out


@pytest.mark.parametrize('precision', ['fp32', 'fp16', 'bf16'])
def test_audio_stream_end_to_end(precision):
    engine, state = eng(precision)
    frames_total = 437
    total = 160 * frames_total + 101
    audio = recording(total, seed=21)
    mel_ref = O.mel_from_audios(audio[:, None])
    ref = O.from_features(state, mel_ref, torch.tensor([frames_total]), is_causal=True).numpy()[0]
    _, mel = E.frontend(audio.cuda())
    plan = frame_pieces([1000, 2561, 77, 4111, 159, 8000], total)
    audio_in, feature_in = engine.audio_stream(500), engine.stream(500)
    a_out, f_out, received, frame = [], [], 0, 0
    for index, (n, k) in enumerate(plan):
        flush = index == len(plan) - 1
        a_out.append(audio_in.push(audio[0, received:received + n].cuda(), flush=flush))
        if k or flush:
            f_out.append(feature_in.push(mel[0, :, frame:frame + k], flush=flush))
        received, frame = received + n, frame + k
        assert sum(p.shape[1] for p in a_out) == sum(p.shape[1] for p in f_out)
    a_out, f_out = torch.cat(a_out, dim=1), torch.cat(f_out, dim=1)
    torch.cuda.synchronize()
    assert a_out.shape == (40, frames_total)
    assert torch.equal(a_out, f_out)
    error = np.abs(a_out.cpu().numpy() - ref).max()
    print(precision, 'audio_stream max-abs error', error)
    assert error < TOL[precision]


@pytest.mark.parametrize('precision', ['fp32', 'fp16', 'bf16'])
def test_batched_audio_stream_end_to_end(precision):
    engine, state = eng(precision)
    batch, n_max = 8, 4000
    totals = [160 * 437 + 101, 160 * 300, 160 * 499 + 159, 4000, 160 * 37 + 59, 160 * 200 + 1, 433 + 160 * 3, 160 * 64]
    audio = recording(max(totals), seed=22, batch=batch)
    audio_in, feature_in = engine.batched_audio_stream(batch, 500, n_max), engine.batched_stream(batch, 500)
    mels = [E.frontend(audio[b:b + 1, :totals[b]].cuda())[1][0] for b in range(batch)]
    received, emitted = [0] * batch, [0] * batch
    a_out, f_out = [[] for _ in range(batch)], [[] for _ in range(batch)]
    for counts, flushes in ragged_schedule(totals, n_max, seed=8):
        chunk = torch.zeros(batch, n_max)
        for b in range(batch):
            chunk[b, :counts[b]] = audio[b, received[b]:received[b] + counts[b]]
            received[b] += counts[b]
        frames = [E.audio_stream_frames(received[b], flushes[b]) - emitted[b] if counts[b] or flushes[b] else 0 for b in range(batch)]
        feats = torch.zeros(batch, 80, max(frames), dtype=torch.float16, device='cuda')
        for b in range(batch):
            feats[b, :, :frames[b]] = mels[b][:, emitted[b]:emitted[b] + frames[b]]
            emitted[b] += frames[b]
        for b, (x, y) in enumerate(zip(audio_in.push(chunk.cuda(), counts, flushes), feature_in.push(feats, frames, flushes))):
            a_out[b].append(x)
            f_out[b].append(y)
    torch.cuda.synchronize()
    for b in range(batch):
        T = totals[b] // 160
        x, y = torch.cat(a_out[b], dim=1), torch.cat(f_out[b], dim=1)
        assert x.shape == (40, T) and torch.equal(x, y), b
        mel_ref = O.mel_from_audios(audio[b:b + 1, None, :totals[b]])
        ref = O.from_features(state, mel_ref, torch.tensor([T]), is_causal=True).numpy()[0]
        error = np.abs(x.cpu().numpy() - ref).max()
        print(precision, 'batched_audio_stream item', b, 'max-abs error', error)
        assert error < TOL[precision], b


def test_long_audio_stream_equals_chunked_causal_forward():
    engine, state = eng('fp32')
    frames_total = 1130
    total = 160 * frames_total + 7
    audio = recording(total, seed=23)
    mel_ref = O.mel_from_audios(audio[:, None])
    ref = O.from_features(state, mel_ref, torch.tensor([frames_total]), is_causal=True).numpy()[0]
    _, mel = E.frontend(audio.cuda())
    plan = frame_pieces([2561, 7000, 161, 15999, 333], total)
    audio_in, feature_in = engine.long_audio_stream(), engine.long_stream()
    a_out, f_out, received, frame = [], [], 0, 0
    for index, (n, k) in enumerate(plan):
        flush = index == len(plan) - 1
        a_out.append(audio_in.push(audio[0, received:received + n].cuda(), flush=flush))
        f_out.append(feature_in.push(mel[0, :, frame:frame + k], flush=flush))
        received, frame = received + n, frame + k
    a_out, f_out = torch.cat(a_out, dim=1), torch.cat(f_out, dim=1)
    torch.cuda.synchronize()
    assert a_out.shape == (40, frames_total)
    assert torch.equal(a_out, f_out)
    error = np.abs(a_out.cpu().numpy() - ref).max()
    print('long_audio_stream max-abs error', error)
    assert error < TOL['fp32']


def test_edges():
    audio = recording(6000, seed=31).cuda()
    stream = E.FrontendStream(2, 4000, 0)
    with pytest.raises(ValueError):                                  # a recording must end with > 432 samples
        stream.push(audio[:1].expand(2, -1)[:, :432], flush=True)
    assert stream.received == [0, 0]                                 # a refused push changes nothing
    with pytest.raises(ValueError):
        stream.push(audio[:1].expand(2, -1)[:, :4001])               # more than max_push_samples
    with pytest.raises(ValueError):
        stream.push(audio[:1].expand(2, -1)[:, :100], counts=[100, 101])
    first = [stream.push(audio[:1].expand(2, -1)[:, :4000].contiguous(), counts=[4000, 3000])]
    first.append(stream.push(audio[:1].expand(2, -1)[:, 4000:].contiguous(), counts=[2000, 0], flush=[True, False]))
    assert first[1][1][1] == 0
    with pytest.raises(ValueError):                                  # item 0 was flushed
        stream.push(audio[:1].expand(2, -1)[:, :10], counts=[10, 0])
    stream.push(audio[:1].expand(2, -1)[:, :10], counts=[0, 10])     # item 1 goes on
    # reset, then a second utterance on the same object equals a fresh object
    stream.reset(0)
    assert stream.received[0] == 0 and stream.emitted[0] == 0 and stream.received[1] == 3010
    again = [stream.push(audio[:1].expand(2, -1)[:, :4000].contiguous(), counts=[4000, 0])]
    again.append(stream.push(audio[:1].expand(2, -1)[:, 4000:].contiguous(), counts=[2000, 0], flush=[True, False]))
    _, whole = E.frontend(audio)
    for pushes in (first, again):
        mel = torch.cat([m[0, :, :k[0]] for m, k in pushes], dim=1)
        assert torch.equal(mel, whole[0])
    stream.reset()
    assert stream.received == [0, 0]
    # the audio-in streams exist for causal engines with 80 input channels only
    for engine in (eng('bf16', causal=False)[0], eng('bf16', causal=True, cin=768)[0]):
        for make in (lambda e: e.audio_stream(100), lambda e: e.batched_audio_stream(2, 100), lambda e: e.long_audio_stream()):
            with pytest.raises(ValueError):
                make(engine)


def test_incremental_frontend_beside_the_encoder_on_another_stream():
    """One incremental-frontend step loop on one HIP stream while Engine.encode runs on another (the pattern of
    test_frontend_and_steps_beside_the_encoder_on_other_streams, where the packed-fp32 / MFMA hazard of DESIGN 4.4
    was found): still the batch frontend's bits.  One pass."""
    engine, _ = eng('bf16', causal=False)
    batch, step, steps = 64, 2560, 300
    generator = torch.Generator().manual_seed(1234)
    feats = torch.randn(32, 80, 1000, generator=generator).half().cuda()
    audio = recording(step * 25, seed=41, batch=batch).cuda()             # 25 steps per utterance, then reset and again
    _, whole = E.frontend(audio)
    stream = E.FrontendStream(batch, step, 0)
    a, b = torch.cuda.Stream(), torch.cuda.Stream()
    torch.cuda.synchronize()
    outs = []
    for index in range(steps):
        k = index % 25
        if index % 5 == 0:
            with torch.cuda.stream(a):
                for _ in range(2):
                    engine.encode(feats, [1000] * 32)
        with torch.cuda.stream(b):
            if k == 0:
                stream.reset()
            outs.append(stream.push(audio[:, k * step:(k + 1) * step], flush=k == 24)[0])
    torch.cuda.synchronize()
    for first in range(0, steps, 25):
        mel = torch.cat(outs[first:first + 25], dim=2)
        assert torch.equal(mel, whole), first
