"""ppgs_amd.alignment.recognize on the GPU: equal to `forced` under a chain and to `decode` without a model, exact
ties, what smoothing is for, the float64 Viterbi of tests/recognize_reference.py, utterances without a path, batches,
streams, poisoned workspaces and the error paths.

The bound on a total is derived as test_gpu_alignment.py derives its own: a clamped input is exact and logf is within
1 ulp, so every emission is within 2^-23 relative; the weights are fp32 numbers given to the reference as they are; a
path's weight is a sequential fp32 sum of 2T + 1 terms of one sign (T emissions, T - 1 transitions, initial and
final), each addition within 2^-24 relative; and the maximum over paths of values each within the bound is within the
bound: (2T + 2) * 2^-23 * |total|.  Paths are compared by cost and validity, never by identity, except where the
input's own margin is orders of magnitude above that bound or every number is exact."""
import math

import numpy as np
import pytest
import torch

from ppgs_amd import alignment, engine as E

import alignment_reference as F
import recognize_reference as R

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -23
INF = math.inf
# 1 and 2; the 32-frame staging chunk, the 64-frame trace-back refill and ballot of labels, and 128, with their edges;
# 4096, the limit of the neighbouring entries, its edges and one length well past it
FRAMES = [1, 2, 31, 32, 33, 63, 64, 65, 127, 128, 129, 4095, 4096, 4097, 5003]


def segmented(frames, generator, shortest=5, longest=9, peak=12.):
    """A PPG of clear segments: (ppg (40, T), labels (T,)); consecutive segments differ."""
    labels = torch.empty(frames, dtype=torch.int64)
    at, before = 0, -1
    while at < frames:
        length = int(torch.randint(shortest, longest + 1, (1,), generator=generator))
        if frames - at - length < shortest:
            length = frames - at
        phoneme = int(torch.randint(0, 40, (1,), generator=generator))
        phoneme = (phoneme + 1) % 40 if phoneme == before else phoneme
        labels[at:at + length] = phoneme
        at, before = at + length, phoneme
    logits = torch.zeros(40, frames)
    logits[labels, torch.arange(frames)] = peak
    return logits, labels


def margin(ppg):
    """The smallest lead of a frame's best log-posterior over its second best."""
    best = torch.from_numpy(F.log_posteriors(ppg)).topk(2, dim=1).values
    return float((best[:, 0] - best[:, 1]).min())


@pytest.mark.parametrize('frames', [T for T in FRAMES if T <= alignment.MAX_FRAMES])
def test_equals_forced_bit_for_bit_under_a_chain(frames):
    generator = torch.Generator().manual_seed(100 + frames)
    for count in (1, 2, 7, 40):
        if count > frames:
            continue
        for scale in (1., 3., 8.):
            ppg = F.random_ppg(frames, scale, generator).cuda()
            sequence = torch.randperm(40, generator=generator)[:count].tolist()
            A, initial, final = alignment.chain(sequence)
            got = alignment.recognize(ppg, transitions=A, initial=initial, final=final)
            ref = alignment.forced(ppg, sequence)
            label = f'T={frames} N={count} scale={scale}'
            assert got.phonemes.tolist() == sequence, label
            assert got.phonemes.dtype == got.starts.dtype == torch.int32 and got.starts.is_cuda
            assert torch.equal(got.starts, ref.starts), label
            for name in ('total', 'score', 'gop'):
                ours, theirs = getattr(got, name), getattr(ref, name)
                assert ours.dtype == torch.float32 and ours.shape == theirs.shape, (label, name)
                assert torch.equal(ours.view(torch.int32), theirs.view(torch.int32)), (label, name)


@pytest.mark.parametrize('frames', FRAMES)
def test_equals_decode_without_a_model(frames):
    generator = torch.Generator().manual_seed(200 + frames)
    logits, labels = segmented(frames, generator, shortest=1, longest=6)
    ppg = torch.softmax(logits + torch.randn(40, frames, generator=generator), dim=0)
    assert margin(ppg) >= 1.0                                   # a condition on the input
    assert torch.equal(ppg.argmax(0), labels)
    phonemes, starts = R.runs(labels.numpy())
    got = alignment.recognize(ppg.cuda(), transitions=torch.zeros(40, 40))
    assert got.phonemes.tolist() == phonemes.tolist() and got.starts.tolist() == starts.tolist()
    assert bool((got.gop == 0).all()) and bool((got.score < 0).all())
    if frames <= alignment.MAX_FRAMES:
        free = alignment.decode(ppg.cuda())
        assert torch.equal(got.phonemes, free.phonemes) and torch.equal(got.starts, free.starts)
    assert torch.equal(alignment.frame_labels(got.starts, got.phonemes, frames).cpu().long(), labels)
    listed = alignment.segments(got)
    assert len(listed) == len(phonemes) and listed[-1][2] == frames * 160 / 16000
    without = alignment.recognize(ppg.cuda(), penalty=0, gop=False)
    assert without.gop is None and torch.equal(without.score, got.score) and torch.equal(without.total, got.total)


@pytest.mark.parametrize('frames', FRAMES)
def test_exact_ties(frames):
    ppg = torch.full((40, frames), 1 / 40).cuda()
    got = alignment.recognize(ppg, transitions=torch.zeros(40, 40))
    assert got.phonemes.tolist() == [0] and got.starts.tolist() == [0, frames]
    assert bool((got.gop == 0).all())
    # staying costs 1 and switching nothing: the path alternates between the two lowest phonemes, ending in 0
    swap = -torch.eye(40)
    got = alignment.recognize(ppg, transitions=swap)
    labels = alignment.frame_labels(got.starts, got.phonemes, frames).tolist()
    assert labels == [(frames - 1 - t) % 2 for t in range(frames)]
    assert got.starts.tolist() == list(range(frames + 1))
    # the float64 reference has the same rule
    logp = F.log_posteriors(ppg.cpu())
    assert R.viterbi(logp, swap.numpy(), np.zeros(40), np.zeros(40))[1].tolist() == labels


@pytest.mark.parametrize('frames', [33, 129, 4096, 5003])
def test_smoothing_removes_isolated_flips_and_nothing_else(frames):
    generator = torch.Generator().manual_seed(400 + frames)
    gain = 4.                                                   # the log-odds by which a flipped frame prefers its flip
    logits, labels = segmented(frames, generator)
    flipped = labels.clone()
    phonemes, starts = R.runs(labels.numpy())
    for n in range(len(phonemes)):                              # flips strictly inside a segment, never adjacent
        for t in range(int(starts[n]) + 1, int(starts[n + 1]) - 1, 3):
            other = (int(phonemes[n]) + 1 + int(torch.randint(0, 39, (1,), generator=generator))) % 40
            logits[other, t] = logits[labels[t], t]
            logits[labels[t], t] -= gain
            flipped[t] = other
    assert int((flipped != labels).sum()) >= frames // 10
    ppg = torch.softmax(logits, dim=0)
    assert torch.equal(ppg.argmax(0), flipped) and margin(ppg) >= gain - 0.01
    noisy_phonemes, noisy_starts = R.runs(flipped.numpy())
    device = ppg.cuda()
    if frames <= alignment.MAX_FRAMES:
        free = alignment.decode(device)
        assert free.phonemes.tolist() == noisy_phonemes.tolist() and free.starts.tolist() == noisy_starts.tolist()
    # a flip gains `gain` and costs two switches: a penalty a factor of two above gain / 2 removes it ...
    clean = alignment.recognize(device, penalty=gain)
    assert clean.phonemes.tolist() == phonemes.tolist() and clean.starts.tolist() == starts.tolist()
    assert bool((clean.gop <= 0).all()) and bool((clean.gop < 0).any())
    # ... and one a factor of two below it keeps it
    noisy = alignment.recognize(device, penalty=gain / 4)
    assert noisy.phonemes.tolist() == noisy_phonemes.tolist() and noisy.starts.tolist() == noisy_starts.tolist()
    assert bool((noisy.gop == 0).all())


def random_model(generator, holes=0.3):
    """(A, initial, final) fp32, every entry in [-5, 0] or -inf."""
    tables = []
    for shape in ((40, 40), (40,), (40,)):
        table = -5 * torch.rand(shape, generator=generator)
        table[torch.rand(shape, generator=generator) < holes] = -INF
        tables.append(table)
    return tables


def check_against_reference(ppg, A, initial, final, label):
    """One utterance on the device against the float64 Viterbi; returns the relative error of the total."""
    frames = ppg.shape[1]
    logp = F.log_posteriors(ppg)
    model = (A.double().numpy(), initial.double().numpy(), final.double().numpy())
    ref_total, ref_labels = R.viterbi(logp, *model)
    assert ref_labels is not None and math.isfinite(ref_total), label              # a condition on the input
    got = alignment.recognize(ppg.cuda(), transitions=A, initial=initial, final=final)
    phonemes, starts, total = got.phonemes.cpu().numpy(), got.starts.cpu().numpy(), float(got.total)
    count = len(phonemes)
    assert count >= 1 and ((phonemes >= 0) & (phonemes < 40)).all() and (phonemes[1:] != phonemes[:-1]).all(), label
    F.check_starts(starts, frames, count)
    bound = (2 * frames + 2) * EPS * abs(ref_total)
    error = abs(total - ref_total)
    print(f'recognize {label}: total {total:.6f} reference {ref_total:.6f} relative error '
          f'{error / abs(ref_total):.3e} (bound {(2 * frames + 2) * EPS:.3e}), {count} runs')
    assert error <= bound, label
    own = R.rescore(R.expand(phonemes, starts), logp, *model)
    print(f'recognize {label}: the device\'s path weighs {own:.6f} in float64, the optimum {ref_total:.6f}')
    assert own > -INF and own >= ref_total - 2 * bound, label
    lengths = np.diff(starts)
    own_frames = logp[np.arange(frames), R.expand(phonemes, starts)]
    ref_score = np.add.reduceat(own_frames, starts[:-1]) / lengths
    ref_gop = np.add.reduceat(own_frames - logp.max(axis=1), starts[:-1]) / lengths
    score, gop = got.score.cpu().numpy().astype(np.float64), got.gop.cpu().numpy().astype(np.float64)
    assert score.shape == gop.shape == (count,)
    worst_score = (np.abs(score - ref_score) - (4e-6 + (lengths + 2) * EPS * np.abs(ref_score))).max()
    worst_gop = (np.abs(gop - ref_gop) - (4e-6 + (lengths + 2) * EPS * np.abs(ref_gop))).max()
    print(f'recognize {label}: score error {np.abs(score - ref_score).max():.3e}, gop error '
          f'{np.abs(gop - ref_gop).max():.3e}; closest to their bounds {worst_score:.3e} {worst_gop:.3e} (<= 0 passes)')
    assert worst_score <= 0 and worst_gop <= 0, label
    assert (gop <= 0).all(), label
    return error / abs(ref_total)


@pytest.mark.parametrize('frames', FRAMES)
def test_optimum_scores_and_gop_against_float64_viterbi(frames):
    generator = torch.Generator().manual_seed(500 + frames)
    worst = 0.
    for scale in (1., 3., 8.):
        ppg = F.random_ppg(frames, scale, generator)
        A, initial, final = random_model(generator)
        worst = max(worst, check_against_reference(ppg, A, initial, final, f'T={frames} scale={scale}'))
    print(f'recognize T={frames}: largest relative error of total {worst:.3e}')


def test_a_recording_at_the_frame_limit():
    frames = alignment.RECOGNIZE_MAX_FRAMES
    generator = torch.Generator().manual_seed(6)
    logits, labels = segmented(frames, generator, shortest=3, longest=40)
    ppg = torch.softmax(logits, dim=0)
    phonemes, starts = R.runs(labels.numpy())
    got = alignment.recognize(ppg.cuda(), penalty=2.)
    assert torch.equal(got.phonemes.cpu().long(), torch.from_numpy(phonemes))
    assert torch.equal(got.starts.cpu().long(), torch.from_numpy(starts))
    assert math.isfinite(float(got.total)) and bool((got.gop == 0).all())


def raw_recognize(ppg, lengths, model, workspace, want_gop=True, frames=None, items=None, size=None, offset=0,
                  missing=()):
    """ppg_recognize through ctypes with the caller's workspace; outputs start as sentinels.  `missing` names the
    pointers to pass as NULL.  (rc, {name: tensor})."""
    lib = E.library()
    count, width = ppg.shape[0], ppg.shape[2]
    out = {'phonemes': torch.full((count, width), -7, dtype=torch.int32, device='cuda'),
           'starts': torch.full((count, width + 1), -7, dtype=torch.int32, device='cuda'),
           'runs': torch.full((count,), -7, dtype=torch.int32, device='cuda'),
           'total': torch.full((count,), -7., device='cuda'),
           'score': torch.full((count, width), -7., device='cuda'),
           'gop': torch.full((count, width), -7., device='cuda')}
    given = {'ppg': ppg, 'lengths': torch.tensor(lengths, dtype=torch.int32).cuda(),
             'transitions': model[0].float().cuda().contiguous(),
             'initial': None if model[1] is None else model[1].float().cuda(),
             'final': None if model[2] is None else model[2].float().cuda(), **out}
    if not want_gop:
        given['gop'] = None

    def pointer(name):
        return None if name in missing or given[name] is None else given[name].data_ptr()
    torch.cuda.synchronize()
    rc = lib.ppg_recognize(
        0, pointer('ppg'), width if frames is None else frames, count if items is None else items,
        pointer('lengths'), pointer('transitions'), pointer('initial'), pointer('final'), pointer('phonemes'),
        pointer('starts'), pointer('runs'), pointer('total'), pointer('score'), pointer('gop'),
        None if 'workspace' in missing else workspace.data_ptr() + offset,
        workspace.numel() - offset if size is None else size, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return rc, out


def untouched(out, names=('phonemes', 'starts', 'score', 'gop')):
    return all(bool((out[name] == -7).all()) for name in names)


@pytest.mark.parametrize('frames', [1, 2, 33, 65])
def test_an_utterance_without_a_path(frames):
    generator = torch.Generator().manual_seed(600 + frames)
    ppg = F.random_ppg(frames, 3., generator)[None].cuda().contiguous()
    A, initial, final = random_model(generator, holes=0.)
    workspace = torch.full((E.library().ppg_recognize_workspace_bytes(1, frames),), 255, dtype=torch.uint8,
                           device='cuda')
    models = [(A, initial, torch.full((40,), -INF))]             # no state may end
    if frames > 1:                                              # the only first state has no way on, and may not end
        dead, only, ends = A.clone(), torch.full((40,), -INF), final.clone()
        dead[13, :], only[13], ends[13] = -INF, 0., -INF
        models.append((dead, only, ends))
    for model in models:
        rc, out = raw_recognize(ppg, [frames], model, workspace)
        assert rc == 0 and out['total'].tolist() == [-INF] and out['runs'].tolist() == [0]
        assert untouched(out)
        got = alignment.recognize(ppg[0], transitions=model[0], initial=model[1], final=model[2])
        assert got.phonemes.shape == (0,) and got.score.shape == got.gop.shape == (0,) and got.starts.tolist() == [0]
        assert float(got.total) == -INF and alignment.segments(got) == []
    if frames == 1:
        return
    # beside it in a batch, an utterance with a path is unharmed: state 13 may begin and end but has no way on, so one
    # frame has a path and more frames have none
    ends = torch.full((40,), -INF)
    ends[13] = 0.
    pair = torch.cat([ppg, ppg])
    wide = torch.full((E.library().ppg_recognize_workspace_bytes(2, frames),), 255, dtype=torch.uint8, device='cuda')
    rc, out = raw_recognize(pair, [frames, 1], (dead, only, ends), wide)
    assert rc == 0 and out['runs'].tolist() == [0, 1] and float(out['total'][0]) == -INF
    assert all(bool((out[name][0] == -7).all()) for name in ('phonemes', 'starts', 'score', 'gop'))
    assert out['phonemes'][1, 0].item() == 13 and out['starts'][1, :2].tolist() == [0, 1]
    assert math.isfinite(float(out['total'][1])) and float(out['score'][1, 0]) == float(out['total'][1])
    assert bool((out['phonemes'][1, 1:] == -7).all()) and bool((out['starts'][1, 2:] == -7).all())


def ragged_batch():
    generator = torch.Generator().manual_seed(33)
    lengths = torch.randint(1, 301, (33,), generator=generator).tolist()
    lengths[0], lengths[1], lengths[2] = 1, 300, 2
    ppg = torch.full((33, 40, 300), float('nan'))
    for b in range(33):
        ppg[b, :, :lengths[b]] = F.random_ppg(lengths[b], (1., 3., 8.)[b % 3], generator)
    return ppg.cuda(), lengths, random_model(generator, holes=0.2)


def equal_recognitions(batch, singles, offset=0):
    for b, one in enumerate(singles):
        at = b - offset
        if not 0 <= at < len(batch.starts):
            continue
        assert torch.equal(batch.starts[at], one.starts) and torch.equal(batch.phonemes[at], one.phonemes), b
        for name in ('score', 'gop'):
            assert torch.equal(getattr(batch, name)[at].view(torch.int32), getattr(one, name).view(torch.int32)), b
        assert torch.equal(batch.total[at].view(torch.int32), one.total.view(torch.int32)), b


def test_ragged_batch_equals_singles_from_streams_split_and_poisoned(monkeypatch):
    ppg, lengths, (A, initial, final) = ragged_batch()
    model = {'transitions': A, 'initial': initial, 'final': final}
    batch = alignment.recognize(ppg, lengths, **model)
    assert batch.total.shape == (33,) and bool(torch.isfinite(batch.total).all())
    singles = [alignment.recognize(ppg[b, :, :lengths[b]], **model) for b in range(33)]
    equal_recognitions(batch, singles)
    assert batch.starts[0].tolist() == [0, 1] and int(batch.starts[1][-1]) == 300
    # a poisoned workspace gives the same bits, and the rest of the outputs is left alone
    size = E.library().ppg_recognize_workspace_bytes(33, 300)
    for fill in (0, 255):
        rc, out = raw_recognize(ppg, lengths, (A, initial, final), torch.full((size,), fill, dtype=torch.uint8,
                                                                               device='cuda'))
        assert rc == 0 and torch.equal(out['total'].view(torch.int32), batch.total.view(torch.int32))
        for b in range(33):
            count = int(out['runs'][b])
            assert torch.equal(out['phonemes'][b, :count], batch.phonemes[b])
            assert torch.equal(out['starts'][b, :count + 1], batch.starts[b])
            assert torch.equal(out['gop'][b, :count].view(torch.int32), batch.gop[b].view(torch.int32))
            assert bool((out['phonemes'][b, count:] == -7).all()) and bool((out['starts'][b, count + 1:] == -7).all())
            assert bool((out['score'][b, count:] == -7).all()) and bool((out['gop'][b, count:] == -7).all())
    rc, out = raw_recognize(ppg, lengths, (A, initial, final), torch.zeros(size, dtype=torch.uint8, device='cuda'),
                            want_gop=False)
    assert rc == 0 and bool((out['gop'] == -7).all()) and torch.equal(out['score'][1, :int(out['runs'][1])],
                                                                      batch.score[1])
    # the two halves from two streams at once
    torch.cuda.synchronize()
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    halves = [(0, 16), (16, 33)]
    results = [[], []]
    for _ in range(3):
        for side, (low, high) in enumerate(halves):
            with torch.cuda.stream(streams[side]):
                results[side].append(alignment.recognize(ppg[low:high], lengths[low:high], **model))
    torch.cuda.synchronize()
    for side, (low, _) in enumerate(halves):
        for result in results[side]:
            equal_recognitions(result, singles, offset=low)
    # a batch that recognize_items has to split: room for five items per call
    monkeypatch.setattr(E, 'RECOGNIZE_WORKSPACE_BYTES', E.library().ppg_recognize_workspace_bytes(5, 300))
    equal_recognitions(alignment.recognize(ppg, lengths, **model), singles)
    monkeypatch.setattr(E, 'RECOGNIZE_WORKSPACE_BYTES', 1)      # less than one item takes: one item per call
    equal_recognitions(alignment.recognize(ppg[:4], lengths[:4], **model), singles)


def test_error_paths_launch_nothing_and_impossible_lengths_give_nan():
    lib = E.library()
    generator = torch.Generator().manual_seed(8)
    ppg = torch.stack([F.random_ppg(100, 3., generator), F.random_ppg(100, 8., generator)]).cuda().contiguous()
    lengths = [100, 83]
    model = random_model(generator, holes=0.1)
    need = lib.ppg_recognize_workspace_bytes(2, 100)
    workspace = torch.zeros(need + 64, dtype=torch.uint8, device='cuda')
    assert workspace.data_ptr() % 16 == 0
    refused = [
        raw_recognize(ppg, lengths, model, workspace, size=need - 1),                      # workspace too small
        raw_recognize(ppg, lengths, model, workspace, offset=8),                           # misaligned
        raw_recognize(ppg, lengths, model, workspace, frames=E.RECOGNIZE_MAX_FRAMES + 1, size=1 << 50),
        raw_recognize(ppg, lengths, model, workspace, items=E.RECOGNIZE_MAX_ITEMS + 1, size=1 << 50),
        raw_recognize(ppg, lengths, model, workspace, items=0),
        raw_recognize(ppg, lengths, model, workspace, frames=0),
    ]
    for name in ('ppg', 'lengths', 'transitions', 'phonemes', 'starts', 'runs', 'total', 'score', 'workspace'):
        refused.append(raw_recognize(ppg, lengths, model, workspace, missing=(name,)))
    for rc, out in refused:
        assert rc == -1 and lib.ppg_last_error()
        assert untouched(out, ('phonemes', 'starts', 'runs', 'total', 'score', 'gop'))
    assert not workspace.any()                                                             # nothing was launched
    # initial, final and gop may be NULL
    rc, plain = raw_recognize(ppg, lengths, (model[0], None, None), workspace, want_gop=False)
    assert rc == 0 and bool(torch.isfinite(plain['total']).all()) and bool((plain['gop'] == -7).all())
    zero = torch.zeros(40)
    rc, same = raw_recognize(ppg, lengths, (model[0], zero, zero), workspace)
    assert rc == 0 and torch.equal(same['total'], plain['total']) and torch.equal(same['starts'], plain['starts'])
    # impossible device-side lengths: total = NaN, runs = 0, nothing else; the neighbour unharmed
    rc, good = raw_recognize(ppg, lengths, model, workspace)
    assert rc == 0 and bool(torch.isfinite(good['total']).all())
    for bad, item in (([0, 83], 0), ([100, 101], 1), ([-5, 83], 0), ([100, 1 << 30], 1)):
        rc, out = raw_recognize(ppg, bad, model, workspace)
        other = 1 - item
        assert rc == 0 and bool(torch.isnan(out['total'][item])) and int(out['runs'][item]) == 0, bad
        assert all(bool((out[name][item] == -7).all()) for name in ('phonemes', 'starts', 'score', 'gop')), bad
        for name in out:
            assert torch.equal(out[name][other], good[name][other]), (bad, name)
