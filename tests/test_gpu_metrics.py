"""Frame metrics on the GPU (ppg_metrics_update, engine.MetricsState, ppgs_amd.evaluate) against the reference's
own accumulators (fixture g13) and the float64 restatement of tests/test_metrics_host.py.  `pytest -m gpu`.

Integer accumulators are compared for equality.  loss, JSD and the matrix cells within rtol 2e-5 / atol 2e-6 per
frame -- the bound test_postops_match_reference_fixture uses for the same clamp-log-sqrt chain -- applied to the
means, and for a matrix cell atol = 2e-6 x frames of its row + n x 2^-32 (the fixed-point quantum).  Order
independence is bit-exact on the raw state.
"""
import json
import math
import os

import numpy as np
import pytest
import torch

import ppgs_amd
from ppgs_amd import engine as E
from ppgs_amd import weights as W
from test_metrics_host import case_inputs, check_against_fixture, mix_of, restate

pytestmark = pytest.mark.gpu

SCALED = ('loss_sum', 'loss_weight_sum', 'jsd_sum', 'distance_matrix', 'confusion')


def real(read):
    """a read() dict with the fixed-point fields as float64 values"""
    out = dict(read)
    for key in SCALED:
        out[key] = np.asarray(read[key], dtype=np.float64) / E.METRICS_FIXED_POINT
    out['loss_sum'], out['jsd_sum'] = float(out['loss_sum']), float(out['jsd_sum'])
    return out


def state_for(g, **kwargs):
    kwargs.setdefault('similarity_mix', mix_of(g))
    kwargs.setdefault('class_weights', torch.from_numpy(g['weights']))
    return E.MetricsState(0, **kwargs)


@pytest.mark.parametrize('case', ['A', 'B', 'C', 'D'])
def test_fixture_cases_match_the_reference_accumulators(golden, case):
    g = golden('g13_metrics')
    logits, labels, _ = case_inputs(g, case)
    similarity, weights = torch.from_numpy(g['similarity']), torch.from_numpy(g['weights'])
    reference = json.loads(str(g[f'{case}_results']))
    for normalize, balanced, dtype in ((True, False, torch.int64), (False, False, torch.int32),
                                       (True, True, torch.int32), (False, True, torch.int64)):
        metrics = ppgs_amd.evaluate.Metrics(
            include_figures=True, normalize=normalize, similarity=similarity, weights=weights,
            class_balanced=balanced)
        metrics.update(logits.cuda(), labels.to(dtype).cuda())
        read = metrics.read()
        assert read['invalid_labels'] == 0
        check_against_fixture(real(read), g, case, normalize=normalize, balanced=balanced, fixed_point=True)
        results = metrics()
        assert list(results)[:len(reference)] == list(reference)
        if normalize and not balanced:
            for key, expected in reference.items():
                if isinstance(expected, float) and math.isnan(expected):
                    assert math.isnan(results[key]), key
                else:
                    assert results[key] == pytest.approx(expected, rel=2e-5, abs=2e-6 + 2.0 ** -32), key
    # the engine layer agrees with the float64 restatement on what the fixture does not hold
    state = state_for(g, k=5, loss_weights=weights)
    state.update(logits.cuda(), labels.cuda())
    got, want = state.read(), restate(logits, labels, k=5, mix=mix_of(g), class_weights=weights, loss_weights=weights)
    assert got['topk_correct'] == want['topk_correct']
    assert got['loss_weight_sum'] / E.METRICS_FIXED_POINT == pytest.approx(want['loss_weight_sum'], rel=1e-6, abs=1e-6)


def raw(state):
    torch.cuda.synchronize()
    return state.state.clone()


def test_order_independence_is_bit_exact(golden):
    g = golden('g13_metrics')
    logits, labels, lengths = case_inputs(g, 'B')
    logits_d, labels_d = logits.cuda(), labels.cuda()
    whole = state_for(g)
    whole.update(logits_d, labels_d)
    expected = raw(whole)
    assert int(expected[0]) == int(g['B_count'])

    cuts = [0, 1, 4, 5, 12, 19, 30, 32]                       # seven uneven slices along the batch
    by_batch = state_for(g)
    for lo, hi in zip(cuts[:-1], cuts[1:]):
        by_batch.update(logits_d[lo:hi], labels_d[lo:hi])
    assert torch.equal(raw(by_batch), expected)

    cuts = [0, 3, 64, 65, 400, 401, 977, 1000]                # along time: the whole batch each call, other frames masked
    by_time = state_for(g)
    frame = torch.arange(1000, device='cuda')[None, :]
    for index, (lo, hi) in enumerate(zip(cuts[:-1], cuts[1:])):
        if index % 2:                                          # alternately by label masking and by a time slice + lengths
            masked = torch.where((frame >= lo) & (frame < hi), labels_d, torch.full_like(labels_d, -100))
            by_time.update(logits_d, masked)
        else:
            by_time.update(logits_d[:, :, lo:hi], labels_d[:, lo:hi], torch.full((32,), hi - lo))
    assert torch.equal(raw(by_time), expected)

    order = torch.randperm(32, generator=torch.Generator().manual_seed(5))
    permuted = state_for(g)
    permuted.update(logits_d[order.cuda()], labels_d[order.cuda()])
    assert torch.equal(raw(permuted), expected)

    # on a side stream while the main stream runs the 32 x 1000 forward
    model = E.Engine(W.seeded_state_dict(seed=1234), 0, 'fp16')
    features = torch.randn(32, 80, 1000, generator=torch.Generator().manual_seed(2)).half().cuda()
    beside = state_for(g)
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    for _ in range(3):
        model.encode(features, [1000] * 32)
    with torch.cuda.stream(side):
        for lo in range(0, 32, 8):
            beside.update(logits_d[lo:lo + 8], labels_d[lo:lo + 8])
    model.encode(features, [1000] * 32)
    assert torch.equal(raw(beside), expected)

    halves = [state_for(g), state_for(g)]
    halves[0].update(logits_d[:13], labels_d[:13])
    halves[1].update(logits_d[13:], labels_d[13:])
    merged = E.MetricsState.merge(halves[0].read(), halves[1].read())
    total = whole.read()
    assert all(np.array_equal(merged[key], total[key]) for key in total)

    whole.reset()
    assert int(raw(whole).abs().sum()) == 0


def test_padding_is_never_read_and_lengths_mask_labels(golden):
    g = golden('g13_metrics')
    logits, labels, lengths = case_inputs(g, 'A')
    clean = state_for(g)
    clean.update(logits.cuda(), labels.cuda())
    dirty_logits, dirty_labels = logits.clone(), labels.clone()
    frames = logits.shape[2]
    padding = torch.arange(frames)[None, :] >= lengths[:, None]
    assert padding.any()
    garbage = torch.tensor([float('nan'), float('inf'), -float('inf'), 1e38])
    dirty_logits.transpose(1, 2)[padding] = garbage[torch.arange(int(padding.sum())) % 4][:, None]
    dirty_labels[padding] = torch.arange(int(padding.sum())) % 40           # in range: only `lengths` masks them
    dirty = state_for(g)
    dirty.update(dirty_logits.cuda(), dirty_labels.cuda(), lengths)
    assert torch.equal(raw(dirty), raw(clean))
    on_device = state_for(g)
    on_device.update(dirty_logits.cuda(), dirty_labels.cuda(), lengths.cuda())
    assert torch.equal(raw(on_device), raw(clean))


def test_invalid_labels_are_counted_and_refused(golden):
    g = golden('g13_metrics')
    logits, labels, _ = case_inputs(g, 'A')
    labelled = (labels != -100).nonzero()
    bad = labels.clone()
    bad[labelled[0, 0], labelled[0, 1]] = 40
    bad[labelled[7, 0], labelled[7, 1]] = -1
    metrics = ppgs_amd.evaluate.Metrics(normalize=False)
    metrics.update(logits.cuda(), bad.cuda())
    read = metrics.read()
    assert read['invalid_labels'] == 2 and read['count'] == int(g['A_count']) - 2
    dropped = labels.clone()
    dropped[labelled[0, 0], labelled[0, 1]] = -100
    dropped[labelled[7, 0], labelled[7, 1]] = -100
    other = ppgs_amd.evaluate.Metrics(normalize=False)
    other.update(logits.cuda(), dropped.cuda())
    expected = raw(other.state)
    expected[3] = 2
    assert torch.equal(raw(metrics.state), expected)
    with pytest.raises(ValueError):
        metrics()
    with pytest.raises(ValueError):
        E.MetricsState(0, k=9)


def test_from_dataloader_scores_the_engines_own_logits(tmp_path):
    checkpoint = W.seeded_state_dict(seed=1234)
    generator = torch.Generator().manual_seed(77)
    batches = []
    for batch, frames in ((3, 420), (5, 777), (2, 1100)):
        features = torch.randn(batch, 80, frames, generator=generator).half()
        lengths = torch.randint(frames // 2, frames + 1, (batch,), generator=generator)
        lengths[0] = frames
        indices = torch.randint(0, 40, (batch, frames), generator=generator)
        indices[torch.rand(batch, frames, generator=generator) < 0.02] = -100
        batches.append((features, indices, lengths))
    metrics = ppgs_amd.evaluate.Metrics(normalize=False, k=3)
    results = ppgs_amd.evaluate.from_dataloader(
        batches, checkpoint=checkpoint, representation='mel', gpu=0, precision='fp32', metrics=metrics)
    got = real(metrics.read())
    model = ppgs_amd.engine_for('mel', checkpoint, 0, 'fp32')
    want, close = None, 0
    exact = True
    for features, indices, lengths in batches:
        logits = model.encode(features.cuda(), lengths, softmax=False).cpu()
        part = restate(logits, indices, lengths)
        # frames whose two largest logits are closer than 1e-6 may be left out of the exact comparison
        masked = indices.clone()
        masked[torch.arange(indices.shape[1])[None, :] >= lengths[:, None]] = -100
        top = logits.topk(2, dim=1).values
        near = ((top[:, 0] - top[:, 1]) < 1e-6) & (masked != -100)
        close += int(near.sum())
        want = part if want is None else {
            key: (value + want[key]) for key, value in part.items()}
    share = close / want['count']
    print(f'from_dataloader: {want["count"]} labelled frames, {close} near ties left out ({share:.4%})')
    assert share < 1e-3
    if close == 0:
        for key in ('count', 'true_positives', 'topk_correct'):
            assert got[key] == want[key], key
        for key in ('class_total', 'class_count'):
            assert np.array_equal(got[key], want[key]), key
    else:
        assert got['count'] == want['count'] and np.array_equal(got['class_count'], want['class_count'])
        assert abs(got['true_positives'] - want['true_positives']) <= close
    n = want['count']
    for key in ('loss_sum', 'jsd_sum'):
        assert abs(got[key] - want[key]) / n <= 2e-6 + 2e-5 * abs(want[key]) / n + 2.0 ** -32, key
    bound = 2e-6 * want['class_count'][:, None] + n * 2.0 ** -32 + 2e-5 * np.abs(want['confusion'])
    assert (np.abs(got['confusion'] - want['confusion']) <= bound).all()
    assert results['Accuracy'] == got['true_positives'] / n and results['loss'] == pytest.approx(want['loss_sum'] / n, rel=2e-5)
    ppgs_amd.evaluate.save(results, 'overall', tmp_path)
    assert json.load(open(tmp_path / 'overall.json'))['Count/aa'] == int(want['class_count'][0])


def test_across_precisions_scores_fp32_against_itself():
    checkpoint = W.seeded_state_dict(seed=1234)
    features = torch.randn(4, 80, 600, generator=torch.Generator().manual_seed(3)).half()
    results = ppgs_amd.evaluate.across_precisions(features, [600, 500, 433, 77], checkpoint)
    assert list(results) == ['fp32', 'fp16x2', 'fp16', 'bf16']
    assert results['fp32']['Accuracy'] == 1.0 and results['fp32']['Top-3 Accuracy/'] == 1.0
    for precision, result in results.items():
        print(precision, {key: result[key] for key in ('Accuracy', 'Top-3 Accuracy/', 'JSD', 'loss')})
        assert math.isfinite(result['Accuracy']) and result['Accuracy'] <= 1.0
        assert math.isfinite(result['loss']) and math.isfinite(result['JSD'])


def test_update_is_capturable_in_a_graph(golden):
    g = golden('g13_metrics')
    logits, labels, lengths = case_inputs(g, 'A')
    logits_d, labels_d, lengths_d = logits.cuda(), labels.cuda(), lengths.cuda()
    eager = state_for(g)
    for _ in range(3):
        eager.update(logits_d, labels_d, lengths_d)
    graphed = state_for(g)
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        graphed.update(logits_d, labels_d, lengths_d)          # warm-up outside the capture
        graphed.reset()
    torch.cuda.current_stream().wait_stream(stream)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        graphed.update(logits_d, labels_d, lengths_d)
    torch.cuda.synchronize()
    graphed.reset()
    for _ in range(3):
        graph.replay()
    assert torch.equal(raw(graphed), raw(eager))
