"""The frame-metrics probes of tests/metrics_probe.py on the GPU (ppg_metrics_update through engine.MetricsState and
ppgs_amd.evaluate.Metrics): a grid-stride loop that goes round three times, tied logits, long label runs with holes and
empty waves, batch boundaries inside a wave, and logits at the extremes.  `pytest -m gpu`.  The criteria and why they
are what they are: tests/metrics_probe.py."""
import numpy as np
import pytest
import torch

import metrics_probe as P
import ppgs_amd
from ppgs_amd import engine as E

pytestmark = pytest.mark.gpu

SCALED = ('loss_sum', 'loss_weight_sum', 'jsd_sum', 'distance_matrix', 'confusion')
# (mix, class weights, loss weights, k, label type, lengths: None = applied to the labels on the host)
CONFIGURATIONS = (
    (True, True, False, 3, torch.int64, 'device'),
    (False, False, True, 5, torch.int32, 'host'),
    (True, False, False, 1, torch.int64, None),
    (False, True, True, 8, torch.int32, 'device'),
)


@pytest.fixture(scope='module')
def g(golden):
    return golden('g13_metrics')


_on_device = {}


def device_logits(name, g):
    if name not in _on_device:
        _on_device[name] = P.family(name, g)[0].cuda()
    return _on_device[name]


def real(words):
    """the raw state (int64 words) as a dict with the fixed-point fields as float64 values"""
    out = E.metrics_fields(np.asarray(words))
    for key in SCALED:
        out[key] = np.asarray(out[key], dtype=np.float64) / E.METRICS_FIXED_POINT
    out['loss_sum'], out['jsd_sum'], out['loss_weight_sum'] = (
        float(out['loss_sum']), float(out['jsd_sum']), float(out['loss_weight_sum']))
    return out


def state_for(g, mix=False, class_weights=False, loss_weights=False, k=3):
    kwargs = P.tables_for(g, mix, class_weights, loss_weights)
    return E.MetricsState(0, k=k, similarity_mix=kwargs['mix'], class_weights=kwargs['class_weights'],
                          loss_weights=kwargs['loss_weights'])


def raw(state):
    torch.cuda.synchronize()
    return state.state.clone()


def arguments(name, g, dtype=torch.int64, where='device', logits=None):
    """update()'s arguments for a family"""
    _, labels, lengths = P.family(name, g)
    logits = device_logits(name, g) if logits is None else logits
    if lengths is None or where is None:
        return logits, P.masked_labels(labels, lengths).to(dtype).cuda(), None
    return logits, labels.to(dtype).cuda(), lengths.cuda() if where == 'device' else lengths


@pytest.mark.parametrize('name', P.FAMILIES)
def test_family_meets_every_criterion(g, name):
    for mix, class_weights, loss_weights, k, dtype, where in CONFIGURATIONS:
        class_weights = class_weights and name != 'ties'
        state = state_for(g, mix, class_weights, loss_weights, k)
        state.update(*arguments(name, g, dtype, where))
        want = P.reference(name, g, mix=mix, class_weights=class_weights, loss_weights=loss_weights)
        failed, ratios = P.judge(real(raw(state).cpu().numpy()), want, k, class_weights, name in P.SUMMED)
        print(f'{name} mix {mix} class weights {class_weights} loss weights {loss_weights} k {k}: worst error / bound',
              {key: round(value, 4) for key, value in ratios.items()})
        assert not failed, (name, mix, class_weights, loss_weights, k, failed)


@pytest.mark.parametrize('name', P.FAMILIES)
def test_top_k_for_every_k(g, name):
    want = P.reference(name, g)
    got = []
    for k in range(1, 9):
        state = state_for(g, k=k)
        state.update(*arguments(name, g, torch.int32 if k % 2 else torch.int64))
        got.append(state.read()['topk_correct'])
    print(f'{name}: top-k correct for k = 1..8 {got}, reference {want["topk_by_k"].tolist()} of {want["count"]}')
    assert got == list(want['topk_by_k']) and got[0] == want['true_positives']


def test_stride_in_one_launch_equals_single_trip_launches_bit_for_bit(g):
    logits, labels, lengths = arguments('stride', g)
    whole = state_for(g, True, True, True)
    whole.update(logits, labels, lengths)
    expected = raw(whole)
    assert int(expected[0]) == P.reference('stride', g)['count']

    by_item = state_for(g, True, True, True)
    for b in range(3):                                         # 172 tiles each: one trip
        by_item.update(logits[b:b + 1], labels[b:b + 1], lengths[b:b + 1])
    assert torch.equal(raw(by_item), expected)

    by_time = state_for(g, True, True, True)
    for lo, hi in zip(P.STRIDE_CUTS[:-1], P.STRIDE_CUTS[1:]):
        by_time.update(logits[:, :, lo:hi], labels[:, lo:hi], (lengths - lo).clamp(0, hi - lo))
    assert torch.equal(raw(by_time), expected)

    # the same launch replayed from a captured graph
    graphed = state_for(g, True, True, True)
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        graphed.update(logits, labels, lengths)                # warm-up outside the capture
        graphed.reset()
    torch.cuda.current_stream().wait_stream(stream)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        graphed.update(logits, labels, lengths)
    torch.cuda.synchronize()
    graphed.reset()
    graph.replay()
    assert torch.equal(raw(graphed), expected)
    graph.replay()
    assert torch.equal(raw(graphed), 2 * expected)


@pytest.mark.parametrize('name', ['edge_lengths', 'stride', 'single_lengths'])
def test_frames_that_do_not_count_are_never_read(g, name):
    states = []
    for fill in ('zero', 'garbage'):
        logits = P.poisoned(P.family(name, g), fill).cuda()
        for where in ('device', 'host', None):
            state = state_for(g, True, True, True)
            state.update(*arguments(name, g, torch.int64, where, logits))
            states.append(raw(state))
    assert int(states[0][0]) == P.reference(name, g)['count']
    assert all(torch.equal(state, states[0]) for state in states[1:])


def test_evaluate_metrics_on_ties_gives_the_reference_ratios(g):
    logits, labels, _ = arguments('ties', g)
    for k in (1, 3, 8):
        want = P.reference('ties', g)
        metrics = ppgs_amd.evaluate.Metrics(k=k, normalize=False)
        metrics.update(logits, labels)
        results = metrics()
        assert results['Accuracy'] == want['true_positives'] / want['count']
        assert results[f'Top-{k} Accuracy/'] == want['topk_by_k'][k - 1] / want['count']
        for index, phoneme in enumerate(ppgs_amd.phonemes.PHONEMES):
            assert results[f'Total/{phoneme}'] == want['class_total'][index]
            assert results[f'Count/{phoneme}'] == want['class_count'][index]


@pytest.mark.parametrize('mix', [True, False])
def test_extreme_frame_by_frame(g, mix):
    logits, labels, _ = P.family('extreme', g)
    loss_weights = not mix
    state = state_for(g, mix, True, loss_weights)
    logits_d = device_logits('extreme', g)
    snapshots = [state.state.clone()]
    for t in range(labels.shape[1]):
        state.update(logits_d, P.only_frame(labels, t).cuda())
        snapshots.append(state.state.clone())
    words = torch.stack(snapshots).cpu()
    delta = (words[1:] - words[:-1]).numpy()
    assert (delta[:, 0] == 1).all() and (delta[:, 3] == 0).all()
    capped = logits[0].gather(0, labels)[0] == -float('inf')
    assert (delta[capped.numpy(), 4] == 2 ** 52).all()         # each adds exactly 2^20 to loss_sum
    loss, jsd = delta[:, 4] / 2.0 ** 32, delta[:, 6] / 2.0 ** 32
    loss_ratio = P.extreme_loss_ratio(loss, g, mix, loss_weights)
    kappa = P.extreme_jsd_kappa(jsd, g, mix, loss_weights)
    print(f'extreme, mix {mix}: loss at {loss_ratio:.3f} of its bound; JSD needs kappa {kappa:.3f} '
          f'(the fp32 restatement {P.KAPPA_REF[mix]}, the bound {P.kappa_gpu(mix)})')
    assert loss_ratio <= 1
    assert kappa <= P.kappa_gpu(mix)
