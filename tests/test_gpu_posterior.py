"""ppgs_amd.alignment.posterior on the GPU (ppg_posterior) against the float64 reference of
tests/posterior_reference.py.

The tolerance.  Let M = 18.43 + the largest finite |weight| of the case (18.43 = -log(1e-8), the largest emission) and d
its largest in-degree or out-degree.  Per frame step the absolute error of a shifted quantity is at most
2**-23 * (4 M + d / 2 + 4): the emission, candidate, shift and scaling roundings on magnitudes <= M; a sum of d + 1
positive terms at 2**-24 relative each, whose relative error is an absolute error of the logarithm; exp2, log2 and two
scalings at 1 ulp.  So
    B(T) = (T + 1) * 2**-23 * (4 M + d / 2 + 4)                 (posterior_cases.bound)
and the tests assert |total - ref64| <= B(T), |gamma - gamma64| <= 3 B(T) gamma64 + 1e-6 (three exponent terms), and the
same for the phoneme posterior plus S * 2**-24 (a sum of up to S occupancies).  The kernels' arithmetic has these
roundings and no more per step: one addition per candidate, one subtraction and one scaling before its exp2, one log2
and one fused multiply-add after the sum, the shift, the emission.  3 B is vacuous at 65536 frames; there gamma and the
phoneme posterior are held to max(8 err32, 1e-5) absolute, err32 the float32 restatement's own largest error on that
input (8 covers hardware exp2 and log2 at 1 ulp against NumPy's 0.5 and another order of addition in a sum).
tests/test_posterior_host.py shows that B cannot hide a dropped arc on the random cases."""
import ctypes
import math

import numpy as np
import pytest
import torch

from ppgs_amd import alignment, engine as E

import posterior_cases as C
import posterior_reference as R

pytestmark = pytest.mark.gpu

INF = math.inf
HELD = 4096                                                    # arcs of a graph the kernels keep in LDS at most


def bits(tensor):
    return tensor.contiguous().view(torch.int64 if tensor.dtype == torch.float64 else torch.int32)


def reference(ppg, graph, dtype=np.float64):
    """(total, gamma (T, S), post (40, T)) of a CPU (40, T) PPG through a Graph."""
    g = R.lists(graph)
    return R.forward_backward(R.emissions(R.prepared(ppg.numpy()), g.sym), g, dtype)


def check(got, ppg, graph, label, expected=None):
    """One utterance's Posterior (made with states=True) against float64 under B(T); returns the largest errors."""
    frames, count = ppg.shape[1], graph.phonemes.shape[0]
    total, gamma, post = expected or reference(ppg, graph)
    b = C.bound(graph, frames)
    ours, states, phonemes = float(got.total), got.states.double().cpu().numpy(), got.phonemes.double().cpu().numpy()
    errors = (abs(ours - total), np.abs(states[:, :count] - gamma).max(), np.abs(phonemes - post).max())
    print(f'{label}: B = {b:.3e}, errors total {errors[0]:.3e} gamma {errors[1]:.3e} post {errors[2]:.3e}')
    assert got.total.dtype == torch.float64 and got.phonemes.dtype == torch.float32
    assert errors[0] <= b, label
    assert bool((np.abs(states[:, :count] - gamma) <= 3. * b * gamma + 1e-6).all()), label
    assert bool((np.abs(phonemes - post) <= 3. * b * post + 1e-6 + count * 2. ** -24).all()), label
    assert bool((states[:, count:] == 0.).all()), label
    assert np.abs(states.sum(axis=1) - 1.).max() <= 64 * 2. ** -23 + count * 2. ** -24, label
    return errors


# ---- 1. exact: one path ----

@pytest.mark.parametrize('count', (1, 2, 64, 65, 1024))
def test_one_path_gives_a_one_hot_occupancy_bit_for_bit(count):
    generator = torch.Generator().manual_seed(1000 + count)
    sequence = torch.randint(0, 40, (count,), generator=generator).tolist()
    ppg = C.random_ppg(1000 + count, count)
    graph = alignment.chain_graph(sequence)
    got = alignment.posterior(ppg.cuda(), graph, states=True)
    assert torch.equal(got.states.cpu(), torch.eye(count))     # 1.0 and 0.0
    one_hot = torch.zeros(40, count)
    one_hot[sequence, torch.arange(count)] = 1.
    assert torch.equal(got.phonemes.cpu(), one_hot)
    forced = alignment.forced(ppg.cuda(), sequence)
    assert abs(float(got.total) - float(forced.total)) <= C.bound(graph, count)


# ---- 2. closed form ----

@pytest.mark.parametrize('frames', (1, 2, 33, 64, 65, 129))
def test_a_free_model_renormalises_the_clamped_input(frames):
    ppg = C.random_ppg(2000 + frames, frames)
    ppg[:, 0] = 0.                                             # a column that the clamp alone holds up
    ppg[3, 0] = 1.
    graph = alignment.model_graph(torch.zeros(40, 40))
    got = alignment.posterior(ppg.cuda(), graph)
    assert got.states is None and got.phonemes.shape == (40, frames) and got.total.shape == ()
    clamped = ppg.clamp(1e-8, 1. - 1e-8).double()
    b = C.bound(graph, frames)
    assert abs(float(got.total) - float(clamped.sum(dim=0).log().sum())) <= b
    expected = clamped / clamped.sum(dim=0)
    error = (got.phonemes.double().cpu() - expected).abs()
    assert bool((error <= 3. * b * expected + 1e-6 + 40 * 2. ** -24).all())


# ---- 3. random graphs against float64 ----

@pytest.mark.parametrize('count,frames,seed', C.RANDOM_CASES)
def test_random_graphs_against_the_float64_reference(count, frames, seed):
    graph, ppg = C.random_graph(seed, count), C.random_ppg(seed, frames)
    got = alignment.posterior(ppg.cuda(), graph, states=True)
    check(got, ppg, graph, f'random {count} x {frames}')
    best = alignment.viterbi(ppg.cuda(), graph)
    assert float(got.total) >= float(best.total) - C.bound(graph, frames)
    again = alignment.posterior(ppg.cuda(), graph, states=True)
    for name in ('total', 'phonemes', 'states'):
        assert torch.equal(bits(getattr(got, name)), bits(getattr(again, name))), name


# ---- 4. arcs from memory, in both passes ----

def large_loop(seed):
    """A loop over 170 words of four phonemes: 170 * 170 arcs between the words and 3 * 170 inside them."""
    generator = torch.Generator().manual_seed(seed)
    lexicon = [(f'w{i}', [torch.randint(0, 40, (4,), generator=generator).tolist()]) for i in range(170)]
    return alignment.word_loop(lexicon, penalty=2., silence=False)[0]


def test_arcs_from_memory_against_the_float64_reference():
    heavy = C.random_graph(41, 700, big=False, most=20)
    assert 6000 < int(heavy.offsets[-1]) < 8000 and int(heavy.offsets[-1]) > HELD
    ppg = C.random_ppg(41, 40)
    check(alignment.posterior(ppg.cuda(), heavy, states=True), ppg, heavy, 'heavy 700')
    loop = large_loop(42)
    assert int(loop.offsets[-1]) == 29410 > HELD and loop.phonemes.shape[0] == 680
    ppg = C.random_ppg(42, 37)
    check(alignment.posterior(ppg.cuda(), loop, states=True), ppg, loop, 'word loop 170')


def test_a_batch_whose_items_differ_in_where_their_arcs_come_from_equals_its_singles():
    heavy = C.random_graph(43, 700, big=False, most=20)
    chain = alignment.chain_graph([4, 4, 11, 30, 2])
    graphs = [chain, heavy] * 4
    lengths = [33, 33, 5, 1, 17, 33, 6, 20]
    ppg = torch.full((8, 40, 33), float('nan'))
    for b, length in enumerate(lengths):
        ppg[b, :, :length] = C.random_ppg(4300 + b, length)
    ppg = ppg.cuda()
    batch = alignment.posterior(ppg, graphs, lengths, states=True)
    assert batch.states.shape == (8, 33, 700) and bool(torch.isfinite(batch.total).all())
    for b in range(8):
        one = alignment.posterior(ppg[b, :, :lengths[b]], graphs[b], states=True)
        count = graphs[b].phonemes.shape[0]
        assert torch.equal(bits(batch.total[b]), bits(one.total)), b
        assert torch.equal(bits(batch.phonemes[b, :, :lengths[b]]), bits(one.phonemes)), b
        assert torch.equal(bits(batch.states[b, :lengths[b], :count]), bits(one.states)), b
        assert bool((batch.phonemes[b, :, lengths[b]:] == 0).all()) and bool((batch.states[b, lengths[b]:] == 0).all())
        assert bool((batch.states[b, :, count:] == 0).all())


# ---- 5. sharpening ----

def spoken_words():
    """(lexicon of ten words, PPG (40, T), labels): six of the words said, every phoneme for 16 frames, the label's
    logit 4 above normal noise."""
    generator = torch.Generator().manual_seed(5000)
    phonemes = torch.randperm(40, generator=generator).tolist()
    lexicon = [(f'w{i}', [phonemes[3 * i:3 * i + 3]]) for i in range(10)]      # no phoneme in two words
    labels = [p for word in (2, 7, 0, 9, 4, 7) for p in lexicon[word][1][0] for _ in range(16)]
    logits = torch.randn(40, len(labels), generator=generator)
    logits[labels, torch.arange(len(labels))] += 4.
    return lexicon, torch.softmax(logits, dim=0).float(), labels


@pytest.mark.parametrize('scale', (1., 4., 16.))
def test_the_occupancy_follows_the_best_path_where_it_is_sure(scale):
    lexicon, ppg, labels = spoken_words()
    graph = alignment.word_loop(lexicon, penalty=1., silence=False)[0]
    graph = graph._replace(weights=graph.weights * scale, initial=graph.initial * scale)
    got = alignment.posterior(ppg.cuda(), graph, states=True)
    path = alignment.viterbi(ppg.cuda(), graph)
    states = alignment.frame_labels(path.starts, path.states, ppg.shape[1]).long()
    along = got.states.gather(1, states[:, None])[:, 0]
    sure = along > 0.9
    assert int(sure.sum()) >= ppg.shape[1] // 2
    assert torch.equal(got.states.argmax(dim=1)[sure], states[sure])
    confidence = alignment.run_confidence(path, got)
    assert confidence.shape == path.states.shape and bool(((confidence >= 0.) & (confidence <= 1. + 1e-6)).all())
    if scale == 1.:
        # the float64 reference meets the condition on this input, so the device has to
        _, gamma, _ = reference(ppg, graph)
        starts = path.starts.tolist()
        expected = [gamma[a:b, n].mean() for n, a, b in zip(path.states.tolist(), starts, starts[1:])]
        assert sum(v >= 0.9 for v in expected) * 2 >= len(expected)
        assert int((confidence >= 0.9).sum()) * 2 >= confidence.shape[0]
        assert np.abs(confidence.double().cpu().numpy() - np.asarray(expected)).max() <= 1e-4


# ---- 6. ragged batch ----

def pack(graphs):
    """The packed arrays of a list of Graphs with their transposes, as host lists."""
    packed = {name: [] for name in ('phonemes', 'stay', 'initial', 'final', 'sources', 'weights', 'targets',
                                    'out_weights')}
    state_begin, arc_begin, out_begin = [0], [], []
    for graph in graphs:
        offsets, targets, weights = alignment._transposed(graph)
        base = len(packed['sources'])
        arc_begin += [base + offset for offset in graph.offsets.tolist()[:-1]]
        out_begin += [base + offset for offset in offsets.tolist()[:-1]]
        for name in ('phonemes', 'stay', 'initial', 'final', 'sources', 'weights'):
            packed[name] += getattr(graph, name).tolist()
        packed['targets'] += targets.tolist()
        packed['out_weights'] += weights.tolist()
        state_begin.append(len(packed['phonemes']))
    arcs = len(packed['sources'])
    return dict(packed, state_begin=state_begin, arc_begin=arc_begin + [arcs], out_begin=out_begin + [arcs])


def raw_posterior(ppg, lengths, which, workspace, arrays, max_states, want_states=True):
    """ppg_posterior through ctypes with the caller's workspace; outputs start as sentinels.  (rc, {name: tensor})."""
    lib = E.library()
    count, width = ppg.shape[0], ppg.shape[2]
    out = {'total': torch.full((count,), -7., dtype=torch.float64, device='cuda'),
           'post': torch.full((count, 40, width), -7., device='cuda'),
           'states': torch.full((count, width, max_states), -7., device='cuda')}
    integer = ('state_begin', 'phonemes', 'arc_begin', 'sources', 'out_begin', 'targets')
    device = {name: torch.as_tensor(value).to(torch.int32 if name in integer else torch.float32).cuda()
              for name, value in arrays.items()}
    n_graphs, n_states, n_arcs = len(arrays['state_begin']) - 1, len(arrays['phonemes']), len(arrays['sources'])
    chosen = None if which is None else torch.tensor(which, dtype=torch.int32).cuda()
    given = torch.tensor(lengths, dtype=torch.int32).cuda()
    torch.cuda.synchronize()
    rc = lib.ppg_posterior(
        0, ppg.data_ptr(), width, count, given.data_ptr(), n_graphs, n_states, n_arcs, max_states,
        device['state_begin'].data_ptr(), device['phonemes'].data_ptr(), device['stay'].data_ptr(),
        device['initial'].data_ptr(), device['final'].data_ptr(), device['arc_begin'].data_ptr(),
        device['sources'].data_ptr() if n_arcs else None, device['weights'].data_ptr() if n_arcs else None,
        device['out_begin'].data_ptr(), device['targets'].data_ptr() if n_arcs else None,
        device['out_weights'].data_ptr() if n_arcs else None, None if chosen is None else chosen.data_ptr(),
        out['total'].data_ptr(), out['post'].data_ptr(), out['states'].data_ptr() if want_states else None, max_states,
        workspace.data_ptr(), workspace.numel(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return rc, out


def ragged_batch():
    generator = torch.Generator().manual_seed(7000)
    lengths = torch.randint(1, 81, (33,), generator=generator).tolist()
    lengths[0], lengths[1], lengths[2] = 1, 80, 2
    ppg = torch.full((33, 40, 80), float('nan'))
    graphs = []
    for b in range(33):
        ppg[b, :, :lengths[b]] = C.random_ppg(7000 + b, lengths[b], (1., 3., 8.)[b % 3])
        kind = b % 4
        if kind == 0:
            graphs.append(C.random_graph(7100 + b, (3, 64, 65, 300)[(b // 4) % 4], big=False))
        elif kind == 1:
            graphs.append(alignment.model_graph(-2. * torch.rand(40, 40, generator=generator)))
        elif kind == 2:
            graphs.append(alignment.chain_graph(torch.randint(0, 40, (min(lengths[b], 3 + 9 * b),),
                                                              generator=generator).tolist()))
        else:
            graphs.append(graphs[b - 3])                        # the same object again: it travels once
    return ppg.cuda(), lengths, graphs


def equal_posteriors(batch, singles, lengths, graphs, offset=0):
    for b, one in enumerate(singles):
        at = b - offset
        if not 0 <= at < batch.total.shape[0]:
            continue
        count = graphs[b].phonemes.shape[0]
        assert torch.equal(bits(batch.total[at]), bits(one.total)), b
        if not math.isfinite(float(one.total)):
            assert bool((batch.phonemes[at] == 0).all()) and bool((batch.states[at] == 0).all()), b
            continue
        assert torch.equal(bits(batch.phonemes[at, :, :lengths[b]]), bits(one.phonemes)), b
        assert torch.equal(bits(batch.states[at, :lengths[b], :count]), bits(one.states)), b
        assert bool((batch.phonemes[at, :, lengths[b]:] == 0).all()), b
        assert bool((batch.states[at, lengths[b]:] == 0).all()) and bool((batch.states[at, :, count:] == 0).all()), b


def test_ragged_batch_with_a_graph_per_item_equals_singles_from_streams_split_and_poisoned(monkeypatch):
    ppg, lengths, graphs = ragged_batch()
    batch = alignment.posterior(ppg, graphs, lengths, states=True)
    assert batch.total.shape == (33,) and batch.phonemes.shape == (33, 40, 80) and batch.states.shape == (33, 80, 300)
    assert not bool(torch.isnan(batch.total).any()) and int(torch.isfinite(batch.total).sum()) >= 25
    singles = [alignment.posterior(ppg[b, :, :lengths[b]], graphs[b], states=True) for b in range(33)]
    equal_posteriors(batch, singles, lengths, graphs)
    again = alignment.posterior(ppg, graphs, lengths, states=True)
    for name in ('total', 'phonemes', 'states'):
        assert torch.equal(bits(getattr(batch, name)), bits(getattr(again, name))), name
    # a poisoned workspace gives the same bits, and the rest of the outputs is left alone
    size = E.library().ppg_posterior_workspace_bytes(33, 80, 300)
    arrays = pack(graphs)
    for fill in (0, 255):
        rc, out = raw_posterior(ppg, lengths, list(range(33)), torch.full((size,), fill, dtype=torch.uint8,
                                                                          device='cuda'), arrays, 300)
        assert rc == 0 and torch.equal(bits(out['total']), bits(batch.total))
        for b in range(33):
            count, length = graphs[b].phonemes.shape[0], lengths[b]
            if not math.isfinite(float(batch.total[b])):
                assert bool((out['post'][b] == -7).all()) and bool((out['states'][b] == -7).all()), b
                continue
            assert torch.equal(bits(out['post'][b, :, :length]), bits(batch.phonemes[b, :, :length])), b
            assert torch.equal(bits(out['states'][b, :length, :count]), bits(batch.states[b, :length, :count])), b
            assert bool((out['post'][b, :, length:] == -7).all()) and bool((out['states'][b, length:] == -7).all()), b
            assert bool((out['states'][b, :, count:] == -7).all()), b
    rc, out = raw_posterior(ppg, lengths, list(range(33)), torch.zeros(size, dtype=torch.uint8, device='cuda'), arrays,
                            300, want_states=False)
    assert rc == 0 and bool((out['states'] == -7).all()) and torch.equal(bits(out['total']), bits(batch.total))
    assert torch.equal(bits(out['post'][1]), bits(batch.phonemes[1]))
    # the two halves from two streams at once
    torch.cuda.synchronize()
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    halves = [(0, 16), (16, 33)]
    results = [[], []]
    for _ in range(3):
        for side, (low, high) in enumerate(halves):
            with torch.cuda.stream(streams[side]):
                results[side].append(alignment.posterior(ppg[low:high], graphs[low:high], lengths[low:high],
                                                         states=True))
    torch.cuda.synchronize()
    for side, (low, _) in enumerate(halves):
        for result in results[side]:
            equal_posteriors(result, singles, lengths, graphs, offset=low)
    # a batch that posterior_items has to split: room for five items per call, then for one
    monkeypatch.setattr(E, 'POSTERIOR_WORKSPACE_BYTES', E.library().ppg_posterior_workspace_bytes(5, 80, 300))
    equal_posteriors(alignment.posterior(ppg, graphs, lengths, states=True), singles, lengths, graphs)
    monkeypatch.setattr(E, 'POSTERIOR_WORKSPACE_BYTES', 1)
    equal_posteriors(alignment.posterior(ppg[:4], graphs[:4], lengths[:4], states=True), singles, lengths, graphs)


# ---- 7. the frame limit ----

def test_a_recording_at_the_frame_limit_and_one_frame_more():
    frames = alignment.POSTERIOR_MAX_FRAMES
    ppg = C.random_ppg(7700, frames, 2.)
    graph = alignment.graph([3, 17, 17, 5, 30], [(0, 1, -1.), (1, 2, -.5), (2, 3, -2.), (3, 4, -1.), (4, 0, -3.),
                                                 (1, 3, -4.), (2, 2, -1.5)], stay=[-.1, -.2, -.3, -.4, -.5],
                        initial=-1., final=-2.)
    got = alignment.posterior(ppg.cuda(), graph, states=True)
    total, gamma, post = reference(ppg, graph)
    total32, gamma32, post32 = reference(ppg, graph, np.float32)
    err32 = max(np.abs(gamma32 - gamma).max(), np.abs(post32 - post).max())
    states, phonemes = got.states.double().cpu().numpy(), got.phonemes.double().cpu().numpy()
    errors = (abs(float(got.total) - total), np.abs(states - gamma).max(), np.abs(phonemes - post).max())
    print(f'limit: B = {C.bound(graph, frames):.3e}, err32 {err32:.3e} (total {abs(total32 - total):.3e}), errors total '
          f'{errors[0]:.3e} gamma {errors[1]:.3e} post {errors[2]:.3e}')
    assert errors[0] <= C.bound(graph, frames)
    assert max(errors[1], errors[2]) <= max(8. * err32, 1e-5)
    with pytest.raises(ValueError, match='65536'):
        alignment.posterior(torch.zeros(40, frames + 1, device='cuda'), graph)


# ---- 8. what the device refuses ----

def test_refused_graphs_and_items_give_nan_and_leave_their_neighbours_alone():
    ppg = torch.stack([C.random_ppg(8000 + b, 50) for b in range(3)]).cuda().contiguous()
    lengths = [50, 41, 50]
    good = alignment.chain_graph([3, 3, 17, 4])
    other = C.random_graph(8001, 5, big=False)
    assert int(other.offsets[-1]) >= 4
    fine = pack([good, other, good])
    single = alignment.posterior(ppg[1, :, :41], good, states=True)
    size = E.library().ppg_posterior_workspace_bytes(3, 50, 1024)
    workspace = torch.full((size,), 255, dtype=torch.uint8, device='cuda')

    def broken(**changes):
        arrays = {name: list(value) for name, value in fine.items()}
        for name, (index, value) in changes.items():
            arrays[name][index] = value
        return arrays
    arcs_other = fine['arc_begin'][4]                           # the first arc of graph 1, in either list
    assert fine['out_begin'][4] == arcs_other
    shorter = broken(out_begin=(8, fine['out_begin'][8] - 1))   # graph 1 and all behind it: one out-arc fewer than in-arcs
    for n in range(9, len(shorter['out_begin'])):
        shorter['out_begin'][n] -= 1
    shorter['targets'], shorter['out_weights'] = shorter['targets'][:-1] + [0], shorter['out_weights'][:-1] + [0.]
    cases = {
        'a target out of range': broken(targets=(arcs_other, 5)),
        'a negative target': broken(targets=(arcs_other, -1)),
        'a decreasing out_begin': broken(out_begin=(6, fine['out_begin'][5] - 1)),
        'an out_begin past the arcs': broken(out_begin=(8, len(fine['sources']) + 7)),
        'a NaN out weight': broken(out_weights=(arcs_other, math.nan)),
        'a +inf out weight': broken(out_weights=(arcs_other, INF)),
        'fewer out-arcs than in-arcs': shorter,
        'a source out of range': broken(sources=(arcs_other, 5)),
        'a decreasing arc_begin': broken(arc_begin=(6, fine['arc_begin'][5] - 1)),
        'a NaN weight': broken(weights=(arcs_other, math.nan)),
        'a +inf final': broken(final=(6, INF)),
        'a phoneme out of range': broken(phonemes=(4, 40)),
    }
    for label, arrays in cases.items():
        rc, out = raw_posterior(ppg, lengths, [0, 0, 1], workspace, arrays, 5)
        assert rc == 0, label
        assert math.isnan(float(out['total'][2])), label
        assert bool((out['post'][2] == -7).all()) and bool((out['states'][2] == -7).all()), label      # the poison stays
        assert torch.equal(bits(out['total'][1]), bits(single.total)), label   # the item beside it is untouched
        assert torch.equal(bits(out['post'][1, :, :41]), bits(single.phonemes)), label
        assert torch.equal(bits(out['states'][1, :41, :4]), bits(single.states)), label
        assert bool((out['post'][1, :, 41:] == -7).all()) and bool((out['states'][1, :, 4:] == -7).all()), label
        assert math.isfinite(float(out['total'][0])), label
    rc, out = raw_posterior(ppg, lengths, [0, 0, 1], workspace, fine, 5)
    assert rc == 0 and all(math.isfinite(v) for v in out['total'].tolist())
    # a graph larger than max_states says
    tiny = alignment.chain_graph([3])
    rc, out = raw_posterior(ppg, lengths, [0, 1, 2], workspace, pack([good, other, tiny, tiny]), 4)
    assert rc == 0 and [math.isnan(v) for v in out['total'].tolist()] == [False, True, False]
    assert bool((out['post'][1] == -7).all())
    # `which` out of range and an impossible length, through engine.posterior_items: zeros stay zeros
    for which, given in (([0, 3, 1], lengths), ([0, -1, 1], lengths), ([0, 1, 1], [50, 0, 50]), ([0, 1, 1], [50, 51, 50])):
        total, post, states = E.posterior_items(
            ppg, given, fine['state_begin'], fine['phonemes'], fine['stay'], fine['initial'], fine['final'],
            fine['arc_begin'], fine['sources'], fine['weights'], fine['out_begin'], fine['targets'], fine['out_weights'],
            which, 5, True)
        assert [math.isnan(v) for v in total.tolist()] == [False, True, False], (which, given)
        assert bool((post[1] == 0).all()) and bool((states[1] == 0).all())
        assert bool((post[0] != 0).any())
    # a graph with no way through: -inf and zeros
    stuck = alignment.graph([1, 2], [(0, 1, -INF)], initial=[0., -INF], final=[-INF, 0.])
    got = alignment.posterior(ppg[0], stuck, states=True)
    assert float(got.total) == -INF and bool((got.phonemes == 0).all()) and bool((got.states == 0).all())
    late = alignment.graph([1, 2], [(0, 1, 0.)], initial=[0., -INF], final=[-INF, 0.])
    assert float(alignment.posterior(ppg[0, :, :1], late).total) == -INF       # one frame cannot reach state 1
    assert math.isfinite(float(alignment.posterior(ppg[0, :, :2], late).total))
