"""The host side of ppgs_amd.alignment.posterior: the float64 reference of the GPU tests against brute force, the host
transpose of every builder's graph, the sensitivity of the GPU tests' random cases to a dropped arc, the refusals raised
before a device is touched, and the library's PPG_EINVAL paths (nothing launched)."""
import ctypes
import math
import os
import re

import numpy as np
import pytest
import torch

from ppgs_amd import alignment, engine as E

import posterior_cases as C
import posterior_reference as R

INF = math.inf
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def small_graph(generator, states, holes):
    """A random graph of a few states: up to 2 arcs per ordered pair of states, so parallel arcs and arcs n -> n occur;
    `holes` is the share of -inf weights."""
    def weight():
        return -INF if float(torch.rand((), generator=generator)) < holes else -2. * float(
            torch.rand((), generator=generator))
    arcs = []
    for target in range(states):
        for source in range(states):
            for _ in range(int(torch.randint(0, 3, (), generator=generator))):
                arcs.append((source, target, weight()))
    order = torch.randperm(len(arcs), generator=generator).tolist()
    return alignment.graph(
        torch.randint(0, 40, (states,), generator=generator).tolist(), [arcs[i] for i in order],
        stay=[weight() for _ in range(states)], initial=[weight() for _ in range(states)],
        final=[weight() for _ in range(states)])


def test_reference_equals_brute_force_in_total_and_occupancy():
    generator = torch.Generator().manual_seed(11)
    seen = dict(path=0, none=0, parallel=0, loop=0, hole=0)
    for trial in range(60):
        states, frames = 1 + trial % 4, 1 + trial % 5
        graph = small_graph(generator, states, (0., 0.3, 0.6)[trial % 3])
        g = R.lists(graph)
        e = -3. * torch.rand(frames, states, generator=generator, dtype=torch.float64).numpy()
        total, gamma, post = R.forward_backward(e, g)
        expected, occupancy = R.brute_force(e, g)
        for n, into in enumerate(g.into):
            sources = [source for source, _ in into]
            seen['parallel'] += len(set(sources)) < len(sources)
            seen['loop'] += n in sources
            seen['hole'] += any(weight == -INF for _, weight in into)
        if expected == -INF:
            assert total == -INF and gamma is None and post is None
            seen['none'] += 1
            continue
        seen['path'] += 1
        assert abs(total - expected) <= 1e-12
        assert np.abs(gamma - occupancy).max() <= 1e-12
        assert np.abs(gamma.sum(axis=1) - 1.).max() <= 1e-12
        assert np.abs(post.sum(axis=0) - 1.).max() <= 1e-12
        for p in range(40):
            assert np.abs(post[p] - gamma[:, g.sym == p].sum(axis=1)).max() <= 1e-15
    assert all(count >= 3 for count in seen.values()), seen


def test_reference_counts_parallel_and_returning_arcs_by_hand():
    # two parallel arcs 0 -> 1 of weight log(1/4) each are one arc of log(1/2); an arc 0 -> 0 beside staying doubles it
    e = np.zeros((2, 2))
    graph = alignment.graph([0, 1], [(0, 1, math.log(.25)), (0, 1, math.log(.25)), (0, 0, 0.)], stay=0.,
                            initial=[0., -INF], final=0.)
    total, gamma, _ = R.forward_backward(e, R.lists(graph))
    # (a Graph holds fp32 weights: log(1/4) is rounded there)
    assert abs(total - math.log(2.5)) <= 1e-7                  # stay, return, and the two arcs of 1/4
    assert np.abs(gamma - np.array([[1., 0.], [.8, .2]])).max() <= 1e-7


def test_float32_restatement_stays_near_the_reference():
    graph, ppg = C.random_graph(10, 64), C.random_ppg(10, 97)
    g = R.lists(graph)
    e = R.emissions(R.prepared(ppg.numpy()), g.sym)
    total, gamma, post = R.forward_backward(e, g)
    total32, gamma32, post32 = R.forward_backward(e, g, np.float32)
    assert gamma32.dtype == np.float32
    assert abs(total32 - total) <= C.bound(graph, 97) / 100.
    assert np.abs(gamma32 - gamma).max() <= 1e-5 and np.abs(post32 - post).max() <= 1e-5


def builders():
    lexicon = {'yes': [['y', 'eh', 's']], 'no': [['n', 'ow'], ['n', 'ah']], 'maybe': [['m', 'ey', 'b', 'iy']]}
    yield 'graph', small_graph(torch.Generator().manual_seed(3), 4, 0.3)
    yield 'chain', alignment.chain_graph(['aa', 'b', 'aa', 'k'])
    yield 'chain optional', alignment.chain_graph(['aa', 'b', 'aa', 'k'], optional=[False, True, False, True])
    yield 'model', alignment.model_graph(torch.randn(40, 40, generator=torch.Generator().manual_seed(4)))
    yield 'pronunciations', alignment.pronunciations([[['dh', 'ah'], ['dh', 'iy']], [['k', 'ae', 't']]])[0]
    yield 'word loop', alignment.word_loop(lexicon, penalty=2.)[0]
    yield 'random', C.random_graph(1, 65)


@pytest.mark.parametrize('name,graph', list(builders()), ids=[name for name, _ in builders()])
def test_transpose_is_the_in_arcs_sorted_by_source_with_their_order_kept(name, graph):
    offsets, targets, weights = alignment._transposed(graph)
    count, arcs = graph.phonemes.shape[0], graph.sources.shape[0]
    assert offsets.shape == (count + 1,) and targets.shape == (arcs,) and weights.shape == (arcs,)
    assert int(offsets[0]) == 0 and int(offsets[-1]) == arcs and bool((offsets[1:] >= offsets[:-1]).all())
    into = R.lists(graph).into
    listed = [(source, n, j) for n, arcs_in in enumerate(into) for j, (source, _) in enumerate(arcs_in)]
    flat = {(n, j): weight for n, arcs_in in enumerate(into) for j, (_, weight) in enumerate(arcs_in)}
    expected = sorted(listed)                                  # by source, then in the order the in-lists hold them
    at = 0
    for source in range(count):
        for k in range(int(offsets[source]), int(offsets[source + 1])):
            s, n, j = expected[at]
            assert s == source and int(targets[k]) == n
            assert float(weights[k]) == flat[(n, j)] or (math.isinf(flat[(n, j)]) and float(weights[k]) == -INF)
            at += 1
    assert at == arcs
    assert alignment._transposed(graph) is alignment._transposed(graph)        # once per graph object


def test_a_dropped_arc_moves_the_total_far_beyond_the_bound():
    """The sensitivity condition of the GPU tests' tolerance: on each random case run there, deleting the last finite
    in-arc of the most occupied state that has one moves the float64 total by at least 100 B(T) in three cases of four,
    so B(T) cannot hide a kernel that drops an arc."""
    ratios = []
    for states, frames, seed in C.RANDOM_CASES:
        graph, ppg = C.random_graph(seed, states), C.random_ppg(seed, frames)
        g = R.lists(graph)
        e = R.emissions(R.prepared(ppg.numpy()), g.sym)
        total, gamma, _ = R.forward_backward(e, g)
        assert total > -INF
        less = C.without_an_arc(graph, gamma)
        assert less is not None
        ratios.append(abs(total - R.forward_backward(e, less)[0]) / C.bound(graph, frames))
    print('total shift / bound:', [round(r, 1) for r in ratios])
    assert sum(r >= 100. for r in ratios) * 4 >= 3 * len(ratios), ratios


def test_random_cases_have_the_degrees_and_weights_the_gpu_tests_rely_on():
    for states, _, seed in C.RANDOM_CASES:
        graph = C.random_graph(seed, states)
        offsets = graph.offsets.long()
        assert int((offsets[1:] - offsets[:-1]).max()) == 255
        assert int(torch.bincount(graph.sources.long()).max()) >= 300
        share = float(torch.isinf(graph.weights).float().mean())
        assert 0.2 < share < 0.4
        assert float(graph.weights[torch.isfinite(graph.weights)].min()) >= -5.


def test_posterior_argument_checks_need_no_device():
    graph = alignment.chain_graph(['aa', 'b'])
    with pytest.raises(ValueError, match='lengths go with a batch'):
        alignment.posterior(torch.rand(40, 5), graph, lengths=[5])
    with pytest.raises(ValueError, match='takes a Graph'):
        alignment.posterior(torch.rand(40, 5), 'aa b')
    with pytest.raises(ValueError, match='a list of graphs'):
        alignment.posterior(torch.rand(3, 40, 5), [graph, graph])
    with pytest.raises(ValueError):
        alignment.posterior(torch.rand(40, alignment.POSTERIOR_MAX_FRAMES + 1), graph)
    with pytest.raises(ValueError, match='states=True'):
        alignment.run_confidence(alignment.Path(*[None] * 6), alignment.Posterior(None, None, None))


def test_run_confidence_is_the_mean_occupancy_of_each_run():
    occupancy = torch.tensor([[.9, .1], [.7, .3], [.2, .8], [.0, 1.], [.6, .4]])
    path = alignment.Path(torch.tensor([0, 1, 0], dtype=torch.int32), None, torch.tensor([0, 2, 4, 5], dtype=torch.int32),
                          None, None, None)
    sure = alignment.run_confidence(path, alignment.Posterior(None, None, occupancy))
    assert torch.allclose(sure, torch.tensor([.8, .9, .6]))
    both = alignment.run_confidence(
        alignment.Path([path.states, path.states[:0]], None, [path.starts, path.starts[:1]], None, None, None),
        alignment.Posterior(None, None, torch.stack([occupancy, occupancy])))
    assert torch.allclose(both[0], sure) and both[1].shape == (0,)


def test_abi_declares_and_binds_the_entries():
    text = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'ppgs_amd.h')).read(), flags=re.S)
    for name in ('ppg_posterior_workspace_bytes', 'ppg_posterior'):
        declared = re.search(r'\b%s\s*\(([^)]*)\)' % name, text)
        assert declared, name
        assert name in E.SYMBOLS and hasattr(E.library(), name)
        assert len(declared.group(1).split(',')) == len(E.SYMBOLS[name][1]), name
    assert E.SYMBOLS['ppg_posterior'][0] is ctypes.c_int and len(E.SYMBOLS['ppg_posterior'][1]) == 28
    assert E.POSTERIOR_MAX_FRAMES == alignment.POSTERIOR_MAX_FRAMES == 65536
    assert re.search(r'#define\s+PPG_POSTERIOR_MAX_FRAMES\s+65536\b', text)


def test_workspace_bytes_is_host_only_and_refuses_impossible_sizes():
    size = E.library().ppg_posterior_workspace_bytes
    for items, frames, states in ((0, 10, 10), (10, 0, 10), (10, 10, 0), (-1, 10, 10), (E.VITERBI_MAX_ITEMS + 1, 10, 10),
                                  (1, E.POSTERIOR_MAX_FRAMES + 1, 10), (1, 10, E.VITERBI_MAX_STATES + 1)):
        assert size(items, frames, states) == 0
    assert size(1, 1, 1) > 0
    # prepared frames, a row of alpha and a float64 shift per frame
    assert size(3, 100, 64) >= 3 * 100 * (176 + 4 * 64 + 8) and size(3, 100, 65) >= 3 * 100 * (176 + 4 * 256 + 8)
    assert size(3, 100, 64) < size(3, 100, 65) == size(3, 100, 256) < size(3, 100, 257) < size(3, 100, 1024)
    assert 65536 * (176 + 4096 + 8) <= size(1, E.POSTERIOR_MAX_FRAMES, 1024) < 300 << 20


def test_library_einval_paths_launch_nothing():
    """Every call here is refused on the host: the defaults alone hold a workspace that is too short, which is the last
    check before the device is selected, and every case adds an earlier refusal."""
    lib = E.library()
    p = ctypes.c_void_p(256)                                   # never dereferenced
    defaults = dict(device=0, ppg=p, frames=10, items=2, lengths=p, graphs=1, n_states=3, n_arcs=2, max_states=3,
                    state_begin=p, state_phonemes=p, stay=p, initial=p, final_=p, arc_begin=p, sources=p, weights=p,
                    out_begin=p, targets=p, out_weights=p, which=None, total=p, post=p, occupancy=None, state_stride=0,
                    workspace=p, workspace_bytes=0, stream=None)

    def call(**changes):
        arguments = dict(defaults, **changes)
        code = lib.ppg_posterior(*arguments.values())
        return code, lib.ppg_last_error().decode()
    code, message = call()
    assert code == -1 and 'workspace of 0 bytes' in message
    need = lib.ppg_posterior_workspace_bytes(2, 10, 3)
    code, message = call(workspace_bytes=need - 1)
    assert code == -1 and f'{need} needed' in message
    code, message = call(workspace=ctypes.c_void_p(264), workspace_bytes=need)
    assert code == -1 and '16-byte aligned' in message
    for changes, text in (
            (dict(ppg=None), 'bad argument'), (dict(lengths=None), 'bad argument'), (dict(frames=0), 'bad argument'),
            (dict(items=0), 'bad argument'), (dict(frames=E.POSTERIOR_MAX_FRAMES + 1), 'at most 65536'),
            (dict(items=E.VITERBI_MAX_ITEMS + 1), 'at most 65535'), (dict(workspace=None), 'bad argument'),
            (dict(graphs=0), 'bad argument'), (dict(n_states=0), 'cannot be'), (dict(n_arcs=-1), 'bad argument'),
            (dict(max_states=0), 'bad argument'), (dict(graphs=E.VITERBI_MAX_GRAPHS + 1, n_states=70000), '65535 per call'),
            (dict(max_states=1025), 'at most 1024 per graph'),
            (dict(graphs=4), 'cannot be'), (dict(n_states=4), 'cannot be'), (dict(n_arcs=32769), 'cannot be'),
            (dict(sources=None), 'bad argument'), (dict(weights=None), 'bad argument'),
            (dict(targets=None), 'bad argument'), (dict(out_weights=None), 'bad argument'),
            (dict(state_begin=None), 'bad argument'), (dict(state_phonemes=None), 'bad argument'),
            (dict(stay=None), 'bad argument'), (dict(initial=None), 'bad argument'), (dict(final_=None), 'bad argument'),
            (dict(arc_begin=None), 'bad argument'), (dict(out_begin=None), 'bad argument'),
            (dict(post=None), 'bad argument'), (dict(total=None), '8-byte aligned'),
            (dict(total=ctypes.c_void_p(260)), '8-byte aligned'),
            (dict(occupancy=p, state_stride=2), 'state stride of 2'),
            (dict(which=ctypes.c_void_p(258)), '4-byte aligned'), (dict(occupancy=ctypes.c_void_p(257), state_stride=3),
                                                                   '4-byte aligned'),
            (dict(targets=ctypes.c_void_p(259)), '4-byte aligned')):
        code, message = call(**changes)
        assert code == -1 and text in message, (changes, message)
    # no arcs at all: the arc arrays may be NULL (the short workspace still refuses the call)
    code, message = call(n_arcs=0, sources=None, weights=None, targets=None, out_weights=None)
    assert code == -1 and 'workspace of 0 bytes' in message
