"""The host side of ppgs_amd.alignment.viterbi: the float64 reference of the GPU tests against brute force and against
the references of `forced`, `forced(optional=)` and `recognize` on the graphs where they coincide, the structure of the
graph builders, every refusal raised before a device is touched, and the library's PPG_EINVAL paths (nothing launched)."""
import ctypes
import math
import os
import re

import numpy as np
import pytest
import torch

from ppgs_amd import alignment, engine as E
from ppgs_amd.phonemes import PHONEMES, PHONEME_TO_INDEX_MAPPING

import alignment_optional_reference as O
import alignment_reference as F
import recognize_reference as R
import viterbi_reference as V

INF = math.inf
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def integer_graph(generator, states, holes, loops=True):
    """A random graph on integer weights (every sum and every tie exact): up to 2 arcs per ordered pair of states,
    so parallel arcs and arcs n -> n occur; `holes` is the share of -inf weights."""
    def weight():
        return -INF if float(torch.rand((), generator=generator)) < holes else float(
            torch.randint(-2, 1, (), generator=generator))
    arcs = []
    for target in range(states):
        for source in range(states):
            if source == target and not loops:
                continue
            for _ in range(int(torch.randint(0, 3, (), generator=generator))):
                arcs.append((source, target, weight()))
    order = torch.randperm(len(arcs), generator=generator).tolist()
    return alignment.graph(
        torch.randint(0, 40, (states,), generator=generator).tolist(), [arcs[i] for i in order],
        stay=[weight() for _ in range(states)], initial=[weight() for _ in range(states)],
        final=[weight() for _ in range(states)])


def test_reference_equals_brute_force_in_total_and_path():
    generator = torch.Generator().manual_seed(11)
    seen = {'none': 0, 'path': 0, 'again': 0, 'parallel': 0}
    for states in (1, 2, 3, 4):
        for frames in (1, 2, 3, 5):
            for holes in (0., 0.3, 0.7):
                for _ in range(2 if states >= 3 and frames == 5 else 5):
                    g = V.lists(integer_graph(generator, states, holes))
                    e = torch.randint(-3, 1, (frames, states), generator=generator).double().numpy()
                    total, path, ordinals = V.viterbi(e, g)
                    ref_total, ref_path, ref_ordinals = V.brute_force(e, g)
                    assert total == ref_total, (states, frames, holes)
                    if ref_path is None:
                        assert path is None and total == -INF
                        seen['none'] += 1
                        continue
                    assert path.tolist() == ref_path.tolist() and ordinals.tolist() == ref_ordinals.tolist()
                    assert V.rescore(path, ordinals, e, g) == total
                    again, same, same_ordinals = V.viterbi(e, g, np.float32)      # exact inputs: the same walk in fp32
                    assert again == total and same.tolist() == path.tolist()
                    assert same_ordinals.tolist() == ordinals.tolist()
                    run_states, starts = V.runs(path, ordinals)
                    assert V.best_rescore(run_states, starts, e, g) == total
                    seen['path'] += 1
                    # an arc n -> n on the path opens a run of the state the run before it has
                    seen['again'] += int((run_states[1:] == run_states[:-1]).any())
                    seen['parallel'] += int(any(len({s for s, _ in into}) < len(into) for into in g.into))
    assert seen['none'] >= 5 and seen['path'] >= 100 and seen['again'] >= 5 and seen['parallel'] >= 50, seen


def test_tie_and_run_rules_of_the_reference_by_hand():
    # two states, everything 0: staying wins, the lowest end state wins: one run of state 0
    g = V.lists(alignment.graph([3, 4], [(0, 1, 0.), (1, 0, 0.)]))
    total, path, ordinals = V.viterbi(np.zeros((4, 2)), g)
    assert total == 0. and path.tolist() == [0] * 4 and ordinals.tolist() == [0] * 4
    # staying forbidden, an arc 0 -> 0 allowed: four runs of state 0; of two parallel arcs the one listed first
    g = V.lists(alignment.graph([3], [(0, 0, 0.), (0, 0, 0.)], stay=-INF))
    total, path, ordinals = V.viterbi(np.zeros((4, 1)), g)
    assert total == 0. and ordinals.tolist() == [0, 1, 1, 1]
    run_states, starts = V.runs(path, ordinals)
    assert run_states.tolist() == [0] * 4 and starts.tolist() == [0, 1, 2, 3, 4]
    # the second of two parallel arcs only if strictly better
    g = V.lists(alignment.graph([3], [(0, 0, -1.), (0, 0, 0.)], stay=-INF))
    assert V.viterbi(np.zeros((3, 1)), g)[2].tolist() == [0, 2, 2]
    # no way through: final forbids every state
    g = V.lists(alignment.graph([3, 4], [(0, 1, 0.)], final=-INF))
    assert V.viterbi(np.zeros((3, 2)), g) == (-INF, None, None)
    assert V.brute_force(np.zeros((3, 2)), g) == (-INF, None, None)


def starts_of_chain(run_states, starts, count, frames):
    """The (N + 1,) starts `forced` reports from the runs of a chain: a state not visited starts where the next does."""
    out = np.full(count + 1, frames, dtype=np.int64)
    for n, t in zip(run_states.tolist(), starts.tolist()):
        out[n] = t
    for n in range(count - 1, -1, -1):
        if n not in set(run_states.tolist()):
            out[n] = out[n + 1]
    return out


def test_reference_equals_forced_under_chain_graph():
    generator = torch.Generator().manual_seed(12)
    for count, frames in ((1, 1), (1, 7), (2, 2), (5, 9), (12, 40), (30, 31)):
        for _ in range(4):
            logp = F.log_posteriors(F.random_ppg(frames, 2., generator))
            phonemes = F.random_phonemes(count, generator)
            if count >= 2:
                phonemes[1] = phonemes[0]                      # a phoneme twice: a state is a position
            g = alignment.chain_graph(phonemes)
            total, path, ordinals = V.viterbi(V.emissions(logp, g.phonemes.tolist()), V.lists(g))
            ref_total, ref_starts = F.programme(F.emissions(logp, phonemes))
            run_states, starts = V.runs(path, ordinals)
            assert total == ref_total and run_states.tolist() == list(range(count))
            assert starts.tolist() == ref_starts.tolist()


def test_reference_equals_forced_optional_under_chain_graph():
    generator = torch.Generator().manual_seed(13)
    done = 0
    while done < 60:
        count = int(torch.randint(2, 14, (), generator=generator))
        frames = int(torch.randint(1, 20, (), generator=generator))
        flags = [False] * count
        for n in range(count):
            if float(torch.rand((), generator=generator)) < 0.4 and not (n and flags[n - 1]):
                flags[n] = True
        phonemes = F.random_phonemes(count, generator)
        if not O.legal(flags, frames) or phonemes[-1] == phonemes[-2]:
            continue                                           # (an exact tie of the two end states: see test_gpu_viterbi)
        done += 1
        logp = F.log_posteriors(F.random_ppg(frames, 2., generator))
        g = alignment.chain_graph(phonemes, flags)
        total, path, ordinals = V.viterbi(V.emissions(logp, phonemes), V.lists(g))
        ref_total, ref_starts = O.programme(F.emissions(logp, phonemes), flags)
        run_states, starts = V.runs(path, ordinals)
        assert total == ref_total
        assert starts_of_chain(run_states, starts, count, frames).tolist() == ref_starts.tolist()
        assert all(flags[n] for n in set(range(count)) - set(run_states.tolist()))


def test_reference_equals_recognize_under_model_graph():
    generator = torch.Generator().manual_seed(14)
    for frames in (1, 2, 9, 33):
        for holes in (0., 0.3):
            tables = []
            for shape in ((40, 40), (40,), (40,)):
                table = -5. * torch.rand(shape, generator=generator)
                table[torch.rand(shape, generator=generator) < holes] = -INF
                tables.append(table)
            logp = F.log_posteriors(F.random_ppg(frames, 2., generator))
            g = alignment.model_graph(*tables)
            total, path, ordinals = V.viterbi(V.emissions(logp, range(40)), V.lists(g))
            ref_total, labels = R.viterbi(logp, *[table.double().numpy() for table in tables])
            assert total == ref_total
            if labels is None:
                assert path is None
                continue
            assert path.tolist() == labels.tolist()
            assert V.runs(path, ordinals)[0].tolist() == R.runs(labels)[0].tolist()


def into(g, n):
    a, b = int(g.offsets[n]), int(g.offsets[n + 1])
    return list(zip(g.sources[a:b].tolist(), g.weights[a:b].tolist()))


def test_builders_structure():
    g = alignment.graph(['aa', 'b', 'aa'], [(0, 1, -1.), (2, 1, -2.), (1, 2, 0.), (0, 1, -3.), (1, 1, -4.)],
                        stay=[0., -1., -2.], initial=[0., -INF, -INF])
    assert isinstance(g, alignment.Graph) and all(not tensor.is_cuda for tensor in g)
    assert g.phonemes.tolist() == [PHONEME_TO_INDEX_MAPPING[p] for p in ('aa', 'b', 'aa')]
    assert g.offsets.tolist() == [0, 0, 4, 5] and g.offsets.dtype == g.sources.dtype == g.phonemes.dtype == torch.int32
    assert into(g, 1) == [(0, -1.), (2, -2.), (0, -3.), (1, -4.)] and into(g, 2) == [(1, 0.)]     # listed order
    assert g.stay.tolist() == [0., -1., -2.] and g.final.tolist() == [0., 0., 0.] and g.weights.dtype == torch.float32
    # the chain, plain and with optional phonemes: arcs in the order advance, skip
    g = alignment.chain_graph(['sh', 'sh', 'iy'])
    assert [into(g, n) for n in range(3)] == [[], [(0, 0.)], [(1, 0.)]]
    assert g.initial.tolist() == [0., -INF, -INF] and g.final.tolist() == [-INF, -INF, 0.]
    g = alignment.chain_graph(['<silent>', 'sh', 'iy', '<silent>'], [True, False, False, True])
    assert [into(g, n) for n in range(4)] == [[], [(0, 0.)], [(1, 0.)], [(2, 0.)]]    # the ends skip by initial, final
    assert g.initial.tolist() == [0., 0., -INF, -INF] and g.final.tolist() == [-INF, -INF, 0., 0.]
    g = alignment.chain_graph(['sh', 'ah', 'iy'], [False, True, False])
    assert into(g, 2) == [(1, 0.), (0, 0.)]
    # the model: 40 states, the diagonal stays, the others in ascending p
    A = torch.arange(1600, dtype=torch.float32).reshape(40, 40).neg()
    g = alignment.model_graph(A, final=torch.full((40,), -1.))
    assert g.phonemes.tolist() == list(range(40)) and g.stay.tolist() == A.diagonal().tolist()
    assert into(g, 7) == [(p, float(A[p, 7])) for p in range(40) if p != 7]
    assert g.initial.tolist() == [0.] * 40 and g.final.tolist() == [-1.] * 40


def test_pronunciations_and_word_loop_structure():
    words = [[['dh', 'ah'], ['dh', 'iy']], [['k', 'ae', 't']]]
    g, word_of, variant_of = alignment.pronunciations(words)
    names = [PHONEMES[p] for p in g.phonemes.tolist()]
    assert names == ['<silent>', 'dh', 'ah', 'dh', 'iy', '<silent>', 'k', 'ae', 't', '<silent>']
    assert word_of == [-1, 0, 0, 0, 0, -1, 1, 1, 1, -1] and variant_of == [-1, 0, 0, 1, 1, -1, 0, 0, 0, -1]
    assert into(g, 1) == [(0, 0.)] and into(g, 3) == [(0, 0.)] and into(g, 2) == [(1, 0.)]
    assert into(g, 5) == [(2, 0.), (4, 0.)]                    # the pause between the words: from both variants' ends
    assert into(g, 6) == [(5, 0.), (2, 0.), (4, 0.)]           # the pause first, then the ends in variant order
    assert into(g, 9) == [(8, 0.)]
    assert [n for n in range(10) if g.initial[n] == 0] == [0, 1, 3] and [n for n in range(10) if g.final[n] == 0] == [8, 9]
    assert set(g.initial.tolist()) == set(g.final.tolist()) == {0., -INF} and not g.stay.any() and not g.weights.any()
    bare, word_of, variant_of = alignment.pronunciations(words, silence=False)
    assert word_of == [0, 0, 0, 0, 1, 1, 1] and into(bare, 4) == [(1, 0.), (3, 0.)] and into(bare, 0) == []
    # one variant per word with silences is the transcript's chain with its optional flags
    phonemes, optional, chain_words = alignment.transcript([['hh', 'ah'], ['l', 'ow']])
    g, word_of, _ = alignment.pronunciations([[['hh', 'ah']], [['l', 'ow']]])
    chain = alignment.chain_graph(phonemes, optional)
    assert word_of == chain_words and all(torch.equal(a, b) for a, b in zip(g, chain))
    # the word loop
    lexicon = {'yes': [['y', 'eh', 's']], 'no': [['n', 'ow'], ['n', 'ah']], 'a': [['ah']]}
    g, word_of = alignment.word_loop(lexicon, penalty=2.)
    assert [PHONEMES[p] for p in g.phonemes.tolist()] == ['<silent>', 'y', 'eh', 's', 'n', 'ow', 'n', 'ah', 'ah']
    assert word_of == [-1, 0, 0, 0, 1, 1, 1, 1, 2]
    ends = [3, 5, 7, 8]
    assert into(g, 0) == [(n, 0.) for n in ends]
    for first in (1, 4, 6, 8):
        assert into(g, first) == [(0, -2.)] + [(n, -2.) for n in ends]
        assert g.initial[first] == -2.
    assert into(g, 2) == [(1, 0.)] and g.initial[0] == 0. and g.initial[2] == -INF
    assert [n for n in range(9) if g.final[n] == 0] == [0] + ends
    bare, word_of = alignment.word_loop(list(lexicon.items()), silence=False)
    assert word_of == [0, 0, 0, 1, 1, 1, 1, 2] and into(bare, 0) == [(2, 0.), (4, 0.), (6, 0.), (7, 0.)]


def test_word_loop_refuses_beyond_the_degree_and_arc_limits():
    def lexicon(words):
        return [(f'w{n}', [[n % 39, (n // 39) % 39]]) for n in range(words)]
    with pytest.raises(ValueError, match='255 word ends.*at most 254 are allowed'):
        alignment.word_loop(lexicon(255))
    with pytest.raises(ValueError, match='256 word ends.*at most 255 are allowed'):
        alignment.word_loop(lexicon(256), silence=False)
    with pytest.raises(ValueError, match='arcs, at most 32768'):
        alignment.word_loop(lexicon(200))                      # 200 ends x 201 entering arcs
    with pytest.raises(ValueError, match='states, at most 1024'):
        alignment.word_loop([(n, [[1] * 11]) for n in range(100)])
    g, word_of = alignment.word_loop(lexicon(170))
    degrees = (g.offsets[1:] - g.offsets[:-1]).tolist()
    assert max(degrees) == 171 and degrees.count(171) == 170 and degrees[0] == 170 and len(word_of) == 341
    assert int(g.offsets[-1]) <= alignment.VITERBI_MAX_ARCS


def test_graph_refusals_name_the_state():
    ok = [(0, 1, 0.)]
    for arguments, message in (
            ((['aa', 'zz'], ok), 'unknown phoneme'),
            (([0, 40], ok), 'phoneme index 40'),
            (([], []), '1 to 1024 states'),
            (([0] * 1025, []), '1 to 1024 states'),
            (([0, 1], [(0, 2, 0.)]), 'arc 0: the target 2'),
            (([0, 1], [(0, 1, 0.), (-1, 1, 0.)]), 'arc 1: the source -1'),
            (([0, 1], [(0, 1.0, 0.)]), 'the target 1.0'),
            (([0, 1], [(0, 1)]), 'arc 0 must be'),
            (([0, 1], [(0, 1, math.nan)]), 'arc 0 into state 1.*finite or -inf'),
            (([0, 1], [(0, 1, INF)]), 'arc 0 into state 1.*finite or -inf'),
            (([0, 1], [(0, 1, 'x')]), 'a weight must be a number'),
            (([0, 1], 'arcs'), 'arcs must be a list'),
            (([0, 1], [(0, 1, 0.)] * 256), 'state 1 has 256 arcs coming in, at most 255')):
        with pytest.raises(ValueError, match=message):
            alignment.graph(*arguments)
    for keyword in ('stay', 'initial', 'final'):
        with pytest.raises(ValueError, match=f'{keyword} of state 1'):
            alignment.graph([0, 1], ok, **{keyword: [0., math.nan]})
        with pytest.raises(ValueError, match=f'{keyword} must be a number or hold one weight per state'):
            alignment.graph([0, 1], ok, **{keyword: [0.]})
        with pytest.raises(ValueError, match=keyword):
            alignment.graph([0, 1], ok, **{keyword: INF})
    many = [(n % 1024, (n // 255) % 1024, 0.) for n in range(32769)]
    with pytest.raises(ValueError, match='at most 32768 arcs, got 32769'):
        alignment.graph([0] * 1024, many)
    assert int(alignment.graph([0] * 1024, many[:-1]).offsets[-1]) == 32768
    assert int(alignment.graph([0, 1], [(0, 1, -INF)] * 255).offsets[-1]) == 255      # the limits themselves are fine


def test_builder_refusals():
    with pytest.raises(ValueError, match='1 to 1024 phonemes'):
        alignment.chain_graph([])
    with pytest.raises(ValueError, match='1 to 1024 phonemes'):
        alignment.chain_graph([0] * 1025)
    with pytest.raises(ValueError, match='two adjacent'):
        alignment.chain_graph([0, 1, 2], [True, True, False])
    with pytest.raises(ValueError, match='every phoneme is optional'):
        alignment.chain_graph([0], [True])
    with pytest.raises(ValueError, match='2 flags for 3 phonemes'):
        alignment.chain_graph([0, 1, 2], [True, False])
    with pytest.raises(ValueError, match='transitions must be'):
        alignment.model_graph(torch.zeros(40, 39))
    with pytest.raises(ValueError, match='NaN or \\+inf'):
        alignment.model_graph(torch.full((40, 40), math.nan))
    with pytest.raises(ValueError, match='final must be'):
        alignment.model_graph(torch.zeros(40, 40), final=torch.zeros(39))
    for words in ([], 'word', [[]], [['dh', 'ah']], [[[]]], [[['zz']]]):
        with pytest.raises(ValueError):
            alignment.pronunciations(words)
    with pytest.raises(ValueError, match='1 to 1024 states'):
        alignment.pronunciations([[[1] * 600]] * 2)
    for lexicon in ({}, [], 'words', [('a',)], {'a': []}, {'a': [[]]}, {'a': ['ah']}):
        with pytest.raises(ValueError):
            alignment.word_loop(lexicon)
    for penalty in (-1., math.nan, INF, True, 'x'):
        with pytest.raises(ValueError, match='penalty'):
            alignment.word_loop({'a': [['ah']]}, penalty=penalty)


def test_viterbi_argument_checks_need_no_device():
    ppg = torch.full((40, 10), 1 / 40)
    g = alignment.chain_graph([1, 2])
    for arguments, message in (
            ((torch.zeros(39, 10), g), '40 channels'),
            ((torch.zeros(40, 0), g), 'at least one frame'),
            ((torch.zeros(40, 1).expand(40, alignment.VITERBI_MAX_FRAMES + 1), g), 'at most 262144 frames'),
            ((ppg, (1, 2)), 'a list of graphs goes with a batch'),
            ((ppg, [g]), 'a list of graphs goes with a batch'),
            ((ppg, 'graph'), 'viterbi takes a Graph'),
            ((ppg, None), 'viterbi takes a Graph'),
            ((ppg[None].expand(2, 40, 10), [g]), 'got 1 for 2'),
            ((ppg[None].expand(2, 40, 10), [g, 'x']), 'viterbi takes a Graph')):
        with pytest.raises(ValueError, match=message):
            alignment.viterbi(*arguments)
    with pytest.raises(ValueError, match='lengths go with a batch'):
        alignment.viterbi(ppg, g, lengths=[10])
    with pytest.raises(ValueError, match='outside'):
        alignment.viterbi(ppg[None], g, lengths=[11])
    # a Graph made by hand is checked as the device would check it
    for field, value, message in (
            ('phonemes', torch.tensor([1, 40], dtype=torch.int32), 'phoneme index'),
            ('phonemes', torch.tensor([1., 2.]), 'integer tensor'),
            ('sources', torch.tensor([2], dtype=torch.int32), 'a source of the graph'),
            ('sources', torch.tensor([-1], dtype=torch.int32), 'a source of the graph'),
            ('offsets', torch.tensor([0, 1, 0], dtype=torch.int32), 'offsets must rise'),
            ('offsets', torch.tensor([0, 0, 2], dtype=torch.int32), 'offsets must rise'),
            ('offsets', torch.tensor([0, 1], dtype=torch.int32), 'Graph.offsets has 2 entries, 3 expected'),
            ('weights', torch.tensor([math.nan]), 'Graph.weights must hold weights'),
            ('weights', torch.tensor([0., 0.]), 'Graph.weights has 2 entries'),
            ('stay', torch.tensor([0., INF]), 'Graph.stay must hold weights'),
            ('initial', torch.tensor([0.]), 'Graph.initial has 1 entries'),
            ('final', torch.tensor([[0., 0.]]), 'one-dimensional CPU tensor'),
            ('final', [0., 0.], 'one-dimensional CPU tensor')):
        with pytest.raises(ValueError, match=message):
            alignment.viterbi(ppg, g._replace(**{field: value}))
    wide = alignment.Graph(torch.zeros(2, dtype=torch.int32), torch.zeros(2), torch.tensor([0, 0, 256], dtype=torch.int32),
                           torch.zeros(256, dtype=torch.int32), torch.zeros(256), torch.zeros(2), torch.zeros(2))
    with pytest.raises(ValueError, match='state 1 has 256 arcs coming in'):
        alignment.viterbi(ppg, wide)
    if not torch.cuda.is_available():
        with pytest.raises(E.PpgError):                        # a missing device is an error, not a CPU path
            alignment.viterbi(ppg, g)


def test_abi_declares_and_binds_the_entries():
    text = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'ppgs_amd.h')).read(), flags=re.S)
    for name in ('ppg_viterbi_workspace_bytes', 'ppg_viterbi'):
        declared = re.search(r'\b%s\s*\(([^)]*)\)' % name, text)
        assert declared, name
        assert name in E.SYMBOLS and hasattr(E.library(), name)
        assert len(declared.group(1).split(',')) == len(E.SYMBOLS[name][1]), name
    assert E.SYMBOLS['ppg_viterbi'][0] is ctypes.c_int and len(E.SYMBOLS['ppg_viterbi'][1]) == 28
    for name, value in (('STATES', 1024), ('ARCS', 32768), ('DEGREE', 255), ('FRAMES', 262144), ('ITEMS', 65535),
                        ('GRAPHS', 65535)):
        assert getattr(E, f'VITERBI_MAX_{name}') == value
        assert re.search(r'#define\s+PPG_VITERBI_MAX_%s\s+%d\b' % (name, value), text), name


def test_workspace_bytes_is_host_only_and_refuses_impossible_sizes():
    size = E.library().ppg_viterbi_workspace_bytes
    for items, frames, states in ((0, 10, 10), (10, 0, 10), (10, 10, 0), (-1, 10, 10), (E.VITERBI_MAX_ITEMS + 1, 10, 10),
                                  (1, E.VITERBI_MAX_FRAMES + 1, 10), (1, 10, E.VITERBI_MAX_STATES + 1)):
        assert size(items, frames, states) == 0
    assert size(1, 1, 1) > 0
    # prepared frames, a back-pointer byte per state and frame, a label per frame
    assert size(3, 100, 64) >= 3 * 100 * (176 + 64 + 4) and size(3, 100, 65) >= 3 * 100 * (176 + 256 + 4)
    assert size(3, 100, 64) < size(3, 100, 65) == size(3, 100, 256) < size(3, 100, 257) < size(3, 100, 1024)
    assert size(E.VITERBI_MAX_ITEMS, E.VITERBI_MAX_FRAMES, 1024) >= 65535 * 262144 * (176 + 1024 + 4)


def test_library_einval_paths_launch_nothing():
    """Every call here is refused on the host: the defaults alone hold a workspace that is too short, which is the last
    check before the device is selected, and every case adds an earlier refusal."""
    lib = E.library()
    p = ctypes.c_void_p(256)                                   # never dereferenced
    defaults = dict(device=0, ppg=p, frames=10, items=2, lengths=p, graphs=1, n_states=3, n_arcs=2, max_states=3,
                    state_begin=p, state_phonemes=p, stay=p, initial=p, final_=p, arc_begin=p, sources=p, weights=p,
                    which=None, states=p, phonemes=p, starts=p, runs=p, total=p, score=p, gop=None, workspace=p,
                    workspace_bytes=0, stream=None)

    def call(**changes):
        arguments = dict(defaults, **changes)
        code = lib.ppg_viterbi(*arguments.values())
        return code, lib.ppg_last_error().decode()
    code, message = call()
    assert code == -1 and 'workspace of 0 bytes' in message
    need = lib.ppg_viterbi_workspace_bytes(2, 10, 3)
    code, message = call(workspace_bytes=need - 1)
    assert code == -1 and f'{need} needed' in message
    code, message = call(workspace=ctypes.c_void_p(264), workspace_bytes=need)
    assert code == -1 and '16-byte aligned' in message
    for changes, text in (
            (dict(ppg=None), 'bad argument'), (dict(lengths=None), 'bad argument'), (dict(frames=0), 'bad argument'),
            (dict(items=0), 'bad argument'), (dict(frames=E.VITERBI_MAX_FRAMES + 1), 'at most 262144'),
            (dict(items=E.VITERBI_MAX_ITEMS + 1), 'at most 65535'), (dict(workspace=None), 'bad argument'),
            (dict(graphs=0), 'bad argument'), (dict(n_states=0), 'bad argument'), (dict(n_arcs=-1), 'bad argument'),
            (dict(max_states=0), 'bad argument'), (dict(graphs=E.VITERBI_MAX_GRAPHS + 1, n_states=70000), '65535 per call'),
            (dict(max_states=1025), 'at most 1024 per graph'),
            (dict(graphs=4), 'cannot be'), (dict(n_states=4), 'cannot be'), (dict(n_arcs=32769), 'cannot be'),
            (dict(sources=None), 'bad argument'), (dict(weights=None), 'bad argument'),
            (dict(state_begin=None), 'bad argument'), (dict(state_phonemes=None), 'bad argument'),
            (dict(stay=None), 'bad argument'), (dict(initial=None), 'bad argument'), (dict(final_=None), 'bad argument'),
            (dict(arc_begin=None), 'bad argument'), (dict(states=None), 'bad argument'),
            (dict(phonemes=None), 'bad argument'), (dict(starts=None), 'bad argument'), (dict(runs=None), 'bad argument'),
            (dict(total=None), 'bad argument'), (dict(score=None), 'bad argument'),
            (dict(which=ctypes.c_void_p(258)), '4-byte aligned'), (dict(gop=ctypes.c_void_p(257)), '4-byte aligned'),
            (dict(sources=ctypes.c_void_p(259)), '4-byte aligned')):
        code, message = call(**changes)
        assert code == -1 and text in message, (changes, message)
    # no arcs at all: sources and weights may be NULL (the short workspace still refuses the call)
    code, message = call(n_arcs=0, sources=None, weights=None)
    assert code == -1 and 'workspace of 0 bytes' in message
