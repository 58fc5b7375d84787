"""ppgs_amd.alignment.search_graph without a GPU: the entry points are declared, exported and bound with matching
argument counts and limits; the workspace helper's layout; every PPG_EINVAL path and every ValueError before a device
is needed; `phrase_graph`; and the tests' own programme (tests/search_graph_reference.py) held against brute force,
against the chain search's reference, on the arc-order tie probe, and against its own mutants."""
import ctypes
import math
import os
import re

import numpy as np
import pytest
import torch

import ppgs_amd
from ppgs_amd import alignment, engine as E

import search_graph_reference as R
import search_reference as S
import viterbi_reference as V

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INF = math.inf


def test_header_declares_library_exports_and_engine_binds_the_entry_points():
    text = open(os.path.join(ROOT, 'include', 'ppgs_amd.h')).read()
    code = re.sub(r'/\*.*?\*/', '', text, flags=re.S)
    for name in ('ppg_search_graph', 'ppg_search_graph_workspace_bytes'):
        declared = re.search(r'\b%s\s*\(([^)]*)\)\s*;' % name, code)
        assert declared, name
        assert name in E.SYMBOLS and hasattr(E.library(), name)
        assert len(declared.group(1).split(',')) == len(E.SYMBOLS[name][1]), name
    assert E.SYMBOLS['ppg_search_graph'][0] is ctypes.c_int and len(E.SYMBOLS['ppg_search_graph'][1]) == 29
    assert E.SYMBOLS['ppg_search_graph_workspace_bytes'][0] is ctypes.c_size_t
    # the graph arguments are ppg_viterbi's, in its order
    viterbi = re.search(r'\bppg_viterbi\s*\(([^)]*)\)\s*;', code).group(1)
    ours = re.search(r'\bppg_search_graph\s*\(([^)]*)\)\s*;', code).group(1)
    packed = re.search(r'int graphs,.*?const float\* weights', viterbi, flags=re.S).group(0)
    assert re.sub(r'\s+', ' ', packed) in re.sub(r'\s+', ' ', ours)

    def limit(name):
        return int(re.search(r'#define\s+PPG_%s\s+(\d+)' % name, code).group(1))
    assert limit('SEARCH_GRAPH_MAX_STATES') == 256 == E.SEARCH_GRAPH_MAX_STATES == alignment.SEARCH_GRAPH_MAX_STATES
    assert limit('SEARCH_GRAPH_MAX_ARCS') == 4096 == E.SEARCH_GRAPH_MAX_ARCS == alignment.SEARCH_GRAPH_MAX_ARCS
    assert limit('SEARCH_MAX_QUERIES') == 65535 == E.SEARCH_GRAPH_MAX_GRAPHS == alignment.SEARCH_GRAPH_MAX_GRAPHS
    assert limit('VITERBI_MAX_DEGREE') == 255 and limit('SEARCH_MAX_FRAMES') == 262144 and limit('SEARCH_MAX_HITS') == 64
    assert alignment.GraphHits._fields == ('begin', 'end', 'total', 'mean', 'count', 'curve')
    assert ppgs_amd.alignment.search_graph is alignment.search_graph


def test_workspace_helper_gives_the_stated_layout_and_zero_outside_the_limits():
    size = E.library().ppg_search_graph_workspace_bytes

    def up(value):
        return (value + 255) // 256 * 256
    for items, frames, graphs in ((1, 1, 1), (1, 57, 1), (3, 301, 5), (64, 1000, 8), (1, 100000, 64), (1, 262144, 1),
                                  (7, 262144, 3), (65535, 4096, 2), (2, 1000, 65535), (65535, 262144, 65535)):
        # the prepared frames once per recording, every pair's totals and begins, a verdict and a one per graph
        expected = up(items * frames * 176) + 2 * up(items * graphs * frames * 4) + 2 * up(graphs * 4)
        assert size(items, frames, graphs) == expected, (items, frames, graphs)
    assert size(65535, 262144, 65535) > 1 << 52                          # never a wrapped number
    for bad in ((0, 10, 5), (-1, 10, 5), (1, 0, 5), (1, 10, 0), (1, -4, 5), (1, 10, -1),
                (E.SEARCH_MAX_ITEMS + 1, 10, 5), (1, E.SEARCH_MAX_FRAMES + 1, 5),
                (1, 10, E.SEARCH_GRAPH_MAX_GRAPHS + 1)):
        assert size(*bad) == 0, bad


ORDER = ('ppg', 'frames', 'items', 'lengths', 'graphs', 'n_states', 'n_arcs', 'max_states', 'state_begin', 'phonemes',
         'stay', 'initial', 'final', 'arc_begin', 'sources', 'weights', 'top', 'threshold', 'begin', 'end', 'total',
         'mean', 'count', 'curve_total', 'curve_begin', 'ws', 'size')
POINTERS = ('ppg', 'lengths', 'state_begin', 'phonemes', 'stay', 'initial', 'final', 'arc_begin', 'sources', 'weights',
            'begin', 'end', 'total', 'mean', 'count', 'ws')


def call_search_graph(lib, **changes):
    dummy = ctypes.c_void_p(256)
    a = dict.fromkeys(POINTERS, dummy)
    a.update(frames=10, items=1, graphs=2, n_states=7, n_arcs=9, max_states=5, top=3, threshold=-1., curve_total=None,
             curve_begin=None, size=lib.ppg_search_graph_workspace_bytes(1, 10, 2))
    a.update(changes)
    return lib.ppg_search_graph(0, *[a[name] for name in ORDER], None)


def test_bad_arguments_return_einval_and_launch_nothing():
    lib = E.library()
    dummy = ctypes.c_void_p(256)
    for name in POINTERS:
        assert call_search_graph(lib, **{name: None}) == -1, name
        if name != 'ws':
            assert call_search_graph(lib, **{name: ctypes.c_void_p(258)}) == -1 and b'aligned' in lib.ppg_last_error()
    assert call_search_graph(lib, ws=ctypes.c_void_p(264)) == -1 and b'aligned' in lib.ppg_last_error()
    for name in ('frames', 'items', 'graphs', 'n_states', 'max_states'):
        assert call_search_graph(lib, **{name: 0}) == -1 and call_search_graph(lib, **{name: -3}) == -1, name
    assert call_search_graph(lib, n_arcs=-1) == -1
    big = dict(size=1 << 52)
    assert call_search_graph(lib, frames=E.SEARCH_MAX_FRAMES + 1, **big) == -1 and b'at most' in lib.ppg_last_error()
    assert call_search_graph(lib, items=E.SEARCH_MAX_ITEMS + 1, **big) == -1 and b'at most' in lib.ppg_last_error()
    assert call_search_graph(lib, graphs=E.SEARCH_GRAPH_MAX_GRAPHS + 1, n_states=1 << 20, **big) == -1
    assert b'at most' in lib.ppg_last_error()
    assert call_search_graph(lib, max_states=E.VITERBI_MAX_STATES + 1) == -1 and b'at most' in lib.ppg_last_error()
    # counts that cannot be: fewer states than graphs, more than graphs * max_states, more arcs than graphs may hold
    assert call_search_graph(lib, n_states=1) == -1 and b'cannot be' in lib.ppg_last_error()
    assert call_search_graph(lib, n_states=11) == -1 and b'cannot be' in lib.ppg_last_error()
    assert call_search_graph(lib, n_arcs=2 * E.VITERBI_MAX_ARCS + 1) == -1 and b'cannot be' in lib.ppg_last_error()
    for top in (0, -1, E.SEARCH_MAX_HITS + 1):
        assert call_search_graph(lib, top=top) == -1 and b'top' in lib.ppg_last_error()
    assert call_search_graph(lib, threshold=math.nan) == -1 and b'NaN' in lib.ppg_last_error()
    assert call_search_graph(lib, curve_total=dummy) == -1 and b'together' in lib.ppg_last_error()
    assert call_search_graph(lib, curve_begin=dummy) == -1 and b'together' in lib.ppg_last_error()
    assert call_search_graph(lib, size=lib.ppg_search_graph_workspace_bytes(1, 10, 2) - 1) == -1
    assert b'workspace' in lib.ppg_last_error()
    assert call_search_graph(lib, items=65535, frames=262144, graphs=65535, n_states=65535, size=1 << 52) == -1
    assert b'workspace' in lib.ppg_last_error()
    if not torch.cuda.is_available():                                    # past every check: no device, said loudly
        assert call_search_graph(lib) == -2 and b'no HIP device' in lib.ppg_last_error()
        assert call_search_graph(lib, n_arcs=0, sources=None, weights=None) == -2     # no arcs: no arc arrays
        assert call_search_graph(lib, curve_total=dummy, curve_begin=dummy, threshold=-math.inf) == -2
        with pytest.raises(E.PpgError):
            alignment.search_graph(torch.rand(40, 5), alignment.chain_graph(['aa', 'b']))
        with pytest.raises(E.PpgError):
            E.search_graph_items(torch.rand(1, 40, 5), [5], [0, 1], [3], [0.], [0.], [0.], [0, 0], [], [])


def test_value_errors_come_before_any_device_call():
    x, bx = torch.rand(40, 5), torch.rand(3, 40, 5)
    chain = alignment.chain_graph(['aa', 'b'])
    wide = alignment.chain_graph([0] * (alignment.SEARCH_GRAPH_MAX_STATES + 1))
    many = alignment.graph([0, 1], [(0, 1, 0.)] * 255 + [(1, 0, 0.)] * 255)          # fine for viterbi ...
    dense = alignment.graph(list(range(20)) * 2, [(p, n, 0.) for n in range(40) for p in range(40) for _ in range(3)])
    assert dense.sources.shape[0] == 4800 > alignment.SEARCH_GRAPH_MAX_ARCS           # ... and this one too
    assert alignment.chain_graph([0] * alignment.SEARCH_GRAPH_MAX_STATES).phonemes.shape[0] == 256
    broken = chain._replace(sources=torch.tensor([5], dtype=torch.int32))
    cases = [
        (torch.rand(39, 5), chain, {}),                                  # channels
        (torch.rand(5), chain, {}),                                      # shape
        (torch.rand(40, 0), chain, {}),                                  # zero frames
        (torch.rand(0, 40, 5), chain, {}),                               # empty batch
        (torch.empty(40, alignment.SEARCH_MAX_FRAMES + 1), chain, {}),   # more than SEARCH_MAX_FRAMES frames
        (x, ['aa', 'b'], {}),                                            # a sequence is not a graph
        (x, [['aa', 'b']], {}),
        (x, [], {}),                                                     # no graph
        (x, None, {}),
        (x, wide, {}),                                                   # 257 states
        (x, [chain, wide], {}),
        (x, dense, {}),                                                  # over 4096 arcs
        (x, broken, {}),                                                 # what viterbi refuses: a source out of range
        (x, chain._replace(stay=torch.tensor([0., math.nan])), {}),
        (x, chain._replace(final=torch.tensor([0., math.inf])), {}),
        (x, chain, {'top': 0}),                                          # top outside 1 .. 64
        (x, chain, {'top': alignment.SEARCH_MAX_HITS + 1}),
        (x, chain, {'top': 1.5}),
        (x, chain, {'top': True}),
        (x, chain, {'threshold': math.nan}),                             # a NaN threshold
        (x, chain, {'lengths': [5]}),                                    # lengths without a batch
        (bx, chain, {'lengths': [5, 5]}),                                # one length per recording
        (bx, chain, {'lengths': [5, 0, 5]}),                             # a length outside [1, padded frames]
        (bx, chain, {'lengths': torch.tensor([5, 6, 5])}),
    ]
    for ppg, graphs, keywords in cases:
        with pytest.raises(ValueError):
            alignment.search_graph(ppg, graphs, **keywords)
    assert many.sources.shape[0] == 510                                  # a legal graph: degree 255 twice


def test_phrase_graph_is_pronunciations_without_the_outer_silences():
    words = [[['iy', 'dh', 'er'], ['ay', 'dh', 'er']], [['w', 'ey'], ['w', 'eh', 'y'], ['ey']], [['t'], ['t', 'ah']]]
    plain, word_of, variant_of = alignment.phrase_graph(words, pauses=False)
    other, other_word, other_variant = alignment.pronunciations(words, silence=False)
    for name in alignment.Graph._fields:
        assert getattr(plain, name).dtype == getattr(other, name).dtype
        assert getattr(plain, name).tolist() == getattr(other, name).tolist(), name
    assert word_of == other_word and variant_of == other_variant
    graph, word_of, variant_of = alignment.phrase_graph(words)
    full, full_word, _ = alignment.pronunciations(words, silence=True)
    quiet = ppgs_amd.PHONEMES.index('<silent>')
    silences = [n for n, word in enumerate(word_of) if word == -1]
    assert len(silences) == len(words) - 1 and all(graph.phonemes[n] == quiet for n in silences)
    assert sum(1 for word in full_word if word == -1) == len(words) + 1
    assert len(word_of) == len(full_word) - 2 and [w for w in word_of if w >= 0] == [w for w in full_word if w >= 0]
    g = V.lists(graph)
    for n in silences:                                                   # each between two words: from one, into the next
        before = {word_of[p] for p, _ in g.into[n]}
        after = {word_of[m] for m in range(len(word_of)) if any(p == n for p, _ in g.into[m])}
        assert len(before) == 1 and after == {before.pop() + 1}
        assert g.initial[n] == -INF and g.final[n] == -INF
    # the path begins in a first state of the first word and ends in a last state of the last
    assert sorted(np.nonzero(g.initial == 0)[0].tolist()) == [0, 3]
    assert all(word_of[n] == len(words) - 1 for n in np.nonzero(g.final == 0)[0])
    assert len(np.nonzero(g.final == 0)[0]) == 2 and set(np.unique(g.final)) == {-INF, 0.}
    # a first state of a later word takes the pause first, then the last states of the word before in variant order
    first = word_of.index(1)
    assert [word_of[p] for p, _ in g.into[first]] == [-1, 0, 0] and [variant_of[p] for p, _ in g.into[first]] == [-1, 0, 1]
    assert alignment.phrase_graph(words, pauses=True)[0].phonemes.tolist() == graph.phonemes.tolist()
    for bad in ([], 'word', [[]], [[[]]], [[['xx']]]):
        with pytest.raises(ValueError):
            alignment.phrase_graph(bad)


def exact_graph(rng, count):
    """A random graph of `count` states whose weights are 0, -1 or -inf: with exact_emissions every sum is exact."""
    def weights(size, open_one=False):
        values = rng.choice([0., -1., -INF], size=size)
        if open_one:
            values[rng.integers(size)] = 0.
        return values
    into = []
    for _ in range(count):
        degree = int(rng.integers(0, 4))
        into.append([(int(rng.integers(count)), float(w)) for w in weights(degree)] if degree else [])
    return V.Lists(np.zeros(count, dtype=np.int64), weights(count), into, weights(count, True), weights(count, True))


def exact_emissions(rng, frames, count):
    return -rng.integers(0, 4, (frames, count)).astype(np.float64)


def test_reference_programme_equals_brute_force_on_every_tiny_case():
    rng = np.random.default_rng(22)
    seen_ties = 0
    for frames in range(1, 7):
        for count in range(1, 5):
            for trial in range(4):
                g = exact_graph(rng, count)
                r = exact_emissions(rng, frames, count) if trial else np.zeros((frames, count))
                total, begin, state, _ = R.programme(r, g)
                single, single_begin, single_state, _ = R.programme(r, g, np.float32)
                assert total.tolist() == single.astype(np.float64).tolist()          # exact sums: fp32 is float64
                assert begin.tolist() == single_begin.tolist() and state.tolist() == single_state.tolist()
                brute = R.brute_force(r, g)
                for t, (best, firsts) in enumerate(brute):
                    assert total[t] == best, (frames, count, t)
                    if best > -INF:
                        assert int(begin[t]) in firsts, (frames, count, t, firsts)   # the begin of SOME optimal path
                        seen_ties += len(firsts) > 1
                    else:
                        assert begin[t] == -1 and state[t] == -1
                # on a fixed span the total is what viterbi maximises there
                again = R.spans(r, g, begin)
                for t in range(frames):
                    if begin[t] >= 0:
                        assert again[t] == total[t]
                        e = r[begin[t]:t + 1]
                        assert V.viterbi(e, g)[0] == total[t]
                    else:
                        assert np.isnan(again[t])
    assert seen_ties > 50                                                # ties were there to be decided


def test_reference_on_a_chain_is_the_chain_search():
    rng = np.random.default_rng(4)
    for frames in (1, 2, 5, 9, 40):
        for count in (1, 2, 3, 7):
            sequence = rng.integers(0, 40, count).tolist()
            g = V.lists(alignment.chain_graph(sequence))
            tables = (exact_emissions(rng, frames, count), np.zeros((frames, count)),
                      np.log(rng.random((frames, count))))
            for index, r in enumerate(tables):
                chain_total, chain_begin = S.programme(r)
                for dtype in (np.float64, np.float32) if index < 2 else (np.float64,):   # fp32 where sums are exact
                    total, begin, state, _ = R.programme(r, g, dtype)
                    assert total.astype(np.float64).tolist() == chain_total.tolist()
                    assert begin.tolist() == chain_begin.tolist()
                    assert ((state == count - 1) | (state == -1)).all()
    # and the emissions are the search's
    logp = S.log_posteriors(torch.rand(40, 6).softmax(0))
    assert R.emissions(logp, [3, 5, 3]).tolist() == S.emissions(logp, [3, 5, 3]).tolist()


def tie_probe(k, first):
    """Three states: a (x, initial 0, stay 0), b (x, initial 0, stay -inf), c (y, final 0) with in-arcs from b and
    from a, the one named `first` listed first; k frames with r = 0 on x, then two on y."""
    arcs = [(1, 2, 0.), (0, 2, 0.)] if first == 'b' else [(0, 2, 0.), (1, 2, 0.)]
    graph = alignment.graph([3, 3, 7], arcs, stay=[0., -INF, 0.], initial=[0., 0., -INF], final=[-INF, -INF, 0.])
    on_x = np.array([0., 0., -5.])
    on_y = np.array([-5., -5., 0.])
    return graph, np.stack([on_x] * k + [on_y] * 2)


def test_arc_order_decides_the_begin_on_the_tie_probe():
    for k in (1, 2, 5):
        for dtype in (np.float64, np.float32):
            graph, r = tie_probe(k, 'b')
            total, begin, _, _ = R.programme(r, V.lists(graph), dtype)
            assert total[k] == 0. and begin[k] == k - 1                  # b is entered fresh every frame: it began at k-1
            graph, r = tie_probe(k, 'a')
            total, begin, _, _ = R.programme(r, V.lists(graph), dtype)
            assert total[k] == 0. and begin[k] == 0                      # a has stayed since frame 0
            assert np.isneginf(total[0]) and begin[0] == -1              # nothing can end in c at frame 0


def test_each_mutant_is_caught_by_its_case():
    # fresh start before the arcs: state a of the tie probe restarts at every frame of a run of zeros
    graph, r = tie_probe(3, 'a')
    g = V.lists(graph)
    assert R.programme(r, g)[1][3] == 0 and R.programme(r, g, mutant='fresh_first')[1][3] == 2
    # >= in place of >: the arc listed LAST wins the tie
    g = V.lists(alignment.chain_graph([3, 7]))
    r = np.zeros((3, 2))
    assert R.programme(r, g)[1].tolist() == [-1, 0, 0] and R.programme(r, g, mutant='not_strict')[1].tolist() != [-1, 0, 0]
    # the highest final state on ties: two final states with equal totals and different begins
    both = alignment.graph([3, 3], [], stay=[0., 0.], initial=[0., 0.], final=[0., 0.])
    r = np.array([[0., -1.], [0., 0.], [0., 0.]])                       # state 1 restarts at frame 1: 0 > -1
    g = V.lists(both)
    good, bad = R.programme(r, g), R.programme(r, g, mutant='highest_final')
    assert good[0].tolist() == bad[0].tolist() == [0., 0., 0.]
    assert good[1].tolist() == [0, 0, 0] and good[2].tolist() == [0, 0, 0]
    assert bad[1].tolist() == [0, 1, 1] and bad[2].tolist() == [0, 1, 1]
    assert set(R.MUTANTS) == {'fresh_first', 'not_strict', 'highest_final'}
