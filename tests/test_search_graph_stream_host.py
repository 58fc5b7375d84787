"""ppgs_amd.alignment.SearchGraphStream without a GPU.  The reference is the float32 programme of
tests/search_graph_reference.py feeding the detector of tests/search_stream_reference.py: its events over random small
graphs are disjoint, ordered, the same under any split into pushes and at most F // Lmin + 2 per push, and on a chain
they are those of the chain search's curve.  Then the search for Lmin on graphs made by hand, the new entry points
declared, exported and bound with matching argument counts, the two size helpers, every argument error of the library
before a device is needed, and every ValueError of SearchGraphStream before any device call."""
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
import search_stream_reference as L
import viterbi_reference as V

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ('ppg_search_graph_stream_state_bytes', 'ppg_search_graph_stream_workspace_bytes',
         'ppg_search_graph_stream_open', 'ppg_search_graph_stream_reset', 'ppg_search_graph_stream_push',
         'ppg_search_graph_stream_flush')
INF = math.inf
QUIET = ppgs_amd.PHONEMES.index('<silent>')


def random_splits(rng, frames):
    cuts = np.sort(rng.integers(0, frames + 1, rng.integers(0, 12)))
    return np.diff(np.concatenate([[0], cuts, [frames]])).tolist()       # empty pushes included


def random_graph(rng, count):
    """`count` <= 6 states, every weight from {0, -1, -inf}: a backbone that is mostly open, arcs from anywhere
    (self-arcs and parallel arcs among them), several places to begin and to end, sometimes none."""
    def weight(closed):
        return -INF if rng.random() < closed else float(-rng.integers(0, 2))
    arcs = []
    for n in range(count):
        if n:
            arcs.append((n - 1, n, weight(0.15)))
        for _ in range(int(rng.integers(0, 3))):
            arcs.append((int(rng.integers(0, count)), n, weight(0.3)))
    return alignment.graph([0] * count, arcs, stay=[weight(0.2) for _ in range(count)],
                           initial=[weight(0.1 if n == 0 else 0.7) for n in range(count)],
                           final=[weight(0.1 if n == count - 1 else 0.7) for n in range(count)])


def emissions(rng, frames, count):
    """Emissions with exact zeros (the state's phoneme is the frame's best) and with ties."""
    return np.where(rng.random((frames, count)) < 0.45, 0., -rng.integers(1, 9, (frames, count)) / 2.)


def test_reference_events_over_random_graphs_are_disjoint_ordered_split_free_and_within_cap():
    rng = np.random.default_rng(423)
    cases = emitted = 0
    for frames, count in ((1, 1), (7, 1), (40, 2), (200, 1), (9, 2), (64, 3), (200, 2), (33, 3), (150, 4), (97, 5),
                          (5, 6), (200, 6)):
        for _ in range(25):
            graph = random_graph(rng, count)
            shortest = alignment.shortest_match(graph)
            assert 1 <= shortest <= count
            total, begin, _, _ = R.programme(emissions(rng, frames, count), V.lists(graph), dtype=np.float32)
            assert total.dtype == np.float32
            threshold = (-np.inf, -3., -1., -0.3)[int(rng.integers(0, 4))]
            patience = int(rng.integers(0, 31))
            whole = L.detect(total, begin, threshold, patience)
            events = L.flat(whole)
            assert len(whole[0]) <= frames // shortest + 2               # the reference alone stays within cap
            # disjoint, in stream order, every one a candidate of its end frame that spans at least Lmin frames
            assert all(0 <= b < e <= frames and e - b >= shortest for b, e, _, _ in events)
            assert all(first[1] <= second[0] for first, second in zip(events, events[1:]))
            for b, e, value, mean in events:
                assert begin[e - 1] == b and value == total[e - 1] and mean >= np.float32(threshold)
                assert mean == value / np.float32(e - b)
            for pushes in ([1] * frames, random_splits(rng, frames), random_splits(rng, frames)):
                split = L.detect(total, begin, threshold, patience, pushes)
                assert L.flat(split) == events, (frames, count, pushes)
                for size, given in zip(pushes, split):
                    assert len(given) <= size // shortest + 2, (frames, count, pushes, shortest)
                assert len(split[-1]) <= 1
            cases += 1
            emitted += len(events)
    assert cases == 300 and emitted > 1000


def test_reference_events_on_a_chain_are_those_of_the_chain_search():
    rng = np.random.default_rng(7)
    for frames, count in ((1, 1), (40, 1), (64, 2), (200, 3), (97, 4), (200, 6)):
        chain = alignment.chain_graph([0] * count)
        assert alignment.shortest_match(chain) == count
        for _ in range(5):
            r = emissions(rng, frames, count)
            total, begin, _, _ = R.programme(r, V.lists(chain), dtype=np.float32)
            chain_total, chain_begin = S.programme(r[None])
            assert np.array_equal(total, chain_total[0].astype(np.float32)) and np.array_equal(begin, chain_begin[0])
            for threshold, patience in ((-np.inf, 0), (-1., 7), (-0.3, 25)):
                pushes = random_splits(rng, frames)
                assert (L.detect(total, begin, threshold, patience, pushes) ==
                        L.detect(chain_total[0].astype(np.float32), chain_begin[0], threshold, patience, pushes))


def test_shortest_match_on_graphs_made_by_hand():
    assert alignment.shortest_match(alignment.chain_graph([3])) == 1
    assert alignment.shortest_match(alignment.chain_graph([3, 4, 5, 6, 7])) == 5
    # optional states at both ends and in the middle: 7 states, 4 of them mandatory
    assert alignment.shortest_match(alignment.chain_graph(
        [QUIET, 3, 3, QUIET, 9, 4, QUIET], optional=[True, False, False, True, False, False, True])) == 4
    # a phrase of 3 + 2 phonemes with a pause between the words that may be skipped, and the same without pauses
    words = [[['iy', 'dh', 'er'], ['ay', 'dh', 'er']], [['w', 'ey'], ['w', 'eh', 'y']]]
    with_pauses = alignment.phrase_graph(words)[0]
    assert with_pauses.phonemes.shape[0] == alignment.phrase_graph(words, pauses=False)[0].phonemes.shape[0] + 1
    assert alignment.shortest_match(with_pauses) == 5
    assert alignment.shortest_match(alignment.phrase_graph(words, pauses=False)[0]) == 5
    # the shorter way round is closed by a weight of -inf; staying adds nothing
    open_skip = alignment.graph([1, 2, 3], [(0, 1, 0.), (1, 2, 0.), (0, 2, -1.)], initial=[0., -INF, -INF],
                                final=[-INF, -INF, 0.])
    shut_skip = alignment.graph([1, 2, 3], [(0, 1, 0.), (1, 2, 0.), (0, 2, -INF)], initial=[0., -INF, -INF],
                                final=[-INF, -INF, 0.])
    assert alignment.shortest_match(open_skip) == 2 and alignment.shortest_match(shut_skip) == 3
    # a state that may both begin and end a match
    assert alignment.shortest_match(alignment.graph([1, 2], [(0, 1, 0.)])) == 1
    # no path from a beginning to an end: the final state is unreachable, or nothing may begin
    unreachable = alignment.graph([1, 2, 3], [(0, 1, 0.)], initial=[0., -INF, -INF], final=[-INF, -INF, 0.])
    nowhere = alignment.graph([1, 2], [(0, 1, 0.)], initial=[-INF, -INF], final=[-INF, 0.])
    assert alignment.shortest_match(unreachable) == 1 and alignment.shortest_match(nowhere) == 1
    total, begin, _, _ = R.programme(np.zeros((20, 3)), V.lists(unreachable), dtype=np.float32)
    assert np.isneginf(total).all() and (begin == -1).all()              # and it never emits anything
    # the least over the graphs of a spotter
    spotter = alignment.SearchGraphStream([alignment.chain_graph([3, 4, 5]), open_skip, unreachable], -1.)
    assert spotter._shortest == 1
    assert alignment.SearchGraphStream([alignment.chain_graph([3, 4, 5]), shut_skip], -1.)._shortest == 3


def test_header_declares_library_exports_and_engine_binds_the_entry_points():
    text = open(os.path.join(ROOT, 'include', 'ppgs_amd.h')).read()
    code = re.sub(r'/\*.*?\*/', '', text, flags=re.S)
    for name in NAMES:
        declared = re.search(r'\b%s\s*\(([^)]*)\)\s*;' % name, code)
        assert declared, name
        assert name in E.SYMBOLS and hasattr(E.library(), name)
        assert len(declared.group(1).split(',')) == len(E.SYMBOLS[name][1]), name
    assert [len(E.SYMBOLS[name][1]) for name in NAMES] == [3, 3, 16, 7, 31, 12]
    assert E.SYMBOLS[NAMES[0]][0] is ctypes.c_size_t and E.SYMBOLS[NAMES[1]][0] is ctypes.c_size_t
    assert all(E.SYMBOLS[name][0] is ctypes.c_int for name in NAMES[2:])
    push = E.SYMBOLS['ppg_search_graph_stream_push'][1]
    assert push[18] is ctypes.c_float and [k for k, kind in enumerate(push) if kind is ctypes.c_float] == [18]
    assert push[29] is ctypes.c_size_t
    assert ppgs_amd.alignment.SearchGraphStream is alignment.SearchGraphStream
    assert issubclass(alignment.SearchGraphStream, alignment.SearchStream)  # the rule and the pushes are written once
    for name in ('search_graph_stream_state', 'search_graph_stream_open', 'search_graph_stream_reset',
                 'search_graph_stream_push', 'search_graph_stream_flush'):
        assert callable(getattr(E, name)), name


def test_size_helpers_give_the_stated_layout_and_zero_outside_the_limits():
    state = E.library().ppg_search_graph_stream_state_bytes
    workspace = E.library().ppg_search_graph_stream_workspace_bytes

    def up(value):
        return (value + 255) // 256 * 256
    for streams, graphs, most in ((1, 1, 1), (1, 1, 64), (1, 1, 65), (3, 5, 70), (64, 8, 8), (1, 64, 256), (2, 3, 1024),
                                  (65535, 65535, 256), (65535, 65535, 64)):
        # positions, verdicts, the detectors (8 words per pair), then D and b: a whole row per pair
        row = 64 if most <= 64 else 256
        expected = (up(streams * 4) + up(graphs * 4) + up(streams * graphs * 32) +
                    2 * up(streams * graphs * row * 4))
        assert state(streams, graphs, most) == expected, (streams, graphs, most)
    assert state(65535, 65535, 256) > 1 << 42                            # never a wrapped number: 8.9e12 bytes
    for bad in ((0, 1, 1), (1, 0, 1), (1, 1, 0), (-1, 1, 1), (1, -2, 1), (1, 1, -3), (E.SEARCH_MAX_ITEMS + 1, 1, 1),
                (1, E.SEARCH_GRAPH_MAX_GRAPHS + 1, 1), (1, 1, E.VITERBI_MAX_STATES + 1)):
        assert state(*bad) == 0, bad
    for streams, frames, graphs in ((1, 1, 1), (1, 16, 1), (64, 16, 8), (1, 1000, 64), (3, 64, 5), (65535, 262144, 1)):
        assert workspace(streams, frames, graphs) == up(streams * frames * 176), (streams, frames, graphs)
    for bad in ((0, 16, 1), (1, 0, 1), (1, 16, 0), (-1, 16, 1), (1, -16, 1), (1, 16, -1), (E.SEARCH_MAX_ITEMS + 1, 16, 1),
                (1, E.SEARCH_MAX_FRAMES + 1, 1), (1, 16, E.SEARCH_GRAPH_MAX_GRAPHS + 1)):
        assert workspace(*bad) == 0, bad


GRAPH_ARGUMENTS = ('state_begin', 'phonemes', 'stay', 'initial', 'final', 'arc_begin', 'sources', 'weights')


def arguments(lib, **changes):
    dummy = ctypes.c_void_p(256)
    a = dict(state=dummy, ppg=dummy, frames=16, streams=1, lengths=dummy, graphs=2, n_states=7, n_arcs=5, max_states=4,
             threshold=-1., patience=25, cap=6, begin=dummy, end=dummy, total=dummy, mean=dummy, count=dummy,
             curve_total=None, curve_begin=None, ws=dummy, size=lib.ppg_search_graph_stream_workspace_bytes(1, 16, 2),
             which=None)
    a.update({name: dummy for name in GRAPH_ARGUMENTS})
    a.update(changes)
    return a


def call_push(lib, **changes):
    a = arguments(lib, **changes)
    return lib.ppg_search_graph_stream_push(
        0, a['state'], a['ppg'], a['frames'], a['streams'], a['lengths'], a['graphs'], a['n_states'], a['n_arcs'],
        a['max_states'], *[a[name] for name in GRAPH_ARGUMENTS], a['threshold'], a['patience'], a['cap'], a['begin'],
        a['end'], a['total'], a['mean'], a['count'], a['curve_total'], a['curve_begin'], a['ws'], a['size'], None)


def call_open(lib, **changes):
    a = arguments(lib, **changes)
    return lib.ppg_search_graph_stream_open(0, a['state'], a['streams'], a['graphs'], a['n_states'], a['n_arcs'],
                                            a['max_states'], *[a[name] for name in GRAPH_ARGUMENTS], None)


def call_reset(lib, **changes):
    a = arguments(lib, **changes)
    return lib.ppg_search_graph_stream_reset(0, a['state'], a['streams'], a['graphs'], a['max_states'], a['which'], None)


def call_flush(lib, **changes):
    a = arguments(lib, **changes)
    return lib.ppg_search_graph_stream_flush(0, a['state'], a['streams'], a['graphs'], a['max_states'], a['which'],
                                             a['begin'], a['end'], a['total'], a['mean'], a['count'], None)


def test_bad_arguments_return_einval():
    lib = E.library()
    dummy, odd, skew = ctypes.c_void_p(256), ctypes.c_void_p(258), ctypes.c_void_p(264)
    required = ('state_begin', 'phonemes', 'stay', 'initial', 'final', 'arc_begin')
    # push: what ppg_search_stream_push refuses ...
    for name in ('state', 'ppg', 'lengths', 'begin', 'end', 'total', 'mean', 'count', 'ws') + required:
        assert call_push(lib, **{name: None}) == -1, name
    for name in ('frames', 'streams', 'graphs', 'max_states', 'n_states'):
        assert call_push(lib, **{name: 0}) == -1 and call_push(lib, **{name: -3}) == -1, name
    assert call_push(lib, frames=E.SEARCH_MAX_FRAMES + 1, size=1 << 40) == -1 and b'at most' in lib.ppg_last_error()
    assert call_push(lib, streams=E.SEARCH_MAX_ITEMS + 1, size=1 << 50) == -1 and b'at most' in lib.ppg_last_error()
    assert call_push(lib, graphs=E.SEARCH_GRAPH_MAX_GRAPHS + 1, n_states=1 << 20) == -1
    assert b'at most' in lib.ppg_last_error()
    assert call_push(lib, threshold=math.nan) == -1 and b'NaN' in lib.ppg_last_error()
    assert call_push(lib, patience=-1) == -1 and b'patience' in lib.ppg_last_error()
    for cap in (0, -1):
        assert call_push(lib, cap=cap) == -1 and b'cap' in lib.ppg_last_error()
    assert call_push(lib, curve_total=dummy) == -1 and b'together' in lib.ppg_last_error()
    assert call_push(lib, curve_begin=dummy) == -1 and b'together' in lib.ppg_last_error()
    assert call_push(lib, size=lib.ppg_search_graph_stream_workspace_bytes(1, 16, 2) - 1) == -1
    assert b'workspace' in lib.ppg_last_error()
    assert call_push(lib, ws=skew) == -1 and b'aligned' in lib.ppg_last_error()
    assert call_push(lib, state=skew) == -1 and b'aligned' in lib.ppg_last_error()
    # ... and what ppg_search_graph refuses
    assert call_push(lib, max_states=E.VITERBI_MAX_STATES + 1) == -1 and b'at most' in lib.ppg_last_error()
    assert call_push(lib, n_states=1) == -1 and b'cannot be' in lib.ppg_last_error()      # fewer states than graphs
    assert call_push(lib, n_states=9) == -1 and b'cannot be' in lib.ppg_last_error()      # more than graphs * max_states
    assert call_push(lib, n_arcs=2 * E.VITERBI_MAX_ARCS + 1) == -1 and b'cannot be' in lib.ppg_last_error()
    assert call_push(lib, n_arcs=-1) == -1
    assert call_push(lib, sources=None) == -1 and call_push(lib, weights=None) == -1      # arcs without their arrays
    for name in ('ppg', 'lengths', 'begin', 'end', 'total', 'mean', 'count', 'sources', 'weights') + required:
        assert call_push(lib, **{name: odd}) == -1 and b'4-byte' in lib.ppg_last_error(), name
    assert call_push(lib, curve_total=odd, curve_begin=dummy) == -1 and b'4-byte' in lib.ppg_last_error()
    # open: the state, its geometry and the graphs
    for name in ('state',) + required:
        assert call_open(lib, **{name: None}) == -1, name
    for name in ('streams', 'graphs', 'max_states', 'n_states'):
        assert call_open(lib, **{name: 0}) == -1 and call_open(lib, **{name: -3}) == -1, name
    assert call_open(lib, streams=E.SEARCH_MAX_ITEMS + 1) == -1 and b'at most' in lib.ppg_last_error()
    assert call_open(lib, graphs=E.SEARCH_GRAPH_MAX_GRAPHS + 1, n_states=1 << 20) == -1
    assert call_open(lib, max_states=E.VITERBI_MAX_STATES + 1) == -1 and b'at most' in lib.ppg_last_error()
    assert call_open(lib, n_states=1) == -1 and call_open(lib, n_states=9) == -1 and call_open(lib, n_arcs=-1) == -1
    assert call_open(lib, n_arcs=2 * E.VITERBI_MAX_ARCS + 1) == -1
    assert call_open(lib, sources=None) == -1 and call_open(lib, weights=None) == -1
    assert call_open(lib, state=skew) == -1 and b'aligned' in lib.ppg_last_error()
    for name in required + ('sources', 'weights'):
        assert call_open(lib, **{name: odd}) == -1 and b'4-byte' in lib.ppg_last_error(), name
    # reset and flush: the state and its geometry, `which`, and flush's outputs
    for call in (call_reset, call_flush):
        for changes in (dict(streams=0), dict(graphs=0), dict(max_states=0), dict(streams=E.SEARCH_MAX_ITEMS + 1),
                        dict(graphs=E.SEARCH_GRAPH_MAX_GRAPHS + 1), dict(max_states=E.VITERBI_MAX_STATES + 1),
                        dict(state=None), dict(state=skew), dict(which=odd)):
            assert call(lib, **changes) == -1, (call.__name__, changes)
    for name in ('begin', 'end', 'total', 'mean', 'count'):
        assert call_flush(lib, **{name: None}) == -1 and call_flush(lib, **{name: odd}) == -1, name


def test_stream_search_fails_loudly_without_gpu():
    if torch.cuda.is_available():
        pytest.skip('GPU present')
    lib = E.library()
    dummy = ctypes.c_void_p(256)
    assert call_push(lib) == -2 and b'no HIP device' in lib.ppg_last_error()
    assert call_push(lib, curve_total=dummy, curve_begin=dummy, threshold=-math.inf, patience=0, cap=1) == -2
    assert call_push(lib, n_arcs=0, sources=None, weights=None) == -2
    assert call_open(lib) == -2 and call_reset(lib) == -2 and call_flush(lib) == -2
    spotter = alignment.SearchGraphStream(alignment.chain_graph(['aa', 'b']), -1.)
    with pytest.raises(E.PpgError):
        spotter.push(torch.rand(40, 5))
    with pytest.raises(E.PpgError):
        spotter.push(torch.rand(40, 0))
    with pytest.raises(E.PpgError):
        spotter.flush()
    with pytest.raises(E.PpgError):
        alignment.SearchGraphStream([alignment.chain_graph(['aa', 'b']), alignment.chain_graph([3])], -1., batch=2,
                                    curve=True).push(torch.rand(2, 40, 5), [5, 0])
    assert spotter.position == [0]


def test_value_errors_come_before_any_device_call():
    chain = alignment.chain_graph(['aa', 'b'])
    broken = chain._replace(sources=torch.tensor([2], dtype=torch.int32))            # a source that is no state
    nan = chain._replace(weights=torch.tensor([math.nan]))
    constructions = [
        ((['aa', 'b'], -1.), {}),                                        # a sequence is not a Graph
        ((None, -1.), {}),
        (([], -1.), {}),                                                 # no graph at all
        (([chain, ['aa']], -1.), {}),
        ((broken, -1.), {}),                                             # what the device would refuse
        ((nan, -1.), {}),
        ((chain._replace(stay=torch.zeros(3)), -1.), {}),
        ((chain._replace(phonemes=torch.zeros(2)), -1.), {}),             # phonemes that are no integers
        ((alignment.chain_graph([n % 40 for n in range(alignment.SEARCH_GRAPH_MAX_STATES + 1)]), -1.), {}),
        (([chain, alignment.chain_graph([n % 40 for n in range(257)])], -1.), {}),
        ((alignment.graph([1, 2] * 100, [(p, n, 0.) for n in range(200) for p in range(21)]), -1.), {}),   # 4200 arcs
        ((chain, math.nan), {}),                                         # a NaN threshold
        ((chain, torch.tensor(math.nan)), {}),
        ((chain, -1.), {'patience': -1}),                                # a negative patience
        ((chain, -1.), {'patience': 2.5}),
        ((chain, -1.), {'patience': True}),
        ((chain, -1.), {'patience': 2 ** 31}),
        ((chain, -1.), {'batch': 0}),                                    # a batch of no streams
        ((chain, -1.), {'batch': -2}),
        ((chain, -1.), {'batch': 1.5}),
        ((chain, -1.), {'batch': E.SEARCH_MAX_ITEMS + 1}),
    ]
    for arguments_, keywords in constructions:
        with pytest.raises(ValueError):
            alignment.SearchGraphStream(*arguments_, **keywords)
    with pytest.raises(TypeError):
        alignment.SearchGraphStream(chain)                               # the threshold has no default
    limit = alignment.graph([1, 2] * 128, [(p, n, 0.) for n in range(256) for p in range(16)])
    assert limit.phonemes.shape[0] == 256 and limit.sources.shape[0] == 4096             # the limits themselves are fine
    assert alignment.SearchGraphStream(limit, -1.)._shortest == 1
    one = alignment.SearchGraphStream(chain, -1.)
    three = alignment.SearchGraphStream([chain, alignment.chain_graph([3])], -math.inf, patience=0, batch=3)
    assert one.position == [0] and three.position == [0, 0, 0] and one.patience == 25
    assert one._shortest == 2 and three._shortest == 1
    pushes = [
        (one, torch.rand(39, 5), {}),                                    # channels
        (one, torch.rand(5), {}),                                        # shape
        (one, torch.rand(1, 40, 5), {}),                                 # a batch into one stream
        (one, [[0.] * 5] * 40, {}),                                      # not a tensor
        (one, torch.rand(40, 5), {'lengths': [5]}),                      # lengths without a batch
        (one, torch.empty(40, alignment.SEARCH_MAX_FRAMES + 1), {}),     # more than SEARCH_MAX_FRAMES frames at once
        (three, torch.rand(40, 5), {}),                                  # one stream into a batch
        (three, torch.rand(2, 40, 5), {}),                               # a batch that does not match
        (three, torch.rand(4, 40, 5), {}),
        (three, torch.rand(3, 41, 5), {}),
        (three, torch.rand(3, 40, 5), {'lengths': [5, 5]}),              # one length per stream
        (three, torch.rand(3, 40, 5), {'lengths': [5, 6, 0]}),           # a length outside [0, padded frames]
        (three, torch.rand(3, 40, 5), {'lengths': torch.tensor([5, -1, 0])}),
        (three, torch.rand(3, 40, 0), {'lengths': [0, 1, 0]}),
    ]
    for spotter, ppg, keywords in pushes:
        with pytest.raises(ValueError):
            spotter.push(ppg, **keywords)
    # a push that would pass 2^31 - 1 frames
    three._position = [0, 2 ** 31 - 1 - 4, 7]
    with pytest.raises(ValueError):
        three.push(torch.rand(3, 40, 5))
    with pytest.raises(ValueError):
        three.push(torch.rand(3, 40, 5), lengths=[5, 5, 0])
    assert three.position == [0, 2 ** 31 - 1 - 4, 7]                     # nothing moved
    for item in (3, -1, 1.5, True):
        with pytest.raises(ValueError):
            three.flush(item=item)
        with pytest.raises(ValueError):
            three.reset(item=item)
    with pytest.raises(ValueError):
        one.flush(item=1)
    with pytest.raises(ValueError):
        one.reset(item=1)
