"""ppgs_amd.alignment.ViterbiStream without a GPU: the reference stream (tests/viterbi_stream_reference.py) against the
Viterbi of tests/viterbi_reference.py over every split when nothing can be forced, and against the reference of the
live recogniser under model_graph, forced commits included; its commit point as a function of the prefix alone; forced
commits as valid paths with the right count; a chain that commits nothing before the flush; what the GPU tests rely on,
on their own inputs; the size helpers' layout, every PPG_EINVAL of the entries before a device is needed and every
ValueError of ViterbiStream before any device call."""
import copy
import ctypes
import math
import os
import re

import numpy as np
import pytest
import torch

from ppgs_amd import alignment, engine as E

import recognize_stream_reference as Q
import viterbi_reference as V
import viterbi_stream_cases as C
import viterbi_stream_reference as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ('ppg_viterbi_stream_state_bytes', 'ppg_viterbi_stream_workspace_bytes', 'ppg_viterbi_stream_open',
         'ppg_viterbi_stream_reset', 'ppg_viterbi_stream_push', 'ppg_viterbi_stream_flush')
INF = math.inf


def random_splits(rng, frames):
    cuts = np.sort(rng.integers(0, frames + 1, rng.integers(0, 8)))
    return np.diff(np.concatenate([[0], cuts, [frames]])).tolist()       # empty pushes included


def small_graph(rng):
    """Integer-valued `Lists` of 1 .. 6 states: -inf weights, parallel arcs and arcs n -> n among them."""
    count = int(rng.integers(1, 7))

    def weights(size, holes):
        values = -rng.integers(0, 5, size).astype(np.float64)
        values[rng.random(size) < holes] = -INF
        return values
    into = []
    for n in range(count):
        degree = int(rng.integers(0, 5))
        sources = rng.integers(0, count, degree).tolist()
        if degree and rng.random() < 0.3:
            sources[0] = n                                               # an arc n -> n
        if degree > 1 and rng.random() < 0.3:
            sources[1] = sources[0]                                      # parallel arcs
        into.append(list(zip(sources, weights(degree, 0.2).tolist())))
    holes = float(rng.choice([0., 0.3, 1.]))                             # 1: no state may begin: no path
    return V.Lists(rng.integers(0, 40, count), weights(count, 0.2), into, weights(count, holes), weights(count, 0.3))


def integer_frames(rng, frames):
    logp = -rng.integers(0, 7, (frames, 40)).astype(np.float64)
    return logp, logp.max(axis=1)


def test_without_force_every_split_gives_the_viterbi_path():
    rng = np.random.default_rng(418)
    found = nowhere = 0
    for _ in range(300):
        frames = int(rng.integers(1, 41))
        g = small_graph(rng)
        logp, top = integer_frames(rng, frames)
        e = V.emissions(logp, g.sym)
        total, states, ordinals = V.viterbi(e, g)
        for pushes in ([1] * frames, random_splits(rng, frames)):
            stream = L.Stream(g, max_lag=None, dtype=np.float64)
            lists = L.feed(stream, logp, top, pushes)
            commits = list(stream.commits)
            runs, sum_, forced = stream.flush()
            assert forced == 0 and stream.p == 0 and stream.c == 0
            got = L.flat(lists) + runs
            assert commits == sorted(commits) and commits[-1] <= frames
            if states is None:                       # no path: the flush commits nothing more and closes the open run
                assert sum_ == -INF and (L.frames_of(got).shape[0] if got else 0) == commits[-1]
                nowhere += 1
                continue
            assert float(sum_) == total, (frames, pushes)
            run_states, starts = V.runs(states, ordinals)
            assert [run[0] for run in got] == run_states.tolist() and [run[2] for run in got] == starts[:-1].tolist()
            assert [run[3] for run in got] == starts[1:].tolist()
            assert [run[1] for run in got] == g.sym[run_states].tolist()
            for state, _, begin, end, score, gop in got:                 # exact: integers summed in float64
                assert score == e[begin:end, state].sum() / (end - begin)
                assert gop == (e[begin:end, state] - top[begin:end]).sum() / (end - begin)
            found += 1
    assert found > 300 and nowhere > 20


@pytest.mark.parametrize('max_lag', [None, 0, 1, 7])
def test_under_model_graph_the_reference_is_that_of_the_live_recogniser(max_lag):
    rng = np.random.default_rng(419)
    forced_somewhere = 0
    for _ in range(12):
        frames = int(rng.integers(1, 80))
        logp, top = integer_frames(rng, frames)
        A = -rng.integers(0, 6, (40, 40)).astype(np.float64)
        A[rng.random((40, 40)) < 0.3] = -INF
        initial = np.where(rng.random(40) < 0.3, -INF, -rng.integers(0, 4, 40).astype(np.float64))
        final = np.where(rng.random(40) < 0.3, -INF, -rng.integers(0, 4, 40).astype(np.float64))
        graph = alignment.model_graph(torch.tensor(A), torch.tensor(initial), torch.tensor(final))
        for pushes in ([1] * frames, random_splits(rng, frames)):
            theirs = Q.Stream(A, initial, max_lag=max_lag, dtype=np.float64)
            mine = L.Stream(V.lists(graph), max_lag=max_lag, dtype=np.float64)
            at = 0
            for size in pushes:
                a = theirs.push(logp[at:at + size], top[at:at + size])
                b = mine.push(logp[at:at + size], top[at:at + size])
                at += size
                assert [run[1:] for run in b] == a and all(run[0] == run[1] for run in b)
                assert (theirs.c, theirs.forced) == (mine.c, mine.forced) and (theirs.d == mine.d).all()
            a, b = theirs.flush(final), mine.flush()
            assert [run[1:] for run in b[0]] == a[0] and a[1:] == b[1:]
            forced_somewhere += a[2] > 0
    assert (forced_somewhere > 0) == (max_lag is not None)


def test_commit_point_depends_on_the_prefix_alone():
    rng = np.random.default_rng(420)
    moved = 0
    for _ in range(120):
        frames = int(rng.integers(1, 41))
        g = small_graph(rng)
        logp, top = integer_frames(rng, frames)
        ones = L.Stream(g, max_lag=None, dtype=np.float64)
        L.feed(ones, logp, top, [1] * frames)
        after = [0] + ones.commits                                       # after[n]: c once n frames are in
        moved += after[-1] > 0
        for _ in range(3):
            pushes = random_splits(rng, frames)
            stream = L.Stream(g, max_lag=None, dtype=np.float64)
            at = 0
            for size in pushes:                                          # (with no state alive nothing is committed)
                stream.push(logp[at:at + size], top[at:at + size])
                at += size
                assert stream.c == after[at] if (stream.d > -INF).any() else stream.c <= after[at], pushes
    assert moved > 30


@pytest.mark.parametrize('max_lag', [0, 1, 7])
def test_forced_commits_give_a_valid_path_and_count_their_frames(max_lag):
    rng = np.random.default_rng(421 + max_lag)
    forced_somewhere = 0
    for _ in range(150):
        frames = int(rng.integers(1, 41))
        g = small_graph(rng)
        logp, top = integer_frames(rng, frames)
        e = V.emissions(logp, g.sym)
        for pushes in ([1] * frames, random_splits(rng, frames)):
            stream = L.Stream(g, max_lag=max_lag, dtype=np.float64)
            got, at, expected = [], 0, 0
            for size in pushes:
                twin = copy.deepcopy(stream)                             # the same push without the forced step
                twin.max_lag = None
                twin.push(logp[at:at + size], top[at:at + size])
                got += stream.push(logp[at:at + size], top[at:at + size])
                at += size
                if (stream.d > -INF).any() or stream.c > twin.c:
                    assert at - stream.c <= max_lag
                    expected += max(0, (at - max_lag) - twin.c)
                    assert stream.c == max(twin.c, at - max_lag)
                assert stream.forced == expected
            committed = stream.c
            origin = [row.copy() for row in stream.origin]
            runs, total, forced = stream.flush()
            assert forced == expected
            got += runs
            if not got:
                assert committed == 0
                continue
            states = L.frames_of(got)                                    # contiguous from frame 0
            assert got[0][2] == 0 and len(states) == (frames if total > -INF else committed)
            ordinals = np.array([origin[t][n] for t, n in enumerate(states)])
            opens = np.zeros(len(states), dtype=bool)
            opens[[run[2] for run in got]] = True
            assert ((ordinals != 0) | (np.arange(len(states)) == 0)).tolist() == opens.tolist()
            if total > -INF:                                             # one path of the graph, finite all the way
                ordinals[0] = 0
                assert total == V.rescore(states, ordinals, e, g)
                assert total <= V.viterbi(e, g)[0]
            forced_somewhere += forced > 0
    assert forced_somewhere > 50


def test_a_chain_commits_nothing_before_the_flush_without_force():
    names, graphs, ppgs = C.first_cases()
    for label in ('chain 5', 'chain 64'):
        at = names.index(label)
        logp, top = L.prepared(ppgs[at])
        stream = L.Stream(V.lists(graphs[at]), max_lag=None, dtype=np.float32)
        # (every alive path is in state 0 in the first frames, so these are committed: their run stays open)
        assert L.flat(L.feed(stream, logp, top, [1, 31, 32, 33, 1, 64, 38])) == []
        assert 1 <= stream.c < 20 and stream.run[:2] == [0, 0]
        runs, total, forced = stream.flush()
        assert [run[0] for run in runs] == list(range(graphs[at].phonemes.shape[0])) and total > -INF and forced == 0


def test_what_the_gpu_tests_rely_on_holds_on_their_inputs():
    names, graphs, ppgs = C.first_cases()
    for label in C.EARLY:                                                # runs come out before the flush
        at = names.index(label)
        logp, top = L.prepared(ppgs[at])
        for pushes in ([1, 31, 32, 33, 1, 64, 38], [C.FRAMES]):
            stream = L.Stream(V.lists(graphs[at]), max_lag=None, dtype=np.float32)
            assert len(L.flat(L.feed(stream, logp, top, pushes))) >= 1, label
    for kind in ('loop', 'model'):                                       # the ring test: a lag of at most max_lag / 2
        graph, ppg = C.wrap_case(kind)
        frames = ppg.shape[1]
        assert frames >= 2 * C.WRAP_WINDOW + 1
        logp, top = L.prepared(ppg)
        for pushes in ([1] * frames, [7] * (frames // 7) + [frames % 7], [32] * (frames // 32) + [frames % 32]):
            stream = L.Stream(V.lists(graph), max_lag=None, dtype=np.float32)
            L.feed(stream, logp, top, pushes)
            lag = max(p - c for p, c in zip(np.cumsum(pushes), stream.commits))
            assert lag - max(pushes) + 1 <= C.WRAP_LAG // 2, (kind, pushes[0], lag)
    assert C.WRAP_LAG + 32 <= C.WRAP_WINDOW                              # a push of 32 at the full lag still fits
    for label, graph, ppg in C.forced_cases():                           # the push patterns of the forced test fit
        assert 200 <= ppg.shape[1] <= 600, label


def test_header_declares_library_exports_and_engine_binds_the_entry_points():
    text = open(os.path.join(ROOT, 'include', 'ppgs_amd.h')).read()
    code = re.sub(r'/\*.*?\*/', '', text, flags=re.S)
    for name in NAMES:
        declared = re.search(r'\b%s\s*\(([^)]*)\)\s*;' % name, code)
        assert declared, name
        assert name in E.SYMBOLS and hasattr(E.library(), name)
        assert len(declared.group(1).split(',')) == len(E.SYMBOLS[name][1]), name
    assert [len(E.SYMBOLS[name][1]) for name in NAMES] == [3, 2, 18, 7, 31, 28]
    assert E.SYMBOLS[NAMES[0]][0] is ctypes.c_size_t and E.SYMBOLS[NAMES[1]][0] is ctypes.c_size_t
    assert all(E.SYMBOLS[name][0] is ctypes.c_int for name in NAMES[2:])
    assert alignment.StateRuns._fields == ('states',) + alignment.Runs._fields


def test_size_helpers_give_the_stated_layout_and_zero_outside_the_limits():
    state, workspace = E.library().ppg_viterbi_stream_state_bytes, E.library().ppg_viterbi_stream_workspace_bytes

    def up(value):
        return (value + 255) // 256 * 256
    for streams, window, states in ((1, 64, 1), (1, 1024, 40), (3, 128, 64), (3, 128, 65), (64, 1024, 300),
                                    (7, 65536, 1024), (65535, 64, 257), (65535, 65536, 1024)):
        row = 64 if states <= 64 else (states + 255) // 256 * 256
        slots = streams * window
        # the heads (8 words), D (row words), the ancestors (row 16-bit words), then per frame of the ring a row of
        # back-pointer bytes, 176 B of prepared frame and a 4 B label, and a verdict per stream
        expected = (up(streams * 32) + up(streams * row * 4) + up(streams * row * 2) + up(slots * row) +
                    up(slots * 176) + up(slots * 4) + up(streams * 4))
        assert state(streams, window, states) == expected, (streams, window, states)
    assert state(65535, 65536, 1024) > 1 << 42                           # never a wrapped number: 5.2e12 bytes
    for bad in ((0, 64, 40), (-1, 64, 40), (E.VITERBI_STREAM_MAX_STREAMS + 1, 64, 40), (1, 0, 40), (1, -64, 40),
                (1, 32, 40), (1, 65, 40), (1, 96, 40), (1, 1000, 40), (1, 65536 + 64, 40), (1, 64, 0), (1, 64, -1),
                (1, 64, 1025)):
        assert state(*bad) == 0, bad
    for streams, frames in ((1, 1), (1, 16), (64, 16), (3, 1000), (65535, 262144)):
        assert workspace(streams, frames) == up(streams * frames * 176), (streams, frames)
    for bad in ((0, 16), (1, 0), (-1, 16), (1, -16), (E.VITERBI_STREAM_MAX_STREAMS + 1, 16),
                (1, E.VITERBI_MAX_FRAMES + 1)):
        assert workspace(*bad) == 0, bad


GRAPH_NAMES = ('state_begin', 'state_phonemes', 'stay', 'initial', 'final', 'arc_begin', 'sources', 'weights')


def arguments(lib, **changes):
    dummy = ctypes.c_void_p(256)
    a = dict(state=dummy, streams=1, window=64, ppg=dummy, frames=16, lengths=dummy, graphs=1, n_states=3, n_arcs=2,
             max_states=3, max_lag=32, cap=48, states=dummy, phonemes=dummy, begin=dummy, end=dummy, score=dummy,
             gop=None, count=dummy, total=dummy, forced=dummy, which=None, ws=dummy,
             size=lib.ppg_viterbi_stream_workspace_bytes(1, 16))
    a.update({name: dummy for name in GRAPH_NAMES})
    a.update(changes)
    a['packed'] = [a[name] for name in ('graphs', 'n_states', 'n_arcs', 'max_states') + GRAPH_NAMES]
    return a


def call_open(lib, **changes):
    a = arguments(lib, **changes)
    return lib.ppg_viterbi_stream_open(0, a['state'], a['streams'], a['window'], *a['packed'], a['which'], None)


def call_push(lib, **changes):
    a = arguments(lib, **changes)
    return lib.ppg_viterbi_stream_push(
        0, a['state'], a['streams'], a['window'], a['ppg'], a['frames'], a['lengths'], *a['packed'], a['max_lag'],
        a['cap'], a['states'], a['phonemes'], a['begin'], a['end'], a['score'], a['gop'], a['count'], a['ws'],
        a['size'], None)


def call_flush(lib, **changes):
    a = arguments(lib, **dict(dict(cap=33), **changes))
    return lib.ppg_viterbi_stream_flush(
        0, a['state'], a['streams'], a['window'], *a['packed'], a['which'], a['cap'], a['states'], a['phonemes'],
        a['begin'], a['end'], a['score'], a['gop'], a['count'], a['total'], a['forced'], None)


def call_reset(lib, **changes):
    a = arguments(lib, **changes)
    return lib.ppg_viterbi_stream_reset(0, a['state'], a['streams'], a['window'], a['max_states'], a['which'], None)


def test_bad_arguments_return_einval():
    lib = E.library()
    odd = ctypes.c_void_p(258)                                           # not on a 4-byte boundary
    required = GRAPH_NAMES[:6]
    outputs = ('states', 'phonemes', 'begin', 'end', 'score', 'count')
    for name in ('state', 'ppg', 'lengths', 'ws') + required + outputs:
        assert call_push(lib, **{name: None}) == -1, name
    for name in ('ppg', 'lengths', 'gop') + GRAPH_NAMES + outputs:
        assert call_push(lib, **{name: odd}) == -1 and b'aligned' in lib.ppg_last_error(), name
    for name in ('state', 'ws'):
        assert call_push(lib, **{name: ctypes.c_void_p(264)}) == -1 and b'aligned' in lib.ppg_last_error(), name
    for frames in (0, -1, E.VITERBI_MAX_FRAMES + 1):
        assert call_push(lib, frames=frames, size=1 << 40) == -1 and b'frames' in lib.ppg_last_error()
    for max_lag in (-1, 64, 1000):
        assert call_push(lib, max_lag=max_lag) == -1 and b'max_lag' in lib.ppg_last_error()
    for cap in (0, -1):
        assert call_push(lib, cap=cap) == -1 and b'cap' in lib.ppg_last_error()
        assert call_flush(lib, cap=cap) == -1 and b'cap' in lib.ppg_last_error()
    assert call_push(lib, size=lib.ppg_viterbi_stream_workspace_bytes(1, 16) - 1) == -1
    assert b'workspace' in lib.ppg_last_error()
    for name in ('state',) + required + outputs + ('total', 'forced'):
        assert call_flush(lib, **{name: None}) == -1, name
    for name in ('which', 'gop', 'total', 'forced') + GRAPH_NAMES + outputs:
        assert call_flush(lib, **{name: odd}) == -1 and b'aligned' in lib.ppg_last_error(), name
    for name in ('state',) + required:
        assert call_open(lib, **{name: None}) == -1, name
    for name in ('which',) + GRAPH_NAMES:
        assert call_open(lib, **{name: odd}) == -1 and b'aligned' in lib.ppg_last_error(), name
    assert call_reset(lib, state=None) == -1 and call_reset(lib, which=odd) == -1
    # what all four share: the state and its geometry; what three share: the graphs
    for call in (call_open, call_push, call_flush, call_reset):
        assert call(lib, state=ctypes.c_void_p(264)) == -1 and b'aligned' in lib.ppg_last_error()
        for streams in (0, -3, E.VITERBI_STREAM_MAX_STREAMS + 1):
            assert call(lib, streams=streams, size=1 << 50) == -1 and b'streams' in lib.ppg_last_error()
        for window in (0, -64, 32, 96, 100, 65536 + 64):
            assert call(lib, window=window, max_lag=0) == -1 and b'window' in lib.ppg_last_error(), window
        for max_states in (0, -1, 1025):
            assert call(lib, max_states=max_states, n_states=1, n_arcs=0) == -1 and b'states' in lib.ppg_last_error()
    for call in (call_open, call_push, call_flush):
        for graphs in (0, -1, 2):                                        # 2: more graphs than streams
            assert call(lib, graphs=graphs) == -1, graphs
        assert call(lib, streams=2, size=1 << 40, graphs=2, n_states=1) == -1            # fewer states than graphs
        assert call(lib, n_states=4) == -1 and call(lib, n_states=0) == -1 and call(lib, n_arcs=-1) == -1
        assert call(lib, n_arcs=32769) == -1
        assert call(lib, sources=None) == -1 and call(lib, weights=None) == -1           # arcs without their arrays


def test_live_viterbi_fails_loudly_without_gpu():
    if torch.cuda.is_available():
        pytest.skip('GPU present')
    lib = E.library()
    dummy = ctypes.c_void_p(256)
    assert call_push(lib) == -2 and b'no HIP device' in lib.ppg_last_error()
    assert call_push(lib, gop=dummy, max_lag=0, cap=1) == -2
    assert call_push(lib, n_arcs=0, sources=None, weights=None) == -2
    assert call_flush(lib) == -2 and call_flush(lib, which=dummy, gop=dummy, cap=1) == -2
    assert call_open(lib) == -2 and call_open(lib, which=dummy) == -2 and call_reset(lib) == -2
    stream = alignment.ViterbiStream(alignment.chain_graph([1, 2, 3]))
    with pytest.raises(E.PpgError):
        stream.push(torch.rand(40, 5))
    with pytest.raises(E.PpgError):
        stream.flush()
    assert stream.position == [0]


def test_value_errors_come_before_any_device_call():
    chain = alignment.chain_graph([1, 2, 3])
    wrong = alignment.Graph(*[value if name != 'sources' else torch.tensor([0, 3], dtype=torch.int32)
                              for name, value in zip(alignment.Graph._fields, chain)])
    constructions = [
        {'graph': None}, {'graph': 'hh'}, {'graph': [1, 2, 3]}, {'graph': wrong},
        {'graph': [chain, chain]},                                       # a list without a batch
        {'graph': [chain, chain], 'batch': 3}, {'graph': [chain, wrong], 'batch': 2}, {'graph': [], 'batch': 1},
        {'graph': chain, 'window': 0}, {'graph': chain, 'window': 32}, {'graph': chain, 'window': 100},
        {'graph': chain, 'window': 65536 + 64}, {'graph': chain, 'window': 128.}, {'graph': chain, 'window': True},
        {'graph': chain, 'max_lag': -1}, {'graph': chain, 'max_lag': 1024},
        {'graph': chain, 'window': 64, 'max_lag': 64}, {'graph': chain, 'max_lag': 2.5},
        {'graph': chain, 'max_lag': True},
        {'graph': chain, 'batch': 0}, {'graph': chain, 'batch': -2}, {'graph': chain, 'batch': 1.5},
        {'graph': chain, 'batch': E.VITERBI_STREAM_MAX_STREAMS + 1},
    ]
    for keywords in constructions:
        with pytest.raises(ValueError):
            alignment.ViterbiStream(**keywords)
    one = alignment.ViterbiStream(chain)
    three = alignment.ViterbiStream([chain, alignment.chain_graph([4, 5]), chain], window=64, max_lag=0, batch=3)
    same = alignment.ViterbiStream(chain, batch=3)                       # one graph for every stream
    assert one.position == [0] and three.position == [0, 0, 0] and same.position == [0, 0, 0]
    assert (one.window, one.max_lag) == (1024, 512) and (three.window, three.max_lag) == (64, 0)
    assert three._graphs.graphs == 2 and three._which_graph.tolist() == [0, 1, 0]      # an object travels once
    assert (three._graphs.states, three._graphs.arcs, three._graphs.max_states) == (5, 3, 3)
    assert three._graphs.state_begin.tolist() == [0, 3, 5] and three._graphs.arc_begin.tolist() == [0, 0, 1, 2, 2, 3]
    assert same._graphs.graphs == 1 and same._which_graph is None
    pushes = [
        (one, torch.rand(39, 5), {}), (one, torch.rand(5), {}), (one, torch.rand(1, 40, 5), {}),
        (one, [[0.] * 5] * 40, {}), (one, torch.rand(40, 5), {'lengths': [5]}),
        (three, torch.rand(40, 5), {}), (three, torch.rand(2, 40, 5), {}), (three, torch.rand(3, 41, 5), {}),
        (three, torch.rand(3, 40, 5), {'lengths': [5, 5]}), (three, torch.rand(3, 40, 5), {'lengths': [5, 6, 0]}),
        (three, torch.rand(3, 40, 5), {'lengths': torch.tensor([5, -1, 0])}),
    ]
    for stream, ppg, keywords in pushes:
        with pytest.raises(ValueError):
            stream.push(ppg, **keywords)
    three._position = [0, 2 ** 31 - 1 - 4, 7]                            # a push that would pass 2^31 - 1 frames
    with pytest.raises(ValueError):
        three.push(torch.rand(3, 40, 5))
    assert three.position == [0, 2 ** 31 - 1 - 4, 7]                     # nothing moved
    for item in (3, -1, 1.5, True):
        with pytest.raises(ValueError):
            three.flush(item=item)
        with pytest.raises(ValueError):
            three.reset(item=item)
    with pytest.raises(ValueError):
        one.flush(item=1)
