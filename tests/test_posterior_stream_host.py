"""The host side of ppgs_amd.alignment.PosteriorStream: the float64 reference stream
(tests/posterior_stream_reference.py) against brute force over every path, the emission schedule, the host-only entries
of the library, every PPG_EINVAL path, the argument errors of the Python class, and the sensitivity condition that keeps
the GPU tests' float64 tolerance from hiding a horizon that is off by one frame."""
import ctypes
import functools
import math
import os
import re

import numpy as np
import pytest
import torch

from ppgs_amd import alignment, engine as E

import posterior_cases as C
import posterior_reference as R
import posterior_stream_reference as L
from test_posterior_host import small_graph

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INF = math.inf
NAMES = ('ppg_posterior_stream_emitted', 'ppg_posterior_stream_block', 'ppg_posterior_stream_state_bytes',
         'ppg_posterior_stream_workspace_bytes', 'ppg_posterior_stream_open', 'ppg_posterior_stream_reset', 'ppg_posterior_stream_push',
         'ppg_posterior_stream_flush')


# ---- the definition against brute force ----

def test_every_block_equals_brute_force_of_its_prefix_under_the_open_graph():
    generator = torch.Generator().manual_seed(20)
    seen = dict(blocks=0, dead=0, parallel=0, loop=0, hole=0, flush_only=0)
    for trial in range(16):
        states, frames = 1 + trial % 4, 2 + trial % 5
        graph = small_graph(generator, states, (0., 0.3, 0.5)[trial % 3])
        g = R.lists(graph)
        e = -3. * torch.rand(frames, states, generator=generator, dtype=torch.float64).numpy()
        for n, into in enumerate(g.into):
            sources = [source for source, _ in into]
            seen['parallel'] += len(set(sources)) < len(sources)
            seen['loop'] += n in sources
            seen['hole'] += any(weight == -INF for _, weight in into)
        for block in range(1, frames + 1):
            for lag in range(0, frames - block + 2):                     # the last one: H + L > T, the flush alone
                pushes = []
                while sum(pushes) < frames:                              # pushes of 1 to 3 frames, and one of none
                    pushes.append(min((trial + len(pushes)) % 4, frames - sum(pushes)))
                pieces = L.stream(e, g, pushes, block, lag)
                assert [(piece['begin'], piece['count']) for piece in pieces] == L.schedule(pushes, block, lag) or \
                    pieces[-1]['total'] == -INF
                position = 0
                for piece, pushed in zip(pieces[:-1], pushes):
                    position += pushed
                    if position == 0:
                        assert piece['evidence'] == 0. and piece['count'] == 0
                        continue
                    if piece['evidence'] == -INF:
                        seen['dead'] += 1
                        break
                    expected, _ = R.brute_force(e[:position], L.open_graph(g))
                    assert abs(piece['evidence'] - expected) <= 1e-12
                    for j in range(piece['count']):
                        t = piece['begin'] + j
                        h = L.horizon(t // block, block, lag)
                        assert position - pushed - 1 < h <= position - 1 or position - pushed < block + lag
                        _, occupancy = R.brute_force(e[:h + 1], L.open_graph(g))
                        assert np.abs(piece['gamma'][j] - occupancy[t]).max() <= 1e-12
                        assert abs(piece['gamma'][j].sum() - 1.) <= 1e-12 and abs(piece['post'][:, j].sum() - 1.) <= 1e-12
                        seen['blocks'] += 1
                else:
                    last = pieces[-1]
                    expected, occupancy = R.brute_force(e, g)
                    if expected == -INF:
                        assert last['total'] == -INF and last['count'] == 0
                    else:
                        assert abs(last['total'] - expected) <= 1e-12
                        assert last['begin'] + last['count'] == frames
                        assert np.abs(last['gamma'] - occupancy[last['begin']:]).max(initial=0.) <= 1e-12
                        seen['flush_only'] += last['count'] == frames
    assert all(count >= 3 for count in seen.values()), seen


# ---- the schedule ----

def test_emitted_is_the_schedule_and_does_not_depend_on_the_pushes():
    lib = E.library()
    rng = np.random.default_rng(3)
    for block in (1, 7, 64):
        for lag in (0, 3, 64):
            for received in range(201):
                expected = L.emitted(received, block, lag)
                assert lib.ppg_posterior_stream_emitted(received, block, lag) == expected
                assert expected % block == 0 and expected <= max(0, received - lag) < expected + block
            for _ in range(5):
                pushes = []
                while sum(pushes) < 200:
                    pushes.append(int(min(rng.integers(0, 40), 200 - sum(pushes))))
                steps = L.schedule(pushes, block, lag)
                assert sum(count for _, count in steps[:-1]) == L.emitted(200, block, lag)
                assert sum(count for _, count in steps) == 200
                assert all(begin == sum(count for _, count in steps[:i]) for i, (begin, _) in enumerate(steps))
                assert all(count <= pushed + block - 1 for (_, count), pushed in zip(steps, pushes))
                assert steps[-1][1] <= block + lag - 1
    assert lib.ppg_posterior_stream_emitted(2 ** 40, 16, 16) == (2 ** 40 - 16) // 16 * 16
    for bad in ((-1, 1, 0), (5, 0, 0), (5, -1, 0), (5, 1, -1)):
        assert lib.ppg_posterior_stream_emitted(*bad) == -1, bad


def test_block_placement_is_the_schedule_in_64_bits():
    """ppg_posterior_stream_block is the rule by which a push's launch (a workgroup per frame and stream) finds the
    block of workgroup `index`: the blocks a push completes and -1 for every other index, also where index * block or
    c + index * block passes 2^31 in arguments the entries accept."""
    block_of = E.library().ppg_posterior_stream_block
    rng = np.random.default_rng(4)
    for block in (1, 7, 64):
        for lag in (0, 3, 64):
            position = 0
            while position < 400:
                pushed = int(rng.integers(0, 90))
                before, after = L.emitted(position, block, lag), L.emitted(position + pushed, block, lag)
                expected = list(range(before, after, block))
                assert len(expected) <= max(pushed, 0) or pushed == 0 and not expected
                got = [block_of(position, position + pushed, block, lag, index) for index in range(max(pushed, 1) + 2)]
                assert got == expected + [-1] * (len(got) - len(expected)), (block, lag, position, pushed)
                position += pushed
    top = 2 ** 31 - 1
    # one push of 65536 frames at block = window = 65536: one block, and 65535 workgroups with nothing to do
    assert block_of(0, 65536, 65536, 0, 0) == 0
    for index in (1, 2, 32767, 32768, 32769, 65535):
        assert block_of(0, 65536, 65536, 0, index) == -1, index
    # block = 32768 on the second push, c >= 32768: index * block reaches 2^31 at index 65536 and beyond
    assert [block_of(32768, 98304, 32768, 0, index) for index in (0, 1, 2, 65535)] == [32768, 65536, -1, -1]
    # a position near INT32_MAX: c + index * block would pass 2^31 in 32 bits
    last = top - top % 16
    assert L.emitted(top, 16, 0) == last
    assert [block_of(top - 40, top, 16, 0, index) for index in range(5)] == [last - 32, last - 16, -1, -1, -1]
    assert [block_of(top - 16, top, 1, 0, index) for index in (0, 15, 16, 65535)] == [top - 16, top - 1, -1, -1]
    assert block_of(top - 65536, top, 65536, 65536, 65535) == -1
    assert block_of(2 ** 40, 2 ** 40 + 48, 16, 0, 2) == 2 ** 40 + 32
    for bad in ((-1, 5, 1, 0, 0), (6, 5, 1, 0, 0), (0, 5, 0, 0, 0), (0, 5, 1, -1, 0), (0, 5, 1, 0, -1)):
        assert block_of(*bad) == -1, bad


# ---- the C ABI on the host ----

def test_header_declares_library_exports_and_engine_binds_the_entry_points():
    text = open(os.path.join(ROOT, 'include', 'ppgs_amd.h')).read()
    code = re.sub(r'/\*.*?\*/', '', text, flags=re.S)
    for name in NAMES:
        declared = re.search(r'\b%s\s*\(([^)]*)\)\s*;' % name, code)
        assert declared, name
        assert name in E.SYMBOLS and hasattr(E.library(), name)
        assert len(declared.group(1).split(',')) == len(E.SYMBOLS[name][1]), name
    assert [len(E.SYMBOLS[name][1]) for name in NAMES] == [3, 5, 3, 2, 23, 7, 32, 28]
    assert E.SYMBOLS[NAMES[0]][0] is ctypes.c_int64 and E.SYMBOLS[NAMES[1]][0] is ctypes.c_int64
    assert E.SYMBOLS[NAMES[2]][0] is ctypes.c_size_t and E.SYMBOLS[NAMES[3]][0] is ctypes.c_size_t
    assert all(E.SYMBOLS[name][0] is ctypes.c_int for name in NAMES[4:])
    assert E.library().ppg_abi_version() == 1
    assert alignment.PosteriorFrames._fields == ('phonemes', 'states', 'begin', 'count', 'evidence', 'total')


def test_size_helpers_give_the_stated_layout_and_zero_outside_the_limits():
    state, workspace = E.library().ppg_posterior_stream_state_bytes, E.library().ppg_posterior_stream_workspace_bytes

    def up(value):
        return (value + 255) // 256 * 256
    for streams, window, states in ((1, 64, 1), (1, 1024, 40), (3, 128, 64), (3, 128, 65), (64, 1024, 300),
                                    (7, 65536, 1024), (65535, 64, 257), (65535, 65536, 1024)):
        row = 64 if states <= 64 else (states + 255) // 256 * 256
        slots = streams * window
        # the heads (40 B), then per frame of the ring a row of `a` (4 * row B) and 176 B of prepared frame, and a
        # verdict per stream
        expected = up(streams * 40) + up(slots * row * 4) + up(slots * 176) + up(streams * 4)
        assert state(streams, window, states) == expected, (streams, window, states)
    assert state(65535, 65536, 1024) > 1 << 43                           # never a wrapped number: 1.8e13 bytes
    for bad in ((0, 64, 40), (-1, 64, 40), (E.VITERBI_STREAM_MAX_STREAMS + 1, 64, 40), (1, 0, 40), (1, -64, 40),
                (1, 32, 40), (1, 65, 40), (1, 96, 40), (1, 1000, 40), (1, 65536 + 64, 40), (1, 64, 0), (1, 64, -1),
                (1, 64, 1025)):
        assert state(*bad) == 0, bad
    for streams, frames in ((1, 1), (1, 16), (64, 16), (3, 1000), (65535, 65536)):
        assert workspace(streams, frames) == up(streams * frames * 176), (streams, frames)
    for bad in ((0, 16), (1, 0), (-1, 16), (1, -16), (E.VITERBI_STREAM_MAX_STREAMS + 1, 16), (1, 65537)):
        assert workspace(*bad) == 0, bad


GRAPH_NAMES = ('state_begin', 'state_phonemes', 'stay', 'initial', 'final', 'arc_begin', 'sources', 'weights',
               'out_begin', 'targets', 'out_weights')
MAY_BE_NULL = ('sources', 'weights', 'targets', 'out_weights')


def arguments(lib, **changes):
    dummy = ctypes.c_void_p(256)
    a = dict(state=dummy, streams=1, window=64, ppg=dummy, frames=16, lengths=dummy, graphs=1, n_states=3, n_arcs=2,
             max_states=3, block=4, lag=3, cap=19, post=dummy, occupancy=None, stride=3, begin=dummy, count=dummy,
             float64=dummy, which=None, ws=dummy, size=lib.ppg_posterior_stream_workspace_bytes(1, 16))
    a.update({name: dummy for name in GRAPH_NAMES})
    a.update(changes)
    a['packed'] = [a[name] for name in ('graphs', 'n_states', 'n_arcs', 'max_states') + GRAPH_NAMES]
    return a


def call_open(lib, **changes):
    a = arguments(lib, **changes)
    return lib.ppg_posterior_stream_open(0, a['state'], a['streams'], a['window'], *a['packed'], a['which'],
                                         a['block'], a['lag'], None)


def call_push(lib, **changes):
    a = arguments(lib, **changes)
    return lib.ppg_posterior_stream_push(
        0, a['state'], a['streams'], a['window'], a['ppg'], a['frames'], a['lengths'], *a['packed'], a['cap'],
        a['post'], a['occupancy'], a['stride'], a['begin'], a['count'], a['float64'], a['ws'], a['size'], None)


def call_flush(lib, **changes):
    a = arguments(lib, **dict(dict(cap=6), **changes))
    return lib.ppg_posterior_stream_flush(
        0, a['state'], a['streams'], a['window'], *a['packed'], a['which'], a['cap'], a['post'], a['occupancy'],
        a['stride'], a['begin'], a['count'], a['float64'], None)


def call_reset(lib, **changes):
    a = arguments(lib, **changes)
    return lib.ppg_posterior_stream_reset(0, a['state'], a['streams'], a['window'], a['max_states'], a['which'], None)


def test_bad_arguments_return_einval():
    lib = E.library()
    dummy, odd = ctypes.c_void_p(256), ctypes.c_void_p(258)              # 258: not on a 4-byte boundary
    required = tuple(name for name in GRAPH_NAMES if name not in MAY_BE_NULL)
    outputs = ('post', 'begin', 'count')
    for name in ('state', 'ppg', 'lengths', 'ws', 'float64') + required + MAY_BE_NULL + outputs:
        assert call_push(lib, **{name: None}) == -1, name
    for name in ('ppg', 'lengths', 'occupancy', 'float64') + GRAPH_NAMES + outputs:
        assert call_push(lib, **{name: odd}) == -1 and b'aligned' in lib.ppg_last_error(), name
    for name in ('state', 'ws'):
        assert call_push(lib, **{name: ctypes.c_void_p(264)}) == -1 and b'aligned' in lib.ppg_last_error(), name
    for call in (call_push, call_flush):
        assert call(lib, float64=ctypes.c_void_p(260)) == -1 and b'8-byte' in lib.ppg_last_error()
        for cap in (0, -1):
            assert call(lib, cap=cap) == -1 and b'cap' in lib.ppg_last_error()
        assert call(lib, occupancy=dummy, stride=2) == -1 and b'stride' in lib.ppg_last_error()
    for frames in (0, -1, 65537):
        assert call_push(lib, frames=frames, size=1 << 40) == -1 and b'frames' in lib.ppg_last_error()
    assert call_push(lib, streams=65535, frames=1025, size=1 << 50) == -1 and b'frames x streams' in lib.ppg_last_error()
    assert call_push(lib, size=lib.ppg_posterior_stream_workspace_bytes(1, 16) - 1) == -1
    assert b'workspace' in lib.ppg_last_error()
    for name in ('state', 'float64') + required + MAY_BE_NULL + outputs:
        assert call_flush(lib, **{name: None}) == -1, name
    for name in ('which', 'occupancy', 'float64') + GRAPH_NAMES + outputs:
        assert call_flush(lib, **{name: odd}) == -1 and b'aligned' in lib.ppg_last_error(), name
    for name in ('state',) + required + MAY_BE_NULL:
        assert call_open(lib, **{name: None}) == -1, name
    for name in ('which',) + GRAPH_NAMES:
        assert call_open(lib, **{name: odd}) == -1 and b'aligned' in lib.ppg_last_error(), name
    for block, lag in ((0, 0), (-1, 3), (4, -1), (33, 32), (65, 0), (1, 64), (2 ** 31 - 1, 2 ** 31 - 1)):
        assert call_open(lib, block=block, lag=lag) == -1 and b'block' in lib.ppg_last_error(), (block, lag)
    assert call_reset(lib, state=None) == -1 and call_reset(lib, which=odd) == -1
    # what all four share: the state and its geometry; what three share: the graphs
    for call in (call_open, call_push, call_flush, call_reset):
        assert call(lib, state=ctypes.c_void_p(264)) == -1 and b'aligned' in lib.ppg_last_error()
        for streams in (0, -3, E.VITERBI_STREAM_MAX_STREAMS + 1):
            assert call(lib, streams=streams, size=1 << 50) == -1 and b'streams' in lib.ppg_last_error()
        for window in (0, -64, 32, 96, 100, 65536 + 64):
            assert call(lib, window=window, block=1, lag=0) == -1 and b'window' in lib.ppg_last_error(), window
        for max_states in (0, -1, 1025):
            assert call(lib, max_states=max_states, n_states=1, n_arcs=0) == -1 and b'states' in lib.ppg_last_error()
    for call in (call_open, call_push, call_flush):
        for graphs in (0, -1, 2):                                        # 2: more graphs than streams
            assert call(lib, graphs=graphs) == -1, graphs
        assert call(lib, streams=2, size=1 << 40, graphs=2, n_states=1) == -1            # fewer states than graphs
        assert call(lib, n_states=4) == -1 and call(lib, n_states=0) == -1 and call(lib, n_arcs=-1) == -1
        assert call(lib, n_arcs=32769) == -1


def test_live_posterior_fails_loudly_without_gpu():
    if torch.cuda.is_available():
        pytest.skip('GPU present')
    lib = E.library()
    dummy = ctypes.c_void_p(256)
    assert call_push(lib) == -2 and b'no HIP device' in lib.ppg_last_error()
    assert call_push(lib, occupancy=dummy) == -2
    assert call_push(lib, n_arcs=0, sources=None, weights=None, targets=None, out_weights=None) == -2
    assert call_flush(lib) == -2 and call_flush(lib, which=dummy, occupancy=dummy, cap=1) == -2
    assert call_open(lib) == -2 and call_open(lib, which=dummy, block=32, lag=32) == -2 and call_reset(lib) == -2
    stream = alignment.PosteriorStream(alignment.chain_graph([1, 2, 3]))
    with pytest.raises(E.PpgError):
        stream.push(torch.rand(40, 5))
    with pytest.raises(E.PpgError):
        stream.flush()
    assert stream.position == [0] and stream.emitted == [0]


# ---- the Python class ----

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
        {'graph': chain, 'block': 0}, {'graph': chain, 'block': -4}, {'graph': chain, 'block': 2.},
        {'graph': chain, 'block': True},
        {'graph': chain, 'lag': -1}, {'graph': chain, 'lag': 1.5}, {'graph': chain, 'lag': False},
        {'graph': chain, 'window': 64, 'block': 33, 'lag': 32}, {'graph': chain, 'block': 1, 'lag': 1024},
        {'graph': chain, 'window': 64, 'block': 65, 'lag': 0},
        {'graph': chain, 'batch': 0}, {'graph': chain, 'batch': -2}, {'graph': chain, 'batch': 1.5},
        {'graph': chain, 'batch': E.VITERBI_STREAM_MAX_STREAMS + 1},
    ]
    for keywords in constructions:
        with pytest.raises(ValueError):
            alignment.PosteriorStream(**keywords)
    one = alignment.PosteriorStream(chain)
    three = alignment.PosteriorStream([chain, alignment.chain_graph([4, 5]), chain], block=32, lag=32, window=64, batch=3)
    same = alignment.PosteriorStream(chain, batch=3)                     # one graph for every stream
    assert one.position == [0] and three.position == [0, 0, 0] and same.emitted == [0, 0, 0]
    assert (one.block, one.lag, one.window, one.states) == (16, 16, 1024, False)
    assert three._host.graphs == 2 and three._which_graph.tolist() == [0, 1, 0]          # an object travels once
    assert (three._host.states, three._host.arcs, three._host.max_states) == (5, 3, 3)
    assert three._host.state_begin.tolist() == [0, 3, 5] and three._host.arc_begin.tolist() == [0, 0, 1, 2, 2, 3]
    # the transposed lists: chain 0 -> 1 -> 2 and 0 -> 1, targets counted inside their graph
    assert three._host.out_begin.tolist() == [0, 1, 2, 2, 3, 3] and three._host.targets.tolist() == [1, 2, 1]
    assert same._host.graphs == 1 and same._which_graph is None
    pushes = [
        (one, torch.rand(39, 5), {}), (one, torch.rand(5), {}), (one, torch.rand(1, 40, 5), {}),
        (one, torch.rand(40, 5), {'lengths': [5]}), (one, [[0.] * 5] * 40, {}),
        (three, torch.rand(40, 5), {}), (three, torch.rand(2, 40, 5), {}),
        (three, torch.rand(3, 40, 5), {'lengths': [5, 5]}), (three, torch.rand(3, 40, 5), {'lengths': [5, 6, 0]}),
        (three, torch.rand(3, 40, 5), {'lengths': [5, -1, 0]}),
    ]
    for stream, ppg, keywords in pushes:
        with pytest.raises(ValueError):
            stream.push(ppg, **keywords)
    for item in (3, -1, 1.5, True):
        with pytest.raises(ValueError):
            three.flush(item)
        with pytest.raises(ValueError):
            three.reset(item)


def test_joined_frames_takes_the_first_count_columns_of_every_piece():
    def piece(columns, count, batch=None):
        values = torch.arange(40 * columns, dtype=torch.float32).reshape(40, columns)
        if batch is None:
            return alignment.PosteriorFrames(values, None, torch.tensor(0), torch.tensor(count), None, None)
        return alignment.PosteriorFrames(torch.stack([values + b for b in range(batch)]), None, torch.zeros(batch),
                                         torch.tensor(count), None, None)
    joined = alignment.joined_frames([piece(5, 3), piece(4, 0), piece(6, -1), piece(2, 2)])
    assert joined.shape == (40, 5) and joined[0].tolist() == [0., 1., 2., 0., 1.]
    both = alignment.joined_frames([piece(5, [3, 0], 2), piece(3, [1, 3], 2)])
    assert [value.shape for value in both] == [(40, 4), (40, 3)] and both[1][0].tolist() == [1., 2., 3.]
    with pytest.raises(ValueError):
        alignment.joined_frames([])


# ---- the sensitivity condition ----

@functools.lru_cache(maxsize=None)
def prefixes_of(count, frames, seed):
    graph, ppg = C.random_graph(seed, count), C.random_ppg(seed, frames)
    g = R.lists(graph)
    return graph, L.Prefixes(R.emissions(R.prepared(ppg.numpy()), g.sym), g)


def moved_share(count, frames, seed, block, lag):
    """The share of the blocks whose gamma moves by at least 100 tolerances of the GPU test when the horizon comes one
    frame early: some entry with |gamma(h) - gamma(h - 1)| >= 100 * (3 B(h + 1) gamma(h) + 1e-6).  (The float64
    reference measures 1.00, 0.97, 0.91, 1.00 at (1, 2) and 0.96, 0.81, 1.00 at (4, 3).)"""
    graph, prefixes = prefixes_of(count, frames, seed)
    moved = blocks = 0
    for k in range(frames // block):
        h = L.horizon(k, block, lag)
        if h > frames - 1:
            break
        here = prefixes.upto(h + 1)[1][k * block:(k + 1) * block]
        early = prefixes.upto(h)[1][k * block:(k + 1) * block]             # (lag >= 1: the block lies inside it)
        tolerance = 3. * C.bound(graph, h + 1) * here + 1e-6
        moved += bool((np.abs(here - early) >= 100. * tolerance).any())
        blocks += 1
    return moved / blocks


@pytest.mark.parametrize('block,lag,cases', ((1, 2, C.RANDOM_CASES), (4, 3, C.RANDOM_CASES[1:])))
def test_the_tolerance_cannot_hide_a_horizon_that_is_off_by_one(block, lag, cases):
    for count, frames, seed in cases:
        share = moved_share(count, frames, seed, block, lag)
        print(f'{count} x {frames} ({block}, {lag}): moved share {share:.2f}')
        assert share >= 0.5, (count, frames, block, lag, share)
