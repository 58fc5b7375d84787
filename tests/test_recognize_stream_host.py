"""ppgs_amd.alignment.RecognizeStream without a GPU: the reference stream (tests/recognize_stream_reference.py) against
the float64 Viterbi of tests/recognize_reference.py over every split when nothing can be forced; its commit point as a
function of the prefix alone; forced commits as valid paths with the right count, the greedy rule at max_lag = 0; the
lag of the reference on the recordings of the GPU ring test; the size helpers' layout, every PPG_EINVAL of the entries
before a device is needed and every ValueError of RecognizeStream before any device call."""
import copy
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from ppgs_amd import alignment, engine as E

import recognize_reference as V
import recognize_stream_reference as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ('ppg_recognize_stream_state_bytes', 'ppg_recognize_stream_workspace_bytes', 'ppg_recognize_stream_reset',
         'ppg_recognize_stream_push', 'ppg_recognize_stream_flush')
K = 40


def random_splits(rng, frames):
    cuts = np.sort(rng.integers(0, frames + 1, rng.integers(0, 12)))
    return np.diff(np.concatenate([[0], cuts, [frames]])).tolist()       # empty pushes included


def random_case(rng, frames):
    """Integer-valued inputs, so float64 is exact and ties are real: e (T, K), top, A, initial, final."""
    e = -rng.integers(0, 7, (frames, K)).astype(np.float64)
    kind = int(rng.integers(0, 4))
    if kind == 3:
        A = -rng.integers(0, 6, (K, K)).astype(np.float64)              # in [-5, 0], 30 % forbidden
        A[rng.random((K, K)) < 0.3] = -np.inf
        initial = np.where(rng.random(K) < 0.3, -np.inf, -rng.integers(0, 4, K).astype(np.float64))
        final = np.where(rng.random(K) < 0.3, -np.inf, -rng.integers(0, 4, K).astype(np.float64))
    else:
        A = L.switch((0., 1., 4.)[kind], K).astype(np.float64)
        initial, final = np.zeros(K), np.zeros(K)
    return e, e.max(axis=1), A, initial, final


def test_without_force_every_split_gives_the_viterbi_path():
    rng = np.random.default_rng(416)
    cases = found = 0
    for _ in range(300):
        frames = int(rng.integers(1, 201))
        e, top, A, initial, final = random_case(rng, frames)
        total, labels = V.viterbi(e, A, initial, final)
        for pushes in ([1] * frames, random_splits(rng, frames)):
            stream = L.Stream(A, initial, max_lag=None, dtype=np.float64)
            lists = L.feed(stream, e, top, pushes)
            commits = list(stream.commits)
            runs, sum_, forced = stream.flush(final)
            assert forced == 0
            got = L.flat(lists) + runs
            if labels is None:                                           # no path: the flush commits nothing more
                assert sum_ == -np.inf and L.flat(lists) == got[:len(L.flat(lists))]
                continue
            assert float(sum_) == total, (frames, pushes)
            assert got[0][1] == 0 and got[-1][2] == frames
            assert (L.labels_of(got) == labels).all(), (frames, pushes)
            phonemes, starts = V.runs(labels)
            assert [run[0] for run in got] == phonemes.tolist() and [run[1] for run in got] == starts[:-1].tolist()
            for label, begin, end, score, gop in got:                    # exact: integers summed in float64
                assert score == e[begin:end, label].sum() / (end - begin)
                assert gop == (e[begin:end, label] - top[begin:end]).sum() / (end - begin)
            assert commits == sorted(commits) and commits[-1] <= frames
            found += 1
        cases += 1
    assert cases == 300 and found > 400


def test_no_path_commits_nothing():
    e = np.zeros((5, K))
    stream = L.Stream(L.switch(1.), np.full(K, -np.inf), max_lag=2, dtype=np.float64)
    assert L.feed(stream, e, e.max(axis=1), [2, 0, 3]) == [[], [], []] and stream.commits == [0, 0, 0]
    assert stream.flush() == ([], -np.inf, 0)
    assert stream.p == 0 and stream.c == 0


def test_commit_point_depends_on_the_prefix_alone():
    rng = np.random.default_rng(417)
    for _ in range(60):
        frames = int(rng.integers(1, 120))
        e, top, A, initial, _ = random_case(rng, frames)
        ones = L.Stream(A, initial, max_lag=None, dtype=np.float64)
        L.feed(ones, e, top, [1] * frames)
        after = [0] + ones.commits                                       # after[n]: c once n frames are in
        for _ in range(3):
            pushes = random_splits(rng, frames)
            stream = L.Stream(A, initial, max_lag=None, dtype=np.float64)
            L.feed(stream, e, top, pushes)
            assert stream.commits == [after[n] for n in np.cumsum(pushes)], pushes


def greedy(e, A, initial):
    """max_lag = 0 with pushes of one frame: every frame's label is the best state given the label before it."""
    labels, forced = [], 0
    with np.errstate(invalid='ignore'):
        d = e[0] + initial
        for t in range(len(e)):
            if t:
                d = e[t] + (d[labels[-1]] + A[labels[-1]])
            if not (d > -np.inf).any():
                break
            forced += int((d > -np.inf).sum() > 1)
            labels.append(int(np.argmax(d)))
    return labels, forced


@pytest.mark.parametrize('max_lag', [0, 1, 7])
def test_forced_commits_give_a_valid_path_and_count_their_frames(max_lag):
    rng = np.random.default_rng(418 + max_lag)
    forced_somewhere = 0
    for _ in range(60):
        frames = int(rng.integers(1, 150))
        e, top, A, initial, final = random_case(rng, frames)
        for pushes in ([1] * frames, random_splits(rng, frames)):
            stream = L.Stream(A, initial, max_lag=max_lag, dtype=np.float64)
            got, at, expected = [], 0, 0
            for size in pushes:
                twin = copy.deepcopy(stream)                             # the same push without the forced step
                twin.max_lag = None
                twin.push(e[at:at + size], top[at:at + size])
                got += stream.push(e[at:at + size], top[at:at + size])
                at += size
                if (stream.d > -np.inf).any() or stream.c > twin.c:
                    assert at - stream.c <= max_lag
                    expected += max(0, (at - max_lag) - twin.c)
                    assert stream.c == max(twin.c, at - max_lag)
                assert stream.forced == expected
            alive = bool((stream.d > -np.inf).any())
            committed = stream.c
            runs, total, forced = stream.flush(final)
            assert forced == expected
            got += runs
            if not got:
                assert committed == 0
                continue
            labels = L.labels_of(got)                                    # contiguous from frame 0
            assert got[0][1] == 0 and len(labels) == (frames if total > -np.inf else committed)
            assert initial[labels[0]] > -np.inf
            assert all(A[p, q] > -np.inf for p, q in zip(labels[:-1], labels[1:]))
            if total > -np.inf:
                assert alive and total == V.rescore(labels, e, A, initial, final)
                assert total <= V.viterbi(e, A, initial, final)[0]
            forced_somewhere += forced > 0
            if max_lag == 0 and pushes == [1] * frames:
                path, count = greedy(e, A, initial)
                assert labels[:len(path)].tolist() == path[:len(labels)] and forced == count
    assert forced_somewhere > 30


def test_the_lag_of_the_ring_recordings_stays_below_the_forced_lag():
    largest = 0
    for scale in L.WRAP_SCALES:
        e, top = L.prepared(L.wrap_ppg(scale))
        assert e.shape == (L.WRAP_FRAMES, K)
        for penalty in L.WRAP_PENALTIES:
            for pushes in ([1] * L.WRAP_FRAMES, [7] * 42 + [6], [32] * 9 + [12]):
                stream = L.Stream(L.switch(penalty), None, max_lag=None, dtype=np.float32)
                L.feed(stream, e, top, pushes)
                lag = max(p - c for p, c in zip(np.cumsum(pushes), stream.commits))
                largest = max(largest, lag)
    assert largest <= L.WRAP_LAG, largest
    assert L.WRAP_LAG + 32 <= L.WRAP_WINDOW                              # a push of 32 at the full lag still fits


def test_header_declares_library_exports_and_engine_binds_the_entry_points():
    text = open(os.path.join(ROOT, 'include', 'ppgs_amd.h')).read()
    code = re.sub(r'/\*.*?\*/', '', text, flags=re.S)
    for name in NAMES:
        declared = re.search(r'\b%s\s*\(([^)]*)\)\s*;' % name, code)
        assert declared, name
        assert name in E.SYMBOLS and hasattr(E.library(), name)
        assert len(declared.group(1).split(',')) == len(E.SYMBOLS[name][1]), name
    assert [len(E.SYMBOLS[name][1]) for name in NAMES] == [2, 2, 6, 20, 16]
    assert E.SYMBOLS[NAMES[0]][0] is ctypes.c_size_t and E.SYMBOLS[NAMES[1]][0] is ctypes.c_size_t
    assert all(E.SYMBOLS[name][0] is ctypes.c_int for name in NAMES[2:])
    assert alignment.Runs._fields == ('phonemes', 'begin', 'end', 'score', 'gop', 'count', 'total', 'forced')


def test_size_helpers_give_the_stated_layout_and_zero_outside_the_limits():
    state, workspace = E.library().ppg_recognize_stream_state_bytes, E.library().ppg_recognize_stream_workspace_bytes

    def up(value):
        return (value + 255) // 256 * 256
    for streams, window in ((1, 64), (1, 1024), (3, 128), (64, 1024), (7, 65536), (65535, 64), (65535, 65536)):
        # the heads (8 words), D and the ancestors (64 words each), then per frame of the ring 64 B of back-pointers,
        # 176 B of prepared frame and a 4 B label
        slots = streams * window
        expected = up(streams * 32) + 2 * up(streams * 256) + up(slots * 64) + up(slots * 176) + up(slots * 4)
        assert state(streams, window) == expected, (streams, window)
    assert state(65535, 65536) > 1 << 39                                 # never a wrapped number: 1.0e12 bytes
    for bad in ((0, 64), (-1, 64), (E.RECOGNIZE_STREAM_MAX_STREAMS + 1, 64), (1, 0), (1, -64), (1, 32), (1, 65), (1, 96),
                (1, 1000), (1, 65536 + 64)):
        assert state(*bad) == 0, bad
    for streams, frames in ((1, 1), (1, 16), (64, 16), (3, 1000), (65535, 262144)):
        assert workspace(streams, frames) == up(streams * frames * 176), (streams, frames)
    for bad in ((0, 16), (1, 0), (-1, 16), (1, -16), (E.RECOGNIZE_STREAM_MAX_STREAMS + 1, 16),
                (1, E.RECOGNIZE_MAX_FRAMES + 1)):
        assert workspace(*bad) == 0, bad


def call_push(lib, **changes):
    dummy = ctypes.c_void_p(256)
    a = dict(state=dummy, streams=1, window=64, ppg=dummy, frames=16, lengths=dummy, transitions=dummy, initial=None,
             max_lag=32, cap=48, phonemes=dummy, begin=dummy, end=dummy, score=dummy, gop=None, count=dummy, ws=dummy,
             size=lib.ppg_recognize_stream_workspace_bytes(1, 16))
    a.update(changes)
    return lib.ppg_recognize_stream_push(
        0, a['state'], a['streams'], a['window'], a['ppg'], a['frames'], a['lengths'], a['transitions'], a['initial'],
        a['max_lag'], a['cap'], a['phonemes'], a['begin'], a['end'], a['score'], a['gop'], a['count'], a['ws'],
        a['size'], None)


def call_flush(lib, **changes):
    dummy = ctypes.c_void_p(256)
    a = dict(state=dummy, streams=1, window=64, final=None, which=None, cap=33, phonemes=dummy, begin=dummy, end=dummy,
             score=dummy, gop=None, count=dummy, total=dummy, forced=dummy)
    a.update(changes)
    return lib.ppg_recognize_stream_flush(
        0, a['state'], a['streams'], a['window'], a['final'], a['which'], a['cap'], a['phonemes'], a['begin'], a['end'],
        a['score'], a['gop'], a['count'], a['total'], a['forced'], None)


def test_bad_arguments_return_einval():
    lib = E.library()
    odd = ctypes.c_void_p(258)                                           # not on a 4-byte boundary
    for name in ('state', 'ppg', 'lengths', 'transitions', 'phonemes', 'begin', 'end', 'score', 'count', 'ws'):
        assert call_push(lib, **{name: None}) == -1, name
    for name in ('ppg', 'lengths', 'transitions', 'initial', 'phonemes', 'begin', 'end', 'score', 'gop', 'count'):
        assert call_push(lib, **{name: odd}) == -1 and b'aligned' in lib.ppg_last_error(), name
    for name in ('state', 'ws'):
        assert call_push(lib, **{name: ctypes.c_void_p(264)}) == -1 and b'aligned' in lib.ppg_last_error(), name
    for streams in (0, -3, E.RECOGNIZE_STREAM_MAX_STREAMS + 1):
        assert call_push(lib, streams=streams, size=1 << 50) == -1 and b'streams' in lib.ppg_last_error()
    for window in (0, -64, 32, 96, 100, 65536 + 64):
        assert call_push(lib, window=window, max_lag=0) == -1 and b'window' in lib.ppg_last_error(), window
    for frames in (0, -1, E.RECOGNIZE_MAX_FRAMES + 1):
        assert call_push(lib, frames=frames, size=1 << 40) == -1 and b'frames' in lib.ppg_last_error()
    for max_lag in (-1, 64, 1000):
        assert call_push(lib, max_lag=max_lag) == -1 and b'max_lag' in lib.ppg_last_error()
    for cap in (0, -1):
        assert call_push(lib, cap=cap) == -1 and b'cap' in lib.ppg_last_error()
        assert call_flush(lib, cap=cap) == -1 and b'cap' in lib.ppg_last_error()
    assert call_push(lib, size=lib.ppg_recognize_stream_workspace_bytes(1, 16) - 1) == -1
    assert b'workspace' in lib.ppg_last_error()
    # flush and reset: the state and its geometry, flush's outputs
    for name in ('state', 'phonemes', 'begin', 'end', 'score', 'count', 'total', 'forced'):
        assert call_flush(lib, **{name: None}) == -1, name
    for name in ('final', 'which', 'phonemes', 'begin', 'end', 'score', 'gop', 'count', 'total', 'forced'):
        assert call_flush(lib, **{name: odd}) == -1 and b'aligned' in lib.ppg_last_error(), name
    assert call_flush(lib, state=ctypes.c_void_p(264)) == -1 and b'aligned' in lib.ppg_last_error()
    dummy = ctypes.c_void_p(256)
    for geometry in ((0, 64), (E.RECOGNIZE_STREAM_MAX_STREAMS + 1, 64), (1, 0), (1, 96), (1, 65536 + 64)):
        assert call_flush(lib, streams=geometry[0], window=geometry[1]) == -1, geometry
        assert lib.ppg_recognize_stream_reset(0, dummy, *geometry, None, None) == -1, geometry
    assert lib.ppg_recognize_stream_reset(0, None, 1, 64, None, None) == -1
    assert lib.ppg_recognize_stream_reset(0, ctypes.c_void_p(264), 1, 64, None, None) == -1
    assert lib.ppg_recognize_stream_reset(0, dummy, 1, 64, odd, None) == -1


def test_live_recogniser_fails_loudly_without_gpu():
    if torch.cuda.is_available():
        pytest.skip('GPU present')
    lib = E.library()
    dummy = ctypes.c_void_p(256)
    assert call_push(lib) == -2 and b'no HIP device' in lib.ppg_last_error()
    assert call_push(lib, initial=dummy, gop=dummy, max_lag=0, cap=1) == -2
    assert call_flush(lib) == -2 and call_flush(lib, final=dummy, which=dummy, gop=dummy, cap=1) == -2
    assert lib.ppg_recognize_stream_reset(0, dummy, 1, 64, None, None) == -2
    stream = alignment.RecognizeStream(penalty=1.)
    with pytest.raises(E.PpgError):
        stream.push(torch.rand(40, 5))
    with pytest.raises(E.PpgError):
        stream.flush()
    assert stream.position == [0]


def test_value_errors_come_before_any_device_call():
    A = alignment.switch_penalty(1.)
    constructions = [
        {},                                                              # neither transitions nor penalty
        {'transitions': A, 'penalty': 1.},                               # both
        {'penalty': -1.}, {'penalty': float('inf')}, {'penalty': True},
        {'transitions': A[:39]}, {'transitions': A.tolist()},
        {'transitions': torch.full((40, 40), float('nan'))}, {'transitions': torch.full((40, 40), float('inf'))},
        {'penalty': 1., 'initial': torch.zeros(39)}, {'penalty': 1., 'initial': torch.full((40,), float('nan'))},
        {'penalty': 1., 'final': torch.zeros(41)}, {'penalty': 1., 'final': torch.full((40,), float('inf'))},
        {'penalty': 1., 'window': 0}, {'penalty': 1., 'window': 32}, {'penalty': 1., 'window': 100},
        {'penalty': 1., 'window': 65536 + 64}, {'penalty': 1., 'window': 128.}, {'penalty': 1., 'window': True},
        {'penalty': 1., 'max_lag': -1}, {'penalty': 1., 'max_lag': 1024}, {'penalty': 1., 'window': 64, 'max_lag': 64},
        {'penalty': 1., 'max_lag': 2.5}, {'penalty': 1., 'max_lag': True},
        {'penalty': 1., 'batch': 0}, {'penalty': 1., 'batch': -2}, {'penalty': 1., 'batch': 1.5},
        {'penalty': 1., 'batch': E.RECOGNIZE_STREAM_MAX_STREAMS + 1},
    ]
    for keywords in constructions:
        with pytest.raises(ValueError):
            alignment.RecognizeStream(**keywords)
    one = alignment.RecognizeStream(penalty=1.)
    three = alignment.RecognizeStream(transitions=A, window=64, max_lag=0, batch=3)
    assert one.position == [0] and three.position == [0, 0, 0]
    assert (one.window, one.max_lag) == (1024, 512) and (three.window, three.max_lag) == (64, 0)
    pushes = [
        (one, torch.rand(39, 5), {}),                                    # channels
        (one, torch.rand(5), {}),                                        # shape
        (one, torch.rand(1, 40, 5), {}),                                 # a batch into one stream
        (one, [[0.] * 5] * 40, {}),                                      # not a tensor
        (one, torch.rand(40, 5), {'lengths': [5]}),                      # lengths without a batch
        (three, torch.rand(40, 5), {}),                                  # one stream into a batch
        (three, torch.rand(2, 40, 5), {}),                               # a batch that does not match
        (three, torch.rand(4, 40, 5), {}),
        (three, torch.rand(3, 41, 5), {}),
        (three, torch.rand(3, 40, 5), {'lengths': [5, 5]}),              # one length per stream
        (three, torch.rand(3, 40, 5), {'lengths': [5, 6, 0]}),           # a length outside [0, padded frames]
        (three, torch.rand(3, 40, 5), {'lengths': torch.tensor([5, -1, 0])}),
        (three, torch.rand(3, 40, 0), {'lengths': [0, 1, 0]}),
    ]
    for stream, ppg, keywords in pushes:
        with pytest.raises(ValueError):
            stream.push(ppg, **keywords)
    three._position = [0, 2 ** 31 - 1 - 4, 7]                            # a push that would pass 2^31 - 1 frames
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
