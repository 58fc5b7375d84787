"""ppgs_amd.alignment.SearchStream without a GPU: the reference detector (tests/search_stream_reference.py) against the
offline picker on the planted input and its properties over random curves (disjoint, ordered, independent of the split
into pushes, at most F // N + 2 events per push); the new entry points declared, exported and bound with matching
argument counts; the two size helpers; every argument error of the library before a device is needed; and every
ValueError of SearchStream before any device call."""
import ctypes
import math
import os
import re

import numpy as np
import pytest
import torch

import ppgs_amd
from ppgs_amd import alignment, engine as E

import search_reference as S
import search_stream_reference as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ('ppg_search_stream_state_bytes', 'ppg_search_stream_workspace_bytes', 'ppg_search_stream_reset',
         'ppg_search_stream_push', 'ppg_search_stream_flush')


def planted_curve():
    ppg, query, places, _ = L.planted()
    total, begin = S.programme(S.emissions(S.log_posteriors(ppg), query))
    return total.astype(np.float32), begin, query, [(starts[0], starts[-1]) for starts in places]


def test_planted_input_is_the_one_of_the_offline_search():
    _, _, query, spans = planted_curve()
    assert query == [3, 11, 22, 11, 30] and spans == [(23, 49), (89, 107), (124, 145)]
    assert L.planted()[0].shape == (40, 176)


@pytest.mark.parametrize('patience', [1, 5, 25, 1000])
def test_detector_gives_the_planted_spans_and_the_hits_of_the_offline_picker(patience):
    total, begin, query, spans = planted_curve()
    events = L.flat(L.detect(total, begin, -1e-3, patience))
    assert [(b, e) for b, e, _, _ in events] == spans                   # in time order
    assert all(value == 0 and mean == 0 for _, _, value, mean in events)
    offline = S.pick(total, begin, len(query), 4, -1e-3, np.float32)
    assert len(offline) == 3 and set(events) == set(offline)


def test_detector_without_patience_ends_each_hit_at_the_first_frame_of_the_last_phoneme():
    total, begin, query, _ = planted_curve()
    places = L.planted()[2]
    events = L.flat(L.detect(total, begin, -1e-3, 0))
    assert [(b, e) for b, e, _, _ in events] == [(starts[0], starts[-2] + 1) for starts in places]


def test_detector_on_curves_worked_by_hand():
    inf = np.inf
    # one phoneme, means 0 (0..0), -1 (0..1: overlaps, worse), 0 (2..2: disjoint), -1/2 (2..3), -4 (4..4: below)
    total = np.array([0., -2., 0., -1., -4.], dtype=np.float32)
    begin = np.array([0, 0, 2, 2, 4])
    assert L.detect(total, begin, -1., 10) == [[(0, 1, 0., 0.)], [(2, 3, 0., 0.)]]
    # patience 0: frame 1 first emits the hit that ended at frame 0; its own candidate begins before `taken`
    assert L.detect(total, begin, -1., 0) == [[(0, 1, 0., 0.), (2, 3, 0., 0.)], []]
    # equal means of overlapping spans: the later end frame stays
    total = np.array([-inf, -1., -1.5, -9.], dtype=np.float32)
    begin = np.array([-1, 0, 0, 0])
    assert L.detect(total, begin, -1., 5) == [[], [(0, 3, -1.5, -0.5)]]
    assert L.detect(total, begin, -inf, 5) == [[], [(0, 3, -1.5, -0.5)]]                # -9 / 4 overlaps and is worse
    assert L.detect(total[:2], begin[:2], -1., 5) == [[], [(0, 2, -1., -0.5)]]
    # nothing reaches the threshold; an empty curve
    assert L.detect(total, begin, 0., 5) == [[], []] and L.detect(total[:0], begin[:0], -1., 5) == [[], []]
    # the events of a push are the ones its frames give out: the first hit leaves when frame 2 + patience + 1 arrives
    total = np.array([0., 0., 0., -9., -9., -9., -9.], dtype=np.float32)
    begin = np.array([0, 0, 0, 0, 0, 0, 0])
    assert L.detect(total, begin, -1., 2, [5, 2]) == [[], [(0, 3, 0., 0.)], []]
    assert L.detect(total, begin, -1., 2, [6, 1]) == [[(0, 3, 0., 0.)], [], []]


def random_splits(rng, frames):
    cuts = np.sort(rng.integers(0, frames + 1, rng.integers(0, 12)))
    return np.diff(np.concatenate([[0], cuts, [frames]])).tolist()       # empty pushes included


def test_detector_properties_over_random_curves():
    rng = np.random.default_rng(2024)
    cases = 0
    for frames, count in ((1, 1), (7, 1), (40, 1), (200, 1), (9, 2), (64, 2), (200, 2), (33, 3), (150, 3), (97, 4),
                          (5, 5), (200, 5)):
        # emissions with exact zeros (the target is the frame's best) and with ties, 25 problems sharing the loop
        r = np.where(rng.random((25, frames, count)) < 0.45, 0., -rng.integers(1, 9, (25, frames, count)) / 2.)
        totals, begins = S.programme(r)
        for k in range(25):
            total, begin = totals[k].astype(np.float32), begins[k]
            threshold = (-np.inf, -3., -1., -0.3)[int(rng.integers(0, 4))]
            patience = int(rng.integers(0, 31))
            whole = L.detect(total, begin, threshold, patience)
            events = L.flat(whole)
            assert len(whole[0]) <= frames // count + 2
            # disjoint, in stream order, every one a candidate of its end frame
            assert all(0 <= b < e <= frames for b, e, _, _ in events)
            assert all(first[1] <= second[0] for first, second in zip(events, events[1:]))
            for b, e, value, mean in events:
                assert begin[e - 1] == b and value == total[e - 1] and mean >= np.float32(threshold)
                assert mean == value / np.float32(e - b)
            for pushes in ([1] * frames, random_splits(rng, frames), random_splits(rng, frames)):
                split = L.detect(total, begin, threshold, patience, pushes)
                assert L.flat(split) == events, (frames, count, k, pushes)
                for size, given in zip(pushes, split):
                    assert len(given) <= size // count + 2, (frames, count, k, pushes)
                assert len(split[-1]) <= 1
            cases += 1
    assert cases == 300


def test_header_declares_library_exports_and_engine_binds_the_entry_points():
    text = open(os.path.join(ROOT, 'include', 'ppgs_amd.h')).read()
    code = re.sub(r'/\*.*?\*/', '', text, flags=re.S)
    for name in NAMES:
        declared = re.search(r'\b%s\s*\(([^)]*)\)\s*;' % name, code)
        assert declared, name
        assert name in E.SYMBOLS and hasattr(E.library(), name)
        assert len(declared.group(1).split(',')) == len(E.SYMBOLS[name][1]), name
    assert [len(E.SYMBOLS[name][1]) for name in NAMES] == [3, 3, 7, 23, 12]
    assert E.SYMBOLS[NAMES[0]][0] is ctypes.c_size_t and E.SYMBOLS[NAMES[1]][0] is ctypes.c_size_t
    assert all(E.SYMBOLS[name][0] is ctypes.c_int for name in NAMES[2:])
    assert E.SYMBOLS['ppg_search_stream_push'][1][10] is ctypes.c_float          # the threshold
    assert ppgs_amd.alignment.SearchStream is alignment.SearchStream


def test_size_helpers_give_the_stated_layout_and_zero_outside_the_limits():
    state, workspace = E.library().ppg_search_stream_state_bytes, E.library().ppg_search_stream_workspace_bytes

    def up(value):
        return (value + 255) // 256 * 256
    for streams, queries, most in ((1, 1, 1), (1, 1, 64), (1, 1, 65), (3, 5, 70), (64, 8, 8), (1, 64, 256),
                                   (65535, 65535, 256), (65535, 65535, 64)):
        # positions, the detectors (8 words per pair), then D and b: a whole wave's strips per pair
        states = 64 if most <= 64 else 256
        expected = up(streams * 4) + up(streams * queries * 32) + 2 * up(streams * queries * states * 4)
        assert state(streams, queries, most) == expected, (streams, queries, most)
    assert state(65535, 65535, 256) > 1 << 42                            # never a wrapped number: 8.9e12 bytes
    for bad in ((0, 1, 1), (1, 0, 1), (1, 1, 0), (-1, 1, 1), (1, -2, 1), (1, 1, -3), (E.SEARCH_MAX_ITEMS + 1, 1, 1),
                (1, E.SEARCH_MAX_QUERIES + 1, 1), (1, 1, E.SEARCH_MAX_PHONEMES + 1)):
        assert state(*bad) == 0, bad
    for streams, frames, queries in ((1, 1, 1), (1, 16, 1), (64, 16, 8), (1, 1000, 64), (3, 64, 5), (65535, 262144, 1)):
        assert workspace(streams, frames, queries) == up(streams * frames * 176), (streams, frames, queries)
    for bad in ((0, 16, 1), (1, 0, 1), (1, 16, 0), (-1, 16, 1), (1, -16, 1), (1, 16, -1), (E.SEARCH_MAX_ITEMS + 1, 16, 1),
                (1, E.SEARCH_MAX_FRAMES + 1, 1), (1, 16, E.SEARCH_MAX_QUERIES + 1)):
        assert workspace(*bad) == 0, bad


def call_push(lib, **changes):
    dummy = ctypes.c_void_p(256)
    a = dict(state=dummy, ppg=dummy, frames=16, streams=1, lengths=dummy, phonemes=dummy, most=4, queries=2,
             counts=dummy, threshold=-1., patience=25, cap=6, begin=dummy, end=dummy, total=dummy, mean=dummy,
             count=dummy, curve_total=None, curve_begin=None, ws=dummy,
             size=lib.ppg_search_stream_workspace_bytes(1, 16, 2))
    a.update(changes)
    return lib.ppg_search_stream_push(
        0, a['state'], a['ppg'], a['frames'], a['streams'], a['lengths'], a['phonemes'], a['most'], a['queries'],
        a['counts'], a['threshold'], a['patience'], a['cap'], a['begin'], a['end'], a['total'], a['mean'], a['count'],
        a['curve_total'], a['curve_begin'], a['ws'], a['size'], None)


def test_bad_arguments_return_einval():
    lib = E.library()
    dummy = ctypes.c_void_p(256)
    for name in ('state', 'ppg', 'lengths', 'phonemes', 'counts', 'begin', 'end', 'total', 'mean', 'count', 'ws'):
        assert call_push(lib, **{name: None}) == -1, name
    for name in ('frames', 'streams', 'most', 'queries'):
        assert call_push(lib, **{name: 0}) == -1 and call_push(lib, **{name: -3}) == -1, name
    assert call_push(lib, frames=E.SEARCH_MAX_FRAMES + 1, size=1 << 40) == -1 and b'at most' in lib.ppg_last_error()
    assert call_push(lib, most=E.SEARCH_MAX_PHONEMES + 1) == -1 and b'at most' in lib.ppg_last_error()
    assert call_push(lib, streams=E.SEARCH_MAX_ITEMS + 1, size=1 << 50) == -1 and b'at most' in lib.ppg_last_error()
    assert call_push(lib, queries=E.SEARCH_MAX_QUERIES + 1) == -1 and b'at most' in lib.ppg_last_error()
    assert call_push(lib, threshold=math.nan) == -1 and b'NaN' in lib.ppg_last_error()
    assert call_push(lib, patience=-1) == -1 and b'patience' in lib.ppg_last_error()
    for cap in (0, -1):
        assert call_push(lib, cap=cap) == -1 and b'cap' in lib.ppg_last_error()
    assert call_push(lib, curve_total=dummy) == -1 and b'together' in lib.ppg_last_error()
    assert call_push(lib, curve_begin=dummy) == -1 and b'together' in lib.ppg_last_error()
    assert call_push(lib, size=lib.ppg_search_stream_workspace_bytes(1, 16, 2) - 1) == -1
    assert b'workspace' in lib.ppg_last_error()
    assert call_push(lib, ws=ctypes.c_void_p(264)) == -1 and b'aligned' in lib.ppg_last_error()
    assert call_push(lib, state=ctypes.c_void_p(264)) == -1 and b'aligned' in lib.ppg_last_error()
    # reset and flush: the state and its geometry, and flush's outputs
    for geometry in ((0, 2, 4), (1, 0, 4), (1, 2, 0), (E.SEARCH_MAX_ITEMS + 1, 2, 4), (1, E.SEARCH_MAX_QUERIES + 1, 4),
                     (1, 2, E.SEARCH_MAX_PHONEMES + 1)):
        assert lib.ppg_search_stream_reset(0, dummy, *geometry, None, None) == -1, geometry
        assert lib.ppg_search_stream_flush(0, dummy, *geometry, None, dummy, dummy, dummy, dummy, dummy, None) == -1
    assert lib.ppg_search_stream_reset(0, None, 1, 2, 4, None, None) == -1
    assert lib.ppg_search_stream_reset(0, ctypes.c_void_p(264), 1, 2, 4, None, None) == -1
    assert lib.ppg_search_stream_flush(0, None, 1, 2, 4, None, dummy, dummy, dummy, dummy, dummy, None) == -1
    for missing in range(5):
        outputs = [None if k == missing else dummy for k in range(5)]
        assert lib.ppg_search_stream_flush(0, dummy, 1, 2, 4, None, *outputs, None) == -1, missing


def test_stream_search_fails_loudly_without_gpu():
    if torch.cuda.is_available():
        pytest.skip('GPU present')
    lib = E.library()
    dummy = ctypes.c_void_p(256)
    assert call_push(lib) == -2 and b'no HIP device' in lib.ppg_last_error()
    assert call_push(lib, curve_total=dummy, curve_begin=dummy, threshold=-math.inf, patience=0, cap=1) == -2
    assert lib.ppg_search_stream_reset(0, dummy, 1, 2, 4, None, None) == -2
    assert lib.ppg_search_stream_flush(0, dummy, 1, 2, 4, None, dummy, dummy, dummy, dummy, dummy, None) == -2
    spotter = alignment.SearchStream(['aa', 'b'], -1.)
    with pytest.raises(E.PpgError):
        spotter.push(torch.rand(40, 5))
    with pytest.raises(E.PpgError):
        spotter.push(torch.rand(40, 0))
    with pytest.raises(E.PpgError):
        spotter.flush()
    with pytest.raises(E.PpgError):
        alignment.SearchStream([['aa', 'b'], [3]], -1., batch=2, curve=True).push(torch.rand(2, 40, 5), [5, 0])
    assert spotter.position == [0]


def test_value_errors_come_before_any_device_call():
    constructions = [
        ((['aa', 'xx'], -1.), {}),                                       # unknown phoneme name
        (([0, 40], -1.), {}),                                            # index outside 0 .. 39
        (([-1], -1.), {}),
        ((torch.tensor([0.5, 1.]), -1.), {}),                            # not integers
        ((torch.zeros(2, 2, dtype=torch.int64), -1.), {}),               # a table is not a sequence
        (('aa', -1.), {}),                                               # a name is not a sequence
        (([], -1.), {}),                                                 # an empty query
        (([['aa'], []], -1.), {}),
        (([['aa'], 'ae'], -1.), {}),                                     # sequences and names mixed
        (([0] * (alignment.SEARCH_MAX_PHONEMES + 1), -1.), {}),          # a query over 256 phonemes
        ((['aa'], math.nan), {}),                                        # a NaN threshold
        ((['aa'], torch.tensor(math.nan)), {}),
        ((['aa'], -1.), {'patience': -1}),                               # a negative patience
        ((['aa'], -1.), {'patience': 2.5}),
        ((['aa'], -1.), {'patience': True}),
        ((['aa'], -1.), {'patience': 2 ** 31}),
        ((['aa'], -1.), {'batch': 0}),                                   # a batch of no streams
        ((['aa'], -1.), {'batch': -2}),
        ((['aa'], -1.), {'batch': 1.5}),
        ((['aa'], -1.), {'batch': E.SEARCH_MAX_ITEMS + 1}),
    ]
    for arguments, keywords in constructions:
        with pytest.raises(ValueError):
            alignment.SearchStream(*arguments, **keywords)
    with pytest.raises(TypeError):
        alignment.SearchStream(['aa'])                                   # the threshold has no default
    one = alignment.SearchStream(['aa', 'b'], -1.)
    three = alignment.SearchStream([['aa', 'b'], [3]], -math.inf, patience=0, batch=3)
    assert one.position == [0] and three.position == [0, 0, 0] and one.patience == 25
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
