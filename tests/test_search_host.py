"""ppgs_amd.alignment.search without a GPU: the entry points are declared, exported and bound with matching argument
counts; the workspace helper's layout arithmetic; every argument error raised before a device is needed; the compute
entry failing loudly without a device; and the tests' own float64 programme and picker (tests/search_reference.py)
held against brute force on every tiny case, on emissions whose sums are exact so that the tie order itself is tested."""
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

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_declares_library_exports_and_engine_binds_the_entry_points():
    text = open(os.path.join(ROOT, 'include', 'ppgs_amd.h')).read()
    code = re.sub(r'/\*.*?\*/', '', text, flags=re.S)
    for name in ('ppg_search', 'ppg_search_workspace_bytes'):
        declared = re.search(r'\b%s\s*\(([^)]*)\)\s*;' % name, code)
        assert declared, name
        assert name in E.SYMBOLS and hasattr(E.library(), name)
        assert len(declared.group(1).split(',')) == len(E.SYMBOLS[name][1]), name
    assert E.SYMBOLS['ppg_search'][0] is ctypes.c_int and len(E.SYMBOLS['ppg_search'][1]) == 21
    assert E.SYMBOLS['ppg_search_workspace_bytes'][0] is ctypes.c_size_t

    def limit(name):
        return int(re.search(r'#define\s+PPG_SEARCH_MAX_%s\s+(\d+)' % name, code).group(1))
    assert limit('FRAMES') == 262144 == E.SEARCH_MAX_FRAMES == alignment.SEARCH_MAX_FRAMES
    assert limit('PHONEMES') == 256 == E.SEARCH_MAX_PHONEMES == alignment.SEARCH_MAX_PHONEMES
    assert limit('HITS') == 64 == E.SEARCH_MAX_HITS == alignment.SEARCH_MAX_HITS
    assert limit('ITEMS') == 65535 == E.SEARCH_MAX_ITEMS and limit('QUERIES') == 65535 == E.SEARCH_MAX_QUERIES
    assert alignment.Hits._fields == ('phonemes', 'begin', 'end', 'total', 'mean', 'count', 'curve')
    assert ppgs_amd.alignment.search is alignment.search


def test_workspace_helper_gives_the_stated_layout_and_zero_outside_the_limits():
    size = E.library().ppg_search_workspace_bytes

    def up(value):
        return (value + 255) // 256 * 256
    for items, frames, queries in ((1, 1, 1), (1, 57, 1), (3, 301, 5), (64, 1000, 8), (1, 100000, 64),
                                   (1, 262144, 1), (7, 262144, 3), (65535, 4096, 2), (2, 1000, 65535),
                                   (65535, 262144, 65535)):
        # the prepared frames once per recording, then every pair's totals and begins, each block 256-byte aligned
        expected = up(items * frames * 176) + 2 * up(items * queries * frames * 4)
        assert size(items, frames, queries) == expected, (items, frames, queries)
    assert size(65535, 262144, 65535) > 1 << 52                          # never a wrapped number: 9.0e15 bytes
    for bad in ((0, 10, 5), (-1, 10, 5), (1, 0, 5), (1, 10, 0), (1, -4, 5), (1, 10, -1),
                (E.SEARCH_MAX_ITEMS + 1, 10, 5), (1, E.SEARCH_MAX_FRAMES + 1, 5), (1, 10, E.SEARCH_MAX_QUERIES + 1)):
        assert size(*bad) == 0, bad


def call_search(lib, **changes):
    dummy = ctypes.c_void_p(256)
    a = dict(ppg=dummy, frames=10, items=1, lengths=dummy, phonemes=dummy, most=4, queries=2, counts=dummy, top=3,
             threshold=-1., begin=dummy, end=dummy, total=dummy, mean=dummy, count=dummy, curve_total=None,
             curve_begin=None, ws=dummy, size=lib.ppg_search_workspace_bytes(1, 10, 2))
    a.update(changes)
    return lib.ppg_search(0, a['ppg'], a['frames'], a['items'], a['lengths'], a['phonemes'], a['most'], a['queries'],
                          a['counts'], a['top'], a['threshold'], a['begin'], a['end'], a['total'], a['mean'],
                          a['count'], a['curve_total'], a['curve_begin'], a['ws'], a['size'], None)


def test_bad_arguments_return_einval():
    lib = E.library()
    dummy = ctypes.c_void_p(256)
    for name in ('ppg', 'lengths', 'phonemes', 'counts', 'begin', 'end', 'total', 'mean', 'count', 'ws'):
        assert call_search(lib, **{name: None}) == -1, name
    for name in ('frames', 'items', 'most', 'queries'):
        assert call_search(lib, **{name: 0}) == -1 and call_search(lib, **{name: -3}) == -1, name
    assert call_search(lib, frames=E.SEARCH_MAX_FRAMES + 1, size=1 << 40) == -1 and b'at most' in lib.ppg_last_error()
    assert call_search(lib, most=E.SEARCH_MAX_PHONEMES + 1) == -1 and b'at most' in lib.ppg_last_error()
    assert call_search(lib, items=E.SEARCH_MAX_ITEMS + 1, size=1 << 50) == -1 and b'at most' in lib.ppg_last_error()
    assert call_search(lib, queries=E.SEARCH_MAX_QUERIES + 1, size=1 << 50) == -1 and b'at most' in lib.ppg_last_error()
    for top in (0, -1, E.SEARCH_MAX_HITS + 1):
        assert call_search(lib, top=top) == -1 and b'top' in lib.ppg_last_error()
    assert call_search(lib, threshold=math.nan) == -1 and b'NaN' in lib.ppg_last_error()
    assert call_search(lib, curve_total=dummy) == -1 and b'together' in lib.ppg_last_error()
    assert call_search(lib, curve_begin=dummy) == -1 and b'together' in lib.ppg_last_error()
    assert call_search(lib, size=lib.ppg_search_workspace_bytes(1, 10, 2) - 1) == -1
    assert b'workspace' in lib.ppg_last_error()
    assert call_search(lib, ws=ctypes.c_void_p(264)) == -1 and b'aligned' in lib.ppg_last_error()
    assert call_search(lib, items=65535, frames=262144, queries=65535, size=1 << 52) == -1      # 9.0e15 bytes needed
    assert b'workspace' in lib.ppg_last_error()


def test_search_fails_loudly_without_gpu():
    if torch.cuda.is_available():
        pytest.skip('GPU present')
    lib = E.library()
    dummy = ctypes.c_void_p(256)
    assert call_search(lib) == -2 and b'no HIP device' in lib.ppg_last_error()
    assert call_search(lib, curve_total=dummy, curve_begin=dummy, threshold=-math.inf) == -2
    with pytest.raises(E.PpgError):
        alignment.search(torch.rand(40, 5), ['aa', 'b'])
    with pytest.raises(E.PpgError):
        alignment.search(torch.rand(2, 40, 5), [['aa', 'b'], [3]], lengths=[5, 4], top=2, threshold=-1., curve=True)
    with pytest.raises(E.PpgError):
        E.search_items(torch.rand(1, 40, 5), [5], torch.zeros(1, 2, dtype=torch.int32), [2])


def test_value_errors_come_before_any_device_call():
    x, bx = torch.rand(40, 5), torch.rand(3, 40, 5)
    cases = [
        (torch.rand(39, 5), ['aa'], {}),                                 # channels
        (torch.rand(3, 41, 5), ['aa'], {}),
        (torch.rand(5), ['aa'], {}),                                     # shape
        (torch.rand(2, 3, 40, 5), ['aa'], {}),
        (torch.rand(40, 0), ['aa'], {}),                                 # zero frames
        (torch.rand(0, 40, 5), ['aa'], {}),                              # empty batch
        (torch.empty(40, alignment.SEARCH_MAX_FRAMES + 1), ['aa'], {}),  # more than SEARCH_MAX_FRAMES frames
        (x, ['aa', 'xx'], {}),                                           # unknown phoneme name
        (x, [0, 40], {}),                                                # index outside 0 .. 39
        (x, [-1], {}),
        (x, torch.tensor([0, 40]), {}),
        (x, torch.tensor([0.5, 1.]), {}),                                # not integers
        (x, torch.zeros(2, 2, dtype=torch.int64), {}),                   # a table is not a sequence
        (x, [1.5], {}),
        (x, 'aa', {}),                                                   # a name is not a sequence
        (x, [], {}),                                                     # an empty query
        (x, [['aa'], []], {}),
        (x, [['aa'], ['xx']], {}),
        (x, [['aa'], 'ae'], {}),                                         # sequences and names mixed
        (x, [0] * (alignment.SEARCH_MAX_PHONEMES + 1), {}),              # a query over 256 phonemes
        (x, [['aa'], [0] * (alignment.SEARCH_MAX_PHONEMES + 1)], {}),
        (x, ['aa'], {'top': 0}),                                         # top outside 1 .. 64
        (x, ['aa'], {'top': alignment.SEARCH_MAX_HITS + 1}),
        (x, ['aa'], {'top': 1.5}),
        (x, ['aa'], {'top': True}),
        (x, ['aa'], {'threshold': math.nan}),                            # a NaN threshold
        (x, ['aa'], {'threshold': torch.tensor(math.nan)}),
        (x, ['aa'], {'lengths': [5]}),                                   # lengths without a batch
        (bx, ['aa'], {'lengths': [5, 5]}),                               # one length per recording
        (bx, ['aa'], {'lengths': [5, 0, 5]}),                            # a length outside [1, padded frames]
        (bx, ['aa'], {'lengths': torch.tensor([5, 6, 5])}),
    ]
    for ppg, phonemes, keywords in cases:
        with pytest.raises(ValueError):
            alignment.search(ppg, phonemes, **keywords)
    # a query longer than the recording is no error: it has no hits
    assert len(alignment._sequence([1, 2, 3, 4, 5, 6])) == 6


def exact_emissions(rng, frames, count):
    """Emissions from {0, -1, -2, -3}: every sum is exact, so equal optima are equal bits and the tie order decides."""
    return -rng.integers(0, 4, (frames, count)).astype(np.float64)


def test_float64_programme_equals_brute_force_on_every_tiny_case():
    rng = np.random.default_rng(13)
    for frames in range(1, 8):
        for count in range(1, 4):
            tables = [exact_emissions(rng, frames, count) for _ in range(12)]
            tables += [np.zeros((frames, count)), -np.ones((frames, count)),         # every segmentation ties
                       np.log(rng.random((frames, count)))]                          # and none does
            for r in tables:
                total, begin = S.programme(r)
                brute_total, brute_begin = S.brute_force(r)
                assert total.tolist() == brute_total.tolist(), (frames, count, r)
                assert begin.tolist() == brute_begin.tolist(), (frames, count, r)
                assert (begin[:count - 1] == -1).all() and np.isneginf(total[:count - 1]).all()
                assert (begin[count - 1:] >= 0).all() and (begin[count - 1:] <= np.arange(frames)[count - 1:] - count + 1).all()
                # the vectorised re-scoring of the programme's own spans finds the same sums
                again = S.rescore(r, begin)
                assert again[count - 1:].tolist() == total[count - 1:].tolist() and np.isnan(again[:count - 1]).all()
            # leading axes are independent problems
            stacked = S.programme(np.stack(tables[:3]))
            for k in range(3):
                one = S.programme(tables[k])
                assert stacked[0][k].tolist() == one[0].tolist() and stacked[1][k].tolist() == one[1].tolist()


def test_float64_programme_on_tables_worked_by_hand():
    # one phoneme: a fresh start only if strictly better than staying, so a run of zeros keeps its first begin
    total, begin = S.programme(np.array([[0.], [0.], [-2.], [0.], [-1.], [-1.]]))
    assert total.tolist() == [0., 0., -2., 0., -1., -1.] and begin.tolist() == [0, 0, 0, 3, 3, 5]
    # two phonemes: the match ending at frame 3 is frames 2 .. 3; at frame 4 staying in the last phoneme costs 3
    r = np.array([[-3., -3.], [-1., -3.], [0., -2.], [-3., 0.], [-3., -3.]])
    total, begin = S.programme(r)
    assert np.isneginf(total[0]) and begin[0] == -1
    assert total[1:].tolist() == [-6., -3., 0., -3.] and begin[1:].tolist() == [0, 1, 2, 2]
    # all zeros: the last phoneme starts as early as it may and so does everything before it: begin 0 throughout
    total, begin = S.programme(np.zeros((6, 3)))
    assert total[2:].tolist() == [0.] * 4 and begin.tolist() == [-1, -1, 0, 0, 0, 0]
    # emissions against the frame's best phoneme: 0 exactly there, the log ratio elsewhere
    ppg = torch.full((40, 2), 0.01)
    ppg[3, 0], ppg[5, 0], ppg[7, 1] = 0.5, 0.25, 0.5
    r = S.emissions(S.log_posteriors(ppg), [3, 5, 7])
    assert r[0, 0] == 0. and r[1, 2] == 0. and np.isclose(r[0, 1], np.log(0.5)) and (r <= 0).all()


def test_picker_equals_its_restatement_by_the_letter():
    rng = np.random.default_rng(5)
    for frames in (1, 2, 5, 9, 14):
        for count in (1, 2, 3):
            for _ in range(30):
                r = exact_emissions(rng, frames, count)
                total, begin = S.programme(r)
                for top in (1, 2, 3, 64):
                    for threshold in (-np.inf, -1.5, -0.5, 0., 0.5):
                        for dtype in (np.float32, np.float64):
                            hits = S.pick(total, begin, count, top, threshold, dtype)
                            assert hits == S.pick_by_the_letter(total, begin, count, top, threshold, dtype)
                            spans = sorted((b, e) for b, e, _, _ in hits)
                            assert all(a[1] <= b[0] for a, b in zip(spans, spans[1:]))       # pairwise disjoint
                            assert all(mean >= threshold and mean == dtype(value) / dtype(e - b)
                                       for b, e, value, mean in hits)
                            assert [h[3] for h in hits] == sorted((h[3] for h in hits), reverse=True)


def test_picker_on_curves_worked_by_hand():
    inf = np.inf
    # four candidates; means -1/2, 0, 0, -1: the tie in the mean goes to the LARGEST end frame
    total = np.array([-inf, -1., 0., 0., -3.])
    begin = np.array([-1, 0, 1, 1, 2])
    assert S.pick(total, begin, 2, 1) == [(1, 4, 0., 0.)]
    # the second round may not touch frames 1 .. 3: only the match over frames 0 .. 1 meets them, as does 2 .. 4
    assert S.pick(total, begin, 2, 3) == [(1, 4, 0., 0.)]
    begin = np.array([-1, 0, 1, 2, 4])
    total = np.array([-inf, -1., 0., 0., -3.])
    # means: t=1 -1/2, t=2 0 (1..2), t=3 0 (2..3), t=4 -3 (4..4); hits 2..3, then 4..4 and 0..1 by their means
    assert S.pick(total, begin, 1, 3) == [(2, 4, 0., 0.), (0, 2, -1., -0.5), (4, 5, -3., -3.)]
    assert S.pick(total, begin, 1, 3, threshold=-0.5) == [(2, 4, 0., 0.), (0, 2, -1., -0.5)]
    assert S.pick(total, begin, 1, 3, threshold=-0.25) == [(2, 4, 0., 0.)]
    assert S.pick(total, begin, 1, 3, threshold=0.25) == []
    assert S.pick(total, begin, 1, 2) == S.pick_by_the_letter(total, begin, 1, 2)
    # equal means in different places, float32 division: 1/3 of -1 twice
    total = np.array([-inf, -inf, -1., -5., -5., -1.])
    begin = np.array([-1, -1, 0, 0, 0, 3])
    hits = S.pick(total, begin, 3, 2)
    assert [h[:2] for h in hits] == [(3, 6), (0, 3)] and hits[0][3] == hits[1][3] == np.float32(-1.) / np.float32(3.)
    # a query longer than its recording
    assert S.pick(np.full(3, -inf), np.full(3, -1), 5, 4) == []


def test_hit_segments_arithmetic():
    nan = math.nan
    one = alignment.Hits(torch.tensor([3, 4]), torch.tensor([10, 200, -1]), torch.tensor([25, 230, -1]),
                         torch.tensor([-1.5, -9., nan]), torch.tensor([-0.1, -0.3, nan]), torch.tensor(2), None)
    assert alignment.hit_segments(one) == [(0.1, 0.25, -1.5, pytest.approx(-0.1)), (2., 2.3, -9., pytest.approx(-0.3))]
    assert alignment.hit_segments(one, sample_rate=8000, hopsize=80)[0][:2] == (0.1, 0.25)
    assert alignment.hit_segments(one._replace(count=torch.tensor(0))) == []
    assert alignment.hit_segments(one._replace(count=torch.tensor(-1))) == []
    two = one._replace(begin=one.begin[None].repeat(2, 1), end=one.end[None].repeat(2, 1),
                       total=one.total[None].repeat(2, 1), mean=one.mean[None].repeat(2, 1), count=torch.tensor([1, 2]))
    nested = alignment.hit_segments(two)
    assert len(nested) == 2 and len(nested[0]) == 1 and nested[1] == alignment.hit_segments(one)
    grid = two._replace(begin=two.begin[None], end=two.end[None], total=two.total[None], mean=two.mean[None],
                        count=two.count[None])
    assert alignment.hit_segments(grid) == [nested]
