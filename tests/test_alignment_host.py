"""ppgs_amd.alignment without a GPU: the tests' own float64 programme against brute force on every tiny case, the
host helpers' arithmetic, every argument error raised before a device is needed, the host-only workspace helper,
and the compute entries failing loudly without a device."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import ppgs_amd
from ppgs_amd import alignment, engine as E

import alignment_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_declares_and_library_exports_the_entry_points():
    text = open(os.path.join(ROOT, 'include', 'ppgs_amd.h')).read()
    code = re.sub(r'/\*.*?\*/', '', text, flags=re.S)
    for name in ('ppg_align', 'ppg_align_workspace_bytes', 'ppg_decode'):
        assert re.search(r'\b%s\s*\(' % name, code), name
        assert name in E.SYMBOLS and hasattr(E.library(), name)

    def limit(name):
        return int(re.search(r'#define\s+PPG_ALIGN_MAX_%s\s+(\d+)' % name, code).group(1))
    assert limit('FRAMES') == 4096 == E.ALIGN_MAX_FRAMES == alignment.MAX_FRAMES
    assert limit('PHONEMES') == 1024 == E.ALIGN_MAX_PHONEMES == alignment.MAX_PHONEMES
    assert limit('ITEMS') == 65535 == E.ALIGN_MAX_ITEMS
    assert ppgs_amd.alignment is alignment and E.library().ppg_abi_version() == 1


def test_float64_programme_equals_brute_force_on_every_tiny_case():
    rng = np.random.default_rng(11)
    for frames in range(1, 8):
        for count in range(1, frames + 1):
            for _ in range(6):
                e = np.log(rng.random((frames, count)))
                total, starts = R.programme(e)
                brute_total, brute_starts = R.brute_force(e)
                assert total == brute_total, (frames, count)        # the same sums in the same order: the same bits
                assert starts.tolist() == brute_starts.tolist(), (frames, count)
                R.check_starts(starts, frames, count)
                assert R.path_total(e, starts) == total
            # every segmentation ties: the trace-back stays wherever it may, so the last phoneme takes the slack
            total, starts = R.programme(np.zeros((frames, count)))
            assert total == 0. and starts.tolist() == list(range(count)) + [frames]
            assert R.brute_force(np.zeros((frames, count)))[1].tolist() == starts.tolist()
            # ties among some optima only, on values whose sums are exact
            e = -rng.integers(0, 3, (frames, count)).astype(np.float64) / 4
            total, starts = R.programme(e)
            brute_total, brute_starts = R.brute_force(e)
            assert total == brute_total and starts.tolist() == brute_starts.tolist(), (frames, count)


def test_float64_programme_on_tables_worked_by_hand():
    # two phonemes over four frames; the best cut is after frame 1: -1 -1 | -1 -1 = -4
    e = np.array([[-1., -9.], [-1., -5.], [-4., -1.], [-9., -1.]])
    total, starts = R.programme(e)
    assert total == -4. and starts.tolist() == [0, 2, 4]
    # a tie between cutting after frame 0 and after frame 1: the later phoneme starts as early as it may
    e = np.array([[-1., -9.], [-2., -2.], [-9., -1.]])
    total, starts = R.programme(e)
    assert total == -4. and starts.tolist() == [0, 1, 3]
    assert R.brute_force(e)[1].tolist() == [0, 1, 3]
    # repeated adjacent phonemes: the same column twice, all ties
    e = np.array([[-1., -1.], [-2., -2.], [-3., -3.]])
    total, starts = R.programme(e)
    assert total == -6. and starts.tolist() == [0, 1, 3]
    # N = T: the diagonal is the only path
    e = -np.arange(9.).reshape(3, 3)
    total, starts = R.programme(e)
    assert total == -(0. + 4. + 8.) and starts.tolist() == [0, 1, 2, 3]
    # scores and GOP on a hand-made PPG: the target is the argmax in the first segment only
    ppg = torch.full((40, 3), 0.01)
    ppg[3, 0] = ppg[3, 1] = 0.5
    ppg[7, 2] = 0.5
    ppg[5, 2] = 0.25
    logp = R.log_posteriors(ppg)
    assert logp.shape == (3, 40)
    score, gop = R.scores(logp, [3, 5], [0, 2, 3])
    assert np.allclose(score, [np.log(np.float32(0.5)), np.log(np.float32(0.25))])
    assert gop[0] == 0. and np.isclose(gop[1], np.log(0.5))
    # the clamp: zeros and ones end at log(1e-8) and log(1) as fp32 sees them
    edge = R.log_posteriors(torch.tensor([[0.], [1.]]).expand(2, 1).repeat(20, 1))
    assert np.isclose(edge[0, 0], np.log(np.float64(np.float32(1e-8)))) and edge[0, 1] == 0.


def test_reference_decode_is_argmax_and_unique_consecutive():
    ppg = torch.zeros(40, 6)
    for t, p in enumerate([4, 4, 9, 9, 9, 4]):
        ppg[p, t] = 1.
    phonemes, starts = R.decode(ppg)
    assert phonemes.tolist() == [4, 9, 4] and starts.tolist() == [0, 2, 5, 6]


def test_frame_labels_and_segments_arithmetic():
    starts = torch.tensor([0, 2, 3, 7], dtype=torch.int32)
    phonemes = torch.tensor([5, 39, 5], dtype=torch.int32)
    labels = alignment.frame_labels(starts, phonemes, 7)
    assert labels.dtype == torch.int32 and labels.tolist() == [5, 5, 39, 5, 5, 5, 5]
    assert alignment.frame_labels(torch.tensor([0, 4]), torch.tensor([8]), 4).tolist() == [8, 8, 8, 8]
    assert alignment.frame_labels(torch.tensor([0, 1, 2]), torch.tensor([1, 2]), 2).tolist() == [1, 2]
    with pytest.raises(ValueError):
        alignment.frame_labels(starts, phonemes[:2], 7)
    with pytest.raises(ValueError):
        alignment.frame_labels(starts, phonemes, 0)
    # every reference segmentation expands to the labels it means
    rng = np.random.default_rng(2)
    for frames, count in ((1, 1), (9, 9), (30, 7)):
        _, cuts = R.programme(np.log(rng.random((frames, count))))
        names = rng.integers(0, 40, count)
        labels = alignment.frame_labels(torch.from_numpy(cuts), torch.from_numpy(names), frames)
        assert labels.tolist() == np.repeat(names, np.diff(cuts)).tolist()

    one = alignment.Alignment(phonemes, starts, torch.tensor(-3.), torch.tensor([-0.5, -1., -0.25]),
                              torch.tensor([0., -0.75, 0.]))
    got = alignment.segments(one)
    assert ppgs_amd.PHONEMES[5] == 'ay' and ppgs_amd.PHONEMES[39] == '<silent>'
    assert got == [('ay', 0., 0.02, -0.5, 0.), ('<silent>', 0.02, 0.03, -1., -0.75), ('ay', 0.03, 0.07, -0.25, 0.)]
    assert alignment.segments(one, sample_rate=8000, hopsize=80)[1][1:3] == (0.02, 0.03)
    assert alignment.segments(one, sample_rate=16000, hopsize=320)[2][1:3] == (0.06, 0.14)
    no_gop = alignment.segments(one._replace(gop=None))
    assert [s[4] for s in no_gop] == [None] * 3 and [s[3] for s in no_gop] == [-0.5, -1., -0.25]
    batch = alignment.Alignment([phonemes, phonemes[:1]], [starts, torch.tensor([0, 4])], torch.zeros(2),
                                [one.score, one.score[:1]], [one.gop, one.gop[:1]])
    both = alignment.segments(batch)
    assert both[0] == got and both[1] == [('ay', 0., 0.04, -0.5, 0.)]
    free = alignment.segments(alignment.Decoding(phonemes, starts))
    assert [s[:3] for s in free] == [s[:3] for s in got] and free[0][3:] == (None, None)
    with pytest.raises(ValueError):
        alignment.segments(one._replace(starts=starts[:3]))


def test_value_errors_come_before_any_device_call():
    x, bx = torch.rand(40, 5), torch.rand(3, 40, 5)
    cases = [
        (torch.rand(39, 5), ['aa'], {}),                                 # channels
        (torch.rand(3, 41, 5), [['aa']] * 3, {}),
        (torch.rand(5), ['aa'], {}),                                     # shape
        (torch.rand(2, 3, 40, 5), ['aa'], {}),
        (torch.rand(40, 0), ['aa'], {}),                                 # zero frames
        (torch.rand(0, 40, 5), [], {}),                                  # empty batch
        (torch.rand(40, alignment.MAX_FRAMES + 1), ['aa'], {}),          # limits
        (torch.rand(40, 2000), [0] * (alignment.MAX_PHONEMES + 1), {}),
        (x, ['aa', 'xx'], {}),                                           # unknown phoneme name
        (x, [0, 40], {}),                                                # index outside 0 .. 39
        (x, [-1], {}),
        (x, torch.tensor([0, 40]), {}),
        (x, torch.tensor([0.5, 1.]), {}),                                # not integers
        (x, [1.5], {}),
        (x, 'aa', {}),                                                   # a name is not a sequence
        (x, [], {}),                                                     # N < 1
        (x, [1, 2, 3, 4, 5, 6], {}),                                     # N > T
        (x, ['aa'], {'lengths': [5]}),                                   # lengths without a batch
        (x, ['aa'], {'phoneme_lengths': [1]}),
        (bx, [['aa']] * 2, {}),                                          # one sequence per item
        (bx, ['aa', 'ae', 'ah'], {}),                                    # names where sequences belong
        (bx, [['aa']] * 3, {'lengths': [5, 5]}),                         # one length per item
        (bx, [['aa']] * 3, {'lengths': [5, 0, 5]}),                      # a length outside [1, padded frames]
        (bx, [['aa']] * 3, {'lengths': torch.tensor([5, 6, 5])}),
        (bx, [['aa'], ['aa', 'ae', 'ah'], ['aa']], {'lengths': [5, 2, 5]}),       # N > the item's own T
        (bx, [['aa']] * 3, {'phoneme_lengths': [1, 1, 1]}),              # phoneme_lengths without a padded tensor
        (bx, torch.zeros(2, 4, dtype=torch.int64), {}),                  # table rows
        (bx, torch.zeros(3, 4, dtype=torch.int64), {'phoneme_lengths': [4, 4]}),
        (bx, torch.zeros(3, 4, dtype=torch.int64), {'phoneme_lengths': [4, 5, 4]}),
        (bx, torch.zeros(3, 4, dtype=torch.int64), {'phoneme_lengths': [4, 0, 4]}),
        (bx, torch.full((3, 4), -1), {}),                                # padding inside the stated lengths
        (bx, torch.zeros(3, 6, dtype=torch.int64), {}),                  # N > T from the table's width
    ]
    for ppg, phonemes, keywords in cases:
        with pytest.raises(ValueError):
            alignment.forced(ppg, phonemes, **keywords)
    for ppg, keywords in ((torch.rand(39, 5), {}), (torch.rand(5), {}), (torch.rand(40, 0), {}),
                          (torch.rand(0, 40, 5), {}), (torch.rand(40, alignment.MAX_FRAMES + 1), {}),
                          (x, {'lengths': [5]}), (bx, {'lengths': [5, 5]}), (bx, {'lengths': [5, 6, 1]}),
                          (bx, {'lengths': torch.tensor([0, 5, 1])})):
        with pytest.raises(ValueError):
            alignment.decode(ppg, **keywords)


def test_workspace_helper_is_host_only_zero_outside_the_limits_and_monotone():
    size = E.library().ppg_align_workspace_bytes
    assert 0 < size(1, 1, 1) < 1 << 12
    for items, frames, phonemes in ((1, 1, 1), (1, 57, 9), (3, 300, 64), (2, 1000, 120), (64, 1000, 257),
                                    (1, 4096, 1024)):
        here = size(items, frames, phonemes)
        # the prepared frames (40 log-posteriors and their maximum) and a direction bit per cell
        assert here >= items * frames * (41 * 4 + phonemes // 8)
        assert here <= items * frames * (176 + 128) + 4096               # the documented layout, no more
        assert size(items + 1, frames, phonemes) > here
        if frames < E.ALIGN_MAX_FRAMES:
            assert size(items, frames + 1, phonemes) >= here and size(items, min(2 * frames + 7, 4096), phonemes) > here
        if phonemes < E.ALIGN_MAX_PHONEMES:
            assert size(items, frames, phonemes + 1) >= here and size(items, frames, E.ALIGN_MAX_PHONEMES) >= here
    assert size(E.ALIGN_MAX_ITEMS, 4096, 1024) > 1 << 36                 # never a wrapped number
    for bad in ((0, 10, 5), (-1, 10, 5), (1, 0, 5), (1, 10, 0), (1, -4, 5), (1, 10, -1),
                (E.ALIGN_MAX_ITEMS + 1, 10, 5), (1, E.ALIGN_MAX_FRAMES + 1, 5), (1, 10, E.ALIGN_MAX_PHONEMES + 1)):
        assert size(*bad) == 0, bad


def call_align(lib, **changes):
    dummy = ctypes.c_void_p(256)
    a = dict(ppg=dummy, frames=10, items=1, lengths=dummy, phonemes=dummy, most=4, counts=dummy, total=dummy,
             starts=dummy, score=dummy, gop=dummy, ws=dummy, size=lib.ppg_align_workspace_bytes(1, 10, 4))
    a.update(changes)
    return lib.ppg_align(0, a['ppg'], a['frames'], a['items'], a['lengths'], a['phonemes'], a['most'], a['counts'],
                         a['total'], a['starts'], a['score'], a['gop'], a['ws'], a['size'], None)


def call_decode(lib, **changes):
    dummy = ctypes.c_void_p(256)
    a = dict(ppg=dummy, frames=10, items=1, lengths=dummy, phonemes=dummy, starts=dummy, runs=dummy)
    a.update(changes)
    return lib.ppg_decode(0, a['ppg'], a['frames'], a['items'], a['lengths'], a['phonemes'], a['starts'], a['runs'], None)


def test_bad_arguments_return_einval():
    lib = E.library()
    for name in ('ppg', 'lengths', 'phonemes', 'counts', 'total', 'starts', 'score', 'ws'):
        assert call_align(lib, **{name: None}) == -1, name
    assert call_align(lib, frames=0) == -1 and call_align(lib, items=0) == -1 and call_align(lib, most=0) == -1
    assert call_align(lib, frames=E.ALIGN_MAX_FRAMES + 1, size=1 << 40) == -1 and b'at most' in lib.ppg_last_error()
    assert call_align(lib, most=E.ALIGN_MAX_PHONEMES + 1, size=1 << 40) == -1 and b'at most' in lib.ppg_last_error()
    assert call_align(lib, items=E.ALIGN_MAX_ITEMS + 1, size=1 << 50) == -1 and b'at most' in lib.ppg_last_error()
    assert call_align(lib, size=lib.ppg_align_workspace_bytes(1, 10, 4) - 1) == -1
    assert b'workspace' in lib.ppg_last_error()
    assert call_align(lib, ws=ctypes.c_void_p(264)) == -1 and b'aligned' in lib.ppg_last_error()
    for name in ('ppg', 'lengths', 'phonemes', 'starts', 'runs'):
        assert call_decode(lib, **{name: None}) == -1, name
    assert call_decode(lib, frames=0) == -1 and call_decode(lib, items=-2) == -1
    assert call_decode(lib, frames=E.ALIGN_MAX_FRAMES + 1) == -1 and b'at most' in lib.ppg_last_error()
    assert call_decode(lib, items=E.ALIGN_MAX_ITEMS + 1) == -1


def test_compute_entries_fail_loudly_without_gpu():
    if torch.cuda.is_available():
        pytest.skip('GPU present')
    lib = E.library()
    assert call_align(lib) == -2 and b'no HIP device' in lib.ppg_last_error()
    assert call_align(lib, gop=None) == -2
    assert call_decode(lib) == -2 and b'no HIP device' in lib.ppg_last_error()
    with pytest.raises(E.PpgError):
        alignment.forced(torch.rand(40, 5), ['aa', 'b'])
    with pytest.raises(E.PpgError):
        alignment.decode(torch.rand(40, 5))
