"""Forced alignment with optional phonemes without a GPU: the tests' float64 programme against brute force over every
(subset of optional phonemes left out x segmentation) on tiny cases, the exported symbols and the host-only workspace
helper, every argument error raised before a device is needed, and the host helpers transcript, word_segments and
frame_labels on hand-written cases."""
import ctypes
import itertools
import math
import os
import re

import numpy as np
import pytest
import torch

import ppgs_amd
from ppgs_amd import alignment, engine as E

import alignment_optional_reference as OR
import alignment_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_declares_and_library_exports_the_entry_points():
    text = open(os.path.join(ROOT, 'include', 'ppgs_amd.h')).read()
    code = re.sub(r'/\*.*?\*/', '', text, flags=re.S)
    for name in ('ppg_align_optional', 'ppg_align_optional_workspace_bytes'):
        assert re.search(r'\b%s\s*\(' % name, code), name
        assert name in E.SYMBOLS and hasattr(E.library(), name)
    assert len(E.SYMBOLS['ppg_align_optional'][1]) == len(E.SYMBOLS['ppg_align'][1]) + 1
    assert E.library().ppg_abi_version() == 1


def legal_flag_sets(count, frames):
    for flags in itertools.product((False, True), repeat=count):
        if OR.legal(flags, frames):
            yield list(flags)


def test_float64_programme_equals_brute_force_on_every_tiny_case():
    rng = np.random.default_rng(23)
    cases = 0
    for frames in range(1, 8):
        for count in range(1, 6):
            for flags in legal_flag_sets(count, frames):
                for kind in range(4):
                    if kind < 3:
                        e = np.log(rng.random((frames, count)))
                    else:                                      # ties among some optima, on values whose sums are exact
                        e = -rng.integers(0, 3, (frames, count)).astype(np.float64) / 4
                    total, starts = OR.programme(e, flags)
                    brute_total, optima = OR.brute_force(e, flags)
                    assert total == brute_total, (frames, count, flags)    # the same sums in the same order
                    assert OR.path_total(e, starts) == total, (frames, count, flags)
                    assert tuple(starts.tolist()) in optima, (frames, count, flags)
                    OR.check_starts(starts, frames, flags)
                    cases += 1
    assert cases > 600
    # without optional phonemes it is the plain programme, boundaries included
    for frames, count in ((1, 1), (5, 3), (7, 7), (30, 11)):
        e = np.log(rng.random((frames, count)))
        total, starts = OR.programme(e, [False] * count)
        plain_total, plain_starts = R.programme(e)
        assert total == plain_total and starts.tolist() == plain_starts.tolist()


def test_float64_programme_on_tables_worked_by_hand():
    # phoneme 1 is optional and fits nowhere: 0 0 | 2 2, phoneme 1 empty at frame 2
    e = np.array([[-1., -9., -9.], [-1., -9., -9.], [-9., -9., -1.], [-9., -9., -1.]])
    total, starts = OR.programme(e, [False, True, False])
    assert total == -4. and starts.tolist() == [0, 2, 2, 4]
    # ... and is present where it pays
    e[1] = [-9., -1., -9.]
    total, starts = OR.programme(e, [False, True, False])
    assert total == -4. and starts.tolist() == [0, 1, 2, 4]
    # an optional first phoneme left out: the path begins in state 1; an optional last one left out: it ends in N - 2
    e = np.array([[-9., -1., -9.], [-9., -1., -9.], [-9., -1., -9.]])
    total, starts = OR.programme(e, [True, False, True])
    assert total == -3. and starts.tolist() == [0, 0, 3, 3]
    # every cell ties: staying wins wherever the state was reachable, so every state is entered as early as it can
    # be -- the last one at frame 1 by the skip over phoneme 1, which is the only way to be there that early
    total, starts = OR.programme(np.zeros((5, 3)), [False, True, False])
    assert total == 0. and starts.tolist() == [0, 1, 1, 5]
    # ... here by an advance from state 1, where the path began: phoneme 0 is left out, and the tie at the end keeps N - 1
    total, starts = OR.programme(np.zeros((5, 3)), [True, False, True])
    assert total == 0. and starts.tolist() == [0, 0, 1, 5]
    # an advance is as good as a skip: the advance is taken (states 1 and 2 are both reachable at frame 1 and 2)
    total, starts = OR.programme(np.zeros((3, 3)), [False, True, False])
    assert starts.tolist() == [0, 1, 1, 3]
    e = np.array([[0., -9., -9.], [-9., 0., -9.], [-1., -1., 0.], [-9., -9., 0.]])
    e[1, 0] = 0.                                              # D[1, 0] == D[1, 1]: into state 2 by advance, not by skip
    total, starts = OR.programme(e, [False, True, False])
    assert total == 0. and starts.tolist() == [0, 1, 2, 4]
    # T equal to the mandatory count: every optional phoneme is left out
    total, starts = OR.programme(np.zeros((2, 5)), [True, False, True, False, True])
    assert starts.tolist() == [0, 0, 1, 1, 2, 2]
    # N > T
    total, starts = OR.programme(-np.ones((1, 3)), [True, False, True])
    assert total == -1. and starts.tolist() == [0, 0, 1, 1]
    # scores: NaN for the phonemes left out, alignment_reference's values for the others
    ppg = torch.full((40, 3), 0.01)
    ppg[3] = 0.5
    logp = R.log_posteriors(ppg)
    score, gop = OR.scores(logp, [39, 3, 39], [0, 0, 3, 3])
    assert math.isnan(score[0]) and math.isnan(gop[2]) and gop[1] == 0.
    assert np.isclose(score[1], np.log(np.float32(0.5)))


def test_workspace_helper_is_host_only_and_zero_outside_the_limits():
    size = E.library().ppg_align_optional_workspace_bytes
    plain = E.library().ppg_align_workspace_bytes
    assert 0 < size(1, 1, 1) < 1 << 12
    for items, frames, phonemes in ((1, 1, 1), (1, 57, 9), (3, 300, 64), (2, 1000, 120), (64, 1000, 257),
                                    (1, 4096, 1024)):
        here = size(items, frames, phonemes)
        # the plain workspace, a second plane of direction bits and the end state of every item
        assert here >= plain(items, frames, phonemes) + items * frames * 128 + items * 4
        assert here <= items * frames * (176 + 256) + items * 4 + 4096
        assert size(items + 1, frames, phonemes) > here
    assert size(E.ALIGN_MAX_ITEMS, 4096, 1024) > 1 << 36                 # never a wrapped number
    for bad in ((0, 10, 5), (-1, 10, 5), (1, 0, 5), (1, 10, 0), (1, -4, 5), (1, 10, -1),
                (E.ALIGN_MAX_ITEMS + 1, 10, 5), (1, E.ALIGN_MAX_FRAMES + 1, 5), (1, 10, E.ALIGN_MAX_PHONEMES + 1)):
        assert size(*bad) == 0, bad


def call_optional(lib, **changes):
    dummy = ctypes.c_void_p(256)
    a = dict(ppg=dummy, frames=10, items=1, lengths=dummy, phonemes=dummy, optional=dummy, most=4, counts=dummy,
             total=dummy, starts=dummy, score=dummy, gop=dummy, ws=dummy,
             size=lib.ppg_align_optional_workspace_bytes(1, 10, 4))
    a.update(changes)
    return lib.ppg_align_optional(0, a['ppg'], a['frames'], a['items'], a['lengths'], a['phonemes'], a['optional'],
                                  a['most'], a['counts'], a['total'], a['starts'], a['score'], a['gop'], a['ws'],
                                  a['size'], None)


def test_bad_arguments_return_einval():
    lib = E.library()
    for name in ('ppg', 'lengths', 'phonemes', 'optional', 'counts', 'total', 'starts', 'score', 'ws'):
        assert call_optional(lib, **{name: None}) == -1, name
    assert call_optional(lib, frames=0) == -1 and call_optional(lib, items=0) == -1
    assert call_optional(lib, most=0) == -1
    assert call_optional(lib, frames=E.ALIGN_MAX_FRAMES + 1, size=1 << 40) == -1 and b'at most' in lib.ppg_last_error()
    assert call_optional(lib, most=E.ALIGN_MAX_PHONEMES + 1, size=1 << 40) == -1 and b'at most' in lib.ppg_last_error()
    assert call_optional(lib, items=E.ALIGN_MAX_ITEMS + 1, size=1 << 50) == -1 and b'at most' in lib.ppg_last_error()
    # the plain workspace is too small for it
    assert call_optional(lib, size=lib.ppg_align_workspace_bytes(1, 10, 4)) == -1
    assert b'workspace' in lib.ppg_last_error()
    assert call_optional(lib, ws=ctypes.c_void_p(264)) == -1 and b'aligned' in lib.ppg_last_error()


def test_compute_entry_fails_loudly_without_gpu():
    if torch.cuda.is_available():
        pytest.skip('GPU present')
    lib = E.library()
    assert call_optional(lib) == -2 and b'no HIP device' in lib.ppg_last_error()
    assert call_optional(lib, gop=None) == -2
    with pytest.raises(E.PpgError):
        alignment.forced(torch.rand(40, 5), ['aa', 'b'], optional=[False, True])
    with pytest.raises(E.PpgError):                                      # more phonemes than frames is legal here
        alignment.forced(torch.rand(40, 2), ['<silent>', 'aa', '<silent>', 'b', '<silent>'],
                         optional=[True, False, True, False, True])


def test_value_errors_come_before_any_device_call():
    x, bx = torch.rand(40, 5), torch.rand(3, 40, 5)
    names = ['aa', 'b', 'd']
    cases = [
        (x, names, {'optional': [False, True]}),                         # a length mismatch
        (x, names, {'optional': [False, True, False, False]}),
        (x, names, {'optional': torch.tensor([False, True])}),
        (x, names, {'optional': [False, True, True]}),                   # adjacent optional phonemes
        (x, names, {'optional': [True, True, False]}),
        (x, names, {'optional': [True, True, True]}),                    # no mandatory phoneme
        (x, ['aa'], {'optional': [True]}),
        (x, ['aa', 'b'] * 6, {'optional': [False, True] * 6}),           # more mandatory phonemes than frames
        (torch.rand(40, 2), names, {'optional': [False, False, False]}),
        (x, names, {'optional': 'no'}),                                  # not flags at all
        (x, names, {'optional': [False, 0.5, False]}),
        (x, names, {'optional': torch.tensor([0., 1., 0.])}),
        (x, names, {'optional': [[False, True, False]]}),
        (bx, [names] * 3, {'optional': [False, True, False]}),           # one list per item
        (bx, [names] * 3, {'optional': [[False, True, False]] * 2}),
        (bx, [names] * 3, {'optional': [[False, True, False], [False, True], [False] * 3]}),
        (bx, [names] * 3, {'optional': [[False, True, False], [True, True, False], [False] * 3]}),
        (bx, [names] * 3, {'optional': torch.zeros(2, 3, dtype=torch.bool)}),        # table rows
        (bx, [names] * 3, {'optional': torch.zeros(3, 2, dtype=torch.bool)}),        # table width
        (bx, [names] * 3, {'optional': torch.ones(3, 3, dtype=torch.int32)}),        # every phoneme optional
        (bx, torch.zeros(3, 4, dtype=torch.int64), {'optional': torch.tensor([[0, 1, 1, 0]] * 3)}),
        (bx, [names] * 3, {'optional': [[False] * 3] * 3, 'lengths': [5, 2, 5]}),    # the item's own frames
        (torch.rand(40, 2000), [0] * (alignment.MAX_PHONEMES + 1), {'optional': [False, True] * 512 + [False]}),
        (x, [], {'optional': []}),
    ]
    for ppg, phonemes, keywords in cases:
        with pytest.raises(ValueError):
            alignment.forced(ppg, phonemes, **keywords)
    # without `optional` more phonemes than frames stay an error; the checks on the transcript itself stay as well
    with pytest.raises(ValueError):
        alignment.forced(x, [1, 2, 3, 4, 5, 6])
    with pytest.raises(ValueError):
        alignment.forced(x, [1, 2, 40], optional=[False, True, False])
    with pytest.raises(ValueError):
        alignment.forced(x, names, optional=None, phoneme_lengths=[3])


def test_transcript_and_word_segments_on_a_hand_written_case():
    phonemes, optional, word_of = alignment.transcript([['hh', 'ah'], ['l', 'ow']])
    assert phonemes == ['<silent>', 'hh', 'ah', '<silent>', 'l', 'ow', '<silent>']
    assert optional == [True, False, False, True, False, False, True]
    assert word_of == [-1, 0, 0, -1, 1, 1, -1]
    assert alignment.transcript([['hh', 'ah'], ['l', 'ow']], silence=False) == (
        ['hh', 'ah', 'l', 'ow'], [False] * 4, [0, 0, 1, 1])
    assert alignment.transcript([[0], [39, 1]])[0] == ['<silent>', 'aa', '<silent>', '<silent>', 'ae', '<silent>']
    assert alignment.transcript([('aa',)]) == (['<silent>', 'aa', '<silent>'], [True, False, True], [-1, 0, -1])
    for bad in ([], 'hh', [[]], [['hh'], []], [['xx']], ['hh', 'ah'], [[40]]):
        with pytest.raises(ValueError):
            alignment.transcript(bad)
    assert OR.legal(optional, 4) and not OR.legal(optional, 3)

    # the leading pause and the one between the words were made, the trailing one was not; 'ow' has no gop to speak of
    index = [ppgs_amd.PHONEME_TO_INDEX_MAPPING[name] for name in phonemes]
    nan = float('nan')
    one = alignment.Alignment(
        torch.tensor(index, dtype=torch.int32), torch.tensor([0, 3, 5, 9, 10, 12, 16, 16], dtype=torch.int32),
        torch.tensor(-3.), torch.tensor([-0.5, -0.25, -0.5, -1., -0.5, -0.125, nan]),
        torch.tensor([0., -0.25, -0.75, 0., -1., 0., nan]))
    words = alignment.word_segments(one, word_of)
    assert words == [(0, 0.03, 0.09, -0.5), (1, 0.10, 0.16, -0.5)]
    assert alignment.word_segments(one, word_of, sample_rate=8000, hopsize=80)[1][1:3] == (0.10, 0.16)
    assert alignment.word_segments(one, word_of, sample_rate=16000, hopsize=320)[0][1:3] == (0.06, 0.18)
    assert [w[3] for w in alignment.word_segments(one._replace(gop=None), word_of)] == [None, None]
    # a word with a phoneme that may be dropped and was: the mean runs over the present ones only; none present: NaN
    dropped = one._replace(starts=torch.tensor([0, 3, 5, 5, 10, 12, 12, 12], dtype=torch.int32),
                           gop=torch.tensor([0., -0.25, nan, 0., -1., nan, nan]))
    words = alignment.word_segments(dropped, [-1, 0, 0, -1, 1, 2, -1])
    assert words[0] == (0, 0.03, 0.05, -0.25) and words[1] == (1, 0.10, 0.12, -1.)
    assert words[2][:3] == (2, 0.12, 0.12) and math.isnan(words[2][3])
    # segments reports the phonemes left out as empty segments with NaN
    listed = alignment.segments(one)
    assert listed[6][0] == '<silent>' and listed[6][1] == listed[6][2] == 0.16 and math.isnan(listed[6][4])
    batch = alignment.Alignment([one.phonemes, one.phonemes[:3]], [one.starts, torch.tensor([0, 3, 5, 9])],
                                torch.zeros(2), [one.score, one.score[:3]], [one.gop, one.gop[:3]])
    both = alignment.word_segments(batch, [word_of, word_of[:3]])
    assert both[0] == alignment.word_segments(one, word_of) and both[1] == [(0, 0.03, 0.09, -0.5)]
    for bad in (word_of[:-1], word_of + [-1], [-1, 0, 1, 0, 1, 1, -1], [-1, 0, 0, -2, 1, 1, -1]):
        with pytest.raises(ValueError):
            alignment.word_segments(one, bad)
    with pytest.raises(ValueError):
        alignment.word_segments(batch, [word_of])


def test_frame_labels_steps_over_empty_segments():
    # bucketize(right=True) counts the boundaries at or below t: duplicates are stepped over together, so a phoneme
    # with an empty segment labels no frame -- in the middle, at the start and at the end
    phonemes = torch.tensor([39, 5, 39, 7, 39], dtype=torch.int32)
    for starts, expected in (
            ([0, 2, 4, 4, 6, 7], [39, 39, 5, 5, 7, 7, 39]),              # the middle pause left out
            ([0, 0, 3, 4, 7, 7], [5, 5, 5, 39, 7, 7, 7]),                # the first and the last
            ([0, 0, 3, 3, 7, 7], [5, 5, 5, 7, 7, 7, 7]),                 # all three
            ([0, 1, 2, 3, 4, 7], [39, 5, 39, 7, 39, 39, 39])):           # none
        labels = alignment.frame_labels(torch.tensor(starts, dtype=torch.int32), phonemes, 7)
        assert labels.dtype == torch.int32 and labels.tolist() == expected, starts
    # every reference segmentation with optional phonemes expands to the labels it means
    rng = np.random.default_rng(5)
    for frames, count in ((1, 3), (4, 7), (9, 9), (30, 13)):
        flags = [n % 2 == 0 for n in range(count)]
        _, cuts = OR.programme(np.log(rng.random((frames, count))), flags)
        names = rng.integers(0, 40, count)
        labels = alignment.frame_labels(torch.from_numpy(cuts), torch.from_numpy(names), frames)
        assert labels.tolist() == np.repeat(names, np.diff(cuts)).tolist()
