"""The host side of ppgs_amd.alignment.recognize: the float64 reference of the GPU tests against brute force, the
transition-model helpers, the argument errors raised before a device is touched, and the workspace helper."""
import math

import numpy as np
import pytest
import torch

from ppgs_amd import alignment, engine as E
from ppgs_amd.phonemes import PHONEMES

import alignment_reference as F
import recognize_reference as R

INF = math.inf


def integer_case(generator, states, frames, holes):
    """Integer-valued weights, so that every sum is exact and ties are exact; `holes` is the share of -inf entries."""
    e = torch.randint(-3, 1, (frames, states), generator=generator).double().numpy()
    tables = []
    for shape in ((states, states), (states,), (states,)):
        table = torch.randint(-2, 1, shape, generator=generator).double()
        table[torch.rand(shape, generator=generator) < holes] = -INF
        tables.append(table.numpy())
    return (e, *tables)


def test_viterbi_equals_brute_force_in_total_and_path():
    generator = torch.Generator().manual_seed(5)
    seen_none, seen_tie = 0, 0
    for states in (1, 2, 3, 4):
        for frames in (1, 2, 3, 5, 6):
            for holes in (0., 0.3, 0.7):
                for _ in range(3 if states ** frames > 1000 else 8):
                    e, A, initial, final = integer_case(generator, states, frames, holes)
                    total, labels = R.viterbi(e, A, initial, final)
                    ref_total, ref_labels = R.brute_force(e, A, initial, final)
                    assert total == ref_total, (states, frames, holes)
                    if ref_labels is None:
                        assert labels is None and total == -INF
                        seen_none += 1
                        continue
                    assert labels.tolist() == ref_labels.tolist(), (states, frames, holes)
                    assert R.rescore(labels, e, A, initial, final) == total
                    # the float32 restatement walks the same path on exact inputs
                    again, same = R.viterbi(e, A, initial, final, np.float32)
                    assert again == total and same.tolist() == labels.tolist()
                    seen_tie += 1
    assert seen_none >= 5 and seen_tie >= 100                   # both kinds were met
    # every weight -inf at the end: no path
    e, A, initial, final = integer_case(generator, 3, 4, 0.)
    assert R.viterbi(e, A, initial, np.full(3, -INF)) == (-INF, None)
    assert R.brute_force(e, A, initial, np.full(3, -INF)) == (-INF, None)


def test_tie_rule_of_the_reference_by_hand():
    e = np.zeros((5, 3))
    zero = np.zeros(3)
    total, labels = R.viterbi(e, np.zeros((3, 3)), zero, zero)
    assert total == 0 and labels.tolist() == [0] * 5            # staying, and the lowest end state
    swap = -np.eye(3)                                           # staying costs 1, switching nothing
    total, labels = R.viterbi(e, swap, zero, zero)
    assert total == 0 and labels.tolist() == [0, 1, 0, 1, 0]    # label[t] = 0 where T-1-t is even, else 1
    assert R.runs(labels)[0].tolist() == [0, 1, 0, 1, 0] and R.runs(labels)[1].tolist() == [0, 1, 2, 3, 4, 5]
    assert R.expand(*R.runs([4, 4, 2, 2, 2, 4])).tolist() == [4, 4, 2, 2, 2, 4]


def test_chain_makes_the_reference_equal_the_forced_alignment():
    generator = torch.Generator().manual_seed(9)
    for frames, count in ((1, 1), (7, 1), (9, 2), (33, 7), (64, 40), (40, 40), (130, 13)):
        ppg = F.random_ppg(frames, 3., generator)
        sequence = torch.randperm(40, generator=generator)[:count].tolist()
        logp = F.log_posteriors(ppg)
        ref_total, ref_starts = F.programme(F.emissions(logp, sequence))
        A, initial, final = alignment.chain(sequence)
        total, labels = R.viterbi(logp, A.numpy(), initial.numpy(), final.numpy())
        phonemes, starts = R.runs(labels)
        assert phonemes.tolist() == sequence and starts.tolist() == ref_starts.tolist()
        assert total == ref_total                               # the same additions in the same order


def test_switch_penalty():
    matrix = alignment.switch_penalty(2.5)
    assert matrix.shape == (40, 40) and matrix.dtype == torch.float32 and not matrix.is_cuda
    assert bool((matrix.diagonal() == 0).all()) and float(matrix.sum()) == -2.5 * 40 * 39
    assert bool((alignment.switch_penalty(0) == 0).all())
    for bad in (-1., INF, math.nan, None, 'x', True):
        with pytest.raises(ValueError):
            alignment.switch_penalty(bad)


def test_bigram_arithmetic_and_errors():
    sequences = [['aa', 'ae', 'aa', 'ae'], [0, 1, 1], torch.tensor([2])]
    A, initial, final = alignment.bigram(sequences, smoothing=0.5, scale=2.)
    for tensor, shape in ((A, (40, 40)), (initial, (40,)), (final, (40,))):
        assert tuple(tensor.shape) == shape and tensor.dtype == torch.float32
    assert PHONEMES[0] == 'aa' and PHONEMES[1] == 'ae'
    # counts: 0 -> 1 three times, 1 -> 0 once, 1 -> 1 once; firsts 0, 0, 2; lasts 1, 1, 2
    np.testing.assert_allclose(float(A[0, 1]), 2 * math.log(3.5 / 23), rtol=1e-6)
    np.testing.assert_allclose(float(A[0, 0]), 2 * math.log(0.5 / 23), rtol=1e-6)
    np.testing.assert_allclose(float(A[1, 0]), 2 * math.log(1.5 / 22), rtol=1e-6)
    np.testing.assert_allclose(float(A[1, 1]), 2 * math.log(1.5 / 22), rtol=1e-6)
    np.testing.assert_allclose(float(A[5, 7]), 2 * math.log(0.5 / 20), rtol=1e-6)
    np.testing.assert_allclose(float(initial[0]), 2 * math.log(2.5 / 23), rtol=1e-6)
    np.testing.assert_allclose(float(initial[2]), 2 * math.log(1.5 / 23), rtol=1e-6)
    np.testing.assert_allclose(float(final[1]), 2 * math.log(2.5 / 23), rtol=1e-6)
    np.testing.assert_allclose(float(final[3]), 2 * math.log(0.5 / 23), rtol=1e-6)
    # every row is a distribution at scale 1
    A, initial, final = alignment.bigram(sequences)
    np.testing.assert_allclose(A.double().exp().sum(1).numpy(), 1., rtol=1e-5)
    np.testing.assert_allclose(float(initial.double().exp().sum()), 1., rtol=1e-5)
    np.testing.assert_allclose(float(final.double().exp().sum()), 1., rtol=1e-5)
    # without smoothing: -inf for the unseen, and every phoneme needs a successor
    cycle = list(range(40)) + [0]
    A, initial, final = alignment.bigram([cycle], smoothing=0)
    assert float(A[3, 4]) == 0 and float(A[3, 5]) == -INF and float(A[39, 0]) == 0
    assert float(initial[0]) == 0 and float(initial[1]) == -INF and float(final[0]) == 0 and float(final[7]) == -INF
    assert not bool(torch.isnan(A).any())
    with pytest.raises(ValueError, match='without counts'):
        alignment.bigram([[0, 1, 2]], smoothing=0)
    for bad in ([], 'aa', [[]], [['nope']], [[40]], [[0.5]]):
        with pytest.raises(ValueError):
            alignment.bigram(bad)
    for keywords in ({'smoothing': -1.}, {'smoothing': INF}, {'scale': 0.}, {'scale': -1.}, {'scale': math.nan}):
        with pytest.raises(ValueError):
            alignment.bigram(sequences, **keywords)


def test_chain_arithmetic_and_errors():
    A, initial, final = alignment.chain(['hh', 'ah', 'l'])
    s = [PHONEMES.index(name) for name in ('hh', 'ah', 'l')]
    zeros = {(s[0], s[0]), (s[0], s[1]), (s[1], s[1]), (s[1], s[2]), (s[2], s[2])}
    for p in range(40):
        for q in range(40):
            assert float(A[p, q]) == (0 if (p, q) in zeros else -INF)
        assert float(initial[p]) == (0 if p == s[0] else -INF) and float(final[p]) == (0 if p == s[2] else -INF)
    assert A.dtype == initial.dtype == final.dtype == torch.float32
    A, initial, final = alignment.chain([5])
    assert int((A == 0).sum()) == 1 and float(A[5, 5]) == 0 and float(initial[5]) == 0 and float(final[5]) == 0
    assert int((alignment.chain(list(range(40)))[0] == 0).sum()) == 79
    for bad in ([], [1, 2, 1], ['aa', 0], [40], 'aa'):
        with pytest.raises(ValueError):
            alignment.chain(bad)


def test_recognize_refuses_bad_arguments_before_touching_a_device():
    ppg = torch.full((40, 5), 1 / 40)
    good = alignment.switch_penalty(1.)
    zero = torch.zeros(40)
    with pytest.raises(ValueError, match='either'):
        alignment.recognize(ppg)
    with pytest.raises(ValueError, match='either'):
        alignment.recognize(ppg, transitions=good, penalty=1.)
    for penalty in (-1., INF, math.nan, 'x'):
        with pytest.raises(ValueError):
            alignment.recognize(ppg, penalty=penalty)
    for transitions in (torch.zeros(40, 39), torch.zeros(40), torch.zeros(1, 40, 40), [[0.] * 40] * 40,
                        torch.zeros(40, 40, dtype=torch.bool)):
        with pytest.raises(ValueError, match='transitions'):
            alignment.recognize(ppg, transitions=transitions)
    for value in (math.nan, INF):
        bad = good.clone()
        bad[7, 3] = value
        with pytest.raises(ValueError, match='transitions'):
            alignment.recognize(ppg, transitions=bad)
        weights = zero.clone()
        weights[11] = value
        with pytest.raises(ValueError, match='initial'):
            alignment.recognize(ppg, transitions=good, initial=weights)
        with pytest.raises(ValueError, match='final'):
            alignment.recognize(ppg, transitions=good, final=weights)
    for name in ('initial', 'final'):
        for weights in (torch.zeros(39), torch.zeros(40, 1), [0.] * 40):
            with pytest.raises(ValueError, match=name):
                alignment.recognize(ppg, penalty=1., **{name: weights})
    with pytest.raises(ValueError, match='lengths go with a batch'):
        alignment.recognize(ppg, lengths=[5], penalty=1.)
    for lengths in ([5], [5, 6], [0, 5], [5, 5, 5]):
        with pytest.raises(ValueError, match='lengths'):
            alignment.recognize(ppg[None].repeat(2, 1, 1), lengths=lengths, penalty=1.)
    for shape in ((39, 5), (40, 0), (0, 40, 5), (40,), (2, 3, 40, 5)):
        with pytest.raises(ValueError):
            alignment.recognize(torch.zeros(shape), penalty=1.)
    with pytest.raises(ValueError, match='at most 262144 frames'):
        alignment.recognize(torch.zeros(40, 1).expand(40, alignment.RECOGNIZE_MAX_FRAMES + 1), penalty=1.)
    assert alignment.Recognition._fields == alignment.Alignment._fields


def test_workspace_bytes_is_zero_beyond_the_limits_and_grows():
    size = E.library().ppg_recognize_workspace_bytes
    assert E.RECOGNIZE_MAX_FRAMES == 262144 and E.RECOGNIZE_MAX_ITEMS == 65535
    for items, frames in ((0, 10), (10, 0), (-1, 10), (10, -1), (E.RECOGNIZE_MAX_ITEMS + 1, 10),
                          (1, E.RECOGNIZE_MAX_FRAMES + 1)):
        assert size(items, frames) == 0
    assert size(1, 1) > 0 and size(E.RECOGNIZE_MAX_ITEMS, E.RECOGNIZE_MAX_FRAMES) > 0
    # per frame: 176 B prepared, 64 B of back-pointers, 4 B of label
    assert size(1, 4096) >= 4096 * (176 + 64 + 4)
    assert size(E.RECOGNIZE_MAX_ITEMS, E.RECOGNIZE_MAX_FRAMES) >= 65535 * 262144 * (176 + 64 + 4)
    previous = 0
    for items, frames in ((1, 100), (1, 1000), (2, 1000), (64, 1000), (64, 4097), (2048, 4097)):
        assert size(items, frames) > previous
        previous = size(items, frames)
        assert size(items, frames) % 256 == 0
