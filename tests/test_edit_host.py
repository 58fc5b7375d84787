"""The edit distance without a GPU: the tests' own fp32 emulation (tests/edit_reference.py) is pinned by a cell-by-cell
walk, the identities and the anchor cases of DESIGN 4.21; every mutant of it is caught by a named probe (and which
probes are blind to which mutant is on record); the C ABI is declared and exported, its workspace helper is host-only,
the compute entry fails loudly without a device, and every argument error of alignment.edit_distance and
evaluate.ErrorRate is raised before a device is needed."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import ppgs_amd
from ppgs_amd import alignment, engine as E, evaluate

import edit_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
A, B = 0, 1


def test_the_two_emulations_agree():
    rng = np.random.default_rng(0)
    for case in range(150):
        rows, columns = rng.integers(0, 13, 2)
        symbols = int(rng.integers(2, 5))
        ref, hyp = rng.integers(0, symbols, rows), rng.integers(0, symbols, columns)
        costs = R.random_costs(case) if case % 2 else R.UNIT
        assert R.same(R.edit(ref, hyp, *costs), R.edit_plain(ref, hyp, *costs)), (ref, hyp, case)


def test_identities():
    rng = np.random.default_rng(1)
    for case in range(40):
        rows, columns = rng.integers(0, 40, 2)
        ref, hyp = rng.integers(0, 3, rows), rng.integers(0, 3, columns)
        for costs in (R.UNIT, R.random_costs(case)):
            total, (hits, subs, dels, inss), ops = R.edit(ref, hyp, *costs)
            assert hits + subs + dels == rows and hits + subs + inss == columns and len(ops) == hits + subs + dels + inss
            if costs is R.UNIT:
                assert total == subs + dels + inss
            # the operations visit every token of either side once and in order
            assert ops[ops[:, 0] != 3, 1].tolist() == list(range(rows))
            assert ops[ops[:, 0] != 2, 2].tolist() == list(range(columns))
            assert all(ref[i] == hyp[j] for kind, i, j in ops if kind == 0)
            assert all(ref[i] != hyp[j] for kind, i, j in ops if kind == 1)
            assert R.histogram(ops, ref, hyp).sum() == len(ops)


def test_anchor_cases():
    assert R.edit([A, B], [B, A])[1] == (0, 2, 0, 0)
    assert R.edit([A, B, A], [B, A, B])[1] == (2, 0, 1, 1)
    assert R.edit([A, A], [A])[2].tolist() == [[2, 0, -1], [0, 1, 0]]            # del a0, hit (1, 0)
    assert R.edit([A], [A, A])[2].tolist() == [[3, -1, 0], [0, 0, 1]]            # ins a0, hit (0, 1)
    total, counts, ops = R.edit(*R.PROBES['a_b_dear_sub'][:2], *R.PROBES['a_b_dear_sub'][2])
    assert total == 2 and ops.tolist() == [[3, -1, 0], [2, 0, -1]]               # ins b, then del a
    # what the other rules would have given
    assert R.edit([A, B], [B, A], mutant='deletion_first')[1] == (1, 0, 1, 1)
    dear = R.PROBES['a_b_dear_sub']
    assert R.edit(*dear[:2], *dear[2], mutant='insertion_first')[2].tolist() == [[2, 0, -1], [3, -1, 0]]
    assert R.edit([], [])[0] == 0 and R.edit([], [])[1] == (0, 0, 0, 0)
    assert R.edit([], [A, B])[1] == (0, 0, 0, 2) and R.edit([A, B], [])[1] == (0, 0, 2, 0)


# mutant -> the probes that catch it; every other probe is blind to it
CATCHES = {
    'deletion_first': {'ab_ba', 'ties2_260x79', 'ties3_257x64', 'ties2_513x130', 'antiphase_300x100'},
    'insertion_first': {'a_b_dear_sub', 'costs_60x70', 'costs_300x517'},
    'not_strict': {'ab_ba', 'a_b_dear_sub', 'ties2_260x79', 'ties3_257x64', 'ties2_513x130', 'ties3_130x513',
                   'antiphase_300x100', 'costs_60x70', 'costs_300x517'},
    'kind_by_cost': {'free_sub', 'costs_60x70', 'costs_300x517'},
    'edge_scan': {'costs_300x0', 'costs_0x300'},
    'block_top_inf': {'ties2_260x79', 'ties3_257x64', 'ties2_513x130', 'antiphase_300x100', 'costs_300x517'},
    'block_top_shifted': {'ties2_260x79', 'ties3_257x64', 'ties2_513x130', 'antiphase_300x100', 'costs_300x517'},
    'strip_row': {'ties2_260x79', 'ties3_257x64', 'ties2_513x130', 'ties3_130x513', 'antiphase_300x100',
                  'costs_60x70', 'costs_300x517'},
    'trace_neighbour': {'ties2_260x79', 'ties3_257x64', 'ties2_513x130', 'ties3_130x513', 'antiphase_300x100',
                        'costs_60x70', 'costs_300x517'},
}


@pytest.fixture(scope='module')
def expected():
    return {name: R.edit(ref, hyp, *costs) for name, (ref, hyp, costs) in R.PROBES.items()}


@pytest.mark.parametrize('mutant', sorted(R.MUTANTS))
def test_every_mutant_is_caught_by_a_named_probe(mutant, expected):
    assert set(CATCHES) == set(R.MUTANTS)
    caught = {name for name, (ref, hyp, costs) in R.PROBES.items()
              if not R.same(R.edit(ref, hyp, *costs, mutant=mutant), expected[name])}
    print(f'{mutant}: caught by {sorted(caught)}; blind: {sorted(set(R.PROBES) - caught)}')
    assert caught, mutant
    assert caught == CATCHES[mutant]


def test_header_declares_and_library_exports_the_entry_points():
    text = open(os.path.join(ROOT, 'include', 'ppgs_amd.h')).read()
    code = re.sub(r'/\*.*?\*/', '', text, flags=re.S)
    for name in ('ppg_edit_distance', 'ppg_edit_workspace_bytes'):
        assert re.search(r'\b%s\s*\(' % name, code), name
        assert name in E.SYMBOLS and hasattr(E.library(), name)
    assert int(re.search(r'#define\s+PPG_EDIT_MAX_TOKENS\s+(\d+)', code).group(1)) == 4096 == E.EDIT_MAX_TOKENS
    assert alignment.EDIT_MAX_TOKENS == 4096
    assert int(re.search(r'#define\s+PPG_EDIT_MAX_PAIRS\s+(\d+)', code).group(1)) == 65535 == E.EDIT_MAX_PAIRS
    assert E.EDIT_STATISTICS == 41 * 41 + 2
    assert ppgs_amd.evaluate.ErrorRate is evaluate.ErrorRate


def test_workspace_helper():
    size = E.library().ppg_edit_workspace_bytes
    assert 0 < size(1, 0, 0, 0) <= 256 and 0 < size(1, 0, 0, 1) <= 512
    for pairs, rows, columns in ((1, 57, 43), (3, 300, 1), (2, 1000, 1000), (1, 4096, 4096), (7, 0, 200)):
        plain, ops = size(pairs, rows, columns, 0), size(pairs, rows, columns, 1)
        assert 0 < plain <= 4 * pairs + 256                         # no table at all without ops
        assert ops >= plain + pairs * rows * (columns + 1)           # + a direction byte per cell
        # no more than the documented padding: rows to a multiple of 256, columns + 64
        assert ops <= plain + pairs * (-(-rows // 256) * 256) * (columns + 64) + 256
        assert size(pairs + 1, rows, columns, 1) >= ops
    assert size(1, 4096, 4096, 1) < 1 << 25
    for bad in ((0, 10, 10, 0), (-1, 10, 10, 0), (1, -1, 10, 0), (1, 10, -1, 1), (1, 4097, 10, 0), (1, 10, 4097, 1),
                (65536, 10, 10, 0)):
        assert size(*bad) == 0, bad


def test_compute_entry_fails_loudly_without_gpu():
    if torch.cuda.is_available():
        pytest.skip('GPU present')
    lib = E.library()
    dummy = ctypes.c_void_p(256)
    need = lib.ppg_edit_workspace_bytes(1, 10, 12, 1)
    rc = lib.ppg_edit_distance(0, dummy, 10, dummy, 12, 1, dummy, dummy, None, None, None, dummy, dummy, dummy, dummy,
                               dummy, dummy, need, None)
    assert rc == -2 and b'no HIP device' in lib.ppg_last_error()


def test_refusals_need_no_device():
    lib = E.library()
    dummy = ctypes.c_void_p(256)
    need = lib.ppg_edit_workspace_bytes(2, 10, 12, 1)

    def call(ref=dummy, rows=10, hyp=dummy, columns=12, pairs=2, len_ref=dummy, len_hyp=dummy, sub=None, dele=None,
             ins=None, total=dummy, counts=dummy, ops=dummy, ops_length=dummy, statistics=dummy, workspace=dummy,
             size=need):
        return lib.ppg_edit_distance(0, ref, rows, hyp, columns, pairs, len_ref, len_hyp, sub, dele, ins, total,
                                     counts, ops, ops_length, statistics, workspace, size, None)
    refused = [dict(ref=None), dict(hyp=None), dict(len_ref=None), dict(len_hyp=None), dict(total=None),
               dict(counts=None), dict(workspace=None), dict(pairs=0), dict(pairs=65536), dict(rows=4097),
               dict(columns=4097), dict(rows=-1), dict(size=need - 1), dict(workspace=ctypes.c_void_p(264)),
               dict(ops_length=None), dict(ops=None, ops_length=None), dict(ops=None, statistics=None),
               dict(sub=dummy), dict(sub=dummy, dele=dummy), dict(dele=dummy, ins=dummy)]
    for arguments in refused:
        assert call(**arguments) == -1, arguments
        assert lib.ppg_last_error().startswith(b'edit:')


def test_edit_distance_checks_its_arguments_first():
    bad = [
        dict(reference=['aa', 'nope'], hypothesis=['aa']),                     # an unknown name
        dict(reference=[0, 40], hypothesis=[1]),                                 # an index out of range
        dict(reference=[0, 1.5], hypothesis=[1]),
        dict(reference='aa', hypothesis=['aa']),                                 # a string is not a sequence
        dict(reference=torch.zeros(3), hypothesis=[1]),                          # a floating-point tensor
        dict(reference=torch.zeros((2, 2), dtype=torch.long), hypothesis=[1]),
        dict(reference=[0] * 4097, hypothesis=[1]),                              # too long
        dict(reference=[1], hypothesis=torch.zeros(4097, dtype=torch.int32)),
        dict(reference=[[0], [1]], hypothesis=[[0]]),                            # a batch of two against one
        dict(reference=[[0], [1]], hypothesis=[0, 1]),                           # a batch against a pair
        dict(reference=[torch.tensor(0), torch.tensor(1)], hypothesis=[0, 1]),   # 0-d tensors are not indices
        dict(reference=[0], hypothesis=[1], sub=torch.ones(40, 39)),
        dict(reference=[0], hypothesis=[1], sub=-torch.ones(40, 40)),
        dict(reference=[0], hypothesis=[1], delete=torch.full((40,), float('inf'))),
        dict(reference=[0], hypothesis=[1], insert=torch.full((40,), float('nan'))),
        dict(reference=[0], hypothesis=[1], insert=[1.] * 40),
        dict(reference=[0], hypothesis=[1], ignore=['nope']),
        dict(reference=[0], hypothesis=[1], ignore=[40]),
    ]
    for arguments in bad:
        with pytest.raises(ValueError):
            alignment.edit_distance(**arguments)
    if not torch.cuda.is_available():
        with pytest.raises(E.PpgError):
            alignment.edit_distance([0, 1], [1])


def test_what_is_a_pair_and_what_a_batch():
    sides = alignment._edit_sides
    assert sides(['aa', 'b'], ['b']) == (False, [['aa', 'b']], [['b']])
    assert sides([], []) == (False, [[]], [[]])                               # one pair of empty sequences
    assert sides([], [1, 2]) == (False, [[]], [[1, 2]])
    assert sides([['aa', 'b']], [['b']]) == (True, [['aa', 'b']], [['b']])
    assert sides([[], [1]], ([2], []))[0] is True
    one = torch.tensor([1, 2])
    assert sides([one], [[1]])[0] is True and sides(one, [1])[0] is False
    assert sides([torch.tensor(1)], [1])[0] is False                           # a sequence; _sequence refuses its members
    with pytest.raises(ValueError, match='a phoneme must be a name or an index'):
        alignment.edit_distance([torch.tensor(1)], [1])
    for reference, hypothesis in (([[1]], [1]), ([[1], [2]], [[1]]), ([], [[1]])):
        with pytest.raises(ValueError, match='a batch is two lists'):
            sides(reference, hypothesis)


def test_error_rate_checks_its_arguments_first():
    for arguments in (dict(sub=torch.ones(3, 3)), dict(delete=-torch.ones(40)), dict(ignore=['nope']),
                      dict(insert=torch.full((40,), float('nan')))):
        with pytest.raises(ValueError):
            evaluate.ErrorRate(**arguments)
    if not torch.cuda.is_available():
        with pytest.raises(E.PpgError):
            evaluate.ErrorRate()


def test_costs_and_ignore_on_the_host():
    assert alignment.edit_costs() is None
    sub, delete, insert = alignment.edit_costs(delete=2 * torch.ones(40, dtype=torch.float64))
    assert sub.dtype == delete.dtype == insert.dtype == torch.float32
    assert torch.equal(sub, 1 - torch.eye(40)) and torch.equal(delete, 2 * torch.ones(40)) and \
        torch.equal(insert, torch.ones(40))
    silent = ppgs_amd.PHONEME_TO_INDEX_MAPPING['<silent>']
    assert alignment._ignored('<silent>') == [silent] == alignment._ignored(['<silent>', silent])
    assert alignment._ignored(None) == []
    rows = alignment._edit_rows([['aa', '<silent>', 'ae'], [], torch.tensor([silent, silent])], 'reference', [silent])
    assert rows == [[ppgs_amd.PHONEME_TO_INDEX_MAPPING['aa'], ppgs_amd.PHONEME_TO_INDEX_MAPPING['ae']], [], []]


def test_result_dict_from_statistics():
    words = np.zeros(E.EDIT_STATISTICS, dtype=np.int64)
    table = words[:-2].reshape(41, 41)
    table[0, 0], table[0, 1], table[1, 40], table[40, 3], words[-2] = 5, 2, 1, 4, 3
    results = evaluate.format_error_rate(words)
    assert results['PER'] == 7 / 8 and results['Pairs'] == 3 and results['Reference phonemes'] == 8
    assert (results['Hits'], results['Substitutions'], results['Deletions'], results['Insertions']) == (5, 2, 1, 4)
    names = ppgs_amd.PHONEMES
    assert results[f'PER/{names[0]}'] == 2 / 7 and results[f'PER/{names[1]}'] == 1.0
    assert np.isnan(results[f'PER/{names[2]}']) and results[f'Insertions/{names[3]}'] == 4
    assert len(results) == 7 + 2 * 40
    assert np.isnan(evaluate.format_error_rate(np.zeros(E.EDIT_STATISTICS, dtype=np.int64))['PER'])
    words[-1] = 2
    with pytest.raises(ValueError, match='2 pairs'):
        evaluate.format_error_rate(words)
