"""tests/dtw_probe.py without a GPU: the fp32 programme that tests/test_gpu_dtw_probe.py holds the device to is the
documented recurrence (it agrees with the float64 programme of dtw_reference.py wherever the table is exactly
representable, and with the tables worked by hand in test_dtw_host.py), every mutant of it is caught by a named probe
input, and the inputs the suite had before catch none of them.

The device's cell costs are replaced here by tables of the same structure: integer 0 / 1 for the symbols of equal cost,
a fixed random 16 x 16 fp32 table with a zero diagonal for the alphabet."""
import numpy as np
import pytest

import dtw_probe as D
import dtw_reference as R

# mutant -> the probe (kind, Tx, Ty) that has to catch it; test_every_mutant_is_caught prints all that do
CAUGHT_BY = {
    'up_first': ('alphabet_mix', 257, 65),
    'left_before_up': ('equal_cost', 257, 65),
    'less_equal': ('equal_cost', 4, 4),
    'count_from_diagonal': ('alphabet_plain', 5, 3),
    'edge_row_inf': ('alphabet_mix', 257, 65),
    'edge_row_shifted': ('alphabet_plain', 513, 130),
    'edge_count': ('equal_cost', 769, 9),
    'strip_carry': ('alphabet_mix', 9, 1),
    'dir_byte': ('alphabet_plain', 65, 257),
}


def table_of(kind, frames_x, frames_y, transpose=False):
    sx, sy = D.probe(kind, frames_x, frames_y)
    return D.cost_table(D.host_cells(kind), sy, sx) if transpose else D.cost_table(D.host_cells(kind), sx, sy)


def test_programme32_is_the_documented_recurrence():
    # the tables worked by hand in test_dtw_host.py
    total, count, path = D.programme32([[1, 2, 3, 4], [2, 1, 2, 3], [3, 2, 1, 1]])
    assert total == 4 and total.dtype == np.float32 and count == 4
    assert path.tolist() == [[0, 0], [1, 1], [2, 2], [2, 3]]
    assert D.programme32(np.zeros((2, 2)))[2].tolist() == [[0, 0], [1, 1]]
    total, count, path = D.programme32([[0, -1], [-1, 5]])
    assert total == 4 and count == 3 and path.tolist() == [[0, 0], [0, 1], [1, 1]]
    assert D.programme32([[1, 2, 3]])[1:][0] == 3 and D.programme32([[1], [2], [3]])[2].tolist() == [[0, 0], [1, 0], [2, 0]]
    # 0 / 1 tables and small-integer tables are exact in fp32 and float64 alike: same total, same path, K = its length
    rng = np.random.default_rng(1)
    tables = [table_of('equal_cost', *shape) for shape in D.SHAPES_TINY + ((257, 65), (65, 257), (300, 300), (513, 130))]
    tables += [rng.integers(0, 4, shape).astype(np.float32) for shape in ((7, 9), (63, 65), (257, 5), (80, 261))]
    for table in tables:
        total, count, path = D.programme32(table)
        ref_total, ref_path = R.dtw(table)
        assert float(total) == ref_total and count == len(ref_path) and np.array_equal(path, ref_path), table.shape
        R.check_path(path, *table.shape)
    # fp32 for fp32's sake: 2^24 + 1 is not a float32
    total, _, _ = D.programme32([[2.0 ** 24, 1.0]])
    assert total == np.float32(2.0 ** 24) and R.dtw([[2.0 ** 24, 1.0]])[0] == 2.0 ** 24 + 1


def test_probe_inputs_are_what_they_claim():
    frames = D.alphabet()
    assert frames.shape == (16, 40) and len({tuple(f.tolist()) for f in frames}) == 16
    a, b, c = D.equal_cost_symbols()
    p, q, r = D.SWAPPED
    assert a[q] == a[r] and a[p] != a[q]
    assert (a != b).nonzero().flatten().tolist() == [p, q] and (a != c).nonzero().flatten().tolist() == [p, r]
    assert (b != c).nonzero().flatten().tolist() == [q, r]
    assert sorted(D.SHAPES) == sorted(set(D.SHAPES)) and len(D.SHAPES) == 25
    for kind, (_, symbols, _, _) in D.KINDS.items():
        for frames_x, frames_y in D.SHAPES:
            sx, sy = D.probe(kind, frames_x, frames_y)
            assert sx.shape == (frames_x,) and sy.shape == (frames_y,)
            assert 0 <= min(sx.min(), sy.min()) and max(sx.max(), sy.max()) < symbols
            again = D.sequences(frames_x, frames_y, symbols, 7, D.KINDS[kind][3])
            assert np.array_equal(again[0], sx) and np.array_equal(again[1], sy)
    # the features sit on the edges they are meant for
    sx, sy = D.probe('alphabet_mix', 513, 130)
    assert sx[255] == sx[256] and sx[511] == sx[512] and (sx[6:11] == sx[6]).all()
    sx, sy = D.probe('alphabet_mix', 130, 513)
    assert sy[255] == sy[256] and sy[511] == sy[512] and (sy[60:68] == sy[60]).all()
    sx, sy = D.probe('alphabet_plain', 513, 130)
    column = 256 * 130 // 513
    assert (sy[column:column + 7] == sx[256]).all() and sx[511] == sx[512]
    sx, sy = D.probe('equal_cost', 513, 130)
    for start in (2, 250):
        assert (sx[start:start + 8:2] == sx[start]).all() and (sx[start + 1:start + 9:2] == sx[start + 1]).all()
        assert sx[start] != sx[start + 1]
    assert (sy[60:70:2] == sy[60]).all() and (sy[61:71:2] == sy[61]).all() and sy[60] != sy[61]
    assert sx[14:20].tolist() == [1, 2, 0, 1, 2, 1] and sy[14:21].tolist() == [1, 2, 2, 1, 0, 2, 1]


def catches(kind, frames_x, frames_y, mutants, transpose=False):
    table = table_of(kind, frames_x, frames_y, transpose)
    base = D.programme32(table)
    return [m for m in mutants if not D.same(base, D.programme32(table, m))]


def test_every_mutant_is_caught_by_a_named_probe():
    for mutant, where in CAUGHT_BY.items():
        assert catches(*where, [mutant]) == [mutant], (mutant, where)
    # and by how many of the probes: one line per mutant
    caught = {m: [] for m in D.MUTANTS}
    for kind in D.KINDS:
        for frames_x, frames_y in D.SHAPES_TINY + D.SHAPES_BLOCK:
            for mutant in catches(kind, frames_x, frames_y, D.MUTANTS):
                caught[mutant].append(D.probe_name(kind, frames_x, frames_y))
    for mutant, names in caught.items():
        print(f'{mutant}: caught by {len(names)} of {3 * 14} probes (the transposes and the long ones not counted), first by '
              f'{names[0]}; named: {D.probe_name(*CAUGHT_BY[mutant])}')
        assert names, mutant


@pytest.mark.parametrize('kind', list(D.KINDS))
def test_every_probe_with_a_choice_catches_a_tie_mutant(kind):
    """The condition that keeps the GPU test honest: an input on which no comparison ties tests no tie rule."""
    for frames_x, frames_y in D.SHAPES:
        if min(frames_x, frames_y) == 1:
            continue                                                       # one path: nothing to choose
        found = catches(kind, frames_x, frames_y, D.TIE_MUTANTS)
        assert found, (kind, frames_x, frames_y)
    # left_before_up needs D[i-1, j] == D[i, j-1] < D[i-1, j-1] on the path: only equal costs give that
    assert catches('equal_cost', 4, 4, D.TIE_MUTANTS) == ['left_before_up', 'less_equal']


def test_the_old_inputs_are_blind():
    # random costs, the small shapes of test_gpu_dtw.py::SIZES: no comparison ever ties
    rng = np.random.default_rng(20)
    for frames_x, frames_y in D.OLD_SMALL_SIZES + ((127, 114),):
        table = rng.random((frames_x, frames_y)).astype(np.float32) * 2
        base = D.programme32(table)
        for mutant in D.TIE_MUTANTS:
            assert D.same(base, D.programme32(table, mutant)), (mutant, frames_x, frames_y)
    # no probe of at most 256 rows has a row that is handed over
    for kind in D.KINDS:
        for frames_x, frames_y in D.SHAPES:
            if frames_x <= D.BLOCK_ROWS:
                assert catches(kind, frames_x, frames_y, D.EDGE_MUTANTS) == [], (kind, frames_x, frames_y)
    # ... and 257 has
    assert catches('alphabet_mix', 257, 65, D.EDGE_MUTANTS) == list(D.EDGE_MUTANTS)


def test_constant_tables_have_a_closed_form():
    for cell in (np.float32(0.1), np.float32(1.7320508), np.float32(0)):
        for frames_x, frames_y in D.CONSTANT_SHAPES:
            total, count, path = D.constant_closed_form(frames_x, frames_y, cell)
            assert D.same((total, count, path), D.programme32(np.full((frames_x, frames_y), cell, dtype=np.float32)))
            R.check_path(path, frames_x, frames_y)
            assert count == len(path) == max(frames_x, frames_y)
    _, _, path = D.constant_closed_form(5, 3, 1)
    assert path.tolist() == [[0, 0], [1, 0], [2, 0], [3, 1], [4, 2]]
    _, _, path = D.constant_closed_form(3, 5, 1)
    assert path.tolist() == [[0, 0], [0, 1], [0, 2], [1, 3], [2, 4]]
    total, _, _ = D.constant_closed_form(300, 300, np.float32(0.1))
    assert total != np.float32(30) and abs(float(total) - 30) < 1e-3          # the sequential sum, not the product
