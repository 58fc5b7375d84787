"""CPU restatement of the weighted edit distance of ppg_edit_distance for the tests
(tests/test_edit_host.py, tests/test_gpu_edit.py): the same fp32 adds in the same order, so every comparison with the
device is on bits.

    D[0, 0] = 0;  every other cell prefers  D[i-1, j-1] + sub[r[i-1], h[j-1]]   (diagonal)
                                    then    D[i-1, j]   + del[r[i-1]]           (deletion)
                                    then    D[i, j-1]   + ins[h[j-1]]           (insertion)
    a later candidate winning only if strictly smaller; a candidate outside the table does not exist.

`edit` is vectorised along anti-diagonals (4096 x 4096 in about two seconds) and can be run as one of MUTANTS: the ways
the device programme could plausibly be wrong.  `edit_plain` walks the table cell by cell and pins `edit`."""
import numpy as np

NP = 40
BLOCK = 256        # table rows per block of the device programme (64 lanes x 4)
STRIP = 4          # table rows per lane

# name -> what the mutant does instead
MUTANTS = {
    'deletion_first': 'the deletion is preferred to the diagonal',
    'insertion_first': 'the insertion is preferred to the deletion',
    'not_strict': 'a later candidate wins a tie (<=)',
    'kind_by_cost': 'a diagonal step is a hit when sub says 0, whatever the tokens',
    'edge_scan': 'row 0 and column 0 are summed by a parallel scan, not in order',
    'block_top_inf': 'the first row of a block sees +inf for the row above',
    'block_top_shifted': 'the first row of a block sees the row above shifted by one column',
    'strip_row': 'the first row of a strip takes the row two above for the row above',
    'trace_neighbour': "the trace-back reads the direction of the strip's neighbouring row",
}


def unit_costs():
    return (1 - np.eye(NP)).astype(np.float32), np.ones(NP, np.float32), np.ones(NP, np.float32)


def _costs(sub, dele, ins):
    unit = unit_costs()
    return tuple(np.ascontiguousarray(unit[k] if c is None else c, dtype=np.float32)
                 for k, c in enumerate((sub, dele, ins)))


def _scan(values):
    """Inclusive prefix sums in fp32 by doubling (Hillis-Steele): what a parallel scan would give."""
    out = np.asarray(values, np.float32).copy()
    step = 1
    while step < len(out):
        out[step:] = out[step:] + out[:-step]
        step *= 2
    return out


def _walk(moves, ref, hyp, sub, mutant=None):
    """The operations (K, 3) in forward order from the direction table, and the counts (H, S, D, I)."""
    i, j = len(ref), len(hyp)
    ops = []
    while i > 0 or j > 0:
        if i == 0:
            move = 2
        elif j == 0:
            move = moves[i, 0]
        else:
            row = i
            if mutant == 'trace_neighbour':
                row = ((i - 1) ^ 1) + 1
                row = row if row <= len(ref) else i
            move = moves[row, j]
        if move == 0:
            if i == 0 or j == 0:        # (only a mutant's table can point outside)
                move = 1 if i else 2
        if move == 0:
            p, q = ref[i - 1], hyp[j - 1]
            hit = sub[p, q] == 0 if mutant == 'kind_by_cost' else p == q
            ops.append((0 if hit else 1, i - 1, j - 1))
            i, j = i - 1, j - 1
        elif move == 1 and i > 0:
            ops.append((2, i - 1, -1))
            i -= 1
        else:
            ops.append((3, -1, j - 1))
            j -= 1
    ops = np.asarray(ops[::-1], dtype=np.int64).reshape(-1, 3)
    counts = tuple(int((ops[:, 0] == kind).sum()) for kind in range(4))
    return ops, counts


def edit(ref, hyp, sub=None, dele=None, ins=None, mutant=None):
    """(total as numpy.float32, (H, S, D, I), ops (K, 3) int64) of the fp32 programme, or of a mutant of it."""
    assert mutant is None or mutant in MUTANTS, mutant
    sub, dele, ins = _costs(sub, dele, ins)
    ref, hyp = np.asarray(ref, dtype=np.int64).reshape(-1), np.asarray(hyp, dtype=np.int64).reshape(-1)
    rows, columns = len(ref), len(hyp)
    inf = np.float32(np.inf)
    table = np.full((rows + 1, columns + 1), inf, dtype=np.float32)
    moves = np.zeros((rows + 1, columns + 1), dtype=np.int8)
    table[0, 0] = 0
    if mutant == 'edge_scan':
        table[0, 1:], table[1:, 0] = _scan(ins[hyp]), _scan(dele[ref])
    else:
        table[0, 1:] = np.add.accumulate(ins[hyp], dtype=np.float32)       # in order: one fp32 add per cell
        table[1:, 0] = np.add.accumulate(dele[ref], dtype=np.float32)
    moves[1:, 0] = 1
    moves[0, 1:] = 2
    # the row a cell takes for "the row above", and the columns it is shifted by (mutants only)
    index = np.arange(rows + 1)
    above = index - 1
    shift = np.zeros(rows + 1, dtype=np.int64)
    blind = np.zeros(rows + 1, dtype=bool)
    first_of_block = (index > 1) & ((index - 1) % BLOCK == 0)
    if mutant == 'block_top_inf':
        blind = first_of_block
    if mutant == 'block_top_shifted':
        shift[first_of_block] = 1
    if mutant == 'strip_row':
        pick = (index > 1) & ((index - 1) % STRIP == 0) & ~first_of_block
        above[pick] = index[pick] - 2
    del_row = dele[ref] if rows else np.zeros(0, np.float32)
    ins_col = ins[hyp] if columns else np.zeros(0, np.float32)
    for t in range(2, rows + columns + 1):
        i = np.arange(max(1, t - columns), min(rows, t - 1) + 1)
        j = t - i
        src, off = above[i], shift[i]
        ju, jd = j - off, j - 1 - off
        up = np.where((ju >= 0) & ~blind[i], table[src, np.maximum(ju, 0)], inf)
        dg = np.where((jd >= 0) & ~blind[i], table[src, np.maximum(jd, 0)], inf)
        cand = (dg + sub[ref[i - 1], hyp[j - 1]], up + del_row[i - 1], table[i, j - 1] + ins_col[j - 1])
        order = {'deletion_first': (1, 0, 2), 'insertion_first': (0, 2, 1)}.get(mutant, (0, 1, 2))
        best, move = cand[order[0]].copy(), np.full(len(i), order[0], dtype=np.int8)
        for which in order[1:]:
            take = cand[which] <= best if mutant == 'not_strict' else cand[which] < best
            best[take], move[take] = cand[which][take], which
        table[i, j], moves[i, j] = best, move
    ops, counts = _walk(moves, ref, hyp, sub, mutant)
    return table[rows, columns], counts, ops


def edit_plain(ref, hyp, sub=None, dele=None, ins=None):
    """The same, cell by cell, as the definition reads."""
    sub, dele, ins = _costs(sub, dele, ins)
    ref, hyp = [int(v) for v in ref], [int(v) for v in hyp]
    rows, columns = len(ref), len(hyp)
    table = [[None] * (columns + 1) for _ in range(rows + 1)]
    moves = np.zeros((rows + 1, columns + 1), dtype=np.int8)
    for i in range(rows + 1):
        for j in range(columns + 1):
            if i == 0 and j == 0:
                table[i][j] = np.float32(0)
                continue
            best, move = None, 0
            if i > 0 and j > 0:
                best, move = np.float32(table[i - 1][j - 1] + sub[ref[i - 1], hyp[j - 1]]), 0
            if i > 0:
                value = np.float32(table[i - 1][j] + dele[ref[i - 1]])
                if best is None or value < best:
                    best, move = value, 1
            if j > 0:
                value = np.float32(table[i][j - 1] + ins[hyp[j - 1]])
                if best is None or value < best:
                    best, move = value, 2
            table[i][j], moves[i, j] = best, move
    ops, counts = _walk(moves, np.asarray(ref, dtype=np.int64), np.asarray(hyp, dtype=np.int64), sub)
    return table[rows][columns], counts, ops


def histogram(ops, ref, hyp):
    """The (41, 41) int64 statistics of a pair's operations: [p, q] matched, [p, 40] deleted, [40, q] inserted."""
    out = np.zeros((NP + 1, NP + 1), dtype=np.int64)
    for kind, i, j in np.asarray(ops).reshape(-1, 3):
        out[ref[i] if kind != 3 else NP, hyp[j] if kind != 2 else NP] += 1
    return out


# ---- the probes: inputs full of exact ties, laid over the edges of the device programme's tiling ---------------------

def random_costs(seed):
    """fp32 costs with many distinct mantissas, so that the order of the adds shows in the bits."""
    rng = np.random.default_rng(seed)
    return (rng.random((NP, NP)).astype(np.float32) * 2, rng.random(NP).astype(np.float32) + np.float32(0.25),
            rng.random(NP).astype(np.float32) + np.float32(0.25))


def tokens(seed, length, symbols):
    return np.random.default_rng(seed).integers(0, symbols, length)


def antiphase(rows, columns, seed):
    """Three random symbols, with `abab...` against `baba...` laid across row 255|256 and column 63|64."""
    ref, hyp = tokens(seed, rows, 3), tokens(seed + 1, columns, 3)
    i, j = np.arange(rows), np.arange(columns)
    r, h = (i >= 236) & (i < 276), (j >= 44) & (j < 84)
    ref[r], hyp[h] = i[r] % 2, (j[h] + 1) % 2
    return ref, hyp


def _zero_sub():
    sub, dele, ins = unit_costs()
    sub[0, 1] = 0            # a substitution that costs nothing is still a substitution
    return sub, dele, ins


UNIT = (None, None, None)
# name -> (reference, hypothesis, costs): what tests/test_edit_host.py holds every mutant against
PROBES = {
    'ab_ba': ([0, 1], [1, 0], UNIT),
    'a_b_dear_sub': ([0], [1], (np.where(np.eye(NP) > 0, 0, 3).astype(np.float32),) + unit_costs()[1:]),
    'free_sub': ([0, 0, 1], [1, 0, 1], _zero_sub()),
    'ties2_260x79': (tokens(10, 260, 2), tokens(11, 79, 2), UNIT),
    'ties3_257x64': (tokens(12, 257, 3), tokens(13, 64, 3), UNIT),
    'ties2_513x130': (tokens(14, 513, 2), tokens(15, 130, 2), UNIT),
    'ties3_130x513': (tokens(16, 130, 3), tokens(17, 513, 3), UNIT),
    'antiphase_300x100': antiphase(300, 100, 18) + (UNIT,),
    'costs_60x70': (tokens(20, 60, NP), tokens(21, 70, NP), random_costs(22)),
    'costs_300x517': (tokens(23, 300, NP), tokens(24, 517, NP), random_costs(25)),
    'costs_300x0': (tokens(26, 300, NP), [], random_costs(27)),
    'costs_0x300': ([], tokens(28, 300, NP), random_costs(29)),
}


def same(got, want):
    """(total, counts, ops) against (total, counts, ops): the total on bits, everything else exactly."""
    return (np.asarray(got[0], np.float32).tobytes() == np.asarray(want[0], np.float32).tobytes() and
            tuple(int(v) for v in got[1]) == tuple(int(v) for v in want[1]) and
            np.array_equal(np.asarray(got[2]).reshape(-1, 3), np.asarray(want[2]).reshape(-1, 3)))


def gpu_shapes():
    """The (rows, columns) the device suite runs, each also with its sides swapped: the empty sides, one cell, every
    row count around the 256-row block with every column count around the 64-column feed, several blocks against
    short and long rows, and the limit."""
    shapes = [(0, 0), (0, 5), (5, 0), (1, 1)]
    shapes += [(rows, columns) for rows in range(254, 261) for columns in range(62, 80)]
    shapes += [(513, 130), (769, 9), (4096, 9)]
    return shapes
