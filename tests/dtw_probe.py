"""Shared by tests/test_dtw_probe_host.py and tests/test_gpu_dtw_probe.py: bit-exact probes of ppg_dtw (ppg_dtw.hip).

Why.  tests/test_gpu_dtw.py feeds random softmax PPGs and compares totals with a float64 programme by cost.  Random
fp32 sums never tie, so the order of the kernel's two comparisons, its `<`, the hand-over of row 255 to row 256 through
LDS, the strip of 4 rows per lane and the packing of four direction bytes per word can all be wrong there without a
test noticing (test_dtw_probe_host.py shows it: the mutants below change nothing on such tables).

How.  Given the cell costs, the recurrence is one fp32 add and two comparisons per cell: `programme32` restates it in
numpy.float32 and is bit-reproducible.  The cell costs come from the device itself: X and Y are sequences over a small
alphabet of S distinct frames, the S x S frame pairs run once as 1 x 1 problems, and C[i, j] = cell[sx[i], sy[j]].  A
table built like that is full of exact ties, and total, K and the whole path must equal the emulation: no tolerance.

No GPU and no file outside tests/ is touched here.
"""
import functools

import numpy as np
import torch

import postops_probe as P

NP = P.NP
BLOCK_ROWS = 256          # rows per block of the programme: the last row of a block reaches the next through LDS
STRIP = 4                 # rows per lane

TIE_MUTANTS = ('up_first', 'left_before_up', 'less_equal')
EDGE_MUTANTS = ('edge_row_inf', 'edge_row_shifted', 'edge_count')
MUTANTS = TIE_MUTANTS + ('count_from_diagonal',) + EDGE_MUTANTS + ('strip_carry', 'dir_byte')


# ---- the fp32 programme ------------------------------------------------------------------------------------------------

def programme32(cost, mutant=None):
    """The kernel's recurrence over `cost` (Tx, Ty) in numpy.float32, vectorised over anti-diagonals:
    -> (total np.float32, K int, path (n, 2) int64 in forward order; n == K for every mutant but count_from_diagonal).

    D[0, 0] = C[0, 0] + 0 (the virtual origin); D[i, j] = C[i, j] + best, best = the diagonal, replaced by (i-1, j) if
    that is strictly smaller, replaced by (i, j-1) if that is strictly smaller still; K rides along with the choice.

    mutant: one fault a refactoring of ppg_dtw.hip could introduce.
      up_first             (i-1, j) is preferred to the diagonal
      left_before_up       (i, j-1) is compared before (i-1, j)
      less_equal           `<=` for `<`
      count_from_diagonal  K comes from the diagonal predecessor whatever was chosen
      edge_row_inf         row 256 k sees +inf above it (the LDS hand-over lost)
      edge_row_shifted     row 256 k reads the row above it one column to the left (the hand-over off by one)
      edge_count           row 256 k reads the counts of the row above it as 0 (the counts' half of the hand-over lost)
      strip_carry          row 4 l, l not a multiple of 64, takes what is above it from row 4 l - 2 (the cross-lane move
                           sends the wrong register)
      dir_byte             the trace-back reads byte (i + 1) & 3 of the direction word (rows 4 l .. 4 l + 3, one column)
    """
    assert mutant is None or mutant in MUTANTS, mutant
    cost = np.asarray(cost, dtype=np.float32)
    frames_x, frames_y = cost.shape
    inf = np.float32(np.inf)
    table = np.full((frames_x + 1, frames_y + 1), inf, dtype=np.float32)
    table[0, 0] = 0
    count = np.zeros((frames_x + 1, frames_y + 1), dtype=np.int32)
    moves = np.zeros((frames_x, frames_y), dtype=np.int8)
    better = np.less_equal if mutant == 'less_equal' else np.less
    for d in range(frames_x + frames_y - 1):
        i = np.arange(max(0, d - frames_y + 1), min(d, frames_x - 1) + 1)
        j = d - i
        diag_d, diag_n = table[i, j].copy(), count[i, j].copy()
        up_d, up_n = table[i, j + 1].copy(), count[i, j + 1].copy()
        left_d, left_n = table[i + 1, j], count[i + 1, j]
        edge = (i % BLOCK_ROWS == 0) & (i > 0)
        if mutant == 'edge_row_inf':
            diag_d[edge], up_d[edge] = inf, inf
        elif mutant == 'edge_row_shifted':
            e, je = i[edge], j[edge]
            up_d[edge], up_n[edge] = table[e, je], count[e, je]
            diag_d[edge] = np.where(je > 0, table[e, np.maximum(je - 1, 0)], inf)
            diag_n[edge] = np.where(je > 0, count[e, np.maximum(je - 1, 0)], 0)
        elif mutant == 'edge_count':
            diag_n[edge], up_n[edge] = 0, 0
        elif mutant == 'strip_carry':
            strip = (i % STRIP == 0) & (i % BLOCK_ROWS != 0)
            s, js = i[strip], j[strip]
            up_d[strip], up_n[strip] = table[s - 1, js + 1], count[s - 1, js + 1]
            diag_d[strip], diag_n[strip] = table[s - 1, js], count[s - 1, js]
        order = [(diag_d, diag_n, 0), (up_d, up_n, 1), (left_d, left_n, 2)]
        if mutant == 'up_first':
            order = [order[1], order[0], order[2]]
        elif mutant == 'left_before_up':
            order = [order[0], order[2], order[1]]
        best, steps = order[0][0].copy(), order[0][1].copy()
        move = np.full(len(i), order[0][2], dtype=np.int8)
        for other_d, other_n, code in order[1:]:
            take = better(other_d, best)
            best[take], steps[take], move[take] = other_d[take], other_n[take], code
        table[i + 1, j + 1] = cost[i, j] + best                    # one fp32 add
        count[i + 1, j + 1] = (diag_n if mutant == 'count_from_diagonal' else steps) + 1
        moves[i, j] = move
    i, j = frames_x - 1, frames_y - 1
    path = [(i, j)]
    while (i, j) != (0, 0):
        row = i if mutant != 'dir_byte' else (i & ~3) + ((i + 1) & 3)
        move = moves[row, j] if row < frames_x else 0
        i, j = i - (move != 2), j - (move != 1)
        if i < 0 or j < 0:                                         # only a mutant walks off the table
            break
        path.append((i, j))
    return table[frames_x, frames_y], int(count[frames_x, frames_y]), np.asarray(path[::-1], dtype=np.int64)


def same(a, b):
    """Two results of programme32 (or of the device): total bit for bit, K and the path."""
    return (np.float32(a[0]).view(np.int32) == np.float32(b[0]).view(np.int32) and int(a[1]) == int(b[1])
            and np.array_equal(np.asarray(a[2]), np.asarray(b[2])))


def constant_closed_form(frames_x, frames_y, cell):
    """All of X one frame, all of Y another: every cell costs `cell` and every comparison ties, so the path is the tie
    rule in closed form -- (0, 0) .. (Tx - Ty, 0) and then the diagonal when Tx > Ty, mirrored along row 0 when
    Ty > Tx -- and the total the sequential fp32 sum of max(Tx, Ty) copies of the cell."""
    longest = max(frames_x, frames_y)
    total = np.float32(0)
    for _ in range(longest):
        total = np.float32(total + np.float32(cell))
    k = np.arange(longest)
    path = np.stack([np.maximum(k - (longest - frames_x), 0) if frames_x < frames_y else k,
                     np.maximum(k - (longest - frames_y), 0) if frames_y < frames_x else k], axis=1)
    return total, longest, path.astype(np.int64)


# ---- alphabets ---------------------------------------------------------------------------------------------------------

# (family, side of postops_probe.pair, frame): soft, peaked, one-hot, uniform, ties, and two near-equal frames
ALPHABET_FRAMES = (('soft', 0, 0), ('soft', 0, 1), ('soft', 1, 0), ('peaked', 0, 0), ('peaked', 0, 1), ('peaked', 1, 0),
                   ('peaked', 1, 1), ('onehot', 0, 0), ('onehot', 0, 1), ('onehot', 1, 1), ('uniform', 0, 0),
                   ('ties', 0, 0), ('ties', 0, 1), ('ties', 1, 0), ('near', 0, 0), ('near', 1, 0))


@functools.lru_cache(maxsize=None)
def alphabet():
    """(16, 40) fp32, sixteen distinct frames.  Never modified."""
    frames = torch.stack([P.pair(family)[side][:, frame] for family, side, frame in ALPHABET_FRAMES]).contiguous()
    assert len({tuple(f.tolist()) for f in frames}) == len(frames)
    return frames


SWAPPED = (3, 17, 29)


@functools.lru_cache(maxsize=None)
def equal_cost_symbols():
    """(3, 40) fp32: a frame `a` with a[17] == a[29] != a[3], `a` with entries 3 and 17 exchanged, `a` with entries 3 and
    29 exchanged.  Without the mix matrix, any two of the three differ in two entries, which hold (u, v) in one and
    (v, u) in the other; every other entry is equal and contributes exactly 0 to a cell, and the two remaining terms are
    T(u, v) and T(v, u) in one order or the other.  So cell[s, s] == 0 and cell[s, t] is ONE value c for all s != t, bit for
    bit: the costs are {0, c}, every D is the sequential fp32 sum of some number of c's, and paths with equally many
    costly cells tie exactly.  The first two symbols are the two-symbol alphabet {a, a with two entries swapped}; the third
    is there because two symbols can show `left_before_up` only where an anti-phase stretch ends in the table's corner
    (no motif of up to 5 x 5 frames inside matching context does), three can anywhere (`transposed` in `sequences`)."""
    p, q, r = SWAPPED
    a = P.pair('soft')[0][:, 2].clone()
    a[r] = a[q]
    assert a[p] != a[q]
    b, c = a.clone(), a.clone()
    b[p], b[q] = a[q], a[p]
    c[p], c[r] = a[r], a[p]
    return torch.stack([a, b, c]).contiguous()


def all_pairs(frames):
    """Every frame pair of an alphabet as a batch of 1 x 1 problems: x, y (S * S, 40, 1); pair s * S + t is (s, t)."""
    count = frames.shape[0]
    x = frames[:, None, :].expand(count, count, NP).reshape(count * count, NP, 1)
    y = frames[None, :, :].expand(count, count, NP).reshape(count * count, NP, 1)
    return x.contiguous(), y.contiguous()


def ppg_of(symbols, frames):
    """The (40, T) PPG of a symbol sequence over an alphabet."""
    return frames[torch.tensor(np.asarray(symbols).tolist(), dtype=torch.long)].T.contiguous()


def cost_table(cells, sx, sy):
    """C[i, j] = cells[sx[i], sy[j]], fp32: look-ups, no arithmetic."""
    return np.asarray(cells, dtype=np.float32)[np.asarray(sx)[:, None], np.asarray(sy)[None, :]]


# ---- symbol sequences --------------------------------------------------------------------------------------------------

SHAPES_TINY = ((1, 1), (1, 9), (9, 1), (3, 5), (4, 4), (5, 3))
SHAPES_BLOCK = ((255, 70), (256, 64), (257, 65), (260, 63), (261, 79), (513, 130), (512, 128), (769, 9))
SHAPES = (SHAPES_TINY + SHAPES_BLOCK + tuple((b, a) for a, b in SHAPES_BLOCK) + ((300, 300), (4096, 9), (9, 4096)))
CONSTANT_SHAPES = ((1, 1), (3, 5), (5, 3), (257, 65), (65, 257), (300, 300), (513, 9))

# test_gpu_dtw.py::SIZES, the small ones: what the suite ran before these probes
OLD_SMALL_SIZES = ((1, 1), (1, 300), (300, 1), (57, 43))


# found by trying every pair of sequences over three symbols of equal cost: with their transposes these catch five of the
# six (tie mutant, orientation) combinations, the most any 3 x 5 or 5 x 3 pair does
TINY_EQUAL_COST = {(3, 5): ((0, 1, 0), (0, 2, 2, 0, 1)), (5, 3): ((0, 0, 0, 1, 2), (1, 2, 0))}


def _underlying(length, symbols, rng):
    """`length` symbols in runs of 1 .. 3, neighbouring runs different."""
    out, last = [], -1
    while len(out) < length:
        s = int(rng.integers(symbols))
        if s == last:
            s = (s + 1 + int(rng.integers(symbols - 1))) % symbols
        out += [s] * int(rng.integers(1, 4))
        last = s
    return np.asarray(out[:length])


def sequences(frames_x, frames_y, symbols, seed, layout=0):
    """-> (sx, sy): X and Y over `symbols` symbols.  Both are one underlying sequence (runs of 1 .. 3, as long as the
    shorter side) at their own tempo, Y with a few substitutions, overlaid -- where the shape has room -- with features
    that start at fixed offsets so that each straddles the kernel edge it is meant for.  A feature at row r sits at
    the column of Y that the tempo puts opposite it (and the other way round).

    layout 0: a vertical run (X holds one frame of Y) of 5 .. 300 frames over rows 255 | 256, a horizontal one (Y holds a
              frame of X) over rows 511 | 512 and in row 256, runs over lanes (rows 6 .. 10) and over columns 63 | 64.
    layout 1: horizontal runs held by rows 255 and 256, a vertical run over rows 511 | 512, runs over lanes (rows 2 .. 8);
              the same transposed for the columns.
    layout 2: (three symbols of equal cost) one tempo but for a single held frame; anti-phase alternations (x = abab..,
              y = baba..) of 9 .. 13 frames from row 2, column 60, row 250, column 250 and into the corner;
              `transposed` motifs from row 14 and column 74; tiny shapes are anti-phase throughout or
              taken from TINY_EQUAL_COST.
    """
    rng = np.random.default_rng([seed, frames_x, frames_y, symbols, layout])
    shorter = min(frames_x, frames_y)
    under = _underlying(shorter, symbols, rng)
    if layout == 2:
        # one tempo for both but for a single held frame a third of the way in: away from it the path is locally diagonal
        def held(frames):
            at = np.arange(frames)
            return np.where(at < shorter // 3, at, np.maximum(at - (frames - shorter), shorter // 3))
        to_x, to_y = held(frames_x), held(frames_y)
    else:
        to_x, to_y = (np.arange(frames_x) * shorter) // frames_x, (np.arange(frames_y) * shorter) // frames_y
    sx, sy = under[to_x].copy(), under[to_y].copy()
    for _ in range(max(1, frames_y // 40) if frames_y > 4 else 0):                 # substitutions
        sy[int(rng.integers(frames_y))] = int(rng.integers(symbols))

    def column_of(row):
        return min(frames_y - 1, int(np.searchsorted(to_y, to_x[min(row, frames_x - 1)])))

    def row_of(column):
        return min(frames_x - 1, int(np.searchsorted(to_x, to_y[min(column, frames_y - 1)])))

    def fresh(*neighbours):
        taken = {int(n) for n in neighbours}
        free = [s for s in range(symbols) if s not in taken]
        return int(rng.choice(free)) if free else int(rng.integers(symbols))

    def x_run(row, length, column=None):                     # vertical: X repeats, Y has the frame once
        column = column_of(row) if column is None else column
        if row < 1 or row + length >= frames_x or not 0 < column < frames_y - 1:
            return
        s = fresh(sx[row - 1], sx[row + length], sy[column - 1], sy[column + 1])
        sx[row:row + length] = s
        sy[column] = s

    def y_run(column, length, row=None):                     # horizontal: Y repeats, X has the frame once
        row = row_of(column) if row is None else row
        if column < 1 or column + length >= frames_y or not 0 < row < frames_x - 1:
            return
        s = fresh(sy[column - 1], sy[column + length], sx[row - 1], sx[row + 1])
        sy[column:column + length] = s
        sx[row] = s

    def anti(row, column, length):
        if row < 0 or column < 0 or row + length > frames_x or column + length > frames_y:
            return
        a = int(rng.integers(symbols))
        b = (a + 1 + int(rng.integers(symbols - 1))) % symbols
        k = np.arange(length)
        sx[row:row + length] = np.where(k % 2 == 0, a, b)
        sy[column:column + length] = np.where(k % 2 == 0, b, a)

    def transposed(row, column):
        """x = p q | a b | r p against y = p q | r b a | r p over three symbols of equal cost: (i-1, j) and (i, j-1) tie
        below the diagonal at the cell of b against a, and the path has to pass it."""
        if symbols < 3 or row < 0 or column < 0 or row + 6 > frames_x or column + 7 > frames_y:
            return
        sx[row:row + 6] = [1, 2, 0, 1, 2, 1]
        sy[column:column + 7] = [1, 2, 2, 1, 0, 2, 1]

    long_run = (5, 12, 40, 300)[int(rng.integers(4))]
    if layout == 0:
        x_run(6, 5)                                          # rows 6 .. 10: lanes 1 | 2
        y_run(6, 5)
        y_run(60, 8)                                         # columns 60 .. 67
        x_run(60, 8)
        start = BLOCK_ROWS - long_run // 2 if long_run < 300 else 100
        x_run(start, min(long_run, max(frames_x - start - 2, 0)))       # over rows 255 | 256
        y_run(start, min(long_run, max(frames_y - start - 2, 0)))
        x_run(505, 14)                                       # over rows 511 | 512
        y_run(505, 14)
    elif layout == 1:
        y_run(column_of(256) - 5, 5, row=255)                # a horizontal run in the last row of block 0
        y_run(column_of(256), 7, row=256)                    # and one in the first row of block 1
        x_run(row_of(256) - 5, 5, column=255)
        x_run(row_of(256), 7, column=256)
        x_run(505, 9)
        y_run(505, 9)
        x_run(2, 7)                                          # rows 2 .. 8: lanes 0 | 1 | 2
        y_run(2, 7)
    else:
        if (frames_x, frames_y) in TINY_EQUAL_COST:
            sx[:], sy[:] = TINY_EQUAL_COST[frames_x, frames_y]
        elif shorter < 20:
            sx[:], sy[:] = np.arange(frames_x) % 2, (np.arange(frames_y) + 1) % 2
        else:
            anti(2, column_of(2), 9)
            transposed(14, column_of(14))                    # rows 14 .. 19: lanes 3 | 4
            anti(row_of(60), 60, 11)
            transposed(row_of(74), 74)
            anti(250, column_of(250), 13)
            anti(row_of(250), 250, 13)
            tail = 9 if frames_x < 300 else 10               # the corner is a forced cell: odd and even lengths
            anti(frames_x - tail, frames_y - tail, tail)
    return sx, sy


# kind -> (alphabet, number of symbols, mix matrix?, layout)
KINDS = {'alphabet_mix': ('alphabet', 16, True, 0), 'alphabet_plain': ('alphabet', 16, False, 1),
         'equal_cost': ('equal', 3, False, 2)}


@functools.lru_cache(maxsize=None)
def probe(kind, frames_x, frames_y):
    """The symbol sequences of one probe.  Never modified."""
    _, symbols, _, layout = KINDS[kind]
    sx, sy = sequences(frames_x, frames_y, symbols, 7, layout)
    sx.setflags(write=False)
    sy.setflags(write=False)
    return sx, sy


def frames_of(kind):
    return alphabet() if KINDS[kind][0] == 'alphabet' else equal_cost_symbols()


def probe_name(kind, frames_x, frames_y):
    return f'{kind} {frames_x}x{frames_y}'


def host_cells(kind):
    """The table the host test uses in place of the device's cells: integer 0 / 1 for the symbols of equal cost, a fixed random
    16 x 16 fp32 table with a zero diagonal for the alphabet."""
    if KINDS[kind][0] == 'equal':
        return np.asarray(1 - np.eye(3), dtype=np.float32)
    table = np.random.default_rng(16).random((16, 16)).astype(np.float32) + np.float32(0.25)
    np.fill_diagonal(table, 0)
    return table
