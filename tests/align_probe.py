"""Shared by tests/test_align_probe_host.py and tests/test_gpu_align_probe.py: bit-exact probes of the alignment family
(ppg_align.hip: forced alignment, optional phonemes, phrase search and its picker, the recogniser, the graph Viterbi,
the run-length decode) on inputs where exact ties decide.

Why.  The GPU tests of these kernels feed random softmax PPGs and compare by cost within (T + 2) * 2^-23 * |total|, or
feed a uniform PPG on which every path ties with every other.  On the first two candidates tie only where a transcript
holds a phoneme twice in a row, and boundaries are compared by cost, so `>=` for `>`, the order of two comparisons or a
wrong direction bit at a strip edge change nothing a test sees; on the second a kernel that reads the wrong state's
emission still passes (tests/test_align_probe_host.py puts the first on record).

How.  A PPG of zeros and ones.  The clamp's upper end, 1.f - 1e-8f, IS 1.0f in fp32, so an entry >= 1 has the emission
logf(1) = +0 exactly, and an entry <= 1e-8 has L = logf(1e-8f), one fp32 number (about -18.420681) that the GPU test reads
from the device.  Every sum a kernel forms then adds L or 0 in frame order: a path that met k cold frames holds S_k with
S_0 = +0, S_k = fl(S_{k-1} + L), and S_k is strictly decreasing up to k = 65536, so the fp32 programme is isomorphic
to an integer programme on the number of cold frames.  Two candidates tie exactly when their counts tie, which happens
all the time.  The float64 references of the suite, fed the emissions 0 and -1, are exact, and with the documented tie
rules they give the ONE path the device must give and the count k, so that the device's total must be S_k bit for bit.

Two exact regimes:  (i) a binary PPG with every transition, stay, initial, final and arc weight in {0, -inf};
(ii) `hot_ppg` (all ones: every emission and maximum is +0) with weights that are multiples of 1/8 in [-4, 0] or -inf,
where every sum is exact in fp32 and float64 alike and the float64 total is the device's to the bit.

The `*_programme` functions restate each recurrence in plain numpy with switchable faults (MUTANTS), one fault a
refactoring of ppg_align.hip could introduce each; the host test shows that the probes of the GPU list catch every one.

No GPU is touched here; of the package only the host-only graph builders of ppgs_amd.alignment are used.
"""
import functools

import numpy as np
import torch

from ppgs_amd import alignment

import alignment_optional_reference as OR
import alignment_reference as R
import recognize_reference as RR
import search_reference as SR
import viterbi_reference as V
from test_gpu_alignment_optional import flags_for

NP = 40
CHUNK = 32                # frames staged in LDS at a time (CHUNK of ppg_align.hip)
WALK = 64                 # frames per LDS refill of the trace-back (WALK)
INF = np.inf
MOST = 65536              # the longest table of S_k that is checked to be strictly decreasing

MUTANTS = ('advance_on_tie', 'skip_before_advance', 'strip_carry', 'state0_fed', 'stale_chunk', 'refill_edge',
           'top_strip_bit', 'begin_not_carried', 'origin_late', 'pick_earliest', 'highest_source', 'switch_beats_stay',
           'last_end_state')


def strip(count):
    """States per lane of the alignment programmes (strip_shift of ppg_align.hip)."""
    return 1 if count <= 64 else 4 if count <= 256 else 16


def search_strip(count):
    """States per lane of the search programme."""
    return 1 if count <= 64 else 4


# ---- inputs ------------------------------------------------------------------------------------------------------------

def binary_ppg(seed, frames, density=0.3, dead=None):
    """(40, frames) fp32 of 0.0 and 1.0: every entry hot with probability `density`, then `dead` whole frames (None:
    one in eight) cleared: their maximum is L and a GOP term there is L - L = 0.  Where the target of a frame is cold
    and another phoneme is hot the GOP term is L; at these densities that is most cold frames."""
    rng = np.random.default_rng([seed, frames, int(round(1000 * density))])
    hot = rng.random((NP, frames)) < density
    count = frames // 8 if dead is None else dead
    if count:
        hot[:, rng.choice(frames, size=min(count, frames), replace=False)] = False
    return torch.from_numpy(hot.astype(np.float32))


def hot_ppg(frames):
    """All ones: every emission and every frame maximum is +0."""
    return torch.ones(NP, frames)


def phoneme_sequence(seed, count):
    """`count` phoneme indices; about one in five repeats the phoneme before it."""
    rng = np.random.default_rng([seed, count, 77])
    out = rng.integers(0, NP, count)
    repeat = rng.random(count) < 0.2
    for n in range(1, count):
        if repeat[n]:
            out[n] = out[n - 1]
    return [int(v) for v in out]


def planted_ppg(seed, frames, query, perfect=(), flawed=()):
    """A binary PPG (density 0.1) in which `query` is said one phoneme per frame from every frame of `perfect` (a match
    of mean +0) and of `flawed` (the same, but its second frame is cold in every phoneme but one other than the target:
    a match with exactly one cold frame).  Occurrences that do not fit are left out."""
    ppg = binary_ppg(seed, frames, 0.1)
    for flaw, places in ((False, perfect), (True, flawed)):
        for at in places:
            if at < 1 or at + len(query) + 1 > frames:
                continue
            ppg[:, at - 1:at + len(query) + 1] = 0.
            for n, p in enumerate(query):
                ppg[p, at + n] = 1.
            for t in (at - 1, at + len(query)):                # fenced: a phoneme the query does not hold is hot
                ppg[next(p for p in range(NP) if p not in query), t] = 1.
            if flaw and len(query) > 1:
                ppg[:, at + 1] = 0.
                ppg[next(p for p in range(NP) if p not in query), at + 1] = 1.
    return ppg


def cold(ppg):
    """(T, 40) float64 of 0 and -1: the log-posterior in units of -L (0 where the entry is 1, -1 where it is 0)."""
    x = ppg.numpy().T
    assert ((x == 0) | (x == 1)).all()
    return np.where(x >= 1, 0., -1.)


# ---- the table S_k -----------------------------------------------------------------------------------------------------

def _sums(bits, count):
    out = np.zeros(count + 1, dtype=np.float32)
    step = np.int32(bits).view(np.float32)
    for k in range(count):
        out[k + 1] = np.float32(out[k] + step)
    out.setflags(write=False)
    return out


_sums_kept = functools.lru_cache(maxsize=8)(_sums)


def sums(L, count):
    """S_0 .. S_count by sequential np.float32 additions of L: S_0 = +0, S_k = fl(S_{k-1} + L).  Never modified."""
    return _sums_kept(int(np.float32(L).view(np.int32)), int(count))


HOST_L = np.log(np.float32(1e-8))             # what the host tests use where the GPU test reads the device's own L


def total_of(value, table, regime):
    """The fp32 total of a float64 reference total: S_k for the count -k of regime (i) ('binary'); the value itself in
    regime (ii) ('grid'), where it is a multiple of 1/8 below 2^15 and so exact in fp32."""
    if value == -INF:
        return np.float32(-INF)
    if regime == 'binary':
        assert value == np.floor(value) <= 0
        return table[int(-value)]
    assert value * 8 == np.floor(value * 8) and abs(value) < 2 ** 15
    return np.float32(value)


def mean32(table, counts, lengths):
    """S_counts / float(lengths): one fp32 division each; 0 / 0 = NaN."""
    with np.errstate(invalid='ignore'):
        return (table[np.asarray(counts, dtype=np.int64)] / np.asarray(lengths).astype(np.float32)).astype(np.float32)


def segment_scores(logp, symbols, starts, table):
    """(score, gop) fp32 of the segments starts[i] .. starts[i + 1] - 1 with targets symbols[i]: S_j / float(length),
    j the segment's cold frames (for gop: the frames where the target is cold and another phoneme is hot)."""
    top = logp.max(axis=1)
    starts = np.asarray(starts, dtype=np.int64)
    cold_frames, below = [], []
    for i, p in enumerate(symbols):
        a, b = starts[i], starts[i + 1]
        cold_frames.append(int(-logp[a:b, p].sum()))
        below.append(int(-(logp[a:b, p] - top[a:b]).sum()))
    lengths = np.diff(starts)
    return mean32(table, cold_frames, lengths), mean32(table, below, lengths)


# ---- what the device must give: the suite's float64 references on integer emissions --------------------------------------

def expect_forced(ppg, phonemes, flags, table):
    logp = cold(ppg)
    e = logp[:, np.asarray(phonemes, dtype=np.int64)]
    total, starts = R.programme(e) if flags is None else OR.programme(e, flags)
    score, gop = segment_scores(logp, phonemes, starts, table)
    return {'starts': starts, 'total': table[int(-total)], 'score': score, 'gop': gop}


def curve32(curve_total, curve_begin, table):
    """The fp32 curve of a float64 curve of counts: S_k where a match ends, -inf elsewhere."""
    counts = np.where(curve_begin >= 0, -curve_total, 0).astype(np.int64)
    return np.where(curve_begin >= 0, table[counts], np.float32(-INF)).astype(np.float32)


def expect_search(ppg, query, table, top):
    r = SR.emissions(cold(ppg), query)
    curve_total, curve_begin = SR.programme(r)
    totals = curve32(curve_total, curve_begin, table)
    hits = SR.pick(totals, curve_begin, len(query), top, dtype=np.float32)
    return {'totals': totals, 'begins': curve_begin, 'hits': hits}


def expect_runs(logp, total, run_states, symbols, starts, table, regime):
    score, gop = segment_scores(logp, symbols, starts, table)
    return {'states': np.asarray(run_states, dtype=np.int64), 'phonemes': np.asarray(symbols, dtype=np.int64),
            'starts': np.asarray(starts, dtype=np.int64), 'total': total_of(total, table, regime), 'score': score,
            'gop': gop}


def nothing_fits():
    empty = np.zeros(0, dtype=np.int64)
    return {'states': empty, 'phonemes': empty, 'starts': np.zeros(1, dtype=np.int64), 'total': np.float32(-INF),
            'score': np.zeros(0, dtype=np.float32), 'gop': np.zeros(0, dtype=np.float32)}


def expect_recognize(ppg, model, table, regime):
    logp = cold(ppg)
    A, initial, final = (np.asarray(v, dtype=np.float64) for v in model)
    total, labels = RR.viterbi(logp, A, initial, final)
    if labels is None:
        return nothing_fits()
    phonemes, starts = RR.runs(labels)
    return expect_runs(logp, total, phonemes, phonemes, starts, table, regime)


def expect_viterbi(ppg, graph, table, regime):
    logp = cold(ppg)
    g = V.lists(graph)
    total, states, ordinals = V.viterbi(V.emissions(logp, g.sym), g)
    if states is None:
        return nothing_fits()
    run_states, starts = V.runs(states, ordinals)
    return expect_runs(logp, total, run_states, g.sym[run_states], starts, table, regime)


def expect_decode(ppg):
    phonemes, starts = R.decode(ppg)
    return {'phonemes': phonemes, 'starts': starts}


# ---- the recurrences restated, with faults -----------------------------------------------------------------------------

def forced_programme(e, flags=None, mutant=None):
    """(total, starts) of forced alignment over e (T, N), with optional flags or None: stay beats advance beats skip.

    mutant:
      advance_on_tie       `>=` for `>` where the path advances
      skip_before_advance  the skip is compared before the advance
      strip_carry          state n, n % S == 0 (S > 1), takes what is below it from frame t instead of t-1 (the cross-lane
                           move after the strip's update)
      state0_fed           the origin 0 stands below state 0 at every frame, not at frame 0 only
      stale_chunk          frame t, t % 32 == 0, reads the emissions of frame t - 32 (the other staging buffer)
      refill_edge          the trace-back reads, at frames t % 64 == 0, the directions of frame t - 1
      top_strip_bit        the advance bit of place S-1 of every strip is dropped
    """
    e = np.asarray(e, dtype=np.float64)
    frames, count = e.shape
    optional = np.zeros(count, dtype=bool) if flags is None else np.asarray(flags).astype(bool)
    size = strip(count)
    index = np.arange(count)
    bottom = (index % size == 0) & (index > 0) & (size > 1)
    may = np.concatenate([[False], optional[:-1]])
    best = np.full(count, -INF)
    direction = np.zeros((frames, count), dtype=np.int8)
    best[0] = e[0, 0]
    direction[0, 0] = 1
    if count > 1 and optional[0]:
        best[1] = e[0, 1]
        direction[0, 1] = 2
    order = (2, 1) if mutant == 'skip_before_advance' else (1, 2)

    def update(stay, advance, skip, now):
        chosen, way = stay.copy(), np.zeros(count, dtype=np.int8)
        for code in order:
            other = advance if code == 1 else skip
            better = other > chosen
            if mutant == 'advance_on_tie' and code == 1:
                better |= (other == chosen) & np.isfinite(other)
            chosen, way = np.where(better, other, chosen), np.where(better, code, way)
        return now + chosen, way

    for t in range(1, frames):
        now = e[t - CHUNK] if mutant == 'stale_chunk' and t % CHUNK == 0 else e[t]
        advance = np.concatenate([[0. if mutant == 'state0_fed' else -INF], best[:-1]])
        skip = np.where(may, np.concatenate([[-INF, -INF], best[:-2]])[:count], -INF)
        fresh, way = update(best, advance, skip, now)
        if mutant == 'strip_carry' and bottom.any():           # the state below a strip's bottom is a strip's top: pass one
            advance[bottom] = fresh[index[bottom] - 1]
            fresh, way = update(best, advance, skip, now)
        best, direction[t] = fresh, way
    end = count - 1
    if optional[count - 1] and count > 1 and best[count - 2] > best[count - 1]:
        end = count - 2
    starts = np.full(count + 1, -1, dtype=np.int64)
    starts[count] = frames
    if end == count - 2:
        starts[count - 1] = frames
    n = end
    for t in range(frames - 1, 0, -1):
        way = direction[t - 1 if mutant == 'refill_edge' and t % WALK == 0 else t, n]
        if mutant == 'top_strip_bit' and n % size == size - 1 and way == 1:
            way = 0
        if way == 2 and n > 1:
            starts[n] = starts[n - 1] = t
            n -= 2
        elif way == 1 and n > 0:
            starts[n] = t
            n -= 1
    if n == 1 and optional[0]:
        starts[1] = 0
    starts[0] = 0
    assert mutant is not None or (n in (0, 1) and (starts >= 0).all())
    return float(best[end]), starts


def search_programme(r, mutant=None):
    """The curve (curve_total, curve_begin) of the search over r (T, N).

    mutant: advance_on_tie, strip_carry (S = 4 above 64 phonemes), stale_chunk as in `forced_programme`, and
      begin_not_carried    state n, n % S == 0, n > 0, keeps its own begin where it advances (the begin's cross-lane move)
      origin_late          a fresh start records the frame after its own as the begin
    """
    r = np.asarray(r, dtype=np.float64)
    frames, count = r.shape
    size = search_strip(count)
    index = np.arange(count)
    bottom = (index % size == 0) & (index > 0)
    best = np.full(count, -INF)
    begin = np.full(count, -1, dtype=np.int64)
    curve_total, curve_begin = np.full(frames, -INF), np.full(frames, -1, dtype=np.int64)

    def update(below, source, now):
        advance = below > best
        if mutant == 'advance_on_tie':
            advance |= (below == best) & np.isfinite(below)
        return now + np.where(advance, below, best), np.where(advance, source, begin)

    for t in range(frames):
        now = r[t - CHUNK] if mutant == 'stale_chunk' and t % CHUNK == 0 and t else r[t]
        below = np.concatenate([[0.], best[:-1]])
        source = np.concatenate([[t + 1 if mutant == 'origin_late' else t], begin[:-1]])
        if mutant == 'begin_not_carried':
            source[bottom] = begin[bottom]
        fresh, first = update(below, source, now)
        if mutant == 'strip_carry' and size > 1 and bottom.any():
            below[bottom], source[bottom] = fresh[index[bottom] - 1], first[index[bottom] - 1]
            fresh, first = update(below, source, now)
        best, begin = fresh, first
        curve_total[t], curve_begin[t] = best[-1], begin[-1]
    return curve_total, curve_begin


def pick(totals, begins, count, top, threshold=-INF, mutant=None):
    """The picker over an fp32 curve: per round the largest mean = total / float(frames), ties to the largest end frame
    (mutant pick_earliest: to the smallest), spans that meet the hit struck out: [(begin, end, total, mean)]."""
    totals, begins = np.asarray(totals, dtype=np.float32), np.asarray(begins, dtype=np.int64)
    time = np.arange(begins.shape[0])
    length = np.where(begins >= 0, time - begins + 1, 1).astype(np.float32)
    mean = np.where(begins >= 0, totals / length, np.float32(-INF)).astype(np.float32)
    alive = (time >= count - 1) & (begins >= 0)
    hits = []
    for _ in range(top):
        if not alive.any():
            break
        best = mean[alive].max()
        if best < threshold:
            break
        tied = time[alive & (mean == best)]
        at = int(tied.min() if mutant == 'pick_earliest' else tied.max())
        hits.append((int(begins[at]), at + 1, totals[at], mean[at]))
        alive &= ~((begins < at + 1) & (time >= begins[at]))
    return hits


def same_hits(a, b):
    return len(a) == len(b) and all(
        x[:2] == y[:2] and np.float32(x[2]).view(np.int32) == np.float32(y[2]).view(np.int32)
        and np.float32(x[3]).view(np.int32) == np.float32(y[3]).view(np.int32) for x, y in zip(a, b))


def model_lists(A, initial, final):
    """The model of `recognize` as viterbi_reference.Lists: state q is phoneme q, its arcs come from every p != q in
    ascending p."""
    A = np.asarray(A, dtype=np.float64)
    into = [[(p, float(A[p, q])) for p in range(A.shape[0]) if p != q] for q in range(A.shape[0])]
    return V.Lists(np.arange(A.shape[0]), np.diag(A).copy(), into, np.asarray(initial, dtype=np.float64),
                   np.asarray(final, dtype=np.float64))


def graph_programme(e, g, mutant=None):
    """(total, states, ordinals) of the graph Viterbi over e (T, S) and viterbi_reference.Lists `g`, vectorised over
    the states: staying wins ties, then the arc listed first, then the lowest end state.  (-inf, None, None) if no path.

    mutant: stale_chunk and refill_edge as in `forced_programme`, and
      switch_beats_stay    an arc that ties with staying is taken
      highest_source       of arcs that tie the one listed last is taken
      last_end_state       of end states that tie the highest is taken
    """
    e = np.asarray(e, dtype=np.float64)
    frames, count = e.shape
    degree = max([len(into) for into in g.into] + [1])
    source = np.zeros((count, degree), dtype=np.int64)
    weight = np.full((count, degree), -INF)
    for n, into in enumerate(g.into):
        for j, (s, w) in enumerate(into):
            source[n, j], weight[n, j] = s, w
    stay, initial, final = (np.asarray(v, dtype=np.float64) for v in (g.stay, g.initial, g.final))
    origin = np.zeros((frames, count), dtype=np.int64)
    d = e[0] + initial
    for t in range(1, frames):
        now = e[t - CHUNK] if mutant == 'stale_chunk' and t % CHUNK == 0 else e[t]
        best, chosen = d + stay, np.zeros(count, dtype=np.int64)
        for j in range(degree):
            c = d[source[:, j]] + weight[:, j]
            take = c > best
            if mutant in ('switch_beats_stay', 'highest_source'):
                take |= (c == best) & np.isfinite(c) & ((chosen == 0) == (mutant == 'switch_beats_stay'))
            best, chosen = np.where(take, c, best), np.where(take, j + 1, chosen)
        d, origin[t] = now + best, chosen
    f = d + final
    last = int(count - 1 - np.argmax(f[::-1])) if mutant == 'last_end_state' else int(np.argmax(f))
    if not f[last] > -INF:
        return -INF, None, None
    states, ordinals = np.empty(frames, dtype=np.int64), np.zeros(frames, dtype=np.int64)
    states[frames - 1] = last
    for t in range(frames - 1, 0, -1):
        n = states[t]
        ordinals[t] = origin[t - 1 if mutant == 'refill_edge' and t % WALK == 0 else t, n]
        states[t - 1] = n if ordinals[t] == 0 else source[n, ordinals[t] - 1]
    return float(f[last]), states, ordinals


def decode_runs(ppg):
    """(phonemes, starts): the runs of the per-frame argmax, the lowest index on ties (phoneme 0 on a dead frame)."""
    return RR.runs(np.argmax(ppg.numpy(), axis=0))


# ---- models and graphs -------------------------------------------------------------------------------------------------

GRID = (0., -0.125, -0.5, -2.)               # regime (ii): few distinct multiples of 1/8 in [-4, 0], so that ties abound


def grid_weights(rng, shape, holes=0.2):
    values = np.asarray(GRID)[rng.integers(0, len(GRID), shape)]
    return np.where(rng.random(shape) < holes, -INF, values)


def banded_model(band=1):
    """Regime (i): A[p, q] = 0 for |p - q| <= band, -inf elsewhere; the path may begin and end anywhere."""
    index = np.arange(NP)
    A = np.where(np.abs(index[:, None] - index[None, :]) <= band, 0., -INF)
    return A, np.zeros(NP), np.zeros(NP)


def grid_model(seed):
    """Regime (ii): transitions, initial and final on the 1/8 grid, with holes.  No step is free and staying costs more
    than the cheapest switch, so the best path keeps moving among the many switches that weigh 1/8."""
    rng = np.random.default_rng([seed, 40])
    A = grid_weights(rng, (NP, NP))
    A = np.where(A == 0, -0.125, A)
    np.fill_diagonal(A, np.where(np.diag(A) >= -0.125, -0.5, np.diag(A)))
    return A, grid_weights(rng, NP), grid_weights(rng, NP)


def model_tensors(model):
    return tuple(torch.from_numpy(np.asarray(v)).float() for v in model)


def tie_graph(count, seed, reach=3, grid=False):
    """(phonemes, arcs, stay, initial, final) of a graph of `count` states for alignment.graph.  State n takes arcs from
    n-1 .. n-reach in a seeded order (so the arc listed first is not the nearest), every fifth state a parallel arc from
    the first of these sources again and every seventh an arc from itself (which ties with staying and, taken, would open
    a run).  The path may begin in every third state and end in states n % 4 in (1, 2): neighbouring end states tie.
    All weights 0 / -inf (regime (i)); with `grid` (regime (ii)) the arcs weigh 1/8, 1/2 or 2, staying 1/8 or 1/2."""
    rng = np.random.default_rng([seed, count, reach, int(grid)])
    phonemes = phoneme_sequence(seed + 1, count)
    arcs = []
    for n in range(count):
        sources = [int(s) for s in rng.permutation(np.arange(max(n - reach, 0), n))]
        if sources and n % 5 == 0:
            sources.append(sources[0])
        if n % 7 == 3:
            sources.insert(len(sources) // 2, n)
        weights = np.zeros(len(sources))
        if grid:                                               # no arc is free: staying (1/8 or 1/2) competes with the arcs
            weights = grid_weights(rng, len(sources), 0.1)
            weights = np.where(weights == 0, -0.125, weights)
        arcs += [(s, n, float(w)) for s, w in zip(sources, weights)]
    if grid:
        # the path begins in a state n % 16 == 0 and ends nine or ten states on: it has to move, a step costs what
        # waiting in a state n % 4 == 0 costs, and so when it moves and by which arcs is for the tie rule to say
        at = np.arange(count)
        stay = np.where(at % 4 == 0, -0.125, -0.5)
        initial = np.where(at % 16 == 0, -0.125 * ((at // 16) % 2), -INF)
        final = np.where(np.isin(at % 16, (9, 10)) | (at == count - 1), 0., -INF)
    else:
        stay = np.zeros(count)
        initial = np.where(np.arange(count) % 3 == 0, 0., -INF)
        final = np.where(np.isin(np.arange(count) % 4, (1, 2)) | (np.arange(count) == count - 1), 0., -INF)
    return phonemes, arcs, stay.tolist(), initial.tolist(), final.tolist()


@functools.lru_cache(maxsize=None)
def probe_graph(kind, count, grid=False):
    """The Graph of a probe: 'chain' (alignment.chain_graph over a seeded sequence with repeats), 'ties' (`tie_graph`,
    reach 3) or 'wide' (`tie_graph`, reach 15: above 4096 arcs at 300 states, more than the programme keeps in LDS)."""
    if kind == 'chain':
        return alignment.chain_graph(phoneme_sequence(5, count))
    phonemes, arcs, stay, initial, final = tie_graph(count, 11, 15 if kind == 'wide' else 3, grid)
    return alignment.graph(phonemes, arcs, stay=stay, initial=initial, final=final)


# ---- the probes of the GPU list ----------------------------------------------------------------------------------------

SEED = 3
DENSITY = 0.3
FORCED_FRAMES = (1, 2, 31, 32, 33, 63, 64, 65, 97, 129)
FORCED_COUNTS = (1, 2, 31, 32, 63, 64, 65)
FORCED_LARGE = ((260, 255), (260, 256), (260, 257), (300, 257), (1030, 1024))
FORCED_SHAPES = tuple((t, n) for t in FORCED_FRAMES for n in FORCED_COUNTS if n <= t) + FORCED_LARGE
PATTERNS = ('even', 'odd', 'edges')
# the mandatory phonemes equal the frames (every optional one must be left out); N > T
OPTIONAL_EXTRA = ((32, 64, 'odd'), (31, 61, 'even'), (129, 257, 'even'))
SEARCH_FRAMES = (97, 130)
SEARCH_COUNTS = (1, 8, 64, 65, 256)          # 257 is beyond SEARCH_MAX_PHONEMES: the GPU test asserts the refusal
SEARCH_EXTRA = ((300, 256),)                 # a recording in which 256 phonemes fit: the 4-state strips to their last lane
SEARCH_TOP = 3
RECOGNIZE_FRAMES = (1, 2, 31, 32, 33, 63, 64, 65, 129, 4100)
VITERBI_FRAMES = (33, 65, 129)
VITERBI_GRAPHS = (('chain', 3), ('ties', 3), ('chain', 64), ('ties', 64), ('ties', 65), ('chain', 65), ('ties', 256),
                  ('ties', 257), ('chain', 257), ('ties', 700), ('wide', 300))
DECODE_FRAMES = (1, 63, 64, 65, 130)
STREAM_FRAMES, STREAM_PUSHES = 97, (1, 31, 33, 32)


def optional_probes():
    """(T, N, pattern) of every legal combination of the forced shapes and the three patterns, and the extras."""
    out = [(t, n, p) for t, n in FORCED_SHAPES for p in PATTERNS if OR.legal(flags_for(n, p), t)]
    return out + [case for case in OPTIONAL_EXTRA if case not in out]


@functools.lru_cache(maxsize=None)
def forced_probe(frames, count, seed=SEED, density=DENSITY):
    """(ppg, phonemes) of a forced probe; with optional phonemes the transcript may be longer than the recording."""
    return binary_ppg(seed, frames, density), tuple(phoneme_sequence(seed, count))


@functools.lru_cache(maxsize=None)
def search_probe(frames, count, seed=SEED):
    """(ppg, query).  Short queries are planted several times, perfectly and with one flaw each, so that the picker's
    tie rule and its striking-out decide; long ones once where they fit."""
    query = phoneme_sequence(seed + 2, count)
    if count == 1:
        return binary_ppg(seed, frames, DENSITY), tuple(query)
    if count <= 8:
        places = [3 + k * (count + 3) for k in range(7)]
        perfect = (0, 2, 5) if frames < 100 else (2,)          # the longer recording: one perfect, six equally flawed
        return planted_ppg(seed, frames, query, perfect=[places[k] for k in perfect],
                           flawed=[at for k, at in enumerate(places) if k not in perfect]), tuple(query)
    ppg = planted_ppg(seed, frames, query, perfect=(5,)) if count + 8 <= frames else binary_ppg(seed, frames, 0.1)
    ppg = torch.maximum(ppg, binary_ppg(seed + 1, frames, DENSITY))     # noise on top: the planted match is one of many
    return ppg, tuple(query)


def recognize_probe(frames, regime):
    """(ppg, model): regime 'binary' (i) or 'grid' (ii)."""
    if regime == 'binary':
        return binary_ppg(SEED, frames, DENSITY), banded_model()
    return hot_ppg(frames), grid_model(SEED)


def viterbi_probe(kind, count, frames, regime):
    """(ppg, graph).  A chain is regime (i) only: its weights are 0 / -inf by construction."""
    if regime == 'binary':
        return binary_ppg(SEED, frames, DENSITY), probe_graph(kind, count)
    return hot_ppg(frames), probe_graph(kind, count, True)


def viterbi_probes():
    """(kind, states, T, regime) of the GPU list: a chain needs as many frames as states."""
    out = []
    for kind, count in VITERBI_GRAPHS:
        for frames in VITERBI_FRAMES:
            if kind == 'chain' and count > frames:
                continue
            out.append((kind, count, frames, 'binary'))
            if kind != 'chain':
                out.append((kind, count, frames, 'grid'))
    return out


def run_mutant(entry, frames, count, seed, mutant, extra=None):
    """What `mutant` (None: no fault) makes of one probe of the GPU list, in a form that `==` compares: the entry is
    'forced', 'optional' (extra: the pattern), 'search', 'pick', 'recognize' (extra: the regime; count is unused) or
    'viterbi' (extra: (kind, regime))."""
    if entry in ('forced', 'optional'):
        ppg, phonemes = forced_probe(frames, count, seed)
        flags = None if entry == 'forced' else flags_for(count, extra)
        total, starts = forced_programme(cold(ppg)[:, list(phonemes)], flags, mutant)
        return total, starts.tolist()
    if entry in ('search', 'pick'):
        ppg, query = search_probe(frames, count, seed)
        curve_total, curve_begin = search_programme(SR.emissions(cold(ppg), list(query)),
                                                    mutant if entry == 'search' else None)
        if entry == 'search':                                  # the curve alone: a broken one need not have means
            return curve_total.tolist(), curve_begin.tolist()
        hits = pick(curve32(curve_total, curve_begin, sums(HOST_L, frames)), curve_begin, count, SEARCH_TOP,
                    mutant=mutant if entry == 'pick' else None)
        return curve_total.tolist(), curve_begin.tolist(), [(b, e, float(t), float(m)) for b, e, t, m in hits]
    if entry == 'recognize':
        ppg, model = recognize_probe(frames, extra)
        total, states, ordinals = graph_programme(cold(ppg), model_lists(*model), mutant)
    else:
        kind, regime = extra
        ppg, graph = viterbi_probe(kind, count, frames, regime)
        g = V.lists(graph)
        total, states, ordinals = graph_programme(V.emissions(cold(ppg), g.sym), g, mutant)
    if states is None:
        return total, None, None
    run_states, starts = V.runs(states, ordinals)
    return total, run_states.tolist(), starts.tolist()


# mutant -> (entry, T, N, seed, extra): one probe of the GPU list whose expected output the mutant changes; the host test
# checks every line and prints every probe that catches each mutant
CAUGHT_BY = {
    'advance_on_tie': ('forced', 97, 65, SEED, None),
    'skip_before_advance': ('optional', 97, 65, SEED, 'edges'),
    'strip_carry': ('forced', 97, 65, SEED, None),
    'state0_fed': ('forced', 33, 2, SEED, None),
    'stale_chunk': ('forced', 33, 31, SEED, None),
    'refill_edge': ('forced', 97, 31, SEED, None),
    'top_strip_bit': ('forced', 97, 65, SEED, None),
    'begin_not_carried': ('search', 97, 8, SEED, None),
    'origin_late': ('search', 97, 8, SEED, None),
    'pick_earliest': ('pick', 97, 8, SEED, None),
    'highest_source': ('recognize', 33, 0, SEED, 'binary'),
    'switch_beats_stay': ('recognize', 33, 0, SEED, 'binary'),
    'last_end_state': ('viterbi', 33, 64, SEED, ('ties', 'binary')),
}

# the forced probes with 1 < N < T on whose optimal path no exact tie lies (`advance_on_tie` leaves `starts` alone): at
# most one in ten, listed by name; the host test asserts this is the list
NO_TIE_ON_THE_PATH = ((65, 64), (129, 2))
