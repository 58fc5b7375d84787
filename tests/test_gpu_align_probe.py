"""The alignment family on the GPU (ppg_align.hip) against tests/align_probe.py, bit for bit: PPGs of
zeros and ones, on which every sum the kernels form is S_k = the sequential fp32 sum of k copies of L = logf(1e-8f), ties
between candidates are exact and frequent, and the suite's float64 references with the documented tie rules give the one
path, the one curve and the counts k the device must give.  L is read from the device once; every other assertion
compares integers or the bits of floats with what align_probe derives from that L.  Nothing here has a tolerance.

tests/test_align_probe_host.py shows, without a GPU, that these probes catch every mutant of align_probe.MUTANTS."""
import math

import numpy as np
import pytest
import torch

from ppgs_amd import alignment

import align_probe as AP
from test_gpu_alignment_optional import flags_for

pytestmark = pytest.mark.gpu

MOST_COLD = 4200                                               # no probe has more frames than this
_kept = {}


def bits(values):
    return np.array(values, dtype=np.float32).view(np.int32)   # (a copy: contiguous, and a scalar stays one)


@pytest.fixture(scope='module')
def table():
    """S_0 .. S_4200 for the device's own L, read once as the total of one cold frame."""
    total = alignment.forced(torch.zeros(40, 1).cuda(), [0]).total
    L = np.float32(total.cpu().numpy())
    distance = abs(int(bits(L)) - int(bits(AP.HOST_L)))
    print(f'the device\'s L = {float(L)!r}, bits {int(bits(L)) & 0xffffffff:#010x}; numpy\'s log(float32(1e-8)) has bits '
          f'{int(bits(AP.HOST_L)) & 0xffffffff:#010x}: {distance} ulp apart')
    assert distance <= 1
    one = alignment.forced(torch.ones(40, 1).cuda(), [0])
    assert int(bits(one.total.cpu().numpy())) == 0             # logf(1) = +0: the clamp's upper end is 1.0f
    return AP.sums(L, MOST_COLD)


def kept(key, make):
    """An expectation computed once and shared by the tests that need it; never modified."""
    if key not in _kept:
        _kept[key] = make()
    return _kept[key]


def same_floats(got, expected):
    """fp32 bit for bit; NaN (a phoneme that was left out) where and only where NaN is expected."""
    got, expected = np.asarray(got.cpu().numpy(), dtype=np.float32), np.asarray(expected, dtype=np.float32)
    if got.shape != expected.shape:
        return False
    nan = np.isnan(expected)
    return bool((np.isnan(got) == nan).all() and (bits(got)[~nan] == bits(expected)[~nan]).all())


def same_ints(got, expected):
    return got.dtype == torch.int32 and got.cpu().tolist() == np.asarray(expected).tolist()


def check(got, expected, label, fields):
    for name in fields:
        value = getattr(got, name)
        if np.asarray(expected[name]).dtype.kind == 'f':
            assert same_floats(value, expected[name]), (label, name, value.cpu().tolist(), expected[name].tolist())
        else:
            assert same_ints(value, expected[name]), (label, name, value.cpu().tolist(), expected[name].tolist())


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.contiguous().view(torch.int32),
                                                                     b.contiguous().view(torch.int32))


def padded(ppgs):
    """(B, 40, Tmax) with NaN past every item's own frames, and the lengths."""
    lengths = [ppg.shape[1] for ppg in ppgs]
    batch = torch.full((len(ppgs), 40, max(lengths)), float('nan'))
    for b, ppg in enumerate(ppgs):
        batch[b, :, :lengths[b]] = ppg
    return batch.cuda(), lengths


# ---- forced alignment, plain and with optional phonemes ----

ALIGNMENT = ('starts', 'total', 'score', 'gop')


def forced_expected(frames, count, pattern, table):
    ppg, phonemes = AP.forced_probe(frames, count)
    flags = None if pattern is None else flags_for(count, pattern)
    return kept(('forced', frames, count, pattern), lambda: AP.expect_forced(ppg, list(phonemes), flags, table))


def forced_cases():
    return [(t, n, None) for t, n in AP.FORCED_SHAPES] + AP.optional_probes()


def test_the_forced_cases_are_the_ones_the_kernels_can_go_wrong_at():
    cases = forced_cases()
    assert {t for t, _, _ in cases} >= {1, 2, 31, 32, 33, 63, 64, 65, 97, 129, 260, 300, 1030}
    assert {n for _, n, _ in cases} >= {1, 2, 31, 32, 63, 64, 65, 255, 256, 257, 1024}
    assert {p for _, _, p in cases} == {None, 'even', 'odd', 'edges'}
    assert any(p and flags_for(n, p).count(False) == t for t, n, p in cases) and any(n > t for t, n, _ in cases)
    assert (1030 - 1) // 16 >= 63 and 1024 == 64 * 16          # lane 63 of the 16-state strips holds states


@pytest.mark.parametrize('frames,count', sorted({(t, n) for t, n, _ in forced_cases()}))
def test_forced_alone(frames, count, table):
    ppg, phonemes = AP.forced_probe(frames, count)
    device = ppg.cuda()
    for _, _, pattern in [case for case in forced_cases() if case[:2] == (frames, count)]:
        expected = forced_expected(frames, count, pattern, table)
        flags = None if pattern is None else flags_for(count, pattern)
        got = alignment.forced(device, list(phonemes), optional=flags)
        check(got, expected, f'forced T={frames} N={count} {pattern}', ALIGNMENT)
        assert got.phonemes.tolist() == list(phonemes)


@pytest.mark.parametrize('optional', [False, True])
def test_forced_in_one_ragged_batch(optional, table):
    cases = [case for case in forced_cases() if (case[2] is not None) == optional]
    probes = [AP.forced_probe(t, n) for t, n, _ in cases]
    batch, lengths = padded([ppg for ppg, _ in probes])
    counts = [n for _, n, _ in cases]
    phonemes = torch.full((len(cases), max(counts)), -1, dtype=torch.int64)
    flags = torch.full((len(cases), max(counts)), -1, dtype=torch.int64)
    for b, ((_, sequence), (_, n, pattern)) in enumerate(zip(probes, cases)):
        phonemes[b, :n] = torch.tensor(sequence)
        if optional:
            flags[b, :n] = torch.tensor(flags_for(n, pattern), dtype=torch.int64)
    got = alignment.forced(batch, phonemes, lengths, counts, optional=flags if optional else None)
    for b, (frames, count, pattern) in enumerate(cases):
        label = f'forced T={frames} N={count} {pattern} as item {b}'
        one = type(got)(got.phonemes[b], got.starts[b], got.total[b], got.score[b], got.gop[b])
        check(one, forced_expected(frames, count, pattern, table), label, ALIGNMENT)
        single = alignment.forced(batch[b, :, :frames], list(probes[b][1]),
                                  optional=flags_for(count, pattern) if optional else None)
        assert torch.equal(one.starts, single.starts) and same_bits(one.total, single.total), label
        assert same_bits(one.score, single.score) and same_bits(one.gop, single.gop), label


# ---- phrase search ----

def search_expected(ppg, query, table, key):
    return kept(('search',) + key, lambda: AP.expect_search(ppg, list(query), table, AP.SEARCH_TOP))


def check_hits(begin, end, total, mean, count, curve, frames, expected, label):
    hits = expected['hits']
    assert int(count) == len(hits), (label, int(count), hits)
    assert begin.tolist() == [hit[0] for hit in hits] + [-1] * (AP.SEARCH_TOP - len(hits)), (label, begin.tolist(), hits)
    assert end.tolist() == [hit[1] for hit in hits] + [-1] * (AP.SEARCH_TOP - len(hits)), (label, end.tolist(), hits)
    rest = [np.float32(np.nan)] * (AP.SEARCH_TOP - len(hits))
    assert same_floats(total, np.asarray([hit[2] for hit in hits] + rest, dtype=np.float32)), (label, total.tolist(), hits)
    assert same_floats(mean, np.asarray([hit[3] for hit in hits] + rest, dtype=np.float32)), (label, mean.tolist(), hits)
    assert same_floats(curve[0][:frames], expected['totals']), label
    assert same_ints(curve[1][:frames], expected['begins']), label
    assert bool((curve[0][frames:] == -math.inf).all()) and bool((curve[1][frames:] == -1).all()), label


@pytest.mark.parametrize('frames,count', [(t, n) for t in AP.SEARCH_FRAMES for n in AP.SEARCH_COUNTS] +
                         list(AP.SEARCH_EXTRA))
def test_search_alone(frames, count, table):
    ppg, query = AP.search_probe(frames, count)
    expected = search_expected(ppg, query, table, (frames, count))
    got = alignment.search(ppg.cuda(), list(query), top=AP.SEARCH_TOP, curve=True)
    check_hits(got.begin, got.end, got.total, got.mean, got.count, got.curve, frames, expected,
               f'search T={frames} N={count}')
    if count > frames:
        assert int(got.count) == 0 and bool((got.curve[1] == -1).all())


def test_search_refuses_a_query_beyond_its_limit():
    assert alignment.SEARCH_MAX_PHONEMES == 256                # 257 phonemes: refused on the host, nothing is launched
    with pytest.raises(ValueError, match='at most 256 phonemes'):
        alignment.search(AP.binary_ppg(AP.SEED, 97).cuda(), AP.phoneme_sequence(AP.SEED, 257), top=AP.SEARCH_TOP)


def test_search_in_one_ragged_batch_of_two_recordings_by_three_queries(table):
    recordings = [AP.search_probe(97, 8)[0], AP.search_probe(130, 8)[0]]
    queries = [list(AP.search_probe(97, n)[1]) for n in (1, 8, 65)]
    batch, lengths = padded(recordings)
    got = alignment.search(batch, queries, lengths, top=AP.SEARCH_TOP, curve=True)
    for b, ppg in enumerate(recordings):
        for q, query in enumerate(queries):
            label = f'search recording {b} query {q}'
            expected = search_expected(ppg, query, table, ('batch', b, q))
            check_hits(got.begin[b, q], got.end[b, q], got.total[b, q], got.mean[b, q], got.count[b, q],
                       (got.curve[0][b, q], got.curve[1][b, q]), lengths[b], expected, label)
            single = alignment.search(batch[b, :, :lengths[b]], query, top=AP.SEARCH_TOP, curve=True)
            assert torch.equal(single.begin, got.begin[b, q]) and torch.equal(single.end, got.end[b, q]), label
            assert same_bits(single.total, got.total[b, q]) and same_bits(single.mean, got.mean[b, q]), label
            assert same_bits(single.curve[0], got.curve[0][b, q, :lengths[b]]), label
            assert torch.equal(single.curve[1], got.curve[1][b, q, :lengths[b]]), label


def test_every_search_probe_in_one_ragged_batch(table):
    """Every probe's recording against every probe's query: the probes themselves are the pairs (b, its own N)."""
    shapes = [(t, n) for t in AP.SEARCH_FRAMES for n in AP.SEARCH_COUNTS] + list(AP.SEARCH_EXTRA)
    recordings = [AP.search_probe(t, n)[0] for t, n in shapes]
    queries = [list(AP.search_probe(AP.SEARCH_FRAMES[0], n)[1]) for n in AP.SEARCH_COUNTS]
    batch, lengths = padded(recordings)
    got = alignment.search(batch, queries, lengths, top=AP.SEARCH_TOP, curve=True)
    for b, (frames, count) in enumerate(shapes):
        assert list(AP.search_probe(frames, count)[1]) == queries[AP.SEARCH_COUNTS.index(count)]
        for q, query in enumerate(queries):
            own = len(query) == count
            expected = search_expected(recordings[b], query, table, (frames, count) if own else ('all', b, q))
            check_hits(got.begin[b, q], got.end[b, q], got.total[b, q], got.mean[b, q], got.count[b, q],
                       (got.curve[0][b, q], got.curve[1][b, q]), frames, expected, f'search recording {b} query {q}')


# ---- the recogniser ----

RUNS = ('phonemes', 'starts', 'total', 'score', 'gop')


def recognize_expected(frames, regime, table):
    ppg, model = AP.recognize_probe(frames, regime)
    return kept(('recognize', frames, regime), lambda: AP.expect_recognize(ppg, model, table, regime))


@pytest.mark.parametrize('regime', ['binary', 'grid'])
@pytest.mark.parametrize('frames', AP.RECOGNIZE_FRAMES)
def test_recognize_alone(frames, regime, table):
    ppg, model = AP.recognize_probe(frames, regime)
    A, initial, final = AP.model_tensors(model)
    got = alignment.recognize(ppg.cuda(), transitions=A, initial=initial, final=final)
    check(got, recognize_expected(frames, regime, table), f'recognize T={frames} {regime}', RUNS)


@pytest.mark.parametrize('regime', ['binary', 'grid'])
def test_recognize_in_one_ragged_batch(regime, table):
    probes = [AP.recognize_probe(frames, regime) for frames in AP.RECOGNIZE_FRAMES]
    A, initial, final = AP.model_tensors(probes[0][1])
    batch, lengths = padded([ppg for ppg, _ in probes])
    got = alignment.recognize(batch, lengths, transitions=A, initial=initial, final=final)
    for b, frames in enumerate(AP.RECOGNIZE_FRAMES):
        label = f'recognize T={frames} {regime} as item {b}'
        one = type(got)(got.phonemes[b], got.starts[b], got.total[b], got.score[b], got.gop[b])
        check(one, recognize_expected(frames, regime, table), label, RUNS)
        single = alignment.recognize(batch[b, :, :frames], transitions=A, initial=initial, final=final)
        assert torch.equal(one.phonemes, single.phonemes) and torch.equal(one.starts, single.starts), label
        assert same_bits(one.total, single.total) and same_bits(one.score, single.score), label
        assert same_bits(one.gop, single.gop), label


# ---- the graph Viterbi ----

PATH = ('states', 'phonemes', 'starts', 'total', 'score', 'gop')


def viterbi_expected(kind, count, frames, regime, table):
    ppg, graph = AP.viterbi_probe(kind, count, frames, regime)
    return kept(('viterbi', kind, count, frames, regime), lambda: AP.expect_viterbi(ppg, graph, table, regime))


def test_the_viterbi_cases_are_the_ones_the_kernel_can_go_wrong_at():
    cases = AP.viterbi_probes()
    assert {n for _, n, _, _ in cases} >= {3, 64, 65, 256, 257, 700} and {t for _, _, t, _ in cases} == {33, 65, 129}
    assert {(kind, regime) for kind, _, _, regime in cases} >= {('chain', 'binary'), ('ties', 'binary'), ('ties', 'grid'),
                                                                ('wide', 'binary'), ('wide', 'grid')}
    assert int(AP.probe_graph('wide', 300).offsets[-1]) > 4096          # VHELD of ppg_align.hip: arcs kept in LDS


@pytest.mark.parametrize('kind,count,frames,regime', AP.viterbi_probes())
def test_viterbi_alone(kind, count, frames, regime, table):
    ppg, graph = AP.viterbi_probe(kind, count, frames, regime)
    got = alignment.viterbi(ppg.cuda(), graph)
    expected = viterbi_expected(kind, count, frames, regime, table)
    check(got, expected, f'viterbi {kind} S={count} T={frames} {regime}', PATH)
    assert math.isfinite(float(expected['total'])) and len(expected['states']) >= 1


def test_viterbi_in_one_ragged_batch_with_a_graph_per_item(table):
    cases = AP.viterbi_probes()
    probes = [AP.viterbi_probe(*case) for case in cases]
    batch, lengths = padded([ppg for ppg, _ in probes])
    graphs = [graph for _, graph in probes]                    # one object stands for several items and travels once
    got = alignment.viterbi(batch, graphs, lengths)
    for b, case in enumerate(cases):
        label = f'viterbi {case} as item {b}'
        one = type(got)(got.states[b], got.phonemes[b], got.starts[b], got.total[b], got.score[b], got.gop[b])
        check(one, viterbi_expected(*case, table), label, PATH)
        single = alignment.viterbi(batch[b, :, :lengths[b]], graphs[b])
        assert torch.equal(one.states, single.states) and torch.equal(one.starts, single.starts), label
        assert same_bits(one.total, single.total) and same_bits(one.score, single.score), label
        assert same_bits(one.gop, single.gop), label


# ---- the run-length decode ----

def decode_probe(frames):
    return AP.binary_ppg(AP.SEED, frames, 0.05, dead=max(1, frames // 8))


def test_decode_takes_the_lowest_index_on_ties_and_0_on_a_dead_frame_alone_and_in_a_batch():
    ppgs = [decode_probe(frames) for frames in AP.DECODE_FRAMES]
    batch, lengths = padded(ppgs)
    together = alignment.decode(batch, lengths)
    for b, ppg in enumerate(ppgs):
        expected = AP.expect_decode(ppg)
        got = alignment.decode(ppg.cuda())
        check(got, expected, f'decode T={lengths[b]}', ('phonemes', 'starts'))
        assert torch.equal(together.phonemes[b], got.phonemes) and torch.equal(together.starts[b], got.starts)
    assert alignment.decode(torch.zeros(40, 1).cuda()).phonemes.tolist() == [0]


# ---- the live decoders: one recording of 97 frames pushed as 1 + 31 + 33 + 32 ----

def pushed(stream, ppg):
    pieces, at = [], 0
    for frames in AP.STREAM_PUSHES:
        pieces.append(stream.push(ppg[:, at:at + frames]))
        at += frames
    assert at == ppg.shape[1] == AP.STREAM_FRAMES
    return pieces


def joined_runs(pieces, names):
    """The runs of the pushes and of the flush behind one another; the slots at or past count are -1 / NaN."""
    out = {name: [] for name in names}
    for piece in pieces:
        count = int(piece.count)
        assert 0 <= count <= piece.begin.shape[0]
        for name in names:
            value = getattr(piece, name)
            out[name].append(value[:count])
            rest = value[count:]
            assert bool((torch.isnan(rest) if rest.is_floating_point() else rest == -1).all()), name
    return {name: torch.cat(values) for name, values in out.items()}


def test_search_stream_gives_the_curve_of_the_whole_recording(table):
    ppg, query = AP.search_probe(AP.STREAM_FRAMES, 8)
    expected = search_expected(ppg, query, table, (AP.STREAM_FRAMES, 8))
    stream = alignment.SearchStream(list(query), threshold=-math.inf, curve=True)
    pieces = pushed(stream, ppg.cuda())
    stream.flush()
    assert same_floats(torch.cat([piece.curve[0] for piece in pieces]), expected['totals'])
    assert same_ints(torch.cat([piece.curve[1] for piece in pieces]), expected['begins'])


def check_stream(pieces, last, expected, names):
    assert int(last.forced) == 0                               # nothing was given out by force
    runs = joined_runs(pieces + [last], names + ('begin', 'end', 'score', 'gop'))
    for name in names:
        assert same_ints(runs[name], expected[name]), (name, runs[name].tolist(), expected[name].tolist())
    assert same_ints(runs['begin'], expected['starts'][:-1]) and same_ints(runs['end'], expected['starts'][1:])
    assert same_floats(runs['score'], expected['score']) and same_floats(runs['gop'], expected['gop'])
    assert same_floats(last.total, expected['total'])


def test_recognize_stream_gives_the_runs_of_the_whole_recording(table):
    ppg, model = AP.recognize_probe(AP.STREAM_FRAMES, 'binary')
    expected = kept(('recognize', AP.STREAM_FRAMES, 'binary'), lambda: AP.expect_recognize(ppg, model, table, 'binary'))
    A, initial, final = AP.model_tensors(model)
    stream = alignment.RecognizeStream(transitions=A, initial=initial, final=final)
    pieces = pushed(stream, ppg.cuda())
    check_stream(pieces, stream.flush(), expected, ('phonemes',))


def test_viterbi_stream_gives_the_runs_of_the_whole_recording(table):
    ppg, graph = AP.viterbi_probe('ties', 64, AP.STREAM_FRAMES, 'binary')
    expected = kept(('viterbi', 'ties', 64, AP.STREAM_FRAMES, 'binary'),
                    lambda: AP.expect_viterbi(ppg, graph, table, 'binary'))
    stream = alignment.ViterbiStream(graph)
    pieces = pushed(stream, ppg.cuda())
    check_stream(pieces, stream.flush(), expected, ('states', 'phonemes'))
