"""The probes of tests/align_probe.py without a GPU: the numpy restatements of the alignment recurrences equal the suite's
float64 references (and brute force on tiny shapes) on every probe of the GPU list, every mutant changes the expected
output of a named probe, the tie mutants are invisible to the inputs the suite had before, and the inputs meet the
conditions that make them probes."""
import numpy as np
import torch

import alignment_optional_reference as OR
import alignment_reference as R
import recognize_reference as RR
import search_reference as SR
import viterbi_reference as V

import align_probe as AP
from test_gpu_alignment import CASES as OLD_CASES
from test_gpu_alignment_optional import flags_for

FORCED_MUTANTS = ('advance_on_tie', 'skip_before_advance', 'strip_carry', 'state0_fed', 'stale_chunk', 'refill_edge',
                  'top_strip_bit')
SEARCH_MUTANTS = ('advance_on_tie', 'strip_carry', 'stale_chunk', 'begin_not_carried', 'origin_late')
GRAPH_MUTANTS = ('stale_chunk', 'refill_edge', 'highest_source', 'switch_beats_stay', 'last_end_state')


def test_the_construction_is_exact():
    """The clamp's upper end is 1.0f, and S_k is strictly decreasing up to 65536 for L and its two fp32 neighbours: the
    device's logf may be either neighbour and the isomorphism with the count of cold frames still holds."""
    assert np.float32(1) - np.float32(1e-8) == np.float32(1)
    assert np.log(np.float32(1)) == 0 and not np.signbit(np.log(np.float32(1)))
    L = AP.HOST_L
    assert L.dtype == np.float32 and abs(float(L) + 18.420681) < 1e-5
    for value in (np.nextafter(L, np.float32(-np.inf)), L, np.nextafter(L, np.float32(0))):
        table = AP.sums(value, AP.MOST)
        assert table.dtype == np.float32 and table[0] == 0 and not np.signbit(table[0]) and table[1] == value
        assert (np.diff(table) < 0).all() and np.isfinite(table).all()
    print(f'L = {float(L)!r} (bits {int(L.view(np.int32)) & 0xffffffff:#010x}), S_65536 = {float(table[-1])!r}')


def test_the_inputs_are_what_they_say():
    ppg = AP.binary_ppg(1, 97, 0.3)
    assert ppg.shape == (40, 97) and ppg.dtype == torch.float32 and set(ppg.unique().tolist()) == {0., 1.}
    assert int((ppg.sum(0) == 0).sum()) >= 97 // 8
    assert torch.equal(AP.binary_ppg(1, 97, 0.3), ppg) and not torch.equal(AP.binary_ppg(2, 97, 0.3), ppg)
    assert bool((AP.hot_ppg(5) == 1).all())
    sequence = AP.phoneme_sequence(3, 65)
    assert len(sequence) == 65 and any(a == b for a, b in zip(sequence, sequence[1:])) and len(set(sequence)) > 20
    for count in (3, 64, 65, 256, 257, 700):
        for kind in ('ties', 'wide'):
            graph = AP.probe_graph(kind, count)
            assert graph.phonemes.shape[0] == count
    assert int(AP.probe_graph('wide', 300).offsets[-1]) > 4096          # more arcs than the programme keeps in LDS
    sources = AP.probe_graph('ties', 64).sources.tolist()
    offsets = AP.probe_graph('ties', 64).offsets.tolist()
    assert any(len(set(sources[a:b])) < b - a for a, b in zip(offsets, offsets[1:]))      # parallel arcs
    assert any(n in sources[a:b] for n, (a, b) in enumerate(zip(offsets, offsets[1:])))   # an arc n -> n
    for value in AP.GRID:
        assert value * 8 == int(value * 8) and -4 <= value <= 0


# ---- the restatements without a fault ----

def test_forced_restatement_equals_the_references_on_every_probe():
    for frames, count in AP.FORCED_SHAPES:
        ppg, phonemes = AP.forced_probe(frames, count)
        e = AP.cold(ppg)[:, list(phonemes)]
        total, starts = AP.forced_programme(e)
        ref_total, ref_starts = R.programme(e)
        assert total == ref_total and starts.tolist() == ref_starts.tolist(), (frames, count)
        again, same = AP.forced_programme(e, [False] * count)
        assert again == total and same.tolist() == starts.tolist()
    for frames, count, pattern in AP.optional_probes():
        ppg, phonemes = AP.forced_probe(frames, count)
        flags = flags_for(count, pattern)
        e = AP.cold(ppg)[:, list(phonemes)]
        total, starts = AP.forced_programme(e, flags)
        ref_total, ref_starts = OR.programme(e, flags)
        assert total == ref_total and starts.tolist() == ref_starts.tolist(), (frames, count, pattern)


def test_restatements_equal_brute_force_on_tiny_shapes():
    for seed in range(6):
        for frames, count in ((4, 2), (6, 3), (7, 4), (8, 2), (5, 5)):
            ppg = AP.binary_ppg(seed, frames, 0.4, dead=1)
            phonemes = AP.phoneme_sequence(seed, count)
            logp = AP.cold(ppg)
            e = logp[:, phonemes]
            total, starts = AP.forced_programme(e)
            brute_total, brute_starts = R.brute_force(e)
            assert total == brute_total and starts.tolist() == brute_starts.tolist()
            for pattern in ('even', 'odd'):
                flags = flags_for(count, pattern)
                if OR.legal(flags, frames):
                    total, starts = AP.forced_programme(e, flags)
                    brute_total, optima = OR.brute_force(e, flags)
                    assert total == brute_total and tuple(starts.tolist()) in optima
            r = SR.emissions(logp, phonemes)
            curve_total, curve_begin = AP.search_programme(r)
            brute_total, brute_begin = SR.brute_force(r)
            assert curve_total.tolist() == brute_total.tolist() and curve_begin.tolist() == brute_begin.tolist()
    rng = np.random.default_rng(4)
    for seed in range(6):
        e = -(rng.random((5, 3)) < 0.5).astype(np.float64)
        A = np.where(rng.random((3, 3)) < 0.2, -np.inf, 0.)
        model = (A, np.zeros(3), np.zeros(3))
        total, states, _ = AP.graph_programme(e, AP.model_lists(*model))
        brute_total, brute_labels = RR.brute_force(e, *model)
        assert total == brute_total and (states is None) == (brute_labels is None)
        assert states is None or states.tolist() == brute_labels.tolist()
        phonemes, arcs, stay, initial, final = AP.tie_graph(4, seed, reach=2)
        g = V.Lists(np.asarray(phonemes), np.asarray(stay), [[(s, w) for s, n, w in arcs if n == m] for m in range(4)],
                    np.asarray(initial), np.asarray(final))
        e = -(rng.random((5, 4)) < 0.5).astype(np.float64)
        got, brute = AP.graph_programme(e, g), V.brute_force(e, g)
        assert got[0] == brute[0] and got[1].tolist() == brute[1].tolist() and got[2].tolist() == brute[2].tolist()


def search_shapes():
    return [(t, n) for t in AP.SEARCH_FRAMES for n in AP.SEARCH_COUNTS] + list(AP.SEARCH_EXTRA)


def test_search_and_pick_restatements_equal_the_references_on_every_probe():
    table = AP.sums(AP.HOST_L, 400)
    perfect = flawed = 0
    for frames, count in search_shapes():
        ppg, query = AP.search_probe(frames, count)
        r = SR.emissions(AP.cold(ppg), list(query))
        curve_total, curve_begin = AP.search_programme(r)
        ref_total, ref_begin = SR.programme(r)
        assert curve_total.tolist() == ref_total.tolist() and curve_begin.tolist() == ref_begin.tolist()
        expected = AP.expect_search(ppg, list(query), table, AP.SEARCH_TOP)
        hits = AP.pick(expected['totals'], curve_begin, count, AP.SEARCH_TOP)
        assert AP.same_hits(hits, expected['hits'])
        assert AP.same_hits(hits, SR.pick_by_the_letter(expected['totals'], curve_begin, count, AP.SEARCH_TOP))
        assert (len(hits) == 0) == (count > frames) and (count > frames or len(hits) >= 1)
        means = [float(hit[3]) for hit in hits]
        perfect += means.count(0.) >= 2
        flawed += any(a == b != 0 for a, b in zip(means, means[1:]))
        print(f'search T={frames} N={count}: hits {[(b, e, float(m)) for b, e, _, m in hits]}')
    # several perfect occurrences and several equally imperfect ones: the picker's tie rule and its striking-out decide
    assert perfect >= 1 and flawed >= 1


def test_recognize_and_viterbi_restatements_equal_the_references_on_every_probe():
    for frames in AP.RECOGNIZE_FRAMES:
        for regime in ('binary', 'grid'):
            ppg, model = AP.recognize_probe(frames, regime)
            e = AP.cold(ppg)
            total, states, _ = AP.graph_programme(e, AP.model_lists(*model))
            ref_total, labels = RR.viterbi(e, *model)
            assert total == ref_total > -np.inf and states.tolist() == labels.tolist(), (frames, regime)
            if frames >= 31:                                   # neither trivial: a cost, and more than one run
                assert total < 0 and len(RR.runs(labels)[0]) > 1, (frames, regime)
    for kind, count, frames, regime in AP.viterbi_probes():
        ppg, graph = AP.viterbi_probe(kind, count, frames, regime)
        g = V.lists(graph)
        e = V.emissions(AP.cold(ppg), g.sym)
        got, ref = AP.graph_programme(e, g), V.viterbi(e, g)
        assert got[0] == ref[0] > -np.inf, (kind, count, frames, regime)
        assert got[1].tolist() == ref[1].tolist() and got[2].tolist() == ref[2].tolist(), (kind, count, frames, regime)
        assert len(V.runs(ref[1], ref[2])[0]) > 1 or count > frames


def test_decode_restatement_equals_the_reference():
    for frames in AP.DECODE_FRAMES:
        ppg = AP.binary_ppg(AP.SEED, frames, 0.05, dead=max(1, frames // 8))
        phonemes, starts = AP.decode_runs(ppg)
        expected = AP.expect_decode(ppg)
        assert phonemes.tolist() == expected['phonemes'].tolist() and starts.tolist() == expected['starts'].tolist()
        labels = RR.expand(phonemes, starts)
        dead = (ppg.sum(0) == 0).numpy()
        assert dead.any() and (labels[dead] == 0).all()                     # 0 on a dead frame
        assert frames < 63 or ((ppg.sum(0) > 1).numpy() & (labels > 0)).any()     # a tie that the lowest index wins


# ---- the mutants ----

def all_probes():
    """(entry, T, N, seed, extra) of the GPU list, but for the recordings above 129 frames of the recogniser."""
    out = [('forced', t, n, AP.SEED, None) for t, n in AP.FORCED_SHAPES]
    out += [('optional', t, n, AP.SEED, p) for t, n, p in AP.optional_probes()]
    out += [(entry, t, n, AP.SEED, None) for entry in ('search', 'pick') for t, n in search_shapes()]
    out += [('recognize', t, 0, AP.SEED, regime) for t in AP.RECOGNIZE_FRAMES if t <= 129 for regime in ('binary', 'grid')]
    out += [('viterbi', t, n, AP.SEED, (kind, regime)) for kind, n, t, regime in AP.viterbi_probes()]
    return out


def mutants_of(entry):
    return {'forced': FORCED_MUTANTS, 'optional': FORCED_MUTANTS, 'search': SEARCH_MUTANTS, 'pick': ('pick_earliest',),
            'recognize': GRAPH_MUTANTS, 'viterbi': GRAPH_MUTANTS}[entry]


def test_every_mutant_is_caught_by_a_named_probe_of_the_gpu_list():
    probes = all_probes()
    assert set(AP.CAUGHT_BY) == set(AP.MUTANTS)
    caught = {mutant: [] for mutant in AP.MUTANTS}
    for probe in probes:
        fine = AP.run_mutant(*probe[:4], None, probe[4])
        for mutant in mutants_of(probe[0]):
            if AP.run_mutant(*probe[:4], mutant, probe[4]) != fine:
                caught[mutant].append(probe)
    for mutant in AP.MUTANTS:
        names = [f'{entry} {t}x{n}' + (f' {extra}' if extra else '') for entry, t, n, _, extra in caught[mutant]]
        print(f'{mutant}: caught by {len(names)} probes: {", ".join(names)}')
        assert caught[mutant], mutant
    for mutant, probe in AP.CAUGHT_BY.items():
        assert probe in probes and mutant in mutants_of(probe[0]), (mutant, probe)
        assert probe in caught[mutant], (mutant, probe)


def test_the_suite_had_no_input_on_which_a_tie_decides():
    """The gap on record: on the random PPGs and seeds of test_gpu_alignment.py::CASES (T <= 300), `>=` for `>` gives
    the reference's own starts, so no comparison of those tests could tell the two apart.  The exception has one
    cause: a random transcript now and then holds a phoneme twice in a row, two neighbouring states then see the same
    emissions and hold the same sum where one was entered from the other, and on a few cases such a tie lies on the
    optimal path.  Those tests compare boundaries by cost, never by identity, and the mutant's path costs exactly what
    the reference's does, so a kernel with that fault passes there as well; without a repeated phoneme the starts never
    move."""
    checked, moved = 0, []
    for frames, count in OLD_CASES:
        if frames > 300:
            continue
        generator = torch.Generator().manual_seed(1000 * frames + count)
        for scale in (1., 3., 8.):
            ppg = R.random_ppg(frames, scale, generator)
            phonemes = R.random_phonemes(count, generator)
            e = R.emissions(R.log_posteriors(ppg), phonemes)
            ref_total, ref_starts = R.programme(e)
            total, starts = AP.forced_programme(e, None, 'advance_on_tie')
            assert total == ref_total and R.path_total(e, starts) == R.path_total(e, ref_starts), (frames, count, scale)
            if starts.tolist() != ref_starts.tolist():
                assert any(a == b for a, b in zip(phonemes, phonemes[1:]))
                moved.append((frames, count, scale))
            checked += 1
    print(f'advance_on_tie on the old inputs: {checked} checked, starts moved (a phoneme twice in a row) on {moved}')
    assert checked >= 30 and len(moved) < checked // 4


# ---- conditions on the inputs ----

def test_the_forced_probes_meet_their_conditions():
    """Per probe of at least 31 frames (one or two frames cannot hold a dead frame, a cold one and a hot one at once):
    the optimum is neither free nor hopeless, a phoneme holds several frames, a frame is dead, a GOP term is not zero;
    and with 1 < N < T an exact tie lies on the optimal path, but for the probes named in NO_TIE_ON_THE_PATH."""
    table = AP.sums(AP.HOST_L, 1100)
    no_tie, eligible = [], 0
    for frames, count in AP.FORCED_SHAPES:
        ppg, phonemes = AP.forced_probe(frames, count)
        logp = AP.cold(ppg)
        e = logp[:, list(phonemes)]
        total, starts = R.programme(e)
        expected = AP.expect_forced(ppg, list(phonemes), None, table)
        assert expected['total'] == table[int(-total)] and expected['starts'].tolist() == starts.tolist()
        if frames >= 31:
            assert 0 < -total < frames, (frames, count)
            assert count == frames or (np.diff(starts) > 1).any()
            assert (logp.max(axis=1) == -1).any(), (frames, count)                       # a dead frame
            assert (expected['gop'] != 0).any() and (expected['gop'] <= 0).all(), (frames, count)
            assert (expected['score'] <= expected['gop']).all()
        if 1 < count < frames:
            eligible += 1
            if AP.forced_programme(e, None, 'advance_on_tie')[1].tolist() == starts.tolist():
                no_tie.append((frames, count))
    print(f'no tie on the optimal path: {no_tie} of {eligible} probes with 1 < N < T')
    assert tuple(no_tie) == AP.NO_TIE_ON_THE_PATH and 10 * len(no_tie) <= eligible


def test_the_optional_probes_leave_phonemes_out_and_keep_some():
    dropped = kept = 0
    cases = AP.optional_probes()
    assert any(flags_for(n, p).count(False) == t for t, n, p in cases) and any(n > t for t, n, _ in cases)
    for frames, count, pattern in cases:
        ppg, phonemes = AP.forced_probe(frames, count)
        flags = flags_for(count, pattern)
        _, starts = OR.programme(AP.cold(ppg)[:, list(phonemes)], flags)
        out = np.diff(starts) == 0
        dropped += bool(out.any())
        kept += bool((~out & np.asarray(flags)).any())
    print(f'optional probes: {len(cases)}, {dropped} leave a phoneme out, {kept} keep an optional one')
    assert dropped >= len(cases) // 2 and kept >= len(cases) // 2
