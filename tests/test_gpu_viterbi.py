"""ppgs_amd.alignment.viterbi on the GPU: equal bit for bit to `recognize`, `forced` and `forced(optional=)` on the graphs
where they coincide, pronunciation variants against every combination, a word loop, the float64 reference of
tests/viterbi_reference.py on random graphs, batches with a graph per item, streams, poisoned workspaces, and what the
device refuses.

The bound on a total is the one test_gpu_recognize.py derives: a clamped input is exact and logf is within 1 ulp, so
every emission is within 2^-23 relative; the weights are fp32 numbers given to the reference as they are; a path's
weight is a sequential fp32 sum of 2T + 1 terms of one sign (T emissions, T - 1 stay or arc weights, initial and
final), each addition within 2^-24 relative; and the maximum over paths of values each within the bound is within the
bound: (2T + 2) * 2^-23 * |total|.  A run's score and gop are sums of `length` such emissions and one division: 4e-6 +
(length + 2) * 2^-23 * |value|, as there.  Paths are compared by cost and validity, never by identity, except where
every number is exact or the input's margin is orders of magnitude above the bound."""
import itertools
import math

import numpy as np
import pytest
import torch

from ppgs_amd import alignment, engine as E
from ppgs_amd.phonemes import PHONEMES

import alignment_reference as F
import viterbi_reference as V

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -23
INF = math.inf
FIELDS = ('phonemes', 'starts', 'total', 'score', 'gop')


def bits(tensor):
    return tensor.view(torch.int32) if tensor.dtype == torch.float32 else tensor


def same_bits(got, ref, label, fields=FIELDS):
    for name in fields:
        ours, theirs = getattr(got, name), getattr(ref, name)
        assert ours.dtype == theirs.dtype and ours.shape == theirs.shape, (label, name, ours.shape, theirs.shape)
        assert torch.equal(bits(ours), bits(theirs)), (label, name)


def random_tables(generator, holes=0.3):
    tables = []
    for shape in ((40, 40), (40,), (40,)):
        table = -5 * torch.rand(shape, generator=generator)
        table[torch.rand(shape, generator=generator) < holes] = -INF
        tables.append(table)
    return tables


# ---- 1. equal to recognize under model_graph ----

@pytest.mark.parametrize('frames', [1, 2, 31, 32, 33, 63, 64, 65, 127, 128, 129, 1025])
def test_equals_recognize_bit_for_bit_under_model_graph(frames):
    generator = torch.Generator().manual_seed(1000 + frames)
    paths = 0
    for scale in (1., 3., 8.):
        ppg = F.random_ppg(frames, scale, generator).cuda()
        A, initial, final = random_tables(generator)
        got = alignment.viterbi(ppg, alignment.model_graph(A, initial, final))
        ref = alignment.recognize(ppg, transitions=A, initial=initial, final=final)
        same_bits(got, ref, f'T={frames} scale={scale}')
        assert torch.equal(got.states, got.phonemes) and got.states.dtype == torch.int32 and got.states.is_cuda
        paths += int(got.states.shape[0] > 0)
    assert paths >= 1                                           # (30 % holes leave a way through nearly always)
    # the exact ties of test_gpu_recognize.py::test_exact_ties
    ppg = torch.full((40, frames), 1 / 40).cuda()
    for A in (torch.zeros(40, 40), -torch.eye(40)):
        got = alignment.viterbi(ppg, alignment.model_graph(A))
        same_bits(got, alignment.recognize(ppg, transitions=A), f'ties T={frames}')
    assert got.starts.tolist() == list(range(frames + 1))
    assert got.states.tolist() == [(frames - 1 - t) % 2 for t in range(frames)]


def test_equals_recognize_on_a_recording_at_the_frame_limit():
    frames = alignment.VITERBI_MAX_FRAMES
    generator = torch.Generator().manual_seed(7)
    labels = torch.randint(0, 40, (frames // 16,), generator=generator).repeat_interleave(16)
    logits = 2. * torch.randn(40, frames, generator=generator)
    logits[labels, torch.arange(frames)] += 4.
    ppg = torch.softmax(logits, dim=0).cuda()
    A, initial, final = random_tables(generator, holes=0.3)
    got = alignment.viterbi(ppg, alignment.model_graph(A, initial, final))
    ref = alignment.recognize(ppg, transitions=A, initial=initial, final=final)
    assert got.states.shape[0] > 1000 and math.isfinite(float(got.total))
    same_bits(got, ref, 'the frame limit')


# ---- 2. equal to forced under chain_graph ----

@pytest.mark.parametrize('count', [1, 2, 63, 64, 65, 255, 256, 257, 1023, 1024])
def test_equals_forced_bit_for_bit_under_chain_graph(count):
    generator = torch.Generator().manual_seed(2000 + count)
    for extra in (0, 1, 33, 70):
        frames = count + extra
        ppg = F.random_ppg(frames, (1., 3., 8., 3.)[extra % 4], generator).cuda()
        sequence = torch.randint(0, 40, (count,), generator=generator).tolist()
        for n in range(1, count, 3):                           # repeats, adjacent and apart
            sequence[n] = sequence[n - 1]
        got = alignment.viterbi(ppg, alignment.chain_graph(sequence))
        ref = alignment.forced(ppg, sequence)
        label = f'N={count} T={frames}'
        assert got.states.tolist() == list(range(count)), label
        same_bits(got, ref, label)


# ---- 3. equal to forced(optional=) under chain_graph(optional) ----

def optional_case(count, frames, generator):
    """(sequence, flags): no two adjacent flags, the mandatory phonemes fit, the last two phonemes differ."""
    while True:
        flags = [False] * count
        for n in range(count):
            if float(torch.rand((), generator=generator)) < 0.45 and not (n and flags[n - 1]):
                flags[n] = True
        if 1 <= flags.count(False) <= frames:
            break
    sequence = torch.randint(0, 40, (count,), generator=generator).tolist()
    for n in range(1, count - 1, 4):
        sequence[n] = sequence[n - 1]
    if sequence[-1] == sequence[-2]:
        sequence[-1] = (sequence[-1] + 1) % 40
    return sequence, flags


@pytest.mark.parametrize('count', [2, 65, 300])
def test_equals_forced_optional_bit_for_bit_on_the_visited_states(count):
    """The one documented exception is excluded by a condition on the input: on an exact tie of the two legal end
    states the graph ends in the lower one and `forced` in N - 1; that needs equal last phonemes, which are not drawn."""
    generator = torch.Generator().manual_seed(3000 + count)
    left_out = 0
    for frames in sorted({count - count // 4, count - 1, count, count + 40}):       # N > T among them
        for _ in range(3):
            sequence, flags = optional_case(count, frames, generator)
            assert sequence[-1] != sequence[-2]                 # the precondition
            ppg = F.random_ppg(frames, 3., generator).cuda()
            got = alignment.viterbi(ppg, alignment.chain_graph(sequence, flags))
            ref = alignment.forced(ppg, sequence, optional=flags)
            label = f'N={count} T={frames}'
            assert torch.equal(bits(got.total), bits(ref.total)), label
            visited = got.states.long()
            present = ref.starts[1:] > ref.starts[:-1]
            assert torch.equal(torch.nonzero(present).reshape(-1), visited), label   # left out = not visited
            assert all(flags[n] for n in torch.nonzero(~present).reshape(-1).tolist()), label
            assert torch.equal(got.starts[:-1], ref.starts[:-1][visited]) and int(got.starts[-1]) == frames, label
            assert torch.equal(got.phonemes, ref.phonemes[visited]), label
            assert torch.equal(bits(got.score), bits(ref.score[visited])), label
            assert torch.equal(bits(got.gop), bits(ref.gop[visited])), label
            left_out += int((~present).sum())
    assert left_out > 0


# ---- 4. variants ----

def random_words(generator, disjoint=False):
    """Three words of one to three variants of one to four phonemes (no silences inside)."""
    pool = torch.randperm(39, generator=generator).tolist()    # 0 .. 38: '<silent>' is 39
    assert PHONEMES[39] == '<silent>'
    words = []
    for _ in range(3):
        variants = []
        for _ in range(int(torch.randint(1, 4, (), generator=generator))):
            length = int(torch.randint(1, 5, (), generator=generator))
            if disjoint:
                variants.append([pool.pop() for _ in range(length)])
            else:
                variants.append(torch.randint(0, 39, (length,), generator=generator).tolist())
        words.append(variants)
    return words


def test_variants_total_is_the_largest_forced_total_over_all_combinations():
    generator = torch.Generator().manual_seed(4000)
    for case in range(8):
        words = random_words(generator)
        frames = int(torch.randint(6, 60, (), generator=generator))
        ppg = F.random_ppg(frames, (1., 3., 8.)[case % 3], generator).cuda()
        graph, word_of, variant_of = alignment.pronunciations(words)
        got = alignment.viterbi(ppg, graph)
        combinations = list(itertools.product(*words))
        transcripts = [alignment.transcript(list(combination)) for combination in combinations]
        ref = alignment.forced(ppg[None].expand(len(combinations), 40, frames), [t[0] for t in transcripts],
                               lengths=[frames] * len(combinations), optional=[t[1] for t in transcripts])
        best = int(ref.total.argmax())
        assert torch.equal(bits(got.total), bits(ref.total[best])), case     # fp32 addition is monotone
        # the path is a legal one: every word once, in order, one variant each
        visited = got.states.tolist()
        said = [(word_of[n], variant_of[n]) for n in visited if word_of[n] >= 0]
        assert [w for w, _ in said] == sorted(w for w, _ in said)
        assert {w for w, _ in said} == {0, 1, 2} and len(set(said)) == 3


def test_variants_name_the_combination_that_was_said():
    generator = torch.Generator().manual_seed(4100)
    for case in range(4):
        words = random_words(generator, disjoint=True)
        chosen = [int(torch.randint(0, len(word), (), generator=generator)) for word in words]
        labels, truth = [], []
        for index, (word, variant) in enumerate(zip(words, chosen)):
            if index != 1:                                      # a pause before the first and the last word, none between 0 and 1
                labels += [39] * 4
            for phoneme in word[variant]:
                length = int(torch.randint(3, 7, (), generator=generator))
                truth.append((index, len(labels)))
                labels += [phoneme] * length
        frames = len(labels)
        logits = torch.randn(40, frames, generator=generator)
        logits[torch.tensor(labels), torch.arange(frames)] += 12.
        graph, word_of, variant_of = alignment.pronunciations(words)
        got = alignment.viterbi(torch.softmax(logits, dim=0).cuda(), graph)
        visited = got.states.tolist()
        assert [variant_of[n] for n in visited if word_of[n] >= 0] == [
            chosen[w] for w, variant in enumerate(chosen) for _ in words[w][variant]], case
        assert got.phonemes.tolist() == [k for k, _ in itertools.groupby(labels)]
        # word times off the states: a word lasts from its first state's run to its last state's
        starts = got.starts.tolist()
        for word in range(3):
            runs = [r for r, n in enumerate(visited) if word_of[n] == word]
            assert starts[runs[0]] == [t for w, t in truth if w == word][0]
        assert torch.equal(alignment.frame_labels(got.starts, got.phonemes, frames).cpu().long(), torch.tensor(labels))
        assert len(alignment.segments(got)) == len(visited)


# ---- 5. the word loop ----

def arcs_of(graph):
    offsets, sources, weights = graph.offsets.tolist(), graph.sources.tolist(), graph.weights.tolist()
    return [(sources[j], n, weights[j]) for n in range(len(offsets) - 1) for j in range(offsets[n], offsets[n + 1])]


def test_word_loop_reads_the_words_and_a_state_of_degree_255_changes_nothing():
    generator = torch.Generator().manual_seed(5000)
    pool = torch.randperm(39, generator=generator).tolist()
    lexicon = [(f'word{w}', [[pool.pop() for _ in range(3)]]) for w in range(10)]     # disjoint phonemes: a clear margin
    string = torch.randint(0, 10, (12,), generator=generator).tolist()
    string[3] = string[2]                                       # a word twice in a row
    labels = [39] * 3
    for position, word in enumerate(string):
        for phoneme in lexicon[word][1][0]:
            labels += [phoneme] * int(torch.randint(3, 6, (), generator=generator))
        if position % 3 == 0:
            labels += [39] * 4                                  # a pause after some words only
    frames = len(labels)
    logits = torch.randn(40, frames, generator=generator)
    logits[torch.tensor(labels), torch.arange(frames)] += 12.
    ppg = torch.softmax(logits, dim=0).cuda()
    graph, word_of = alignment.word_loop(lexicon, penalty=1.5)
    got = alignment.viterbi(ppg, graph)
    degrees = (graph.offsets[1:] - graph.offsets[:-1]).tolist()
    firsts = {n for n, degree in enumerate(degrees) if degree == 11}
    assert len(firsts) == 10 and degrees[0] == 10
    assert [word_of[n] for n in got.states.tolist() if n in firsts] == string
    assert got.phonemes.tolist() == [k for k, _ in itertools.groupby(labels)]
    # the same graph with one state's arcs filled up to 255 by parallel arcs that never win: nothing changes
    crowded = 1 + 3 * string[5]
    assert crowded in firsts
    arcs = arcs_of(graph)
    at = max(j for j, arc in enumerate(arcs) if arc[1] == crowded) + 1
    arcs[at:at] = [(int(torch.randint(0, len(degrees), (), generator=generator)), crowded, -50. - k) for k in range(244)]
    wide = alignment.graph(graph.phonemes, arcs, stay=graph.stay, initial=graph.initial, final=graph.final)
    assert int(wide.offsets[crowded + 1] - wide.offsets[crowded]) == alignment.VITERBI_MAX_DEGREE
    again = alignment.viterbi(ppg, wide)
    assert torch.equal(again.states, got.states)
    same_bits(again, got, 'degree 255')
    # ... and with the winning arc moved to the last of the 255 places, it is still found
    arcs = arcs_of(wide)
    mine = [j for j, arc in enumerate(arcs) if arc[1] == crowded]
    block = [arcs[j] for j in mine]
    block = block[11:] + block[:11]
    for j, arc in zip(mine, block):
        arcs[j] = arc
    last = alignment.graph(graph.phonemes, arcs, stay=graph.stay, initial=graph.initial, final=graph.final)
    again = alignment.viterbi(ppg, last)
    assert torch.equal(again.states, got.states)
    same_bits(again, got, 'the 255th arc')


# ---- 6. random graphs against the float64 reference ----

def random_graph(count, generator, holes=0.2, wide=2):
    """Degrees 0 .. 6, and `wide` states of degree 255, 254 and then 200 .. 255."""
    def weights(size):
        values = -5 * torch.rand(size, generator=generator)
        values[torch.rand(size, generator=generator) < holes] = -INF
        return values.tolist()
    arcs = []
    wide = torch.randperm(count, generator=generator)[:wide].tolist()
    for target in range(count):
        degree = int(torch.randint(0, 7, (), generator=generator))
        if target == wide[0]:
            degree = 255
        elif len(wide) > 1 and target == wide[1]:
            degree = 254
        elif target in wide:
            degree = int(torch.randint(200, 256, (), generator=generator))
        sources = torch.randint(0, count, (degree,), generator=generator).tolist()
        arcs += [(source, target, weight) for source, weight in zip(sources, weights(degree))]
    initial = weights(count)
    initial[0] = -1.                                            # some state may begin, some may end
    final = weights(count)
    final[count - 1] = -1.
    return alignment.graph(torch.randint(0, 40, (count,), generator=generator).tolist(), arcs,
                           stay=weights(count), initial=initial, final=final)


def against_reference(graph, ppg, label):
    """One utterance on the device against the float64 reference: the relative error of the total, None without a path."""
    frames = ppg.shape[1]
    logp = F.log_posteriors(ppg)
    g = V.lists(graph)
    e = V.emissions(logp, g.sym)
    ref_total, _, _ = V.viterbi(e, g)
    got = alignment.viterbi(ppg.cuda(), graph)
    if ref_total == -INF:
        assert float(got.total) == -INF and got.states.shape == (0,) and got.starts.tolist() == [0], label
        return None
    total = float(got.total)
    bound = (2 * frames + 2) * EPS * abs(ref_total)
    error = abs(total - ref_total)
    print(f'viterbi {label}: total {total:.6f} reference {ref_total:.6f} relative error '
          f'{error / abs(ref_total):.3e} (bound {(2 * frames + 2) * EPS:.3e}), {got.states.shape[0]} runs')
    assert error <= bound, label
    states, starts = got.states.cpu().numpy().astype(np.int64), got.starts.cpu().numpy().astype(np.int64)
    assert got.phonemes.tolist() == g.sym[states].tolist(), label
    own = V.best_rescore(states, starts, e, g)                  # None: not a path of the graph
    print(f'viterbi {label}: the device\'s path weighs {own} in float64, the optimum {ref_total:.6f}')
    assert own is not None and own > -INF and own >= ref_total - 2 * bound, label
    lengths = np.diff(starts)
    own_frames = e[np.arange(frames), np.repeat(states, lengths)]
    ref_score = np.add.reduceat(own_frames, starts[:-1]) / lengths
    ref_gop = np.add.reduceat(own_frames - logp.max(axis=1), starts[:-1]) / lengths
    score, gop = got.score.cpu().numpy().astype(np.float64), got.gop.cpu().numpy().astype(np.float64)
    worst_score = (np.abs(score - ref_score) - (4e-6 + (lengths + 2) * EPS * np.abs(ref_score))).max()
    worst_gop = (np.abs(gop - ref_gop) - (4e-6 + (lengths + 2) * EPS * np.abs(ref_gop))).max()
    print(f'viterbi {label}: score error {np.abs(score - ref_score).max():.3e}, gop error '
          f'{np.abs(gop - ref_gop).max():.3e}; closest to their bounds {worst_score:.3e} {worst_gop:.3e} (<= 0 passes)')
    assert worst_score <= 0 and worst_gop <= 0 and (gop <= 0).all(), label
    return error / abs(ref_total)


@pytest.mark.parametrize('count', [3, 64, 65, 700])
def test_total_path_scores_and_gop_against_the_float64_reference(count):
    generator = torch.Generator().manual_seed(6000 + count)
    errors = []
    for frames in ((1, 2, 40, 97) if count < 700 else (1, 37)):
        graph = random_graph(count, generator)
        errors.append(against_reference(graph, F.random_ppg(frames, 3., generator), f'S={count} T={frames}'))
    errors = [error for error in errors if error is not None]
    assert len(errors) >= 2
    print(f'viterbi S={count}: largest relative error of total {max(errors):.3e}')


# ---- 6b. more arcs than the programme keeps in LDS: the arcs come from memory, in the programme and the trace-back ----

HELD = 4096                                                     # VHELD of ppg_align.hip


@pytest.mark.parametrize('count', [300, 700])
def test_arcs_from_memory_against_the_float64_reference(count):
    """One pass and a half (300 states) and three passes (700) with twenty-two states of degree 200 .. 255."""
    generator = torch.Generator().manual_seed(6500 + count)
    errors = []
    for frames in (1, 2, 33):
        graph = random_graph(count, generator, wide=22)
        assert int(graph.offsets[-1]) > HELD                    # the condition on the input
        errors.append(against_reference(graph, F.random_ppg(frames, 3., generator),
                                        f'S={count} T={frames} arcs={int(graph.offsets[-1])}'))
    errors = [error for error in errors if error is not None]
    assert len(errors) >= 2
    print(f'viterbi S={count}, arcs from memory: largest relative error of total {max(errors):.3e}')


def large_loop(generator, words=170):
    """(lexicon, graph, word_of): `words` words of two different phonemes each, no two alike: 29 410 arcs at 170."""
    pairs = [(a, b) for a in range(39) for b in range(39) if a != b]
    chosen = torch.randperm(len(pairs), generator=generator)[:words].tolist()
    lexicon = [(f'word{w}', [list(pairs[index])]) for w, index in enumerate(chosen)]
    graph, word_of = alignment.word_loop(lexicon, penalty=1.5)
    return lexicon, graph, word_of


def spoken(lexicon, string, generator, pause_every=3):
    """(ppg, labels) of a word string said clearly, with a pause before it and after every `pause_every`-th word."""
    labels = [39] * 3
    for position, word in enumerate(string):
        for phoneme in lexicon[word][1][0]:
            labels += [phoneme] * int(torch.randint(3, 6, (), generator=generator))
        if position % pause_every == 0:
            labels += [39] * 4
    frames = len(labels)
    logits = torch.randn(40, frames, generator=generator)
    logits[torch.tensor(labels), torch.arange(frames)] += 12.
    return torch.softmax(logits, dim=0), labels


def test_a_word_loop_whose_arcs_come_from_memory_reads_the_words():
    generator = torch.Generator().manual_seed(6600)
    lexicon, graph, word_of = large_loop(generator)
    assert int(graph.offsets[-1]) == 29410 > HELD and graph.phonemes.shape[0] == 341
    string = []
    while len(string) < 9:                                      # a word never begins with the phoneme the last one ended in
        word = int(torch.randint(0, 170, (), generator=generator))
        if not string or lexicon[word][1][0][0] != lexicon[string[-1]][1][0][1]:
            string.append(word)
    string[4] = string[3]                                       # a word twice in a row (its two phonemes differ)
    if lexicon[string[5]][1][0][0] == lexicon[string[4]][1][0][1]:
        string[5] = string[3]
    ppg, labels = spoken(lexicon, string, generator)
    got = alignment.viterbi(ppg.cuda(), graph)
    degrees = (graph.offsets[1:] - graph.offsets[:-1]).tolist()
    visited = got.states.tolist()
    assert [word_of[n] for n in visited if degrees[n] == 171] == string
    assert got.phonemes.tolist() == [k for k, _ in itertools.groupby(labels)]
    # the path is one of the graph, and its float64 weight is the device's total within the bound of a total
    g = V.lists(graph)
    e = V.emissions(F.log_posteriors(ppg), g.sym)
    own = V.best_rescore(np.asarray(visited), got.starts.cpu().numpy(), e, g)
    assert own is not None and abs(float(got.total) - own) <= (2 * len(labels) + 2) * EPS * abs(own)


def test_a_batch_whose_items_differ_in_where_their_arcs_come_from_equals_its_singles():
    generator = torch.Generator().manual_seed(6700)
    lexicon, loop, _ = large_loop(generator)
    heavy = random_graph(700, generator, holes=0.1, wide=22)
    chain = alignment.chain_graph([4, 4, 11, 30, 2])
    model = alignment.model_graph(*random_tables(generator, holes=0.2))
    small = random_graph(65, generator, holes=0.1)
    graphs = [chain, loop, model, heavy, small, loop, chain, heavy]
    assert [int(g.offsets[-1]) > HELD for g in graphs] == [False, True, False, True, False, True, False, True]
    said = spoken(lexicon, [3, 9, 3], generator)[0]             # item 1 says words of its loop; the others are noise
    lengths = [70, said.shape[1], 1, 33, 70, 7, 5, 70]
    assert said.shape[1] <= 70
    ppg = torch.full((8, 40, 70), float('nan'))
    for b, length in enumerate(lengths):
        ppg[b, :, :length] = said if b == 1 else F.random_ppg(length, (1., 3., 8.)[b % 3], generator)
    ppg = ppg.cuda()
    batch = alignment.viterbi(ppg, graphs, lengths)
    singles = [alignment.viterbi(ppg[b, :, :lengths[b]], graphs[b]) for b in range(8)]
    equal_paths(batch, singles)
    assert int(torch.isfinite(batch.total).sum()) >= 6 and batch.states[1].shape[0] >= 6
    # from a poisoned workspace, every graph packed on its own
    size = E.library().ppg_viterbi_workspace_bytes(8, 70, 700)
    for fill in (0, 255):
        rc, out = raw_viterbi(ppg, lengths, graphs, list(range(8)), torch.full((size,), fill, dtype=torch.uint8,
                                                                                device='cuda'), max_states=700)
        assert rc == 0 and torch.equal(bits(out['total']), bits(batch.total))
        for b in range(8):
            count = int(out['runs'][b])
            assert torch.equal(out['states'][b, :count], batch.states[b]), b
            assert count == 0 or torch.equal(out['starts'][b, :count + 1], batch.starts[b]), b
            assert torch.equal(bits(out['gop'][b, :count]), bits(batch.gop[b])), b


# ---- 7. batches ----

def raw_viterbi(ppg, lengths, graphs, which, workspace, want_gop=True, arrays=None, max_states=None):
    """ppg_viterbi through ctypes with the caller's workspace; outputs start as sentinels.  `arrays` replaces the
    packed graph arrays by hand-made ones.  (rc, {name: tensor})."""
    lib = E.library()
    count, width = ppg.shape[0], ppg.shape[2]
    out = {'states': torch.full((count, width), -7, dtype=torch.int32, device='cuda'),
           'phonemes': torch.full((count, width), -7, dtype=torch.int32, device='cuda'),
           'starts': torch.full((count, width + 1), -7, dtype=torch.int32, device='cuda'),
           'runs': torch.full((count,), -7, dtype=torch.int32, device='cuda'),
           'total': torch.full((count,), -7., device='cuda'),
           'score': torch.full((count, width), -7., device='cuda'),
           'gop': torch.full((count, width), -7., device='cuda')}
    packed = dict(arrays) if arrays is not None else pack(graphs)
    integer = ('state_begin', 'phonemes', 'arc_begin', 'sources')
    device = {name: torch.as_tensor(value).to(torch.int32 if name in integer else torch.float32).cuda()
              for name, value in packed.items()}
    n_graphs, n_states, n_arcs = len(packed['state_begin']) - 1, len(packed['phonemes']), len(packed['sources'])
    if max_states is None:
        max_states = min(1024, n_states)
    chosen = None if which is None else torch.tensor(which, dtype=torch.int32).cuda()
    given = torch.tensor(lengths, dtype=torch.int32).cuda()
    torch.cuda.synchronize()
    rc = lib.ppg_viterbi(
        0, ppg.data_ptr(), width, count, given.data_ptr(), n_graphs, n_states, n_arcs, max_states,
        device['state_begin'].data_ptr(), device['phonemes'].data_ptr(), device['stay'].data_ptr(),
        device['initial'].data_ptr(), device['final'].data_ptr(), device['arc_begin'].data_ptr(),
        device['sources'].data_ptr() if n_arcs else None, device['weights'].data_ptr() if n_arcs else None,
        None if chosen is None else chosen.data_ptr(), out['states'].data_ptr(), out['phonemes'].data_ptr(),
        out['starts'].data_ptr(), out['runs'].data_ptr(), out['total'].data_ptr(), out['score'].data_ptr(),
        out['gop'].data_ptr() if want_gop else None, workspace.data_ptr(), workspace.numel(),
        torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return rc, out


def pack(graphs):
    """The packed arrays of a list of Graphs, as host lists."""
    packed = {name: [] for name in ('phonemes', 'stay', 'initial', 'final', 'sources', 'weights')}
    state_begin, arc_begin = [0], []
    for graph in graphs:
        arc_begin += [len(packed['sources']) + offset for offset in graph.offsets.tolist()[:-1]]
        for name in packed:
            packed[name] += getattr(graph, name).tolist()
        state_begin.append(len(packed['phonemes']))
    return dict(packed, state_begin=state_begin, arc_begin=arc_begin + [len(packed['sources'])])


def ragged_batch():
    generator = torch.Generator().manual_seed(7000)
    lengths = torch.randint(1, 201, (33,), generator=generator).tolist()
    lengths[0], lengths[1], lengths[2] = 1, 200, 2
    ppg = torch.full((33, 40, 200), float('nan'))
    graphs = []
    for b in range(33):
        ppg[b, :, :lengths[b]] = F.random_ppg(lengths[b], (1., 3., 8.)[b % 3], generator)
        kind = b % 4
        if kind == 0:
            graphs.append(random_graph((3, 64, 65, 300)[(b // 4) % 4], generator, holes=0.1))
        elif kind == 1:
            graphs.append(alignment.model_graph(*random_tables(generator, holes=0.2)))
        elif kind == 2:
            graphs.append(alignment.chain_graph(torch.randint(0, 40, (min(lengths[b], 1 + 9 * b),),
                                                              generator=generator).tolist()))
        else:
            graphs.append(graphs[b - 3])                        # the same object again: it travels once
    return ppg.cuda(), lengths, graphs


def equal_paths(batch, singles, offset=0):
    for b, one in enumerate(singles):
        at = b - offset
        if not 0 <= at < len(batch.starts):
            continue
        assert torch.equal(batch.states[at], one.states), b
        for name in FIELDS:
            ours = getattr(batch, name)[at]
            assert torch.equal(bits(ours), bits(getattr(one, name))), (b, name)


def test_ragged_batch_with_a_graph_per_item_equals_singles_from_streams_split_and_poisoned(monkeypatch):
    ppg, lengths, graphs = ragged_batch()
    batch = alignment.viterbi(ppg, graphs, lengths)
    assert batch.total.shape == (33,) and not bool(torch.isnan(batch.total).any())
    assert int(torch.isfinite(batch.total).sum()) >= 25
    singles = [alignment.viterbi(ppg[b, :, :lengths[b]], graphs[b]) for b in range(33)]
    equal_paths(batch, singles)
    assert batch.starts[0].tolist()[-1] == 1 and int(batch.starts[1][-1]) in (0, 200)
    # a poisoned workspace gives the same bits, and the rest of the outputs is left alone
    size = E.library().ppg_viterbi_workspace_bytes(33, 200, 300)
    for fill in (0, 255):
        rc, out = raw_viterbi(ppg, lengths, graphs, list(range(33)), torch.full((size,), fill, dtype=torch.uint8,
                                                                                 device='cuda'), max_states=300)
        assert rc == 0 and torch.equal(bits(out['total']), bits(batch.total))
        for b in range(33):
            count = int(out['runs'][b])
            assert torch.equal(out['states'][b, :count], batch.states[b])
            assert torch.equal(out['phonemes'][b, :count], batch.phonemes[b])
            assert torch.equal(out['starts'][b, :count + 1], batch.starts[b]) or count == 0
            assert torch.equal(bits(out['score'][b, :count]), bits(batch.score[b]))
            assert torch.equal(bits(out['gop'][b, :count]), bits(batch.gop[b]))
            for name in ('states', 'phonemes', 'score', 'gop'):
                assert bool((out[name][b, count:] == -7).all()), (b, name)
            assert bool((out['starts'][b, (count + 1 if count else 0):] == -7).all()), b
    rc, out = raw_viterbi(ppg, lengths, graphs, list(range(33)), torch.zeros(size, dtype=torch.uint8, device='cuda'),
                          want_gop=False, max_states=300)
    assert rc == 0 and bool((out['gop'] == -7).all()) and torch.equal(bits(out['total']), bits(batch.total))
    # the two halves from two streams at once
    torch.cuda.synchronize()
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    halves = [(0, 16), (16, 33)]
    results = [[], []]
    for _ in range(3):
        for side, (low, high) in enumerate(halves):
            with torch.cuda.stream(streams[side]):
                results[side].append(alignment.viterbi(ppg[low:high], graphs[low:high], lengths[low:high]))
    torch.cuda.synchronize()
    for side, (low, _) in enumerate(halves):
        for result in results[side]:
            equal_paths(result, singles, offset=low)
    # a batch that viterbi_items has to split: room for five items per call, then for one
    monkeypatch.setattr(E, 'VITERBI_WORKSPACE_BYTES', E.library().ppg_viterbi_workspace_bytes(5, 200, 300))
    equal_paths(alignment.viterbi(ppg, graphs, lengths), singles)
    monkeypatch.setattr(E, 'VITERBI_WORKSPACE_BYTES', 1)
    equal_paths(alignment.viterbi(ppg[:4], graphs[:4], lengths[:4]), singles)
    # one graph for every item, and gop left out
    chain = alignment.chain_graph([5, 5, 9])
    fits = [b for b in range(33) if lengths[b] >= 3][:6]
    shared = alignment.viterbi(ppg[fits], chain, [lengths[b] for b in fits], gop=False)
    assert shared.gop is None
    for at, b in enumerate(fits):
        one = alignment.forced(ppg[b, :, :lengths[b]], [5, 5, 9])
        assert torch.equal(shared.starts[at], one.starts) and torch.equal(bits(shared.score[at]), bits(one.score))


# ---- 8. what the device refuses ----

def test_refused_graphs_and_items_give_nan_and_leave_their_neighbours_alone():
    generator = torch.Generator().manual_seed(8000)
    ppg = torch.stack([F.random_ppg(50, 3., generator) for _ in range(3)]).cuda().contiguous()
    lengths = [50, 41, 50]
    good = alignment.chain_graph([3, 3, 17, 4])
    other = random_graph(5, generator, holes=0.)
    fine = pack([good, other, good])
    single = alignment.viterbi(ppg[1, :, :41], good)
    size = E.library().ppg_viterbi_workspace_bytes(3, 50, 1024)
    workspace = torch.full((size,), 255, dtype=torch.uint8, device='cuda')

    def broken(**changes):
        arrays = {name: list(value) for name, value in fine.items()}
        for name, (index, value) in changes.items():
            if index is None:
                arrays[name] = value
            else:
                arrays[name][index] = value
        return arrays
    arcs_other = fine['arc_begin'][4]                           # the first arc of graph 1
    wide_begin = list(fine['arc_begin'])
    cases = {
        'a source out of range': broken(sources=(arcs_other, 5)),
        'a negative source': broken(sources=(arcs_other, -1)),
        'a NaN weight': broken(weights=(arcs_other, math.nan)),
        'a +inf weight': broken(weights=(arcs_other, INF)),
        'a NaN stay': broken(stay=(5, math.nan)),
        'a +inf final': broken(final=(6, INF)),
        'a phoneme out of range': broken(phonemes=(4, 40)),
        'a decreasing arc_begin': broken(arc_begin=(6, fine['arc_begin'][5] - 1)),
        'an arc_begin past the arcs': broken(arc_begin=(8, len(fine['sources']) + 7)),
        'a state_begin past the states': broken(state_begin=(2, len(fine['phonemes']) + 1)),
    }
    # a degree of 256: `good` and beside it one state with 256 arcs from itself
    loops = {'state_begin': [0, 4, 5], 'phonemes': fine['phonemes'][:4] + [7], 'stay': fine['stay'][:4] + [0.],
             'initial': fine['initial'][:4] + [0.], 'final': fine['final'][:4] + [0.],
             'arc_begin': fine['arc_begin'][:4] + [3, 3 + 256], 'sources': fine['sources'][:3] + [0] * 256,
             'weights': fine['weights'][:3] + [0.] * 256}
    cases['a degree of 256'] = {name: list(value) for name, value in loops.items()}
    for label, arrays in cases.items():
        rc, out = raw_viterbi(ppg, lengths, None, [0, 0, 1], workspace, arrays=arrays)
        assert rc == 0, label
        assert math.isnan(float(out['total'][2])) and int(out['runs'][2]) == 0, label
        for name in ('states', 'phonemes', 'starts', 'score', 'gop'):
            assert bool((out[name][2] == -7).all()), (label, name)             # the poison stays
        count = int(out['runs'][1])                             # the item beside it is untouched by the refusal
        assert torch.equal(out['states'][1, :count], single.states), label
        assert torch.equal(out['starts'][1, :count + 1], single.starts), label
        assert torch.equal(bits(out['total'][1]), bits(single.total)), label
        assert torch.equal(bits(out['gop'][1, :count]), bits(single.gop)), label
        assert not math.isnan(float(out['total'][0])), label
    loops['arc_begin'][-1], loops['sources'], loops['weights'] = 3 + 255, loops['sources'][:-1], loops['weights'][:-1]
    rc, out = raw_viterbi(ppg, lengths, None, [0, 0, 1], workspace, arrays=loops)
    assert rc == 0 and not any(math.isnan(v) for v in out['total'].tolist())              # a degree of 255 is fine
    assert torch.equal(bits(out['total'][1]), bits(single.total))
    # a graph larger than max_states says
    tiny = alignment.chain_graph([3])
    rc, out = raw_viterbi(ppg, lengths, [good, other, tiny, tiny], [0, 1, 2], workspace, max_states=4)
    assert rc == 0 and [math.isnan(v) for v in out['total'].tolist()] == [False, True, False]
    # `which` out of range and an impossible length, through engine.viterbi_items: zeros stay zeros
    for which, given in (([0, 3, 1], lengths), ([0, -1, 1], lengths), ([0, 1, 1], [50, 0, 50]), ([0, 1, 1], [50, 51, 50])):
        states, phonemes, starts, runs, total, score, gop = E.viterbi_items(
            ppg, given, fine['state_begin'], fine['phonemes'], fine['stay'], fine['initial'], fine['final'],
            fine['arc_begin'], fine['sources'], fine['weights'], which=which)
        assert math.isnan(float(total[1])) and int(runs[1]) == 0
        assert not any(bool(tensor[1].any()) for tensor in (states, phonemes, starts, score, gop))
        assert torch.equal(bits(total[0]), bits(alignment.viterbi(ppg[0], good).total)) and int(runs[0]) == 4
        assert not math.isnan(float(total[2]))
    # a graph with no way through gives -inf, not NaN
    dead = alignment.graph([1, 2], [(0, 1, 0.)], initial=[0., -INF], final=[-INF, -INF])
    got = alignment.viterbi(ppg[0], dead)
    assert float(got.total) == -INF and got.states.shape == (0,) and got.starts.tolist() == [0]
    assert alignment.segments(got) == []
    walled = alignment.graph([1, 2], [(0, 1, -INF)], stay=[0., 0.], initial=[0., -INF], final=[-INF, 0.])
    assert float(alignment.viterbi(ppg[0], walled).total) == -INF
