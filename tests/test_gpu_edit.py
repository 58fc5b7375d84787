"""ppg_edit_distance on the GPU, bit for bit against the fp32 emulation of tests/edit_reference.py: the total on
bits, the four counts, K and every operation.  Nothing here has a tolerance: the emulation does the same fp32 adds in
the same order.

The probes are sequences over 2 and 3 symbols under the unit costs, where nearly every cell is a tie, laid over the
edges of the programme's tiling (the 256-row blocks, the 4-row strips, the 64-column feed of lane 0, empty sides, the
limit of 4096), plus random fp32 costs; tests/test_edit_host.py has which mutant of the programme each named probe
catches.  Every probe runs alone, and again inside a ragged batch whose padding holds the token 9999 -- had the kernel
read padding, the pair would have come out NaN."""
import numpy as np
import pytest
import torch

import ppgs_amd
from ppgs_amd import alignment, engine as E, evaluate

import edit_reference as R

pytestmark = pytest.mark.gpu
PADDING = 9999


def device_costs(costs):
    return None if costs[0] is None else [torch.from_numpy(np.ascontiguousarray(c)).cuda() for c in costs]


def keywords(costs):
    return {} if costs[0] is None else dict(zip(('sub', 'delete', 'insert'), (torch.from_numpy(c) for c in costs)))


def alone(ref, hyp, costs, ops=True):
    out = alignment.edit_distance(torch.as_tensor(np.asarray(ref, dtype=np.int64)),
                                  torch.as_tensor(np.asarray(hyp, dtype=np.int64)), ops=ops, **keywords(costs))
    assert out.total.shape == () and out.total.dtype == torch.float32 and out.total.is_cuda
    counts = tuple(int(v) for v in (out.hits, out.substitutions, out.deletions, out.insertions))
    return out.total.cpu().numpy(), counts, out.ops.cpu().numpy() if ops else None


def padded(sequences, fill=PADDING):
    width = max(1, max(len(s) for s in sequences))
    table = np.full((len(sequences), width), fill, dtype=np.int32)
    for row, sequence in zip(table, sequences):
        row[:len(sequence)] = sequence
    return torch.from_numpy(table).cuda(), [len(s) for s in sequences]


def batch(cases, costs, want_ops=True, statistics=None):
    """The cases as one ragged call of the engine: a list of (total, counts, ops or None)."""
    ref, lengths_ref = padded([c['ref'] for c in cases])
    hyp, lengths_hyp = padded([c['hyp'] for c in cases])
    total, counts, ops, count = E.edit_pairs(ref, hyp, lengths_ref, lengths_hyp, device_costs(costs), want_ops,
                                             statistics)
    total, counts = total.cpu().numpy(), counts.cpu().numpy()
    if ops is None:
        return [(total[b], tuple(counts[b]), None) for b in range(len(cases))]
    ops, count = ops.cpu().numpy(), count.cpu().numpy()
    assert (count == counts.sum(axis=1)).all()
    return [(total[b], tuple(counts[b]), ops[b, :count[b]]) for b in range(len(cases))]


def explain(case, got):
    want = case['want']
    first = next((k for k, (a, b) in enumerate(zip(np.asarray(got[2]).tolist(), want[2].tolist())) if a != b), None)
    return (f"{case['name']}: total {got[0]!r} counts {got[1]} for {want[0]!r} {want[1]}; ops "
            f"{'-' if got[2] is None else len(got[2])} for {len(want[2])}, first difference at {first}")


@pytest.fixture(scope='module')
def cases():
    """Every probe with what the emulation says of it.  Computed once; never modified."""
    out = []
    for k, (rows, columns) in enumerate(R.gpu_shapes()):
        for swapped, (n, m) in enumerate(((rows, columns), (columns, rows))):
            if swapped and n == m:
                continue
            symbols = 2 + (k + swapped) % 2
            out.append(dict(name=f'ties{symbols}_{n}x{m}', ref=R.tokens(2 * k + swapped, n, symbols),
                            hyp=R.tokens(1000 + 2 * k + swapped, m, symbols), costs=R.UNIT))
    for name, (ref, hyp, costs) in R.PROBES.items():
        out.append(dict(name=name, ref=np.asarray(ref, dtype=np.int64), hyp=np.asarray(hyp, dtype=np.int64),
                        costs=costs))
        out.append(dict(name=name + '_swapped', ref=out[-1]['hyp'], hyp=out[-1]['ref'], costs=costs))
    out.append(dict(name='ties3_4096x4096', ref=R.tokens(77, 4096, 3), hyp=R.tokens(78, 4096, 3), costs=R.UNIT))
    for case in out:
        case['want'] = R.edit(case['ref'], case['hyp'], *case['costs'])
    return out


def test_every_probe_alone(cases):
    failures = []
    for case in cases:
        got = alone(case['ref'], case['hyp'], case['costs'])
        if not R.same(got, case['want']):
            failures.append(explain(case, got))
    assert not failures, '\n'.join(failures)


def groups_of(cases):
    """Ragged batches: the cases that share their costs, by size, so that a small pair also sits beside a large one."""
    out = {}
    for case in cases:
        longest = max(len(case['ref']), len(case['hyp']))
        out.setdefault((id(case['costs'][0]) if case['costs'][0] is not None else 0,
                        0 if longest <= 130 else 1 if longest <= 769 else 2), []).append(case)
    groups = list(out.values())
    for group in groups[1:]:
        group.extend(c for c in groups[0][:3] if c['costs'] is group[0]['costs'] or
                     (c['costs'][0] is None and group[0]['costs'][0] is None))
    return groups


def test_every_probe_in_a_ragged_batch_with_poisoned_padding(cases):
    failures = []
    for group in groups_of(cases):
        for case, got in zip(group, batch(group, group[0]['costs'])):
            if not R.same(got, case['want']):
                failures.append(explain(case, got))
    assert not failures, '\n'.join(failures)


def test_counts_without_a_table(cases):
    """A call without ops has no direction table and no trace-back: the same total and counts."""
    for group in groups_of(cases):
        for case, got in zip(group, batch(group, group[0]['costs'], want_ops=False)):
            want = case['want']
            assert got[2] is None
            assert np.asarray(got[0], np.float32).tobytes() == np.asarray(want[0], np.float32).tobytes() and \
                tuple(got[1]) == want[1], explain(case, (got[0], got[1], want[2]))
    small = cases[5]
    got = alone(small['ref'], small['hyp'], small['costs'], ops=False)
    assert got[2] is None and got[0] == small['want'][0] and got[1] == small['want'][1]


def test_the_anchor_cases():
    a, b = 0, 1
    assert alone([a, b], [b, a], R.UNIT)[1] == (0, 2, 0, 0)
    assert alone([a, b, a], [b, a, b], R.UNIT)[1] == (2, 0, 1, 1)
    assert alone([a, a], [a], R.UNIT)[2].tolist() == [[2, 0, -1], [0, 1, 0]]
    assert alone([a], [a, a], R.UNIT)[2].tolist() == [[3, -1, 0], [0, 0, 1]]
    ref, hyp, costs = R.PROBES['a_b_dear_sub']
    total, counts, ops = alone(ref, hyp, costs)
    assert total == 2 and counts == (0, 0, 1, 1) and ops.tolist() == [[3, -1, 0], [2, 0, -1]]
    total, counts, ops = alone([], [], R.UNIT)
    assert total == 0 and counts == (0, 0, 0, 0) and ops.shape == (0, 3)


def test_batch_equals_single_calls_and_every_kind_of_sequence(cases):
    few = [c for c in cases if c['costs'][0] is None and max(len(c['ref']), len(c['hyp'])) <= 270][:9]
    names = ppgs_amd.PHONEMES
    # names, indices, CPU tensors and device tensors, mixed in one batch
    as_kind = [lambda s: [names[v] for v in s], lambda s: [int(v) for v in s], lambda s: torch.as_tensor(s),
               lambda s: torch.as_tensor(s).cuda(), lambda s: torch.as_tensor(s, dtype=torch.int32).cuda()]
    references = [as_kind[k % 5](c['ref']) for k, c in enumerate(few)]
    hypotheses = [as_kind[(k + 2) % 5](c['hyp']) for k, c in enumerate(few)]
    out = alignment.edit_distance(references, hypotheses, ops=True)
    assert out.total.shape == (len(few),) and out.hits.dtype == torch.int32 and len(out.ops) == len(few)
    total = out.total.cpu().numpy()
    counts = torch.stack([out.hits, out.substitutions, out.deletions, out.insertions], 1).cpu().numpy()
    for k, case in enumerate(few):
        got = (total[k], tuple(counts[k]), out.ops[k].cpu().numpy())
        assert R.same(got, case['want']), explain(case, got)
        assert R.same(got, alone(case['ref'], case['hyp'], case['costs']))


def test_ignore_on_the_host_and_on_the_device():
    rng = np.random.default_rng(5)
    silent = ppgs_amd.PHONEME_TO_INDEX_MAPPING['<silent>']
    other = 3
    pairs = []
    for k in range(6):
        ref, hyp = rng.integers(0, 4, 20 + 7 * k), rng.integers(0, 4, 31 - 3 * k)
        ref[rng.random(len(ref)) < 0.3] = silent
        hyp[rng.random(len(hyp)) < 0.3] = silent
        pairs.append((ref, hyp))
    pairs.append((np.full(5, silent), np.asarray([1, silent])))           # a side that becomes empty
    for ignore, dropped in (('<silent>', {silent}), ([silent, other], {silent, other})):
        want = [R.edit([v for v in r if v not in dropped], [v for v in h if v not in dropped]) for r, h in pairs]
        for on_device in (False, True):
            move = (lambda s: torch.as_tensor(s).cuda()) if on_device else (lambda s: s.tolist())
            out = alignment.edit_distance([move(r) for r, _ in pairs], [move(h) for _, h in pairs], ignore=ignore,
                                          ops=True)
            for k in range(len(pairs)):
                got = (out.total[k].cpu().numpy(), (int(out.hits[k]), int(out.substitutions[k]),
                                                    int(out.deletions[k]), int(out.insertions[k])),
                       out.ops[k].cpu().numpy())
                assert R.same(got, want[k]), (ignore, on_device, k)


@pytest.fixture(scope='module')
def corpus():
    """Seven small pairs over five phonemes and the (41, 41) histogram of each one's operations."""
    rng = np.random.default_rng(9)
    pairs = [(rng.integers(0, 5, n), rng.integers(0, 5, m))
             for n, m in ((12, 9), (0, 4), (30, 33), (7, 0), (65, 70), (1, 1), (260, 90))]
    tables = [R.histogram(R.edit(r, h)[2], r, h) for r, h in pairs]
    return pairs, tables


def read(rate):
    words = rate.statistics.cpu().numpy()
    return words[:-2].reshape(41, 41), int(words[-2]), int(words[-1])


def test_statistics_are_the_histogram_of_the_operations(corpus):
    pairs, tables = corpus
    rate = evaluate.ErrorRate()
    rate.update([torch.as_tensor(r) for r, _ in pairs], [h.tolist() for _, h in pairs])
    table, count, invalid = read(rate)
    assert np.array_equal(table, sum(tables)) and count == len(pairs) and invalid == 0
    assert torch.equal(rate.confusion().cpu(), torch.from_numpy(sum(tables)))
    results = rate()
    total = sum(tables)
    hits = int(np.trace(total[:40, :40]))
    assert results['Hits'] == hits and results['Substitutions'] == int(total[:40, :40].sum()) - hits
    assert results['Deletions'] == int(total[:40, 40].sum()) and results['Insertions'] == int(total[40].sum())
    assert results['Reference phonemes'] == sum(len(r) for r, _ in pairs) and results['Pairs'] == len(pairs)
    assert results['PER'] == (results['Substitutions'] + results['Deletions'] + results['Insertions']) / \
        results['Reference phonemes']
    # a second update adds; reset() starts again
    rate.update([r.tolist() for r, _ in pairs], [torch.as_tensor(h).cuda() for _, h in pairs])
    table, count, _ = read(rate)
    assert np.array_equal(table, 2 * sum(tables)) and count == 2 * len(pairs)
    rate.reset()
    assert not rate.statistics.any()


def test_statistics_do_not_depend_on_order_or_grouping(corpus):
    pairs, tables = corpus
    whole = evaluate.ErrorRate()
    whole.update([r.tolist() for r, _ in pairs], [h.tolist() for _, h in pairs])
    order = [4, 0, 6, 2, 5, 1, 3]
    parts = evaluate.ErrorRate()
    for group in (order[:3], order[3:6], order[6:]):
        parts.update([pairs[k][0].tolist() for k in group], [pairs[k][1].tolist() for k in group])
    assert torch.equal(whole.statistics, parts.statistics)
    assert list(whole()) == list(parts())
    assert all(a == b or (a != a and b != b) for a, b in zip(whole().values(), parts().values()))
    assert np.array_equal(read(whole)[0], sum(tables))


def test_error_rate_with_costs_and_an_invalid_pair(corpus):
    pairs, _ = corpus
    costs = R.random_costs(3)
    rate = evaluate.ErrorRate(**keywords(costs))
    rate.update([r.tolist() for r, _ in pairs], [h.tolist() for _, h in pairs])
    want = sum(R.histogram(R.edit(r, h, *costs)[2], r, h) for r, h in pairs)
    assert np.array_equal(read(rate)[0], want)
    with pytest.raises(ValueError):
        rate.update([[0]], [[1], [2]])
    rate.update([torch.tensor([1, 2, 40]).cuda(), [1, 2]], [[1, 2], [1, 3]])       # a device sequence is checked there
    table, count, invalid = read(rate)
    assert invalid == 1 and count == len(pairs) + 1
    assert np.array_equal(table, want + R.histogram(R.edit([1, 2], [1, 3], *costs)[2], [1, 2], [1, 3]))
    with pytest.raises(ValueError, match='1 pairs'):
        rate()


def test_a_batch_split_under_the_workspace_cap_equals_the_whole(corpus, monkeypatch):
    """engine.edit_pairs runs a batch whose workspace would pass EDIT_WORKSPACE_BYTES as several library calls: the
    same bits as the one call, operations, K and statistics included, in groups of 3 + 3 + 1."""
    pairs, tables = corpus
    ref, lengths_ref = padded([r for r, _ in pairs])
    hyp, lengths_hyp = padded([h for _, h in pairs])
    lib = E.library()
    calls = []
    entry = lib.ppg_edit_distance

    def spy(*arguments):
        calls.append(arguments[5])
        return entry(*arguments)
    monkeypatch.setattr(lib, 'ppg_edit_distance', spy)
    for want_ops, with_statistics in ((False, False), (True, False), (True, True), (False, True)):
        outputs = []
        for split in (False, True):
            per_pair = lib.ppg_edit_workspace_bytes(1, ref.shape[1], hyp.shape[1], int(want_ops or with_statistics))
            monkeypatch.setattr(E, 'EDIT_WORKSPACE_BYTES', 3 * per_pair + 1 if split else 1 << 30)
            statistics = torch.zeros(E.EDIT_STATISTICS, dtype=torch.int64).cuda() if with_statistics else None
            del calls[:]
            outputs.append(E.edit_pairs(ref, hyp, lengths_ref, lengths_hyp, None, want_ops, statistics) + (statistics,))
            assert calls == ([3, 3, 1] if split else [7]), (want_ops, with_statistics, split, calls)
        whole, parts = outputs
        assert torch.equal(whole[0].view(torch.int32), parts[0].view(torch.int32)) and torch.equal(whole[1], parts[1])
        assert (whole[2] is None) == (not want_ops) == (parts[2] is None)
        if want_ops:
            assert torch.equal(whole[2], parts[2]) and torch.equal(whole[3], parts[3])
        if with_statistics:
            assert torch.equal(whole[4], parts[4])
            assert np.array_equal(parts[4][:-2].cpu().numpy().reshape(41, 41), sum(tables))
            assert torch.equal(parts[3], parts[1].sum(1).to(torch.int32))


def test_a_device_index_beyond_int32_is_invalid():
    """A device sequence is narrowed to int32 for the kernel; an index that would wrap into [0, 40) must not."""
    wrapped = torch.tensor([1, 2 ** 32 + 5, 2], dtype=torch.int64).cuda()
    out = alignment.edit_distance([wrapped, torch.tensor([1, 5, 2]).cuda()], [[1, 5, 2], [1, 5, 2]])
    assert torch.isnan(out.total[0]) and int(out.hits[0]) == 0 and float(out.total[1]) == 0 and int(out.hits[1]) == 3
    for value in (-(2 ** 32) + 3, 40, -1, 2 ** 40):
        out = alignment.edit_distance(torch.tensor([value], dtype=torch.int64).cuda(), [3], ignore=[7])
        assert torch.isnan(out.total), value
    rate = evaluate.ErrorRate()
    rate.update([wrapped], [[1, 5, 2]])
    assert read(rate)[1:] == (0, 1) and not read(rate)[0].any()


# ---- the raw C entry point ----------------------------------------------------------------------------------------

def raw(ref_table, ref_lengths, hyp_table, hyp_lengths, want_ops=True, statistics=None, buffer=None, **override):
    """One call of ppg_edit_distance on device tensors, `override` replacing arguments of the C call by name:
    (code, total, counts, ops, ops_length, workspace)."""
    lib = E.library()
    pairs, rows, columns = ref_table.shape[0], ref_table.shape[1], hyp_table.shape[1]
    ref_lengths = torch.tensor(ref_lengths, dtype=torch.int32).cuda()
    hyp_lengths = torch.tensor(hyp_lengths, dtype=torch.int32).cuda()
    if buffer is None:
        buffer = torch.zeros(lib.ppg_edit_workspace_bytes(pairs, rows, columns, int(want_ops)), dtype=torch.uint8).cuda()
    total = torch.full((pairs,), -5., dtype=torch.float32).cuda()
    counts = torch.full((pairs, 4), -7, dtype=torch.int32).cuda()
    ops = torch.full((pairs, rows + columns, 3), -7, dtype=torch.int32).cuda()
    ops_length = torch.full((pairs,), -7, dtype=torch.int32).cuda()
    arguments = dict(
        device=0, ref=ref_table.data_ptr(), rows=rows, hyp=hyp_table.data_ptr(), columns=columns, pairs=pairs,
        lengths_ref=ref_lengths.data_ptr(), lengths_hyp=hyp_lengths.data_ptr(), sub=None, dele=None, ins=None,
        total=total.data_ptr(), counts=counts.data_ptr(), ops=ops.data_ptr() if want_ops else None,
        ops_length=ops_length.data_ptr() if want_ops else None,
        statistics=statistics.data_ptr() if statistics is not None else None, workspace=buffer.data_ptr(),
        size=buffer.numel(), stream=torch.cuda.current_stream().cuda_stream)
    assert set(override) <= set(arguments)
    arguments.update(override)
    code = lib.ppg_edit_distance(*arguments.values())
    torch.cuda.synchronize()
    return code, total, counts, ops, ops_length, buffer


@pytest.fixture(scope='module')
def raw_pairs():
    sequences = [(R.tokens(40, 300, 2), R.tokens(41, 70, 2)), (R.tokens(42, 5, 3), R.tokens(43, 90, 3)),
                 (np.zeros(0, dtype=np.int64), R.tokens(44, 3, 2)), (R.tokens(45, 257, 3), R.tokens(46, 64, 3))]
    ref, lengths_ref = padded([r for r, _ in sequences])
    hyp, lengths_hyp = padded([h for _, h in sequences])
    return sequences, ref, lengths_ref, hyp, lengths_hyp, [R.edit(r, h) for r, h in sequences]


def test_raw_abi_poisoned_and_reused_workspace(raw_pairs):
    sequences, ref, lengths_ref, hyp, lengths_hyp, want = raw_pairs
    size = E.library().ppg_edit_workspace_bytes(len(sequences), ref.shape[1], hyp.shape[1], 1)
    poisoned = torch.full((size,), 0xFF, dtype=torch.uint8).cuda()
    first = raw(ref, lengths_ref, hyp, lengths_hyp, buffer=poisoned)
    again = raw(ref, lengths_ref, hyp, lengths_hyp, buffer=first[5])           # the workspace as the call left it
    clean = raw(ref, lengths_ref, hyp, lengths_hyp)
    for out in (first, again, clean):
        assert out[0] == 0
        for k in range(1, 5):
            assert torch.equal(out[k].view(torch.int32), first[k].view(torch.int32))
    code, total, counts, ops, ops_length, _ = first
    for b, expected in enumerate(want):
        count = int(ops_length[b])
        got = (total[b].cpu().numpy(), tuple(counts[b].tolist()), ops[b, :count].cpu().numpy())
        assert R.same(got, expected), b
        assert (ops[b, count:] == -7).all()                                       # rows >= K are left alone
    # lengths above the width count as the width; the table is then the whole padded row
    full = torch.from_numpy(np.stack([R.tokens(50, 70, 2), R.tokens(51, 70, 2)]).astype(np.int32)).cuda()
    out = raw(full, [70, 1000], full.flip(0).contiguous(), [99, 70])
    for b in range(2):
        expected = R.edit(full[b].cpu().numpy(), full[1 - b].cpu().numpy())
        got = (out[1][b].cpu().numpy(), tuple(out[2][b].tolist()), out[3][b, :int(out[4][b])].cpu().numpy())
        assert R.same(got, expected)


def test_raw_abi_refusals_touch_nothing(raw_pairs):
    sequences, ref, lengths_ref, hyp, lengths_hyp, _ = raw_pairs
    pairs, rows, columns = ref.shape[0], ref.shape[1], hyp.shape[1]
    size = E.library().ppg_edit_workspace_bytes(pairs, rows, columns, 1)
    statistics = torch.full((E.EDIT_STATISTICS,), 11, dtype=torch.int64).cuda()
    costs = torch.ones(40 * 40).cuda()
    refusals = [dict(ref=None), dict(hyp=None), dict(lengths_ref=None), dict(lengths_hyp=None), dict(total=None),
                dict(counts=None), dict(workspace=None), dict(pairs=0), dict(pairs=65536), dict(rows=4097),
                dict(columns=4097), dict(columns=-1), dict(size=size - 1), dict(ops_length=None), dict(ops=None),
                dict(sub=costs.data_ptr()), dict(sub=costs.data_ptr(), ins=costs.data_ptr())]
    for override in refusals:
        workspace = torch.full((size + 16,), 0x5A, dtype=torch.uint8).cuda()
        out = raw(ref, lengths_ref, hyp, lengths_hyp, statistics=statistics, buffer=workspace[:size], **override)
        assert out[0] == -1, override
        assert (out[1] == -5).all() and (out[2] == -7).all() and (out[3] == -7).all() and (out[4] == -7).all(), override
        assert (workspace == 0x5A).all() and (statistics == 11).all(), override
    workspace = torch.full((size + 16,), 0x5A, dtype=torch.uint8).cuda()
    out = raw(ref, lengths_ref, hyp, lengths_hyp, buffer=workspace[8:], size=size)            # unaligned
    assert out[0] == -1 and (workspace == 0x5A).all() and (out[1] == -5).all()
    out = raw(ref, lengths_ref, hyp, lengths_hyp, want_ops=False, statistics=statistics)       # statistics without ops
    assert out[0] == -1 and (statistics == 11).all() and (out[1] == -5).all()


def test_raw_abi_invalid_pairs_stand_alone(raw_pairs):
    sequences, ref, lengths_ref, hyp, lengths_hyp, want = raw_pairs
    statistics = torch.zeros((E.EDIT_STATISTICS,), dtype=torch.int64).cuda()
    spoiled = ref.clone()
    spoiled[1, 3] = 40                                        # inside pair 1's length of 5
    spoiled[2, 0] = -1                                        # pair 2 has no reference: this is padding
    lengths = list(lengths_hyp)
    lengths[3] = -1                                           # a negative length
    code, total, counts, ops, ops_length, _ = raw(spoiled, lengths_ref, hyp, lengths, statistics=statistics)
    assert code == 0
    for b in (1, 3):
        assert torch.isnan(total[b]) and (counts[b] == 0).all() and int(ops_length[b]) == 0 and (ops[b] == -7).all()
    histogram = np.zeros((41, 41), dtype=np.int64)
    for b in (0, 2):
        count = int(ops_length[b])
        got = (total[b].cpu().numpy(), tuple(counts[b].tolist()), ops[b, :count].cpu().numpy())
        assert R.same(got, want[b]), b
        histogram += R.histogram(want[b][2], *sequences[b])
    words = statistics.cpu().numpy()
    assert np.array_equal(words[:-2].reshape(41, 41), histogram) and words[-2] == 2 and words[-1] == 2


# ---- through the layers -------------------------------------------------------------------------------------------

def test_from_a_ppg_to_the_error_rate():
    hypothesis = [5, 9, 2, 17, 30, 11, 24, 8, 3, 36, 14, 21]
    frames = torch.full((40, 3 * len(hypothesis)), 0.1 / 39)
    for k, phoneme in enumerate(hypothesis):
        frames[phoneme, 3 * k:3 * k + 3] = 0.9
    decoded = alignment.decode(frames.cuda())
    assert decoded.phonemes.tolist() == hypothesis
    # the transcript: one phoneme said differently, one the speaker left out, one the speaker added
    reference = list(hypothesis)
    reference[2] = 33                                         # -> a substitution of 33 by 2
    reference.insert(6, 27)                                   # -> a deletion of 27
    del reference[10]                                         # hypothesis[9] = 36 -> an insertion
    rate = evaluate.ErrorRate()
    rate.update([reference], [decoded.phonemes])
    results = rate()
    count = len(reference)
    assert (results['Hits'], results['Substitutions'], results['Deletions'], results['Insertions']) == \
        (count - 2, 1, 1, 1)
    assert results['Reference phonemes'] == count == 12 and results['Pairs'] == 1 and results['PER'] == 3 / count
    names = ppgs_amd.PHONEMES
    assert results[f'PER/{names[33]}'] == 1.0 and results[f'PER/{names[27]}'] == 1.0
    assert results[f'PER/{names[5]}'] == 0.0 and results[f'Insertions/{names[36]}'] == 1
    table = rate.confusion().cpu()
    assert table[33, 2] == 1 and table[27, 40] == 1 and table[40, 36] == 1 and table.sum() == count + 1
    single = alignment.edit_distance(reference, decoded.phonemes, ops=True)
    assert float(single.total) == 3 and single.ops.shape == (count + 1, 3)
    assert single.ops[single.ops[:, 0] != 0].tolist() == [[1, 2, 2], [2, 6, -1], [3, -1, 9]]
