"""The frame-metrics probes of tests/metrics_probe.py, host side (no GPU): the families are what they claim to be, the
fp32 restatement of the kernel's arithmetic passes every criterion (and KAPPA_REF is its measurement), every mutant
is caught by a criterion on a family, and the fixture-based checks of test_metrics_host.py accept most of them."""
import math

import pytest
import torch

import metrics_probe as P
from test_metrics_host import case_inputs, check_against_fixture, restate

SWITCHES = (dict(mix=True, class_weights=True, loss_weights=False), dict(mix=False, class_weights=False, loss_weights=True))


@pytest.fixture(scope='module')
def g(golden):
    return golden('g13_metrics')


def switches_of(name):
    return [dict(s, class_weights=s['class_weights'] and name != 'ties') for s in SWITCHES]


def test_stride_takes_three_trips_and_merges_runs(g):
    logits, labels, lengths = P.family('stride', g)
    assert tuple(logits.shape) == (3, 40, 22000) and lengths.tolist() == [22000, 9001, 22000]
    total = labels.numel()
    tiles = -(-total // P.TILE)
    trips = [len(range(block, tiles, P.MAX_BLOCKS)) for block in range(P.MAX_BLOCKS)]
    assert tiles == 516 and trips[:4] == [3] * 4 and set(trips[4:]) == {2} and total - (tiles - 1) * P.TILE == 80
    flat = P.masked_labels(labels, lengths).flatten()
    padded = torch.cat([flat, torch.full((tiles * P.TILE - total,), -100)])
    wave_empty = (padded.view(-1, 64) == -100).all(dim=1)
    trip_of_wave = torch.arange(len(wave_empty)) // 2 // P.MAX_BLOCKS
    labelled_before = torch.cumsum(~wave_empty, 0) > 0
    for trip in (0, 1, 2):                       # a whole wave without a label in every trip, labelled waves around it
        inside = wave_empty & (trip_of_wave == trip) & labelled_before
        assert inside.any() and (~wave_empty[int(inside.nonzero()[0]):]).any(), trip
    # a workgroup whose one wave has labels and whose other has none
    assert (wave_empty.view(-1, 2).sum(dim=1) == 1).any()
    for item, first, count in P.STRIDE_SPANS:
        assert count >= 200 and first % 64 and (first + count) % 64 and (item * 22000 + first) % 64
        assert (labels[item, first:first + count] == -100).all()
    lengths_of_runs = torch.cat([P.runs(row) for row in P.masked_labels(labels, lengths)])
    print(f'stride: {len(lengths_of_runs)} runs, longest {int(lengths_of_runs.max())}, '
          f'median {float(lengths_of_runs.median())}, {int((flat != -100).sum())} labelled frames')
    assert int(lengths_of_runs.max()) >= 64 and float(lengths_of_runs.median()) > 8
    # single-frame holes inside a run: the frames on both sides share a label
    inner = (labels[:, 1:-1] == -100) & (labels[:, :-2] == labels[:, 2:]) & (labels[:, :-2] != -100)
    assert int(inner.sum()) > 100
    # the largest logit is not the label's on a fifth of the frames or more, and for a whole run of 30+ somewhere
    want = P.reference('stride', g, class_weights=True)
    kept = flat != -100
    top = logits.transpose(1, 2).flatten(0, 1).argmax(dim=1)
    off = (top != flat) & kept
    assert 0.2 < int(off.sum()) / int(kept.sum()) < 0.5
    longest, current = 0, 0
    for value in off[kept].tolist():
        current = current + 1 if value else 0
        longest = max(longest, current)
    assert longest >= 30
    assert want['count'] == int(kept.sum())


def test_every_argmax_is_decided_by_a_wide_margin(g):
    weights = P.tables(g)[1]
    for name in P.FAMILIES:
        if name == 'ties':
            continue
        logits, labels, lengths = P.family(name, g)
        counts = P.masked_labels(labels, lengths) != -100
        for w in (None, weights):
            gap = P.weighted_gap(logits, w)[counts]
            assert float(gap.min()) >= P.GAP, (name, float(gap.min()))


def test_ties_family_is_full_of_ties(g):
    logits, labels, lengths = P.family('ties', g)
    assert tuple(logits.shape) == (5, 40, 333) and lengths is None
    counts = labels != -100
    top = logits.max(dim=1).values
    tied_top = ((logits == top[:, None]).sum(dim=1) > 1) & counts
    own = logits.gather(1, labels.clamp(min=0)[:, None])[:, 0]
    own_tied = ((logits == own[:, None]).sum(dim=1) > 1) & counts
    own_tied_at_top = own_tied & (own == top)
    all_equal = (logits == top[:, None]).all(dim=1)
    n = int(counts.sum())
    print(f'ties: {n} frames, tied maximum {int(tied_top.sum()) / n:.3f}, label tied {int(own_tied.sum()) / n:.3f}, '
          f'label tied at the maximum {int(own_tied_at_top.sum()) / n:.3f}, all equal {int(all_equal.sum()) / n:.3f}')
    assert int(tied_top.sum()) / n > 0.3 and int(own_tied_at_top.sum()) / n > 0.2 and int(own_tied.sum()) / n > 0.6
    assert 0.07 < int((all_equal & counts).sum()) / n < 0.13
    assert {0, 39} <= set(labels[all_equal & counts].tolist())
    assert logits.unique().numel() < 30


def test_other_families_have_their_edges(g):
    logits, labels, lengths = P.family('single', g)
    assert tuple(logits.shape) == (4097, 40, 1) and lengths is None and 20 < int((labels == -100).sum()) < 80
    lengths = P.family('single_lengths', g)[2]
    assert set(lengths.tolist()) == {0, 1, 5} and torch.equal(P.family('single_lengths', g)[0], logits)
    logits, labels, lengths = P.family('edge_lengths', g)
    assert tuple(logits.shape) == (7, 40, 45) and lengths.tolist() == list(P.EDGE_LENGTHS)
    assert int(labels.min()) >= 0 and int(labels.max()) < 40
    padding = torch.arange(45)[None, :] >= lengths[:, None]
    assert (~torch.isfinite(logits.transpose(1, 2)[padding]) | (logits.transpose(1, 2)[padding] == 1e38)).all()
    assert torch.isfinite(logits.transpose(1, 2)[~padding]).all()
    logits, labels, lengths = P.family('extreme', g)
    assert tuple(logits.shape) == (1, 40, 197) and not torch.isnan(logits).any() and not (logits == math.inf).any()
    own = logits[0].gather(0, labels)[0]
    assert int((own == -math.inf).sum()) == 8
    top2 = logits[0].topk(2, dim=0).values
    confident = (torch.arange(197) % 3 != 2) & (torch.arange(197) < 189)
    assert float((top2[0] - top2[1])[confident].min()) >= 20
    correct = logits[0].argmax(dim=0) == labels[0]
    assert correct[confident][0::2].all() and not correct[confident][1::2].any()
    assert int((logits[0] == -math.inf).sum(dim=0)[(torch.arange(197) % 3 == 2) & (torch.arange(197) < 189)].min()) >= 2
    probs32 = torch.softmax(logits[0], dim=0)
    assert int((probs32 == 0).sum()) > 1000                                  # probabilities that underflow to 0


@pytest.mark.parametrize('name', P.FAMILIES)
def test_fp32_restatement_passes_every_criterion(g, name):
    for switches in switches_of(name):
        for k in (1, 3, 8):
            got = P.restate32(*P.family(name, g), k=k, **P.tables_for(g, **switches))
            failed, ratios = P.judge(got, P.reference(name, g, **switches), k, switches['class_weights'],
                                     name in P.SUMMED)
            assert not failed, (name, switches, k, failed)
        print(name, switches, 'worst error / bound:', {key: round(value, 4) for key, value in ratios.items()})


def measured_kappa(g, mix):
    loss, jsd = P.frame_by_frame(P.restate32, g, mix, loss_weights=not mix)
    return P.extreme_loss_ratio(loss, g, mix, not mix), P.extreme_jsd_kappa(jsd, g, mix, not mix)


def test_kappa_ref_is_a_measurement(g):
    for mix in (True, False):
        loss_ratio, kappa = measured_kappa(g, mix)
        rounded = max(math.ceil(kappa / 0.05 - 1e-9), 1) * 0.05
        print(f'extreme, mix {mix}: restate32 loss at {loss_ratio:.3f} of its bound, JSD needs kappa {kappa:.4f} '
              f'-> {rounded:.2f}; the kernel is held to {P.kappa_gpu(mix)}')
        assert loss_ratio <= 1
        assert P.KAPPA_REF[mix] == pytest.approx(rounded, abs=1e-9)


def catches(kind, g):
    """[(family, criterion)] that reject the mutant"""
    evaluate, found = P.mutant(kind), []
    for name in P.FAMILIES:
        switches = switches_of(name)[1 if kind == 'loss_unclamped' else 0]
        got = evaluate(*P.family(name, g), k=3, **P.tables_for(g, **switches))
        failed, _ = P.judge(got, P.reference(name, g, **switches), 3, switches['class_weights'], name in P.SUMMED)
        found += [(name, criterion) for criterion in failed]
    if kind == 'loss_unclamped':
        loss, _ = P.frame_by_frame(evaluate, g, False, True)
        if P.extreme_loss_ratio(loss, g, False, True) > 1:
            found.append(('extreme', 'loss per frame'))
    return found


@pytest.mark.parametrize('kind', P.MUTANTS)
def test_every_mutant_is_caught(g, kind):
    found = catches(kind, g)
    print(f'{kind}: caught by', ', '.join(f'{criterion} on {name}' for name, criterion in found) or 'nothing')
    assert found
    expected = {'argmax_tie_highest': 'ties', 'topk_tie_label_first': 'ties', 'trip_dropped': 'stride',
                'trip_twice': 'stride', 'run_tail_lost': 'stride', 'hole_breaks_row': 'stride',
                'batch_stride': 'single', 'length_inclusive': 'edge_lengths', 'loss_unclamped': 'extreme'}[kind]
    assert expected in {name for name, _ in found}


# What the fixture-based check makes of each mutant.  run_tail_lost and hole_breaks_row ARE rejected on cases A and B
# (their labels have runs of two now and then, and 1 % holes): the fixture guards the walk's bookkeeping at run length
# 1 .. 2, the probes guard it at long runs, across spans of holes and with empty waves.  Everything else passes g13.
G13_ACCEPTS = {kind: 'ABCD' for kind in P.MUTANTS}
G13_ACCEPTS.update(run_tail_lost='CD', hole_breaks_row='CD')


@pytest.mark.parametrize('kind', P.MUTANTS)
def test_fixture_checks_accept_the_mutants(g, kind):
    evaluate = P.mutant(kind)
    matrix, weights = P.tables(g)
    accepted = ''
    for case in 'ABCD':
        logits, labels, lengths = case_inputs(g, case)
        try:
            check_against_fixture(evaluate(logits, labels, lengths, mix=matrix, class_weights=weights), g, case)
            check_against_fixture(evaluate(logits, labels, lengths, class_weights=weights, loss_weights=weights), g,
                                  case, normalize=False, balanced=True)
            accepted += case
        except AssertionError:
            pass
    print(f'{kind}: the g13 checks accept it on cases {accepted or "-"}')
    assert accepted == G13_ACCEPTS[kind]


def test_reference_extensions_leave_the_fixture_results_alone(g):
    logits, labels, _ = case_inputs(g, 'A')
    want = restate(logits, labels, k=3)
    assert want['topk_by_k'][2] == want['topk_correct'] == int(g['A_topk_correct']) and want['invalid_labels'] == 0
    assert list(want['topk_by_k']) == sorted(want['topk_by_k']) and want['topk_by_k'][0] == want['true_positives']
    bad = labels.clone()
    at = (labels != -100).nonzero()[0]
    bad[at[0], at[1]] = 40
    assert restate(logits, bad)['invalid_labels'] == 1 and restate(logits, bad)['count'] == want['count'] - 1
