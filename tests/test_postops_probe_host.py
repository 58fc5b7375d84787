"""The post-op and resampler probes of tests/postops_probe.py, checked on the CPU: that their float64 references are the
reference project's functions (fixtures g9_postops, g10_resample), that their constants are measurements on the fp32
oracle, and that they see the catalogued faults -- the ones the first-generation tests accept included.

Distance.  KAPPA_REF[family, mix] is asserted against oracle.distance.  With the "+ 1" (an absolute ulp of each log) in the
allowance every combination needs 0 .. 0.28; without it `peaked` without the mix needs about 6.  Mutants of the float64
restatement, share of the 197 frames outside E_t(4 max(KAPPA_REF, 1)):
    clamp floor 1e-7       uniform 79 % / 100 % (mix / none), peaked 16 % / 100 %; soft 0 % / 4 % -- and the old criterion
                           (rtol 2e-5, atol 2e-6, all three reductions) accepts it on `soft` and on the fixture with the mix
    mix not transposed     soft, uniform 100 %, peaked 99 %, ties 92 %     (the old criterion rejects it too)
    exponent 1.0           soft, peaked, uniform, ties 100 %                (the old criterion rejects it too)
    frames >= 64 from t-64 68 % on five families: all 133 displaced frames; the fixture's 57 frames cannot show it
  `near` catches none of the matrix mutants: its bound is as wide as cancellation forces, it is there to show that a
  correct kernel is not failed by it.
Sparsify.  No free element at q = 0, 0.3, 0.5, 0.85, 1 on any family (`ties`: what lies near a cut is exactly equal to it,
and must be dropped).  q = 1 / 3 is an interior integer position (fp32(1 / 3) * 39 == 13.0 exactly, lo == hi: asserted);
q = 10 / 39 is not (fp32(10 / 39) * 39 = 10.00000095: lo 10, hi 11, w 9.5e-7, a cut one rounding above order statistic 10).
At both, the free elements of a frame share ONE value, that order statistic -- one element on soft / peaked, up to 8
equal ones on ties -- and free elements of equal value must share one fate.  The oracle's kept set obeys the rule
everywhere; the kernel's algorithm restated in numpy fp32 passes the whole criterion.  Mutants: `>=` and index-free tie ranks are accepted by all four
fixture calls of the old test and rejected here (q = 0, q = 1, a threshold equal to a value; ties at every q); the k
smallest and item 0's offset are rejected by both.
Resampler.  oracle.resample needs kappa 0.3 .. 4.2 and at most 0.23 of the bound; the four mutants are off by 1e3 .. 1e7
bounds or fail the shape.  The old criterion (2e-6 absolute against fixture g10) rejects them too, except where a mutant
is the identity: phases and blocks exchanged at 48000 -> 16000 (one phase), floor for ceil at 8000 -> 16000 (an exact
length) -- asserted per rate; the bank equals the exact-rational closed form bit for bit.
"""
import numpy as np
import pytest
import torch

import postops_probe as P
from oracle import ppg_oracle as O


@pytest.fixture(scope='module')
def g9(golden):
    return golden('g9_postops')


@pytest.fixture(scope='module')
def sim(g9):
    return torch.from_numpy(g9['similarity']), float(g9['exponent'])


def mix_of(sim, normalize):
    return P.mix_matrix(*sim) if normalize else None


def test_probe_families():
    for family in P.FAMILIES:
        x, y = P.pair(family)
        assert x.shape == y.shape == (P.NP, P.FULL) and x.dtype == y.dtype == torch.float32
        assert torch.allclose(x.sum(0), torch.ones(P.FULL), atol=1e-5) and torch.allclose(y.sum(0), torch.ones(P.FULL), atol=1e-5)
    x, y = P.pair('soft')
    assert 1e-10 < float(x.min()) and float(x.max()) < 0.999                  # the clamp is idle, as in the fixture
    x, y = P.pair('peaked')
    assert float((x < 1e-8).float().mean()) > 0.2 and float(x.max()) > 0.999   # both ends of the clamp are active
    x, y = P.pair('near')
    assert 0 < float((x - y).abs().max()) < 1e-2
    x, y = P.pair('onehot')
    assert set(x.unique().tolist()) == {0.0, 1.0} and bool((x[:, ::3] == y[:, ::3]).all()) and not torch.equal(x, y)
    x, y = P.pair('uniform')
    assert bool((x == np.float32(1 / 40)).all())
    for family in P.SPARSIFY_FAMILIES:
        assert P.batch(family).shape == (P.BATCH, P.NP, P.FULL)
    v = np.sort(P.batch('ties').numpy(), axis=1)
    assert ((v[:, 1:] == v[:, :-1]).sum(axis=1) >= 20).all()                 # 40 values out of 9: ties in every frame
    v = np.sort(P.batch('soft').numpy(), axis=1)
    assert (v[:, 1:] > v[:, :-1]).all()                                     # and none in soft
    assert P.FRAMES == (1, 63, 64, 65, 197)


def test_references_pinned_to_fixtures(golden, g9, sim):
    for normalize in (1, 0):
        # the reference project's own fp32 output lies inside the criterion, at the oracle's kappa (measured: 0.25)
        mix = mix_of(sim, normalize)
        fixture = g9[f'distance_{normalize}_none']
        needed = P.distance_kappa(fixture, g9['x'], g9['y'], mix)
        print(f'fixture distance_{normalize}_none needs kappa {needed:.3f}')
        assert not P.distance_violations(fixture, g9['x'], g9['y'], mix, 0.5).any()
        ref = P.distance64(g9['x'], g9['y'], mix)[0]
        assert np.allclose(ref.mean(), g9[f'distance_{normalize}_mean'], rtol=1e-5, atol=1e-6)
    batch = g9['batch']
    for method, threshold, key in FIXTURE_CALLS:
        v = batch[:1] if method == 'topk' else batch
        expected = g9[key].reshape(v.shape)
        assert np.allclose(P.sparsify_restated(v, method, threshold), expected, atol=P.OLD_SPARSIFY_ATOL)
        rule = P.topk_rule(v, threshold) if method == 'topk' else P.cut_rule(
            v, P.percentile_cut(v, threshold) if method == 'percentile' else np.float64(np.float32(threshold)))
        report = P.sparsify_report(v, expected, *rule, threshold_method=method != 'topk')
        assert report['dropped'] == 0 and report['kept'] == 0 and report['split'] == 0, (key, report)
        # the float64 renormalisation against the reference project's own values (softmax(log(v + 1e-8)), which rounds
        # differently from the kernel's product form): inside the same 42 * 2^-24, measured 0.45 / 0.32 of it at most
        print(f"{key}: the fixture is at {report['renorm']:.2f} (values) and {report['total']:.2f} (sums) of the bound")
        assert report['renorm'] <= 1.0 and report['total'] <= 1.0, (key, report['renorm'], report['total'])
    g10 = golden('g10_resample')
    for rate in (48000, 44100, 22050, 8000):
        ref = P.resample64(g10[f'audio_{rate}'][:, 0], rate, 16000)[0]
        assert ref.shape == g10[f'out_{rate}'][:, 0].shape
        assert np.abs(ref - g10[f'out_{rate}'][:, 0]).max() < 3e-8              # the bank's fp32 rounding on 0.1-scale audio


FIXTURE_CALLS = (('percentile', 0.85, 'sparsify_percentile'), ('percentile', 0.5, 'sparsify_percentile_50'),
                 ('constant', 0.1, 'sparsify_constant'), ('topk', 3, 'sparsify_topk3'))


# ---- distance ------------------------------------------------------------------------------------------------------

def test_kappa_ref_is_a_measurement(sim):
    assert set(P.KAPPA_REF) == {(family, mix) for family in P.FAMILIES for mix in (True, False)}
    measured = {}
    for (family, normalize), recorded in P.KAPPA_REF.items():
        x, y = P.pair(family)
        mix = mix_of(sim, normalize)
        ref = P.distance64(x, y, mix)[0]
        assert not P.distance_violations(ref, x, y, mix, 0.0).any()             # the exact result needs no allowance
        out = O.distance(x, y, sim[0] if normalize else None, sim[1], 'none').numpy()
        needed = P.distance_kappa(out, x, y, mix)
        print(f'{family} mix={normalize}: the fp32 oracle needs kappa {needed:.3f} (recorded {recorded})')
        assert needed <= recorded, (family, normalize, needed)
        measured[family, normalize] = needed
        assert not P.distance_violations(out, x, y, mix, recorded).any()
        assert P.kappa_gpu(family, normalize) == 4.0 * max(recorded, 1.0)
        for frames in P.FRAMES[:-1]:                                             # the shorter probes are subsets
            assert not P.distance_violations(out[:frames], x[:, :frames], y[:, :frames], mix, recorded).any()
    # one-sided per entry (another host's blocked sums and vectorised log may need less); that the table is a
    # measurement and not a generous guess: the largest entry is within a factor 3 of what is needed here
    assert max(measured.values()) > max(P.KAPPA_REF.values()) / 3


def test_bound_is_tight_on_ordinary_frames_and_wide_under_cancellation(sim):
    for normalize in (True, False):
        mix = mix_of(sim, normalize)
        for family, low, high in (('soft', 1e-6, 1e-4), ('uniform', 1e-6, 1e-4), ('near', 5e-4, 1e-2)):
            x, y = P.pair(family)
            ref, avg, unit = P.distance64(x, y, mix)
            bound = P.distance_bound(avg, unit, P.kappa_gpu(family, normalize))
            assert low < np.median(bound) < high, (family, normalize, np.median(bound))
    x, y = P.pair('near')
    assert np.median(P.distance64(x, y)[0]) < 1e-2                              # the distances themselves: cancellation


def share_outside(kind, family, sim, normalize):
    x, y = P.pair(family)
    out = P.distance_mutant(kind, x, y, sim[0], sim[1], normalize)
    return float(P.distance_violations(out, x, y, mix_of(sim, normalize), P.kappa_gpu(family, normalize)).mean())


@pytest.mark.parametrize('kind', P.DISTANCE_MUTANTS)
def test_distance_mutant_is_rejected(sim, kind):
    modes = (True,) if kind in ('mix_not_transposed', 'exponent_1') else (True, False)
    for normalize in modes:
        shares = {family: share_outside(kind, family, sim, normalize) for family in P.FAMILIES}
        print(kind, 'mix' if normalize else 'no mix', {f: round(s, 2) for f, s in shares.items()})
        assert max(shares.values()) >= 0.5, (kind, normalize, shares)
        assert shares['peaked'] >= 0.5 or shares['uniform'] >= 0.5
        if kind != 'floor_1e-7':
            assert shares['near'] <= 0.02                                      # too wide there, by design


@pytest.mark.parametrize('kind', ['mix_not_transposed', 'exponent_1'])
def test_matrix_mutants_fail_the_old_criterion_too(g9, sim, kind):
    """Not new catches: rtol 2e-5 / atol 2e-6 rejects them on the fixture and on `soft`, in every reduction."""
    out = P.distance_mutant(kind, g9['x'], g9['y'], sim[0], sim[1], True)
    assert not P.old_distance_accepts(out, g9['distance_1_none'])
    assert not P.old_distance_accepts(out.mean(), g9['distance_1_mean']) and not P.old_distance_accepts(out.sum(), g9['distance_1_sum'])
    x, y = P.pair('soft')
    out = P.distance_mutant(kind, x, y, sim[0], sim[1], True)
    oracle = O.distance(x, y, sim[0], sim[1], 'none').numpy()
    assert not P.old_distance_accepts(out, oracle)
    assert not P.old_distance_accepts(out.mean(), oracle.mean()) and not P.old_distance_accepts(out.sum(), oracle.sum())


def test_clamp_floor_mutant_passes_the_old_criterion(g9, sim):
    """What test_postops_match_reference_fixture asks, on the fixture itself and on the soft family."""
    for x, y, refs in ((g9['x'], g9['y'], {r: g9[f'distance_1_{r}'] for r in ('none', 'mean', 'sum')}), P.pair('soft') + (None,)):
        out = P.distance_mutant('floor_1e-7', x, y, sim[0], sim[1], True)
        if refs is None:
            oracle = O.distance(x, y, sim[0], sim[1], 'none').numpy()
            refs = {'none': oracle, 'mean': oracle.mean(), 'sum': oracle.sum()}
        assert P.old_distance_accepts(out, refs['none'])
        assert P.old_distance_accepts(out.mean(), refs['mean']) and P.old_distance_accepts(out.sum(), refs['sum'])
    assert share_outside('floor_1e-7', 'soft', sim, True) == 0.0                # fixture-like input cannot see it at all
    # the one-block fixture cannot see a block-offset fault either
    out = P.distance_mutant('block_offset', g9['x'], g9['y'], sim[0], sim[1], True)
    assert P.old_distance_accepts(out, g9['distance_1_none'])


# ---- sparsify ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('family', P.SPARSIFY_FAMILIES)
def test_sparsify_free_element_caps(family):
    v = P.batch(family).numpy()
    for method, threshold, must_keep, must_drop in P.sparsify_cases(family):
        assert not (must_keep & must_drop).any()
        free = P.free_per_frame(must_keep, must_drop)
        if method == 'topk':
            continue                                                           # equals of the k-th value: judged by count
        if method == 'percentile' and threshold in (P.INTEGER_POSITION, P.NEAR_INTEGER_POSITION):
            assert (P.free_values_per_frame(v, must_keep, must_drop) <= 1).all()
            if family in ('soft', 'peaked'):
                assert free.max() == 1
            continue
        assert free.sum() == 0, (family, method, threshold, int(free.sum()))
    # what the two special quantiles are, in the kernel's own arithmetic (one fp32 multiply)
    position = np.float32(P.INTEGER_POSITION) * np.float32(P.NP - 1)
    assert position == 13.0 and np.floor(position) == np.ceil(position)         # interior, lo == hi
    position = np.float32(P.NEAR_INTEGER_POSITION) * np.float32(P.NP - 1)
    assert np.floor(position) == 10.0 and np.ceil(position) == 11.0 and position - 10.0 < 1e-6
    if family == 'ties':                                                       # what sits at a cut there is equal to it
        cut = P.percentile_cut(v, 0.3)
        assert ((v == cut).sum(axis=1) >= 2).mean() > 0.3


@pytest.mark.parametrize('family', P.SPARSIFY_FAMILIES)
def test_oracle_and_restatement_meet_the_sparsify_criterion(family):
    batch = P.batch(family)
    v = batch.numpy()
    for method, threshold, must_keep, must_drop in P.sparsify_cases(family):
        oracle = O.sparsify(batch, method, P.fp32(threshold) if method != 'topk' else threshold).numpy()
        report = P.sparsify_report(v, oracle, must_keep, must_drop, threshold_method=method != 'topk')
        assert report['dropped'] == 0 and report['kept'] == 0 and report['split'] == 0, (family, method, threshold, report)
        restated = P.sparsify_report(v, P.sparsify_restated(v, method, threshold), must_keep, must_drop,
                                     threshold_method=method != 'topk')
        print(f"{family} {method} {threshold:.4g}: restated renorm {restated['renorm']:.2f} sum {restated['total']:.2f} of the bound")
        assert P.sparsify_passes(restated), (family, method, threshold, restated)
        if method == 'topk':
            assert P.topk_passes(v, report['mask'], threshold) and P.topk_passes(v, restated['mask'], threshold)
            if family in ('soft', 'peaked'):
                readable = v >= P.READABLE
                assert np.array_equal(report['mask'] & readable, restated['mask'] & readable)


def rejected_cases(mutant, family):
    v = P.batch(family).numpy()
    out = []
    for method, threshold, must_keep, must_drop in P.sparsify_cases(family):
        report = P.sparsify_report(v, P.sparsify_restated(v, method, threshold, mutant), must_keep, must_drop,
                                   threshold_method=method != 'topk')
        if not (P.sparsify_passes(report) and (method != 'topk' or P.topk_passes(v, report['mask'], threshold))):
            out.append((method, threshold))
    return out


def old_accepts_sparsify(mutant, g9):
    verdicts = []
    for method, threshold, key in FIXTURE_CALLS:
        v = g9['batch'][:1] if method == 'topk' else g9['batch']
        out = P.sparsify_restated(v, method, threshold, mutant)
        verdicts.append(bool(np.allclose(out, g9[key].reshape(out.shape), atol=P.OLD_SPARSIFY_ATOL)))
    return verdicts


def test_sparsify_mutants(g9):
    # `>=` for `>`: invisible without a value equal to the cut
    assert old_accepts_sparsify('greater_equal', g9) == [True] * 4
    rejected = rejected_cases('greater_equal', 'soft')
    assert ('percentile', 0.0) in rejected and ('percentile', 1.0) in rejected
    assert ('constant', P.constant_thresholds('soft')[1]) in rejected
    assert {q for m, q in rejected_cases('greater_equal', 'ties') if m == 'percentile'} == set(P.QUANTILES)
    # ties ranked without the index rule: invisible without ties
    assert old_accepts_sparsify('ties_without_index', g9) == [True] * 4
    assert rejected_cases('ties_without_index', 'soft') == []
    rejected = rejected_cases('ties_without_index', 'ties')
    assert {('percentile', 0.3), ('percentile', 0.5), ('percentile', 0.85), ('topk', 1), ('topk', 3), ('topk', 39)} <= set(rejected)
    # the k smallest: the fixture's top-3 sees it, and so does every k < 40 here
    assert old_accepts_sparsify('k_smallest', g9) == [True, True, True, False]
    for family in ('soft', 'onehot', 'ties'):
        assert {('topk', 1), ('topk', 3), ('topk', 39)} <= set(rejected_cases('k_smallest', family))
    # item 1 read at item 0's offset: the two-item fixture sees it, and so does every case here
    assert old_accepts_sparsify('item_offset', g9) == [False, False, False, True]
    cases = [(m, t) for m, t, _, _ in P.sparsify_cases('soft')]
    assert set(rejected_cases('item_offset', 'soft')) == set(cases) - {('percentile', 1.0)}    # (q = 1 drops everything)


# ---- resampler -----------------------------------------------------------------------------------------------------

ALL_CASES = P.RESAMPLE_CASES + P.RESAMPLE_DEGENERATE + P.RESAMPLE_CEIL


def test_resample_oracle_kappa():
    kappas = {}
    for rate, target, samples in ALL_CASES:
        x = P.signal(samples, rate)
        out = O.resample(x, rate, target).numpy()
        assert out.shape == (2, P.output_length(samples, rate, target))
        worst, kappas[rate, target, samples] = P.resample_report(out, x.numpy(), rate, target)
        print(f'{rate} -> {target}, {samples} samples: oracle kappa {kappas[rate, target, samples]:.2f}, {worst:.3f} of the bound')
        assert worst <= 1.0
    assert P.KAPPA_REF_RESAMPLE / 2 < max(kappas.values()) <= P.KAPPA_REF_RESAMPLE
    assert P.output_length(1, 44100, 16000) == 1 and P.output_length(5, 44100, 16000) == 2 and P.output_length(3, 48000, 16000) == 1
    assert [P.output_length(n, 44100, 16000) for n in (881, 882, 883)] == [320, 320, 321]
    assert [P.output_length(n, 16000, 44100) for n in (319, 320, 321)] == [880, 882, 885]
    assert P.rates(16000, 44100) == (160, 441)


def test_bank_equals_the_closed_form_taps():
    """An impulse at sample s makes every output one bank entry: the bank (phase and block split, clamped argument)
    against the filter at exact rational sample times."""
    for rate, target, samples in P.RESAMPLE_CASES:
        for position in (0, samples // 2, samples - 1):
            x = P.impulse(samples, position)
            ref = P.resample64(x.numpy(), rate, target)[0][0]
            tap = P.closed_form_tap(rate, target, position, np.arange(len(ref)))
            assert (np.abs(ref - tap.astype(np.float32)) <= P.ulp32(tap)).all()
            assert (ref != 0).sum() >= 6
            assert np.array_equal(O.resample(x, rate, target).numpy()[0], ref.astype(np.float32))


@pytest.mark.parametrize('mutant', P.RESAMPLE_MUTANTS)
def test_resample_mutant_is_rejected(mutant):
    rejected = 0
    for rate, target, samples in ALL_CASES:
        x = P.signal(samples, rate).numpy()
        worst, _ = P.resample_report(P.resample64(x, rate, target, mutant)[0], x, rate, target)
        rejected += worst > 1.0
        if mutant in ('first_off_by_one', 'unscaled'):
            assert worst > 100, (mutant, rate, target, samples, worst)
    rate, target, samples = P.RESAMPLE_CASES[4]                                  # 16000 -> 44100: now = 441, orig = 160
    x = P.signal(samples, rate).numpy()
    assert P.resample_report(P.resample64(x, rate, target, mutant)[0], x, rate, target)[0] > 100
    print(f'{mutant}: rejected in {rejected} of {len(ALL_CASES)} cases')
    assert rejected >= {'phase_block_exchanged': 10, 'floor_length': 12}.get(mutant, len(ALL_CASES))


@pytest.mark.parametrize('mutant', P.RESAMPLE_MUTANTS)
def test_resample_mutant_under_the_old_criterion(golden, mutant):
    """test_resample_matches_closed_form_fixture's 2e-6 absolute against fixture g10 (16001 Hz left out: its bank is
    about 1 GB).  It rejects the mutants as well -- none of them is a new catch -- except where one is the identity."""
    g10 = golden('g10_resample')
    accepted = set()
    for rate in (48000, 44100, 22050, 8000):
        out = P.resample64(g10[f'audio_{rate}'][:, 0], rate, 16000, mutant)[0]
        ref = g10[f'out_{rate}'][:, 0]
        assert np.abs(P.resample64(g10[f'audio_{rate}'][:, 0], rate, 16000)[0] - ref).max() < P.OLD_RESAMPLE_ATOL
        if out.shape == ref.shape and np.abs(out - ref).max() < P.OLD_RESAMPLE_ATOL:
            accepted.add(rate)
    assert accepted == {'phase_block_exchanged': {48000}, 'floor_length': {8000}}.get(mutant, set())
