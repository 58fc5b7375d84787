"""ppgs_amd.distance / sparsify / edit.grid.sample / resample on the GPU against float64 at multi-block shapes and edges:
the probes and criteria of tests/postops_probe.py (why the fixture tests of test_gpu_parity.py cannot see a wrong clamp
floor, a block-offset fault, `>=` for `>` or tie ranks without the index rule, and that these can:
tests/test_postops_probe_host.py).

* distance: six PPG families x with / without the mix matrix x 1, 63, 64, 65, 197 frames (four blocks, a 5-frame tail),
  every frame inside E_t(4 max(KAPPA_REF, 1)); distance(x, x) exactly 0; the three reductions consistent; fp16 and
  transposed-storage inputs give the bits of their fp32 contiguous copies.
* sparsify: (3, 40, 197) of four families; q in {0, 10/39, 0.3, 1/3 (position exactly 13), 0.5, 0.85, 1}, constant thresholds 0.1 / a value present
  / 0, k in {1, 3, 39, 40}: the kept-set rule, equal free values sharing one fate, exactly k kept, the renormalisation of the mask the kernel produced
  within 42 * 2^-24; shorter inputs give the bits of the long one's first frames.
* grid sample: bit-equal to the oracle at 4120 rows (the second trip of the row loop), 257 and 300 grid values (a
  second block), one frame, and NaN exactly in the columns of a NaN / +inf / -inf grid value.
* resampler: noise and a 1 kHz tone through five rate pairs (16000 -> 44100 included), inputs of 1, 3 and 5 samples,
  lengths around a multiple of `orig`, inside (n + 2) 2^-24 sum |x| |h|; unit impulses within one fp32 ulp of the
  closed-form tap; the filter-bank cache alternated A, B, A.

The kernel's own kappa per family and the resampler's kappa: not yet recorded -- this file was written without a GPU at
hand; every case prints its kappa beside its bound and records it as a test property (`--junitxml` keeps them; DESIGN
4.10 is to take them from the first MI355X run).
"""
import numpy as np
import pytest
import torch

import postops_probe as P
import ppgs_amd
from oracle import ppg_oracle as O
from ppgs_amd.edit import grid

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def sim(golden):
    g = golden('g9_postops')
    return torch.from_numpy(g['similarity']), float(g['exponent'])


def bits(x):
    return x.detach().cpu().contiguous().numpy().view(np.int32)


def distance(x, y, sim, normalize, reduction='none'):
    return ppgs_amd.distance(x, y, reduction=reduction, normalize=normalize, exponent=sim[1], similarity=sim[0])


# ---- distance ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('family', P.FAMILIES)
def test_distance_probe(sim, family, record_property):
    x, y = P.pair(family)
    for normalize in (True, False):
        mix = P.mix_matrix(*sim) if normalize else None
        bound = P.kappa_gpu(family, normalize)
        for frames in P.FRAMES:
            xs, ys = x[:, :frames].contiguous(), y[:, :frames].contiguous()
            out = distance(xs.cuda(), ys.cuda(), sim, normalize)
            assert out.is_cuda and out.shape == (frames,) and out.dtype == torch.float32
            out = out.cpu().numpy()
            needed = P.distance_kappa(out, xs, ys, mix)
            print(f'{family} mix={normalize} frames={frames}: the kernel needs kappa {needed:.3f} (bound {bound}, oracle '
                  f'{P.KAPPA_REF[family, normalize]})')
            record_property(f"kappa_{'mix' if normalize else 'plain'}_{frames}", round(needed, 3))
            bad = P.distance_violations(out, xs, ys, mix, bound)
            if bad.any():
                t = int(np.argmax(bad))
                ref, avg, unit = P.distance64(xs, ys, mix)
                pytest.fail(f'{family} mix={normalize} frames={frames}: {bad.sum()} frames outside kappa {bound} (the kernel '
                            f'needs {needed:.2f}); the first is frame {t}: {out[t]!r} for {ref[t]:.9g}, allowance '
                            f'{P.distance_bound(avg, unit, bound)[t]:.3g}')


@pytest.mark.parametrize('normalize', [True, False])
def test_distance_identities(sim, normalize):
    for family in ('peaked', 'onehot', 'ties'):
        x = P.pair(family)[0].cuda()
        assert not distance(x, x, sim, normalize).any(), family                   # (a + a) * 0.5 == a: exactly 0
    x, y = (p.cuda() for p in P.pair('peaked'))
    frames = distance(x, y, sim, normalize).cpu().double()
    rounding = P.FULL * P.U                                                        # an fp32 sum of 197 positive terms
    total, mean = float(distance(x, y, sim, normalize, 'sum')), float(distance(x, y, sim, normalize, 'mean'))
    assert abs(total - float(frames.sum())) <= rounding * float(frames.sum())
    assert abs(mean - float(frames.mean())) <= rounding * float(frames.mean())
    assert torch.equal(distance(x, y, sim, normalize, None), distance(x, y, sim, normalize))
    # fp16 inputs and a transposed-storage view: the bits of their fp32 contiguous copies
    x16, y16 = x.half(), y.half()
    assert np.array_equal(bits(distance(x16, y16, sim, normalize)), bits(distance(x16.float(), y16.float(), sim, normalize)))
    xt, yt = x.T.contiguous().T, y.T.contiguous().T
    assert not xt.is_contiguous() and torch.equal(xt, x)
    assert np.array_equal(bits(distance(xt, yt, sim, normalize)), bits(distance(x, y, sim, normalize)))


# ---- sparsify ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('family', P.SPARSIFY_FAMILIES)
def test_sparsify_probe(family, record_property):
    batch = P.batch(family)
    v, device = batch.numpy(), batch.cuda()
    for method, threshold, must_keep, must_drop in P.sparsify_cases(family):
        out = ppgs_amd.sparsify(device, method, threshold)
        assert out.is_cuda and out.shape == batch.shape and out.dtype == torch.float32
        report = P.sparsify_report(v, out.cpu().numpy(), must_keep, must_drop, threshold_method=method != 'topk')
        print(f"{family} {method} {threshold:.6g}: {report['dropped']} wrongly dropped, {report['kept']} wrongly kept, "
              f"{report['split']} frames with equal free values of two fates, renormalisation {report['renorm']:.3f} and sum "
              f"{report['total']:.3f} of the bound")
        record_property(f'renorm_{method}_{threshold:.4g}', round(max(report['renorm'], report['total']), 3))
        assert P.sparsify_passes(report), (family, method, threshold,
                                           {k: report[k] for k in ('dropped', 'kept', 'split', 'renorm', 'total')})
        if method == 'topk':
            assert P.topk_passes(v, report['mask'], threshold), (family, threshold)
            if family in ('soft', 'peaked'):
                oracle = P.sparsify_report(v, O.sparsify(batch, 'topk', threshold).numpy(), must_keep, must_drop)
                readable = v >= P.READABLE
                assert np.array_equal(report['mask'] & readable, oracle['mask'] & readable)
        if (method, threshold) in (('percentile', 0.85), ('topk', 3)):
            for frames in P.FRAMES[:-1]:                                         # per-frame work: the same bits at any length
                short = ppgs_amd.sparsify(device[:, :, :frames].contiguous(), method, threshold)
                assert np.array_equal(bits(short), bits(out[:, :, :frames])), (family, method, frames)


# ---- grid sample ---------------------------------------------------------------------------------------------------

def test_grid_sample_rows_blocks_and_one_frame():
    gen = torch.Generator().manual_seed(21)
    ppg = torch.softmax(3 * torch.randn(103, 40, 7, generator=gen), dim=1)           # 4120 rows: the row loop's second trip
    index = torch.linspace(-2, 9, 300)
    out = grid.sample(ppg.cuda(), index)
    assert out.shape == (103, 40, 300) and np.array_equal(bits(out), bits(O.grid_sample(ppg, index)))
    ppg = torch.softmax(3 * torch.randn(2, 40, 33, generator=gen), dim=1)
    index = torch.rand(257, generator=gen) * 40 - 3                                   # a second block of one thread
    assert np.array_equal(bits(grid.sample(ppg.cuda(), index)), bits(O.grid_sample(ppg, index)))
    ppg = torch.softmax(3 * torch.randn(3, 40, 1, generator=gen), dim=1)
    index = torch.tensor([-1.0, -0.25, 0.0, 0.5, 1.0, 3.0])
    out = grid.sample(ppg.cuda(), index)
    assert out.shape == (3, 40, 6) and np.array_equal(bits(out), bits(O.grid_sample(ppg, index)))


def test_grid_sample_non_finite_grid_values():
    gen = torch.Generator().manual_seed(22)
    ppg = torch.softmax(3 * torch.randn(2, 40, 9, generator=gen), dim=1)
    index = torch.tensor([0.5, float('nan'), 2.25, float('inf'), 3.0, float('-inf'), 8.0, -0.5, float('nan'), 7.75])
    finite = torch.isfinite(index)
    out = grid.sample(ppg.cuda(), index).cpu()
    assert out.shape == (2, 40, 10)
    assert bool(torch.isnan(out[..., ~finite]).all())
    # (the oracle on the finite columns only: .long() of NaN is undefined)
    assert np.array_equal(bits(out[..., finite]), bits(O.grid_sample(ppg, index[finite])))


# ---- resampler -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('rate,target,samples', P.RESAMPLE_CASES + P.RESAMPLE_DEGENERATE + P.RESAMPLE_CEIL)
def test_resample_probe(rate, target, samples, record_property):
    x = P.signal(samples, rate)
    out = ppgs_amd.resample(x.cuda(), rate, target)
    assert out.is_cuda and out.shape == (2, P.output_length(samples, rate, target))
    worst, kappa = P.resample_report(out.cpu().numpy(), x.numpy(), rate, target)
    print(f'{rate} -> {target}, {samples} samples: the kernel is at {worst:.3f} of the bound, kappa {kappa:.2f} '
          f'(oracle at most {P.KAPPA_REF_RESAMPLE})')
    record_property('kappa', round(kappa, 3))
    record_property('share_of_bound', round(worst, 4))
    assert worst <= 1.0


def test_resample_impulses_are_the_closed_form_taps():
    for rate, target, samples in P.RESAMPLE_CASES:
        for position in (0, samples // 2, samples - 1):
            out = ppgs_amd.resample(P.impulse(samples, position).cuda(), rate, target).cpu().numpy()[0]
            tap = P.closed_form_tap(rate, target, position, np.arange(len(out)))
            assert len(out) == P.output_length(samples, rate, target)
            off = np.abs(out.astype(np.float64) - tap.astype(np.float32)) / P.ulp32(tap)
            assert off.max() <= 1.0, (rate, target, position, off.max())
            assert (out != 0).sum() >= 6


def test_resample_bank_cache_alternation():
    a, b = P.signal(2000, 44100).cuda(), P.signal(400, 16000).cuda()
    first = ppgs_amd.resample(a, 44100, 16000)
    other = ppgs_amd.resample(b, 16000, 44100)
    again = ppgs_amd.resample(a, 44100, 16000)
    # each right by itself (a cache that ignored its key would hand B the bank of A), then A unchanged by B
    assert P.resample_report(first.cpu().numpy(), a.cpu().numpy(), 44100, 16000)[0] <= 1.0
    assert P.resample_report(other.cpu().numpy(), b.cpu().numpy(), 16000, 44100)[0] <= 1.0
    assert np.array_equal(bits(again), bits(first))
    assert np.array_equal(bits(ppgs_amd.resample(b, 16000, 44100)), bits(other))
