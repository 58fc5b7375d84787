"""The mel frontend on the GPU against float64 on tonal and onset input: the probes and criteria of
tests/frontend_probe.py (why white noise cannot see an FFT error of 1e-6 of the peak, crosstalk between the two frames
of one complex transform or a band table one bin short -- and that the probes can: tests/test_frontend_probe_host.py).

* Each probe through E.frontend(spectrogram=True, mel=True): shapes, every spectrogram value inside the criterion at
  KAPPA_GPU = 4 KAPPA_REF, the mel inside the mel criterion against the float64 filterbank of the spectrogram the
  kernel returned.  The smallest kappa the kernel passes at is printed per probe (DESIGN 4.4 records it: what a
  rewrite of the FFT is compared with).
* onsets: the mel-only and the spectrogram-only launch return the bits of the combined one; every row through the
  incremental frontend in the pushes of test_gpu_audio_stream.py, flushed with and without samples, gives the
  whole-recording bits.
* every 32nd sweep row from a buffer 4 bytes past a 16-byte boundary (the narrow staging path): the aligned bits.

If a spectrogram value fails, the message names row, bin, frame (its parity = real or imaginary part of the shared
transform), the value, |Z| and the pair's peak; if a mel value fails, the filter and frame.
"""
import numpy as np
import pytest
import torch

import frontend_probe as F
from ppgs_amd import engine as E
from test_gpu_audio_stream import PIECES, stream_one

pytestmark = pytest.mark.gpu


class Lab:
    """Per probe, once: the float64 spectrum and the kernel's combined launch."""

    def __init__(self):
        self._z, self._out = {}, {}

    def z(self, name):
        if name not in self._z:
            self._z[name] = F.spectrum64(F.probes()[name])
            self._z[name].setflags(write=False)
        return self._z[name]

    def out(self, name):
        """(spec16, mel16) numpy of E.frontend(probe, spectrogram=True, mel=True)"""
        if name not in self._out:
            spec, mel = E.frontend(F.probes()[name].cuda(), spectrogram=True, mel=True)
            torch.cuda.synchronize()
            self._out[name] = (spec.cpu().numpy(), mel.cpu().numpy())
        return self._out[name]


@pytest.fixture(scope='module')
def lab():
    return Lab()


def bits(x):
    return x.detach().cpu().numpy().view(np.int16)


@pytest.mark.parametrize('name', F.PROBES)
def test_probe(lab, name):
    audio = F.probes()[name]
    rows, frames = audio.shape[0], audio.shape[1] // 160
    spec16, mel16 = lab.out(name)
    assert spec16.shape == (rows, 513, frames) and mel16.shape == (rows, 80, frames)
    assert spec16.dtype == mel16.dtype == np.float16
    Z = lab.z(name)
    needed = F.smallest_kappa(spec16, Z)
    worst, equal = F.mel_report(mel16, spec16)
    print(f'{name}: smallest passing kappa {needed:.2f} (KAPPA_GPU {F.KAPPA_GPU:.1f}); mel worst error {worst:.3f} of the '
          f'tolerance, {equal:.5f} equal')
    bad = F.spec_violations(spec16, Z, F.KAPPA_GPU)
    if bad.any():
        row, k, frame = np.argwhere(bad)[0]
        peak = F.pair_peak(Z)[row, 0, frame]
        pytest.fail(f'{name}: {bad.sum()} spectrogram values outside kappa {F.KAPPA_GPU} (the kernel needs {needed:.2f}); the '
                    f'first at row {row} bin {k} frame {frame}: {float(spec16[row, k, frame])!r}, |Z| = {abs(Z[row, k, frame]):.6g}, '
                    f'pair peak {peak:.6g}')
    if not (worst <= 1.0 and equal >= F.MEL_EQUAL):
        ref = F.mel64(spec16)
        excess = np.abs(mel16.astype(np.float64) - ref) / np.maximum(F.ulp16(ref.astype(np.float16)), F.MEL_ABS)
        row, m, frame = np.unravel_index(np.nanargmax(excess), excess.shape)
        pytest.fail(f'{name}: mel {worst:.2f} x the tolerance off at row {row} filter {m} frame {frame} '
                    f'({float(mel16[row, m, frame])!r} for {ref[row, m, frame]:.6f}), {equal:.5f} equal')


def test_single_output_launches_equal_the_combined_one(lab):
    audio = F.probes()['onsets'].cuda()
    spec16, mel16 = lab.out('onsets')
    spec, none = E.frontend(audio, spectrogram=True, mel=False)
    assert none is None and np.array_equal(bits(spec), spec16.view(np.int16))
    none, mel = E.frontend(audio, spectrogram=False, mel=True)
    assert none is None and np.array_equal(bits(mel), mel16.view(np.int16))


def test_unaligned_rows_equal_aligned_ones(lab):
    """Rows a multiple of 4 samples long stage 16 bytes per lane when the buffer is 16-byte aligned and 4 bytes per
    lane when it is not (test_gpu_parity.py::test_frontend_sample_staging_paths_vs_oracle): the same bits, which are
    those of the rows inside the whole sweep."""
    audio = F.probes()['sweep'][::32].contiguous().cuda()
    assert audio.shape == (17, 1600) and audio.data_ptr() % 16 == 0
    spec, mel = E.frontend(audio, spectrogram=True, mel=True)
    buf = torch.empty(audio.numel() + 1, device='cuda')
    view = buf[1:].view_as(audio)
    view.copy_(audio)
    assert view.data_ptr() % 16 == 4
    shifted_spec, shifted_mel = E.frontend(view, spectrogram=True, mel=True)
    assert np.array_equal(bits(shifted_spec), bits(spec)) and np.array_equal(bits(shifted_mel), bits(mel))
    spec16, mel16 = lab.out('sweep')
    assert np.array_equal(bits(spec), spec16[::32].view(np.int16)) and np.array_equal(bits(mel), mel16[::32].view(np.int16))


@pytest.mark.parametrize('flush_with_samples', [True, False])
def test_onsets_streamed_equal_the_whole_recording(lab, flush_with_samples):
    """Driven as test_gpu_audio_stream.py::test_streamed_mel_equals_batch_frontend_bit_for_bit drives it."""
    audio = F.probes()['onsets'].cuda()
    whole = lab.out('onsets')[1]
    pieces = PIECES if flush_with_samples else PIECES[::-1]
    for row in range(audio.shape[0]):
        mel = stream_one(audio[row], pieces, flush_with_samples)
        torch.cuda.synchronize()
        assert mel.shape == (80, audio.shape[1] // 160)
        assert np.array_equal(bits(mel), whole[row].view(np.int16)), F.ONSETS[row]
