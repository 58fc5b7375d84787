"""Shared by tests/test_frontend_probe_host.py and tests/test_gpu_frontend_probe.py: tonal and onset signals for the mel
frontend (ppg_frontend.hip), a float64 reference of it, and two criteria stated in terms of what the kernel computes
instead of an fp16 ulp count against an fp32 fixture.

Why.  Every other frontend test feeds 0.1-amplitude white noise: all 513 bins carry the same energy, so an FFT error
of 1e-6 of the peak sits three orders of magnitude below the fp16 rounding of every output, the two frames that share
one complex transform are equally loud, so what leaks from one into the other cannot be seen, and a filter's edge
weight (2.2e-5 at the smallest) multiplies a bin no louder than its neighbours.  A full-scale tone has one bin at 256
and the rest at the sqrt(1e-6) floor: the same errors then move a quiet bin, a silent partner frame or a mel value by
tens of fp16 ulps.  On such input the fp32 oracle itself (torch.fft.rfft, CPU) is up to 13 fp16 ulps from float64 and
97.6 .. 98.4 % bit-equal, so "<= 1 ulp, >= 99.5 % equal against the oracle" cannot be asked of the kernel there.

Spectrogram criterion (every value).  Z is the float64 DFT of the windowed frame.  Frames are paired (2 j, 2 j + 1) within
a row, as the kernel pairs them in one complex transform; P is the largest |Z| over both frames of the pair and all
bins (the last frame of an odd count stands alone), E = kappa 2^-24 P.  An fp16 value h at a bin with |Z| = z passes iff
    lo - ulp16(lo) <= h <= hi + ulp16(hi),   lo = fp16(sqrt(1e-6 + max(z - E, 0)^2)),   hi = fp16(sqrt(1e-6 + (z + E)^2)).
KAPPA_REF is the smallest kappa (rounded up to one decimal) at which the oracle's own fp32 arithmetic passes on all
probes; the kernel is held to KAPPA_GPU = 4 KAPPA_REF: two frames share one transform (twice the energy, one more
rounding in the split), three table-twiddled passes replace pocketfft's, the window multiply is fused.  A relative
error of 1e-6 of the peak is still far outside.

Mel criterion, decoupled from the FFT.  The expected log-mel is computed in float64 from the fp16 spectrogram THE
KERNEL RETURNED -- the data its filterbank consumed: ref = log(max(basis64 @ spec16, 1e-5)), basis64 the oracle's
float32 mel_basis() widened.  |mel - ref| <= max(1 fp16 ulp of ref, 4e-6) for every value and >= 99.5 % bit-equal to
fp16(ref).  4e-6: an fp32 accumulation of at most 64 positive terms has relative error <= 64 2^-24 = 3.8e-6, which the
log turns into an absolute error, and near log-mel = 0 an fp16 ulp is smaller than that.

The probes (:func:`probes`; rows of a probe have one length, a multiple of 4 samples except `scale`):
  sweep     513 rows x 1600 samples, row k = cos(2 pi k n / 1024 + 0.37 k): every bin, 0 and 512 included, hence
            every filter edge; frames 3 .. 6 are pure bin-centred tones, the outer ones carry the reflect kink.
  two_level 16 rows: 0.9 at bin k plus 9e-4 (-60 dB) at k + 5.5, k over 2 .. 500: Hann sidelobes, quiet beside loud.
  onsets    rows of 160 * 53 samples (three 16-frame groups + 5 frames; frame 52 has no partner): digital silence
            except a full-scale tone that starts or ends at ONSETS[row] -- a silent frame beside a loud one inside a
            pair, across a pair boundary (the control), across a group boundary, and the unpartnered frame loudest.
  scale     3 x (160 * 37 + 59) white noise at 1.0 (clipped), 1e-3 and 1e-5, and 0.5 DC + 1e-3 noise.
"""
import functools

import numpy as np
import torch

from oracle import ppg_oracle as O

FLOOR = 1e-6                 # under the square root (reference spectrogram.py:47)
MEL_CLAMP = 1e-5
MEL_ABS = 4e-6               # 64 * 2^-24, see above
MEL_EQUAL = 0.995

# measured by tests/test_frontend_probe_host.py::test_kappa_ref_is_a_measurement (the fp32 oracle, CPU torch, needs
# 0.86 on sweep, 1.19 on two_level, 0.86 on onsets, 0.49 on scale; it passes everywhere at 1.2 and fails at 0.6)
KAPPA_REF = 1.2
KAPPA_GPU = 4 * KAPPA_REF

# Mutants of the float64 reference, each at the largest size the EXISTING criterion still accepts: the 0.1 white noise
# of test_gpu_parity.py::test_frontend_odd_frames_vs_oracle, <= 1 fp16 ulp from and >= 99.5 % equal to the oracle --
# applied to the spectrogram as well as the mel, as test_frontend_matches_reference_fixture applies it (on the mel
# alone, which is what the white-noise test looks at, the sizes would be 2^-16 and 2^-19).  Measured by
# tests/test_frontend_probe_host.py::test_mutant_*: each is accepted at this size and rejected at the next larger one.
MUTANT_EDGE = (59, 220)          # (a) (filter, bin): the largest outermost non-zero weight, 3.5e-5, that may be set to 0
MUTANT_CROSSTALK = 2.0 ** -19    # (b) eps: eps Z[2 j + 1] added to Z[2 j]
MUTANT_NOISE = 2.0 ** -20        # (c) eps: a complex error of size eps P and seeded phase added to every bin

SIZE = (O.NUM_FFT - O.HOPSIZE) // 2


# ---- signals -----------------------------------------------------------------------------------------------------

ONSET_SAMPLES = O.HOPSIZE * 53
# (kind, sample, tone bin): 'on' = silence before `sample`, 'off' = silence from `sample` on; the tone peaks at its
# first ('on') or last ('off') sample.  Frame t reads samples [160 t - 432, 160 t + 592), so a silent frame's neighbour
# catches 160 samples of tone under the window's tail, where a low bin (the phase barely turns) is loudest: P = 11.
ONSETS = (
    ('on', 160 * 10 + 592, 1),           # frame 10 silent, 11 catches its last 160 samples: inside pair (10, 11)
    ('off', 160 * 21 - 432, 1),          # frame 21 silent, 20 catches its first 160: inside pair (20, 21)
    ('on', 160 * 11 + 592, 1),           # control: frame 11 silent, 12 catches 160: between pairs
    ('off', 160 * 22 - 432, 1),          # control: frame 22 silent, 21 catches 160: between pairs
    ('on', 160 * 15 + 592, 333),         # frame 15 silent, 16 catches 160: the boundary of groups 0 and 1
    ('off', 160 * 32 - 432, 498),        # frame 32 silent, 31 catches 160: the boundary of groups 1 and 2
    ('on', ONSET_SAMPLES - 80, 5),       # the last 80 samples: frame 52, which has no partner, is the loudest
)


def _sweep():
    n = np.arange(1600, dtype=np.float64)[None]
    k = np.arange(513, dtype=np.float64)[:, None]
    return np.cos(2 * np.pi * k * n / O.NUM_FFT + 0.37 * k)


def _two_level(seed=11):
    rng = np.random.default_rng(seed)
    n = np.arange(1600, dtype=np.float64)[None]
    k = np.round(np.linspace(2, 500, 16))[:, None]
    p1, p2 = rng.uniform(0, 2 * np.pi, (2, 16, 1))
    return 0.9 * np.cos(2 * np.pi * k * n / O.NUM_FFT + p1) + 9e-4 * np.cos(2 * np.pi * (k + 5.5) * n / O.NUM_FFT + p2)


def _onsets():
    n = np.arange(ONSET_SAMPLES, dtype=np.float64)
    rows = []
    for kind, sample, k in ONSETS:
        on = kind == 'on'
        tone = np.cos(2 * np.pi * k * (n - (sample if on else sample - 1)) / O.NUM_FFT)
        rows.append(np.where(n >= sample if on else n < sample, tone, 0.0))
    return np.stack(rows)


def _scale(seed=5):
    generator = torch.Generator().manual_seed(seed)
    noise = torch.randn(3, O.HOPSIZE * 37 + 59, generator=generator).double().numpy()
    rows = [np.clip(noise, -1.0, 1.0), 1e-3 * noise, 1e-5 * noise, 0.5 + 1e-3 * noise[:1]]
    return np.concatenate(rows)


@functools.lru_cache(maxsize=None)
def probes():
    """{name: (rows, samples) float32 tensor on the host}; computed once, never modified."""
    made = {'sweep': _sweep(), 'two_level': _two_level(), 'onsets': _onsets(), 'scale': _scale()}
    return {name: torch.from_numpy(rows.astype(np.float32)) for name, rows in made.items()}


PROBES = ('sweep', 'two_level', 'onsets', 'scale')


def white_noise():
    """The input of test_gpu_parity.py::test_frontend_odd_frames_vs_oracle, (3, samples)."""
    generator = torch.Generator().manual_seed(5)
    return (0.1 * torch.randn(3, 1, O.HOPSIZE * 37 + 59, generator=generator))[:, 0]


# ---- float64 reference -------------------------------------------------------------------------------------------

def spectrum64(audio):
    """oracle.spectrogram_fp32 restated in float64 up to the DFT: audio (B, N) -> Z (B, 513, T) complex128 numpy
    (reflect pad 432, frames of 1024 at hop 160, periodic Hann, one-sided DFT)."""
    audio = torch.as_tensor(audio).double()
    padded = torch.nn.functional.pad(audio[:, None], (SIZE, SIZE), mode='reflect')[:, 0]
    window = torch.hann_window(O.NUM_FFT, dtype=torch.float64)
    frames = padded.unfold(-1, O.NUM_FFT, O.HOPSIZE)
    return torch.fft.rfft(frames * window, dim=-1).transpose(1, 2).numpy()


def magnitude64(Z):
    return np.sqrt(Z.real ** 2 + Z.imag ** 2 + FLOOR)


@functools.lru_cache(maxsize=None)
def basis64():
    return O.mel_basis().astype(np.float64)


def mel64(spec, basis=None):
    """oracle.linear_to_mel restated in float64: spec (B, 513, T) of any float dtype -> (B, 80, T) float64."""
    basis = basis64() if basis is None else basis
    return np.log(np.maximum(np.matmul(basis, np.asarray(spec, dtype=np.float64)), MEL_CLAMP))


def render(Z, basis=None):
    """What a frontend that computed Z exactly would return: (spec16, mel16), rounded where the reference rounds."""
    spec16 = magnitude64(Z).astype(np.float16)
    return spec16, mel64(spec16, basis).astype(np.float16)


# ---- criteria ----------------------------------------------------------------------------------------------------

def ulp_diff(a, b):
    """fp16 values apart, the existing criterion's measure (test_gpu_parity.py)."""
    return np.abs(a.view(np.int16).astype(np.int32) - b.view(np.int16).astype(np.int32))


def old_criterion(a, b):
    d = ulp_diff(np.ascontiguousarray(a), np.ascontiguousarray(b))
    return bool(d.max() <= 1 and (d == 0).mean() >= 0.995)


def ulp16(x):
    """The spacing of fp16 at x (fp16 values), float64."""
    return np.spacing(np.abs(x).astype(np.float16)).astype(np.float64)


def pair_peak(Z):
    """(B, 1, T): the largest |Z| over all bins of frames 2 j and 2 j + 1."""
    peak = np.abs(Z).max(axis=1)                                       # (B, T)
    B, T = peak.shape
    padded = np.concatenate([peak, np.zeros((B, T % 2))], axis=1)
    pairs = padded.reshape(B, -1, 2).max(axis=2)
    return np.repeat(pairs, 2, axis=1)[:, None, :T]


def _accepts(h, z, E):
    lo = np.sqrt(FLOOR + np.maximum(z - E, 0.0) ** 2).astype(np.float16)
    hi = np.sqrt(FLOOR + (z + E) ** 2).astype(np.float16)
    return (lo.astype(np.float64) - ulp16(lo) <= h) & (h <= hi.astype(np.float64) + ulp16(hi))


def spec_violations(spec16, Z, kappa):
    """(B, 513, T) bool: the values outside the spectrogram criterion at `kappa`."""
    assert spec16.dtype == np.float16 and spec16.shape == Z.shape, (spec16.dtype, spec16.shape, Z.shape)
    h = spec16.astype(np.float64)
    return ~_accepts(h, np.abs(Z), kappa * 2.0 ** -24 * np.broadcast_to(pair_peak(Z), Z.shape)) | ~np.isfinite(h)


def smallest_kappa(spec16, Z, ceiling=1024.0):
    """The smallest kappa at which every value passes, to 1 %, rounded up (`ceiling` if none below it does)."""
    bad = spec_violations(spec16, Z, 0.0)
    if not bad.any():
        return 0.0
    h, z = spec16.astype(np.float64)[bad], np.abs(Z)[bad]
    unit = 2.0 ** -24 * np.broadcast_to(pair_peak(Z), Z.shape)[bad]
    if not _accepts(h, z, ceiling * unit).all():
        return ceiling
    lo, hi = 0.0, ceiling
    while hi - lo > 0.01 * hi:
        mid = 0.5 * (lo + hi)
        lo, hi = (lo, mid) if _accepts(h, z, mid * unit).all() else (mid, hi)
    return hi


def mel_report(mel16, spec16, basis=None):
    """-> (worst |mel - ref| / tolerance, share bit-equal to fp16(ref)); the criterion holds iff the first is <= 1 and
    the second >= MEL_EQUAL."""
    assert mel16.dtype == np.float16 and spec16.dtype == np.float16
    ref = mel64(spec16, basis)
    assert mel16.shape == ref.shape
    ref16 = ref.astype(np.float16)
    tolerance = np.maximum(ulp16(ref16), MEL_ABS)
    error = np.abs(mel16.astype(np.float64) - ref)
    error = np.where(np.isfinite(error), error, np.inf)
    return float((error / tolerance).max()), float((mel16 == ref16).mean())


def mel_passes(mel16, spec16, basis=None):
    worst, equal = mel_report(mel16, spec16, basis)
    return worst <= 1.0 and equal >= MEL_EQUAL


# ---- mutants of the float64 reference ------------------------------------------------------------------------------

def edge_candidates():
    """[(weight, filter, bin)]: every filter's two outermost non-zero weights, ascending."""
    basis = O.mel_basis()
    out = []
    for m in range(basis.shape[0]):
        bins = np.flatnonzero(basis[m])
        out += [(float(basis[m, bins[0]]), m, int(bins[0])), (float(basis[m, bins[-1]]), m, int(bins[-1]))]
    return sorted(set(out))


def edge_mutant(filter_index, bin_index):
    """(a) the basis with one filter's outermost non-zero weight set to 0: a band table one bin short."""
    basis = basis64().copy()
    bins = np.flatnonzero(basis[filter_index])
    assert bin_index in (bins[0], bins[-1])
    basis[filter_index, bin_index] = 0.0
    return basis


def crosstalk_mutant(Z, eps):
    """(b) eps Z[2 j + 1] leaks into Z[2 j]: an imperfect conjugate-symmetry split."""
    out = Z.copy()
    T = Z.shape[2]
    out[:, :, 0:T - 1:2] += eps * Z[:, :, 1:T:2]
    return out


def noise_mutant(Z, eps, seed=13):
    """(c) a complex error of size eps P and seeded phase in every bin: a sloppy twiddle table."""
    rng = np.random.default_rng(seed)
    phase = rng.uniform(0, 2 * np.pi, Z.shape)
    return Z + eps * pair_peak(Z) * np.exp(1j * phase)
