"""Shared by tests/test_postops_probe_host.py and tests/test_gpu_postops_probe.py: seeded posteriorgrams and signals for
the post-ops (ppg_postops.hip: distance, sparsify) and the resampler (ppg_resample.hip), float64 references of them,
and criteria that a correct fp32 kernel cannot fail.  No GPU and no file outside tests/ is touched here.

Why.  test_gpu_parity.py feeds softmax(3 randn) at 57 / 33 frames: one block of either kernel, a clamp that is never
active (a floor of 1e-7 instead of 1e-8 passes rtol 2e-5 / atol 2e-6 there), no ties, no integer quantile position; and
resamples white noise to 16 kHz only, judged by 2e-6 absolute.

Distance criterion (every frame).  Clamp in fp32 as the reference project does, then float64: a = M x, b = M y (or x, y),
m = (a + b) / 2, avg_p = (a_p (ln a_p - ln m_p) + b_p (ln b_p - ln m_p)) / 2, ref_t = sum_p sqrt(max(avg_p, 0)).  An fp32
evaluation cannot know avg_p better than
    d_p = kappa 2^-24 (a_p (|ln a_p| + |ln m_p| + 1) + b_p (|ln b_p| + |ln m_p| + 1)) / 2
(each log is known to a relative ulp of its value AND to an absolute ulp, the relative rounding of its argument: the
"+ 1"; without it a frame whose m is near 1 -- ln m near 0 -- has no allowance for the rounding of (a + b) / 2, and the
peaked family without the mix matrix needs kappa 6 where every other needs < 0.5), so a frame passes iff
    |out_t - ref_t| <= E_t(kappa) = sum_p [ sqrt(max(avg_p, 0) + d_p) - sqrt(max(avg_p - d_p, 0)) ].
KAPPA_REF[family, mix] is the smallest kappa at which the fp32 oracle passes on every frame (measured by the host test);
the kernel is held to 4 max(KAPPA_REF, 1): the device logf (1 .. 2 ulp against the host's <= 1) and sequential 40-term
sums against torch.mm's blocked ones -- the margin of the frontend probe.

Sparsify criterion.  Kept set: cut64 = torch.quantile in float64 (or the fp32 threshold, or the k-th largest value),
eps = 2^-21; v > cut64 (1 + eps) must be kept, v < cut64 (1 - eps) must be dropped, v == cut64 must be dropped (the test
is a strict >), anything else is free, and free elements of equal value share one fate.  Renormalisation: every value against the float64 (v keep + 1e-8) / sum of the
mask THE KERNEL PRODUCED (read off the output by ratios to an element whose fate is known), (40 + 2) 2^-24 relative, the
frame's sum within 42 2^-24 of 1.

Resampler criterion.  The published filter in closed form in float64, the bank rounded to fp32 as the product stores
it, the dot products in float64; |out - ref| <= (n + 2) 2^-24 sum_k |x_k| |h_k| with n the number of taps inside the signal
for that output: the a-priori bound of a sequential fmaf chain of n terms (plus one ulp of a bank entry, whose double
evaluation may round to the neighbouring fp32 value on another libm).
"""
import functools
import math

import numpy as np
import torch

NP = 40
U = 2.0 ** -24                       # unit roundoff of fp32
FRAMES = (1, 63, 64, 65, 197)        # one thread per frame, 64 per block: 197 = four blocks with a 5-frame tail
FULL = FRAMES[-1]
FAMILIES = ('soft', 'peaked', 'near', 'onehot', 'uniform', 'ties')
SPARSIFY_FAMILIES = ('soft', 'peaked', 'onehot', 'ties')
BATCH = 3

# The smallest kappa at which oracle.distance (fp32, CPU torch) is inside E_t on every frame at 197 frames, rounded
# up; measured and asserted by tests/test_postops_probe_host.py::test_kappa_ref_is_a_measurement.  (family, mix)
KAPPA_REF = {
    ('soft', True): 0.25, ('soft', False): 0.25,
    ('peaked', True): 0.20, ('peaked', False): 0.20,
    ('near', True): 0.10, ('near', False): 0.30,
    ('onehot', True): 0.30, ('onehot', False): 0.05,
    ('uniform', True): 0.15, ('uniform', False): 0.25,
    ('ties', True): 0.20, ('ties', False): 0.20,
}
# (entries are rounded up to 0.05; onehot without the mix is exact, 0, recorded as 0.05.  All are below 1, so the kernel's
# bound is kappa 4 for every family: the table records what the oracle needs, it does not move the bound.)


def kappa_gpu(family, mix):
    return 4.0 * max(KAPPA_REF[family, bool(mix)], 1.0)


OLD_RTOL, OLD_ATOL = 2e-5, 2e-6      # test_gpu_parity.py::test_postops_match_reference_fixture, distance
OLD_SPARSIFY_ATOL = 1e-6             # the same test, sparsify
OLD_RESAMPLE_ATOL = 2e-6             # test_resample_matches_closed_form_fixture, on 0.1-scale noise

EPS_CUT = 2.0 ** -21
RENORM = (NP + 2) * U
# 1 / 3: fp32(1 / 3) * 39 is exactly 13.0 in fp32, an interior integer position (lo == hi == 13, the cut IS order statistic
# 13); 10 / 39: fp32(10 / 39) * 39 is 10.00000095, lo = 10, hi = 11, w = 9.5e-7 -- a cut one rounding above order statistic 10.
# At both, that order statistic (and its equals) may lie within eps of the float64 cut and be free; nowhere else.
QUANTILES = (0.0, 10.0 / 39.0, 0.3, 1.0 / 3.0, 0.5, 0.85, 1.0)
INTEGER_POSITION = 1.0 / 3.0
NEAR_INTEGER_POSITION = 10.0 / 39.0
READABLE = 1e-8 * 2.0 ** -16         # below this, kept and dropped differ by less than the renormalisation bound can tell
TOPK = (1, 3, 39, 40)


# ---- posteriorgrams ----------------------------------------------------------------------------------------------

def _randn(seed, *shape):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed), dtype=torch.float64)


def _onehot(seed, *shape):
    index = torch.randint(0, NP, shape[:-2] + (1,) + shape[-1:], generator=torch.Generator().manual_seed(seed))
    return torch.zeros(shape, dtype=torch.float64).scatter_(-2, index, 1.0)


def _ties(seed, *shape):
    counts = torch.randint(0, 9, shape, generator=torch.Generator().manual_seed(seed)).double()
    counts[..., 0, :] += (counts.sum(dim=-2) == 0)                         # never an empty frame
    return counts / counts.sum(dim=-2, keepdim=True)


@functools.lru_cache(maxsize=None)
def pair(family):
    """(x, y): two (40, 197) fp32 PPGs of the family; the shorter probes are their first F frames.  Never modified."""
    F = FULL
    if family == 'soft':
        x, y = torch.softmax(3 * _randn(101, NP, F), 0), torch.softmax(3 * _randn(102, NP, F), 0)
    elif family == 'peaked':
        x, y = torch.softmax(12 * _randn(103, NP, F), 0), torch.softmax(12 * _randn(104, NP, F), 0)
    elif family == 'near':
        logits = 6 * _randn(105, NP, F)
        x, y = torch.softmax(logits, 0), torch.softmax(logits + 1e-3 * _randn(106, NP, F), 0)
    elif family == 'onehot':
        x, y = _onehot(107, NP, F), _onehot(108, NP, F)
        y[:, ::3] = x[:, ::3]                                              # a third of the frames identical
    elif family == 'uniform':
        x, y = torch.full((NP, F), 1.0 / NP, dtype=torch.float64), torch.softmax(12 * _randn(109, NP, F), 0)
    elif family == 'ties':
        x, y = _ties(110, NP, F), _ties(111, NP, F)
    else:
        raise KeyError(family)
    return x.float().contiguous(), y.float().contiguous()


@functools.lru_cache(maxsize=None)
def batch(family):
    """(3, 40, 197) fp32 for sparsify.  Never modified."""
    shape = (BATCH, NP, FULL)
    if family == 'soft':
        out = torch.softmax(3 * _randn(201, *shape), 1)
    elif family == 'peaked':
        out = torch.softmax(12 * _randn(202, *shape), 1)
    elif family == 'onehot':
        out = _onehot(203, *shape)
    elif family == 'ties':
        out = _ties(204, *shape)
    else:
        raise KeyError(family)
    return out.float().contiguous()


def mix_matrix(similarity, exponent, transpose=True):
    """What ppgs_amd.distance hands the kernel: (S.T ** exponent) in fp32."""
    s = torch.as_tensor(similarity).float()
    return ((s.T if transpose else s) ** float(exponent)).contiguous()


# ---- distance ------------------------------------------------------------------------------------------------------

def distance64(x, y, mix=None, floor=1e-8):
    """-> (ref (F,), avg (40, F), unit (40, F)) float64 numpy; d_p = kappa * unit_p."""
    a = torch.as_tensor(x).float().clamp(floor, 1 - floor).double()
    b = torch.as_tensor(y).float().clamp(floor, 1 - floor).double()
    if mix is not None:
        m64 = torch.as_tensor(mix).double()
        a, b = m64 @ a, m64 @ b
    a, b = a.numpy(), b.numpy()
    m = (a + b) / 2
    la, lb, lm = np.log(a), np.log(b), np.log(m)
    avg = (a * (la - lm) + b * (lb - lm)) / 2
    unit = U * (a * (np.abs(la) + np.abs(lm) + 1) + b * (np.abs(lb) + np.abs(lm) + 1)) / 2
    return np.sqrt(np.maximum(avg, 0)).sum(axis=0), avg, unit


def distance_bound(avg, unit, kappa):
    """E_t(kappa), (F,); kappa a number or (F,)."""
    d = np.asarray(kappa, dtype=np.float64) * unit
    return (np.sqrt(np.maximum(avg, 0) + d) - np.sqrt(np.maximum(avg - d, 0))).sum(axis=0)


def distance_violations(out, x, y, mix, kappa):
    """(F,) bool: the frames of `out` outside E_t(kappa), non-finite ones included."""
    ref, avg, unit = distance64(x, y, mix)
    out = np.asarray(out, dtype=np.float64)
    assert out.shape == ref.shape, (out.shape, ref.shape)
    return ~(np.abs(out - ref) <= distance_bound(avg, unit, kappa))


def distance_kappa(out, x, y, mix, ceiling=4096.0):
    """The smallest kappa at which every frame of `out` passes, to 1 %, from above (`ceiling` if none below does)."""
    ref, avg, unit = distance64(x, y, mix)
    error = np.abs(np.asarray(out, dtype=np.float64) - ref)
    if not np.isfinite(error).all() or (error > distance_bound(avg, unit, ceiling)).any():
        return ceiling
    lo, hi = np.zeros_like(error), np.full_like(error, ceiling)              # per frame: E_t is monotone in kappa
    for _ in range(40):
        mid = 0.5 * (lo + hi)
        ok = error <= distance_bound(avg, unit, mid)
        lo, hi = np.where(ok, lo, mid), np.where(ok, mid, hi)
    return float(np.where(error == 0, 0.0, hi).max())


def old_distance_accepts(out, ref):
    return bool(np.allclose(out, ref, rtol=OLD_RTOL, atol=OLD_ATOL))


DISTANCE_MUTANTS = ('floor_1e-7', 'mix_not_transposed', 'exponent_1', 'block_offset')


def distance_mutant(kind, x, y, similarity, exponent, normalize):
    """The float64 restatement with one fault, (F,)."""
    mix = mix_matrix(similarity, exponent) if normalize else None
    if kind == 'floor_1e-7':
        return distance64(x, y, mix, floor=1e-7)[0]
    if kind == 'mix_not_transposed':
        assert normalize
        return distance64(x, y, mix_matrix(similarity, exponent, transpose=False))[0]
    if kind == 'exponent_1':
        assert normalize
        return distance64(x, y, mix_matrix(similarity, 1.0))[0]
    if kind == 'block_offset':
        ref = distance64(x, y, mix)[0]
        out = ref.copy()
        out[64:] = ref[:max(len(ref) - 64, 0)]                                       # frames >= 64 taken from t - 64
        return out
    raise KeyError(kind)


# ---- sparsify ------------------------------------------------------------------------------------------------------

def fp32(value):
    return float(np.float32(value))


def percentile_cut(v, q):
    """torch.quantile in float64 at the fp32 value of q (what the kernel is handed), (B, 1, F) numpy."""
    return torch.quantile(torch.as_tensor(v).double(), fp32(q), dim=-2, keepdim=True).numpy()


def cut_rule(v, cut):
    """-> (must_keep, must_drop) bool arrays; neither = free."""
    v = np.asarray(v, dtype=np.float64)
    must_keep = v > cut * (1 + EPS_CUT)
    must_drop = (v < cut * (1 - EPS_CUT)) | (v == cut)
    return must_keep, must_drop


def topk_rule(v, k):
    """Above the k-th largest value: kept; below: dropped; equal to it: kept when all of the equals fit into the k,
    else free (which of equals is no contract)."""
    v = np.asarray(v, dtype=np.float64)
    kth = np.sort(v, axis=-2)[..., NP - k:NP - k + 1, :]
    all_fit = (v >= kth).sum(axis=-2, keepdims=True) == k
    return (v > kth) | ((v == kth) & all_fit), v < kth


def kernel_mask(v, out, must_keep, must_drop):
    """The keep mask behind `out`, decided without knowing the frame's sum: out_p / out_r = (v_p keep_p + 1e-8) /
    (v_r keep_r + 1e-8) for an anchor r whose fate is known (the largest must-keep value, else a dropped one).
    A value below READABLE (exact zeros, the underflowed tail of a peaked frame) carries no decision the output could
    show: it follows the rule, and the renormalisation bound judges what it contributes."""
    v, out = np.asarray(v, dtype=np.float64), np.asarray(out, dtype=np.float64)
    numerator = np.where(must_keep, v + 1e-8, np.where(must_drop, 1e-8, -1.0))
    r = numerator.argmax(axis=-2)[..., None, :]
    anchor = np.take_along_axis(numerator, r, axis=-2)
    assert (anchor > 0).all(), 'a frame without an element of known fate'
    estimate = out / np.take_along_axis(out, r, axis=-2) * anchor
    return np.where(v >= READABLE, estimate > np.sqrt(1e-8 * (v + 1e-8)), must_keep)


def sparsify_report(v, out, must_keep, must_drop, threshold_method=True):
    """-> dict: wrongly dropped / wrongly kept counts, the mask, worst relative renormalisation error and worst
    |sum - 1|, both in units of RENORM (the criterion holds iff no wrong element and both <= 1)."""
    v64, out64 = np.asarray(v, dtype=np.float64), np.asarray(out, dtype=np.float64)
    assert v64.shape == out64.shape, (v64.shape, out64.shape)
    if not np.isfinite(out64).all() or (out64 <= 0).any():
        return dict(dropped=v64.size, kept=v64.size, split=0, mask=np.zeros(v64.shape, dtype=bool), renorm=np.inf,
                    total=np.inf)
    mask = kernel_mask(v64, out64, must_keep, must_drop)
    numerator = v64 * mask + 1e-8
    ref = numerator / numerator.sum(axis=-2, keepdims=True)
    return dict(dropped=int((must_keep & ~mask).sum()), kept=int((must_drop & mask).sum()),
                split=split_fates(v64, mask, must_keep, must_drop) if threshold_method else 0, mask=mask,
                renorm=float((np.abs(out64 - ref) / ref).max() / RENORM),
                total=float(np.abs(out64.sum(axis=-2) - 1).max() / RENORM))


def sparsify_passes(report):
    return (report['dropped'] == 0 and report['kept'] == 0 and report['split'] == 0 and report['renorm'] <= 1
            and report['total'] <= 1)


def split_fates(v, mask, must_keep, must_drop):
    """How many frames hold two free elements of EQUAL value of which one is kept and one dropped: a strict > against
    one threshold cannot do that (top-k may: pass its rule's arrays only where the method is a threshold)."""
    v = np.asarray(v, dtype=np.float64)
    free = ~must_keep & ~must_drop
    pairs = (free[..., :, None, :] & free[..., None, :, :] & (v[..., :, None, :] == v[..., None, :, :])
             & (mask[..., :, None, :] != mask[..., None, :, :]))
    return int(pairs.any(axis=(-3, -2)).sum())


def topk_passes(v, mask, k):
    """Exactly k kept in every frame whose k-th largest value is READABLE (among unreadable equals the count cannot be
    seen), and no readable dropped value above a kept one."""
    v = np.asarray(v, dtype=np.float64)
    kth = np.sort(v, axis=-2)[..., NP - k, :]
    count_ok = (mask.sum(axis=-2) == k) | (kth < READABLE)
    lowest_kept = np.where(mask, v, np.inf).min(axis=-2)
    highest_dropped = np.where(~mask & (v >= READABLE), v, -np.inf).max(axis=-2)
    return bool(count_ok.all() and (lowest_kept >= highest_dropped).all())


def free_values_per_frame(v, must_keep, must_drop):
    """How many DISTINCT values the free elements of a frame have, (B, F)."""
    free = np.where(~must_keep & ~must_drop, np.asarray(v, dtype=np.float64), np.nan)
    ordered = np.sort(free, axis=-2)                                            # NaN last
    distinct = np.isfinite(ordered[..., 1:, :]) & (ordered[..., 1:, :] != ordered[..., :-1, :])
    return np.isfinite(ordered[..., 0, :]) + distinct.sum(axis=-2)


def free_per_frame(must_keep, must_drop):
    return (~must_keep & ~must_drop).sum(axis=-2)


def constant_thresholds(family):
    """0.1, a value present in the input (the strict > must drop it), and 0."""
    return (0.1, float(batch(family)[1, 7, 100]), 0.0)


def sparsify_cases(family):
    """Every (method, threshold, must_keep, must_drop) of the probe on batch(family)."""
    v = batch(family).numpy()
    for q in QUANTILES:
        yield ('percentile', q) + cut_rule(v, percentile_cut(v, q))
    for threshold in constant_thresholds(family):
        yield ('constant', threshold) + cut_rule(v, np.float64(np.float32(threshold)))
    for k in TOPK:
        yield ('topk', k) + topk_rule(v, k)


SPARSIFY_MUTANTS = ('greater_equal', 'ties_without_index', 'k_smallest', 'item_offset')


def sparsify_restated(v, method, threshold, mutant=None):
    """The kernel's algorithm in numpy fp32 (rank by counting, ties by index, torch.lerp), optionally with one fault.
    (B, 40, F) -> (B, 40, F) float32."""
    v = np.asarray(v, dtype=np.float32)
    if mutant == 'item_offset' and v.shape[0] > 1:
        v = v.copy()
        v[1] = v[0]
    p = np.arange(NP)
    below = v[:, None, :, :] < v[:, :, None, :]                               # [b, p, q, f]: v_q < v_p
    if mutant != 'ties_without_index':
        below = below | ((v[:, None, :, :] == v[:, :, None, :]) & (p[None, :] < p[:, None])[None, :, :, None])
    rank = below.sum(axis=2)
    if method == 'constant':
        thr = np.float32(threshold)
    elif method == 'percentile':
        pos = np.float32(threshold) * np.float32(NP - 1)
        lo, hi = int(np.floor(pos)), int(np.ceil(pos))
        w = np.float32(pos - np.float32(lo))
        a = np.where(rank == lo, v, np.float32(0)).max(axis=1, keepdims=True)    # the kernel's select, values >= 0
        b = np.where(rank == hi, v, np.float32(0)).max(axis=1, keepdims=True)
        thr = a + w * (b - a) if w < 0.5 else b - (b - a) * (np.float32(1) - w)
    if method == 'topk':
        k = int(threshold + 0.5)
        keep = rank < k if mutant == 'k_smallest' else rank >= NP - k
    else:
        keep = v >= thr if mutant == 'greater_equal' else v > thr
    kept = np.where(keep, v, np.float32(0)) + np.float32(1e-8)
    total = np.zeros_like(kept[:, 0])
    for q in range(NP):
        total = total + kept[:, q]
    return kept * (np.float32(1) / total)[:, None]


# ---- resampler -----------------------------------------------------------------------------------------------------

LOWPASS, ROLLOFF = 6.0, 0.99

RESAMPLE_CASES = ((48000, 16000, 1000), (44100, 16000, 2000), (22050, 16000, 1500), (8000, 16000, 700),
                  (16000, 44100, 400))
RESAMPLE_DEGENERATE = ((44100, 16000, 1), (44100, 16000, 5), (48000, 16000, 3))
RESAMPLE_CEIL = tuple((rate, target, orig * 2 + extra)
                      for rate, target, orig in ((44100, 16000, 441), (16000, 44100, 160), (48000, 16000, 3))
                      for extra in (-1, 0, 1))


def rates(rate, target):
    g = math.gcd(int(rate), int(target))
    return int(rate) // g, int(target) // g


def output_length(samples, rate, target):
    orig, now = rates(rate, target)
    return -((-now * samples) // orig)                                         # ceil in integers


@functools.lru_cache(maxsize=None)
def bank(rate, target, scaled=True):
    """-> (h (now, taps) float64 holding fp32 values, width): the polyphase bank of the published filter."""
    orig, now = rates(rate, target)
    base = min(orig, now) * ROLLOFF
    width = math.ceil(LOWPASS * orig / base)
    k = np.arange(2 * width + orig, dtype=np.float64)[None]
    i = np.arange(now, dtype=np.float64)[:, None]
    t = np.clip((-i / now + (k - width) / orig) * base, -LOWPASS, LOWPASS)
    h = np.sinc(t) * np.cos(t * np.pi / LOWPASS / 2) ** 2 * (base / orig if scaled else 1.0)
    h = h.astype(np.float32).astype(np.float64)
    h.setflags(write=False)
    return h, width


def closed_form_tap(rate, target, source, n):
    """The filter weight of input sample `source` in output sample `n`, from exact rational sample times (no bank,
    no phase / block split), float64; arrays broadcast."""
    orig, now = rates(rate, target)
    base = min(orig, now) * ROLLOFF
    t = (np.asarray(source, dtype=np.int64) * now - np.asarray(n, dtype=np.int64) * orig).astype(np.float64) / (orig * now) * base
    return np.where(np.abs(t) < LOWPASS, np.sinc(t) * np.cos(np.pi * t / (2 * LOWPASS)) ** 2, 0.0) * (base / orig)


def resample64(x, rate, target, mutant=None):
    """-> (ref, scale, taps_inside), each (rows, ceil(now samples / orig)) float64: the bank's fp32 values, float64
    dot products; scale = sum_k |x_k| |h_k|.  `mutant`: one of RESAMPLE_MUTANTS."""
    x = np.asarray(x, dtype=np.float64)
    rows, samples = x.shape
    orig, now = rates(rate, target)
    h, width = bank(rate, target, scaled=mutant != 'unscaled')
    taps = h.shape[1]
    blocks = -(-output_length(samples, rate, target) // now)
    shift = 1 if mutant == 'first_off_by_one' else 0
    padded = np.zeros((rows, width + shift + (blocks - 1) * orig + taps))
    padded[:, width + shift:width + shift + samples] = x                     # blocks * orig >= samples: it fits
    inside = np.zeros(padded.shape[1])
    inside[width + shift:width + shift + samples] = 1
    index = (np.arange(blocks) * orig)[:, None] + np.arange(taps)[None]        # (blocks, taps)
    windows = padded[:, index]                                                 # (rows, blocks, taps)
    out = windows @ h.T                                                        # (rows, blocks, now)
    scale = np.abs(windows) @ np.abs(h.T)
    count = np.broadcast_to(inside[index].sum(axis=1)[None, :, None], out.shape)
    if mutant == 'phase_block_exchanged':
        out = out.transpose(0, 2, 1)
    length = (now * samples) // orig if mutant == 'floor_length' else output_length(samples, rate, target)
    flat = lambda a: np.ascontiguousarray(a).reshape(rows, -1)[:, :length]
    return flat(out), flat(scale), flat(count)


# oracle.resample (fp32 conv1d, CPU torch): the largest |error| / (2^-24 sum |x| |h|) over all cases is 4.16, at most 0.23
# of the bound; measured and asserted by tests/test_postops_probe_host.py::test_resample_oracle_kappa
KAPPA_REF_RESAMPLE = 4.2

RESAMPLE_MUTANTS = ('first_off_by_one', 'phase_block_exchanged', 'floor_length', 'unscaled')


def resample_report(out, x, rate, target):
    """-> (worst |out - ref| / ((n + 2) 2^-24 scale), kappa = worst |out - ref| / (2^-24 scale)); inf on a wrong
    shape or a non-finite value.  The criterion holds iff the first is <= 1."""
    ref, scale, count = resample64(x, rate, target)
    out = np.asarray(out, dtype=np.float64)
    if out.shape != ref.shape or not np.isfinite(out).all():
        return np.inf, np.inf
    error = np.abs(out - ref)
    quiet = scale == 0
    if (error[quiet] != 0).any():
        return np.inf, np.inf
    safe = np.where(quiet, 1.0, scale)
    return float((error / ((count + 2) * U * safe)).max()), float((error / (U * safe)).max())


@functools.lru_cache(maxsize=None)
def signal(samples, rate):
    """(2, samples) fp32: 0.5-scale white noise and a 0.9-amplitude 1 kHz tone at `rate`.  Never modified."""
    noise = 0.5 * _randn(300 + samples + rate % 1000, samples)
    tone = 0.9 * torch.sin(2 * math.pi * 1000.0 / rate * torch.arange(samples, dtype=torch.float64) + 0.3)
    return torch.stack([noise, tone]).float().contiguous()


def impulse(samples, position):
    out = torch.zeros(1, samples)
    out[0, position] = 1.0
    return out


def ulp32(x):
    return np.spacing(np.abs(np.asarray(x, dtype=np.float32))).astype(np.float64)
