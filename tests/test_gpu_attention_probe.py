"""The attention kernel's mask edges on the GPU: the staircase probe of tests/attention_probe.py (a one-layer network
in which the visible marked key with the largest index takes the softmax, so one key too many or too few moves the
logits by O(1) in every precision) through every instantiation of ppg_attn.hip's attn_body -- key tiles of 16, 32 and
64 keys, query tiles of 64 and 128 -- with `valid` and the causal diagonal on, before and behind every tile boundary.
Why the seeded checkpoint cannot see such an error, and that the probe can: tests/test_attention_probe_host.py.

Cases: fp32, fp16x2, fp16, bf16 x hidden 256 (d = 128) / 512 (d = 256) x causal or not, one batch of the 24 valid
lengths of attention_probe.VALID at 300 frames, logits (softmax=False) against float64 inside the mask, exactly 0
behind it.  Bounds:
* fp32 and fp16x2: 2e-4, the project's logits bound (test_gpu_parity.py::test_single_window_fp32, stated there for
  logits of magnitude about 4.4; the probe's are at most 4.0 and the fp32 oracle is 2.5e-6 from float64).
* fp16 and bf16: 1.6 x the format cost -- the float64 reference with every MFMA operand rounded to the format where
  the kernels round it -- the rule of test_fused_layer_kernel_vs_oracle_and_unfused.
Each case runs again with every workspace filled with 0xFF (a key read past `valid` is then a spotlight or a NaN) and
must give the same bits; with PPGS_AMD_ATTN_REBASE=always; and on an engine with PPGS_AMD_ATTN_NARROW=0 (128-query
tiles everywhere at d = 128), to the same bounds.  At fp16 the default run already re-bases at every edge tile: a step
of 16 nats is 2^23, past kProbCeil = 2^10 (bf16 / fp32 re-base past 2^40, i.e. at every second edge).

Other routes to the same kernel (bf16 and fp16, hidden 256): the batch tiled 4 x (96 x 300 frames: ppg_head32.hip
writes the K rows and the permuted V^T); chunked items (T = 850: windows of 500 / 500 / 100 frames whose valid
lengths are 500, 215, 167, 116 and, for the items added to the issue's four, 128, 129, 192, 256 -- on and beside
edges -- and 100 / 0); a KV-cached stream of 300 frames pushed in steps of 1, 16 and 37 frames (Stream /
ppg_stream_push: q0 not a tile multiple, push boundaries before, on and behind edges).

If a case fails the staircase says which query / key pair is wrong: the failing query's logits equal the reference of
the neighbouring step (the assertion message names item, frame and valid).

Measured on an MI355X (max |logits - float64| inside the mask; format cost; smallest mutant effect of the host test):
    precision  hidden  non-causal  causal    format cost (non-causal / causal)   smallest mutant effect (nc / causal)
    fp32        256     7.2e-6      6.7e-6         --                              0.45 / 0.18
    fp32        512     8.5e-6      9.1e-6         --                              0.36 / 0.20
    fp16x2      256     4.8e-6      4.7e-6         --                              0.45 / 0.18
    fp16x2      512     5.8e-6      6.1e-6         --                              0.36 / 0.20
    fp16        256     2.2e-3      2.4e-3      2.1e-3 / 2.4e-3                    0.45 / 0.18
    fp16        512     3.6e-3      3.6e-3      3.6e-3 / 3.6e-3                    0.36 / 0.20
    bf16        256     1.8e-2      1.9e-2      1.8e-2 / 1.8e-2                    0.45 / 0.18
    bf16        512     2.1e-2      2.1e-2      2.0e-2 / 2.0e-2                    0.36 / 0.20
re-base always and 128-query tiles: the same figures (bf16, hidden 256, non-causal, re-base always: 1.7e-2).  96 x 300:
the figures of the 24-item batch.  Chunked (hidden 256): bf16 2.0e-2 / 2.0e-2 of a format cost of 2.0e-2, fp16
2.3e-3 / 2.7e-3 of 2.3e-3 / 2.6e-3.  Stream, every step size: bf16 1.7e-2, fp16 1.9e-3.  The whole file: 8 s.
With the key loop of attn_body ended one key early (`kend = w.valid - 1` in a scratch build) the bf16 cases fail by
0.14 .. 2.5 (10 of 11; the stream in steps of 16 never has `valid - 1` on a tile boundary) while
test_gpu_parity.py::test_16bit_modes passes.  (`kend = w.valid + 1` alone computes the same result: the per-query
mask still hides key `valid`.  With `w.valid + 1` there too, 8 of the 11 fail by 0.4 .. 3.5 -- the stream has no key
behind `valid` -- and test_16bit_modes notices as well, by 2 x its bar, at its 37-frame item.)
"""
import numpy as np
import pytest
import torch

import attention_probe as A
from ppgs_amd import engine as E

pytestmark = pytest.mark.gpu

FP32_LOGITS_TOL = 2e-4
PRECISIONS = ['fp32', 'fp16x2', 'fp16', 'bf16']


@pytest.fixture(scope='module')
def lab():
    return A.Lab()


_engines = {}


def engine_of(case, precision, monkeypatch=None, narrow=True):
    """One engine per (case, precision, tile widths); PPGS_AMD_ATTN_NARROW is read when the engine is created."""
    key = (case.hidden, case.causal, precision, narrow)
    if key not in _engines:
        if not narrow:
            monkeypatch.setenv('PPGS_AMD_ATTN_NARROW', '0')
        _engines[key] = E.Engine(case.state, 0, precision, case.causal)
        if not narrow:
            monkeypatch.delenv('PPGS_AMD_ATTN_NARROW')
    return _engines[key]


def logits(engine, feats, valid):
    out = engine.encode(feats.cuda(), list(valid), softmax=False)
    torch.cuda.synchronize()
    return out.cpu().numpy()


def poison(engine):
    for workspace in engine._workspaces.values():
        workspace.view(torch.int16).fill_(-1)          # 0xffff.. = NaN as bf16, fp16 and fp32


def bound_of(case, precision):
    return FP32_LOGITS_TOL if precision in ('fp32', 'fp16x2') else A.bound16(case.cost(precision))


def check(case, out, bound, what, ref=None, valid=None):
    """max |out - float64| inside the mask < bound, exactly 0 behind it; the message names the worst frame."""
    ref = case.ref if ref is None else ref
    valid = case.valid if valid is None else valid
    inside = A.inside(valid, ref.shape[-1])
    assert out.shape == ref.shape
    assert np.isfinite(out).all(), what
    assert np.all(out[~np.broadcast_to(inside, out.shape)] == 0), f'{what}: frames >= valid are not exactly 0'
    err = np.abs(out - ref) * inside
    item, _, frame = np.unravel_index(err.argmax(), err.shape)
    print(f'{what}: error {err.max():.3e} bound {bound:.3e}')
    assert err.max() < bound, f'{what}: {err.max():.3e} >= {bound:.3e} at item {item} (valid {valid[item]}) frame {frame}'
    return float(err.max())


@pytest.mark.parametrize('causal', [False, True])
@pytest.mark.parametrize('hidden', [256, 512])
@pytest.mark.parametrize('precision', PRECISIONS)
def test_mask_edges(lab, monkeypatch, precision, hidden, causal):
    case = lab.case(hidden, causal)
    bound = bound_of(case, precision)
    tag = f'{precision} hidden {hidden} {"causal" if causal else "non-causal"}'
    engine = engine_of(case, precision)
    out = logits(engine, case.feats, case.valid)
    check(case, out, bound, tag)
    poison(engine)
    assert np.array_equal(out, logits(engine, case.feats, case.valid)), f'{tag}: depends on what the workspace held'
    monkeypatch.setenv('PPGS_AMD_ATTN_REBASE', 'always')
    eager = logits(engine, case.feats, case.valid)
    monkeypatch.delenv('PPGS_AMD_ATTN_REBASE')
    check(case, eager, bound, tag + ' re-base always')
    wide = engine_of(case, precision, monkeypatch, narrow=False)
    check(case, logits(wide, case.feats, case.valid), bound, tag + ' 128-query tiles')


@pytest.mark.parametrize('causal', [False, True])
@pytest.mark.parametrize('precision', ['bf16', 'fp16'])
def test_large_batch(lab, precision, causal):
    """The 24 items tiled 4 x: enough 160-token tiles for the head kernel, which then writes layer 0's K rows and
    permuted V^T (as test_head_kernel_vs_three_launches asserts it)."""
    case = lab.case(256, causal)
    valid = list(case.valid) * 4
    feats = case.feats.repeat(4, 1, 1)
    _, info = E.plan_windows(len(valid), A.FRAMES, valid)
    assert info.tokens >= 128 * 160
    engine = engine_of(case, precision)
    ref = np.tile(case.ref, (4, 1, 1))
    tag = f'{precision} {"causal" if causal else "non-causal"} 96 x 300'
    out = logits(engine, feats, valid)
    check(case, out, bound_of(case, precision), tag, ref, valid)
    poison(engine)
    assert np.array_equal(out, logits(engine, feats, valid)), f'{tag}: depends on what the workspace held'


# the issue's four items, and four whose second window's valid length lies on or beside an edge (length - 350)
CHUNKED = (850, 565, 517, 466, 478, 479, 542, 606)


@pytest.mark.parametrize('causal', [False, True])
@pytest.mark.parametrize('precision', ['bf16', 'fp16'])
def test_chunked(lab, precision, causal):
    """T = 850: three windows per item (500 / 500 / 100 frames, 50 of left context), each with the staircase at its
    own rows 0 .. 256 -- the table is window-relative."""
    case = lab.case(256, causal, CHUNKED, 850)
    windows = A.O.plan_windows(850, CHUNKED)
    assert [w['Tc'] for w in windows] == [500, 500, 100]
    assert windows[1]['clens'] == [500, 215, 167, 116, 128, 129, 192, 256]
    engine = engine_of(case, precision)
    tag = f'{precision} {"causal" if causal else "non-causal"} chunked'
    out = logits(engine, case.feats, case.valid)
    check(case, out, bound_of(case, precision), tag)
    poison(engine)
    assert np.array_equal(out, logits(engine, case.feats, case.valid)), f'{tag}: depends on what the workspace held'


@pytest.mark.parametrize('step', [1, 16, 37])
@pytest.mark.parametrize('precision', ['bf16', 'fp16'])
def test_kv_cached_stream(lab, precision, step):
    """The 300-frame item pushed `step` frames at a time through Stream (ppg_stream_push -> the same launch_attn, with
    q0 wherever the push began): the causal forward of the whole utterance, to the bounds of the one-shot case."""
    case = lab.case(256, True)
    item = case.valid.index(A.FRAMES)
    feats = case.feats[item].cuda()
    stream = engine_of(case, precision).stream(A.FRAMES)
    pieces = [stream.push(feats[:, at:at + step], softmax=False) for at in range(0, A.FRAMES, step)]
    pieces.append(stream.push(None, flush=True, softmax=False))
    torch.cuda.synchronize()
    out = torch.cat(pieces, dim=1).cpu().numpy()[None]
    check(case, out, bound_of(case, precision), f'{precision} stream in steps of {step}', case.ref[item:item + 1], [A.FRAMES])
