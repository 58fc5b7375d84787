"""Every per-channel parameter of the PPG encoder on the GPU: the loud probe networks of tests/encoder_params.py
(biases ten and more times the seeded ones, LayerNorm gains in U(0.25, 1.75), shifts in U(-1, 1); truncated to 1, 2, 3
and 5 layers so that every layer is judged as the last one) through every route that packs a bias, an affine or a
position row into a tile layout of its own.  Why the seeded checkpoint cannot see a misplaced block of one of them,
and that these networks can (each modelled fault is at least 4 x the bound): tests/test_encoder_params_host.py.

Every case: logits (softmax=False) of Engine.encode against the float64 oracle inside the mask, exactly 0 behind it,
and a second run with every workspace filled with 0xFF must give the same bits.  Bounds, none of them new:
* fp16 and bf16: 1.6 x the format cost (attention_probe.bound16, the rule of
  test_fused_layer_kernel_vs_oracle_and_unfused);
* fp32 and fp16x2: the project's logits bound 2e-4, stated for logits of magnitude 4.4
  (test_gpu_parity.py::test_single_window_fp32), scaled by max(1, max |ref| / 4.4).

Routes, each at the smallest batch that reaches it (asserted with E.plan_windows):
* token-split kernels: the probe batch alone (12 items x 300 frames, valid lengths on, before and behind 16- and
  160-token boundaries, 0, 1 and 300; hidden 512 in two halves) -- fp32, fp16x2, fp16, bf16 x hidden 256 / 512 x depth
  1, 2, 3, 5 x causal or not;
* the feature-split layer kernel ppg_layer32.hip (16-bit): the batch tiled 2 x at hidden 256 (> 6144 tokens: sub-tile
  workgroups, with the head kernel) and alone at hidden 512 (> 2048), windows at odd 16-token blocks and a partial last
  tile, again with PPGS_AMD_LAYER32=0, OP_FUSED=0 + QKV_FUSED=0, QKV_FUSED=0, FFN_MIXED=0 and FFN_UNFUSED=1;
* the head kernel ppg_head32.hip and whole-tile layer32 workgroups: the batch tiled 7 x (>= 128 x 160 tokens), again
  with PPGS_AMD_HEAD32=0; and 144 touching windows of exactly 160 rows;
* ppg_outconv.hip (the default of every 16-bit case at hidden 256) against PPGS_AMD_OUTCONV=0;
* fp16x2 on ppg_ffn32x2.hip (the batch tiled 4 x) with PPGS_AMD_FFN32X2 = 3, 2, 1 and 0, hidden 256 and 512;
* chunked items (T = 850: windows of 500 / 500 / 100 frames whose position rows are window-relative);
* a KV-cached stream (the stream packs its own copies of the parameters) pushed in steps of 16 and 37 frames.

If a case fails, the message names item, valid length, frame and output channel; compare `out - ref` with
`reference64(mutant) - ref` over encoder_params.MUTANTS to find the parameter block the pattern matches.

Format costs (float64 with the operands rounded, encoder_params.format_cost; the bound is 1.6 x): bf16 0.015 .. 0.020
and fp16 0.0019 .. 0.0025 at both hidden sizes and every depth, on logits of magnitude <= 4.7; the fp32 oracle is 2e-6
from float64.  NOT YET MEASURED on an MI355X: the GPU errors per precision and hidden size, the run time of this file,
and the scratch experiment (ppg_layer32.hip reading linear1.bias 16 channels off: does this file notice, does
test_gpu_parity.py::test_16bit_modes?) -- this file was written and its route preconditions checked without a GPU at
hand; every case prints its error beside its bound, to be entered here and in DESIGN.md from its first GPU run.
"""
import numpy as np
import pytest
import torch

import encoder_params as P
from ppgs_amd import engine as E

pytestmark = pytest.mark.gpu

PRECISIONS = ['fp32', 'fp16x2', 'fp16', 'bf16']
SIXTEEN = ['bf16', 'fp16']


@pytest.fixture(scope='module')
def lab():
    return P.Lab()


_engines = {}


def engine_of(net, precision, monkeypatch=None, **switches):
    """One engine per (network, precision, switches): PPGS_AMD_<SWITCH> is read when the engine is created."""
    key = (net.hidden, net.depth, net.causal, id(net.state), precision, tuple(sorted(switches.items())))
    if key not in _engines:
        for name, value in switches.items():
            monkeypatch.setenv('PPGS_AMD_' + name, str(value))
        _engines[key] = E.Engine(net.state, 0, precision, net.causal)
        for name in switches:
            monkeypatch.delenv('PPGS_AMD_' + name)
    return _engines[key]


def logits(engine, feats, valid):
    out = engine.encode(feats.cuda(), list(valid), softmax=False)
    torch.cuda.synchronize()
    return out.cpu().numpy()


def poison(engine):
    for workspace in engine._workspaces.values():
        workspace.view(torch.int16).fill_(-1)          # 0xffff.. = NaN as bf16, fp16 and fp32


def check(out, ref, valid, bound, what):
    """max |out - float64| inside the mask < bound, exactly 0 behind it; the message names the worst element."""
    inside = P.A.inside(valid, ref.shape[-1])
    assert out.shape == ref.shape
    assert np.isfinite(out).all(), what
    assert np.all(out[~np.broadcast_to(inside, out.shape)] == 0), f'{what}: frames >= valid are not exactly 0'
    err = np.abs(out - ref) * inside
    item, channel, frame = np.unravel_index(err.argmax(), err.shape)
    print(f'{what}: error {err.max():.3e} bound {bound:.3e}')
    assert err.max() < bound, (f'{what}: {err.max():.3e} >= {bound:.3e} at item {item} (valid {valid[item]}) '
                               f'frame {frame} output channel {channel}')
    return float(err.max())


def run(engine, feats, valid, ref, bound, what):
    out = logits(engine, feats, valid)
    check(out, ref, valid, bound, what)
    poison(engine)
    assert np.array_equal(out, logits(engine, feats, valid)), f'{what}: depends on what the workspace held'


def odd_block_windows(windows):
    return [w for w in windows if w.valid > 0 and (w.tok_off // 16) % 2 == 1]


@pytest.mark.parametrize('causal', [False, True])
@pytest.mark.parametrize('depth', P.DEPTHS)
@pytest.mark.parametrize('hidden', list(P.GEOMETRY))
@pytest.mark.parametrize('precision', PRECISIONS)
def test_token_split_kernels(lab, precision, hidden, depth, causal):
    """Below the token counts of every feature-split kernel (a window takes 304 token rows whatever its valid length):
    hidden 256 the probe batch alone, hidden 512 -- whose split-hidden regime ends at 2048 rows -- in two halves."""
    net = lab.net(hidden, depth, causal)
    half = len(net.valid) // 2
    for items in ([slice(None)] if hidden == 256 else [slice(0, half), slice(half, None)]):
        valid = net.valid[items]
        _, info = E.plan_windows(len(valid), net.frames, valid)
        assert info.tokens <= (6144 if hidden == 256 else 2048)
        run(engine_of(net, precision), net.feats[items], valid, net.ref[items], net.bound(precision),
            f'{precision} {net} items {items.start or 0}..')


LAYER32_VARIANTS = [{}, {'LAYER32': 0}, {'OP_FUSED': 0, 'QKV_FUSED': 0}, {'QKV_FUSED': 0}, {'FFN_MIXED': 0},
                    {'FFN_UNFUSED': 1}]


@pytest.mark.parametrize('causal', [False, True])
@pytest.mark.parametrize('hidden,depth', [(256, 1), (256, 2), (256, 5), (512, 1), (512, 5)])
@pytest.mark.parametrize('precision', SIXTEEN)
def test_feature_split_layer_kernel(lab, monkeypatch, precision, hidden, depth, causal):
    """ppg_layer32.hip: out-projection + LayerNorm 1 + FFN + LayerNorm 2 + the next layer's Q/K/V in one launch, with
    bo, g1, e1, b1, b2, g2, e2 and the next b_qkv in its own layouts.  Each switched-off fusion against float64 too."""
    net = lab.net(hidden, depth, causal)
    times = 2 if hidden == 256 else 1
    feats, valid, ref = P.tiled(net, times)
    windows, info = E.plan_windows(len(valid), net.frames, valid)
    tile = 160 if hidden == 256 else 96
    assert info.tokens > (6144 if hidden == 256 else 2048)
    assert odd_block_windows(windows) and info.tokens % tile != 0
    for switches in LAYER32_VARIANTS:
        tag = ' '.join(f'{k}={v}' for k, v in switches.items()) or 'default'
        run(engine_of(net, precision, monkeypatch, **switches), feats, valid, ref, net.bound(precision),
            f'{precision} {net} x {times} {tag}')


@pytest.mark.parametrize('causal', [False, True])
@pytest.mark.parametrize('depth', [1, 2, 5])
@pytest.mark.parametrize('precision', SIXTEEN)
def test_head_kernel(lab, monkeypatch, precision, depth, causal):
    """ppg_head32.hip: gather + input convolution (input bias, position rows) + layer 0's Q/K/V (in_proj_bias) in one
    kernel, from half a chip of 160-token tiles; the layers behind it run whole-tile layer32 workgroups."""
    net = lab.net(256, depth, causal)
    feats, valid, ref = P.tiled(net, 7)
    windows, info = E.plan_windows(len(valid), net.frames, valid)
    assert info.tokens >= 128 * 160 and info.tokens % 160 != 0 and odd_block_windows(windows)
    for switches in ({}, {'HEAD32': 0}):
        tag = ' '.join(f'{k}={v}' for k, v in switches.items()) or 'default'
        run(engine_of(net, precision, monkeypatch, **switches), feats, valid, ref, net.bound(precision),
            f'{precision} {net} x 7 {tag}')


@pytest.fixture(scope='module')
def touching():
    """The layout of test_head_kernel_vs_three_launches: 144 windows of exactly 160 rows, no padding rows between
    them, ragged valid lengths -- with loud parameters at depth 1."""
    generator = torch.Generator().manual_seed(23)
    valid = [160] * 8 + torch.randint(1, 161, (136,), generator=generator).tolist()
    return P.Net(256, 1, False, valid, 160)


@pytest.mark.parametrize('precision', SIXTEEN)
def test_head_kernel_touching_windows(touching, monkeypatch, precision):
    net = touching
    windows, info = E.plan_windows(len(net.valid), net.frames, net.valid)
    assert info.tokens == 144 * 160 and all(w.tok_off % 160 == 0 for w in windows)
    for switches in ({}, {'HEAD32': 0}):
        tag = ' '.join(f'{k}={v}' for k, v in switches.items()) or 'default'
        run(engine_of(net, precision, monkeypatch, **switches), net.feats, net.valid, net.ref, net.bound(precision),
            f'{precision} touching windows {tag}')


@pytest.mark.parametrize('causal', [False, True])
@pytest.mark.parametrize('depth', [1, 5])
@pytest.mark.parametrize('precision', SIXTEEN)
def test_output_convolution(lab, monkeypatch, precision, depth, causal):
    """ppg_outconv.hip (LDS-resident weights, its own copy of the output bias; hidden 256, 16-bit) is the default of
    every case above; here against the generic k-tap kernel on the same batch."""
    net = lab.net(256, depth, causal)
    for switches in ({}, {'OUTCONV': 0}):
        tag = ' '.join(f'{k}={v}' for k, v in switches.items()) or 'default'
        run(engine_of(net, precision, monkeypatch, **switches), net.feats, net.valid, net.ref, net.bound(precision),
            f'{precision} {net} {tag}')


@pytest.mark.parametrize('causal', [False, True])
@pytest.mark.parametrize('hidden,depth', [(256, 1), (256, 2), (256, 5), (512, 1), (512, 5)])
def test_fp16x2_feature_split_ffn(lab, monkeypatch, hidden, depth, causal):
    """fp16x2 on ppg_ffn32x2.hip (hidden 256, from half a chip of 96-token tiles): 3 = out-projection + LayerNorm 1 +
    FFN + LayerNorm 2 + Q/K/V tail, 2 = without the tail, 1 = the FFN block, 0 = the token-split kernels.  Hidden 512
    has no such kernel: the switch must change nothing there."""
    net = lab.net(hidden, depth, causal)
    times = 4 if hidden == 256 else 1
    feats, valid, ref = P.tiled(net, times)
    _, info = E.plan_windows(len(valid), net.frames, valid)
    if hidden == 256:
        assert info.tokens >= 128 * 96 and info.tokens % 96 != 0
    for level in (3, 2, 1, 0):
        run(engine_of(net, 'fp16x2', monkeypatch, FFN32X2=level), feats, valid, ref, net.bound('fp16x2'),
            f'fp16x2 {net} x {times} FFN32X2={level}')


@pytest.mark.parametrize('depth', [1, 5])
@pytest.mark.parametrize('precision', SIXTEEN)
def test_chunked(lab, precision, depth):
    """T = 850: three windows per item (500 / 500 / 100 frames, 50 of left context); every window adds the position
    rows 0 .. Tc (the host test's mutant: the second window with the rows of its absolute frames)."""
    net = lab.net(256, depth, False, P.CHUNKED_VALID, P.CHUNKED_FRAMES)
    windows = P.O.plan_windows(P.CHUNKED_FRAMES, P.CHUNKED_VALID)
    assert [w['Tc'] for w in windows] == [500, 500, 100] and windows[1]['clens'] == [500, 215, 116, 51]
    run(engine_of(net, precision), net.feats, net.valid, net.ref, net.bound(precision), f'{precision} {net} chunked')


@pytest.mark.parametrize('step', [16, 37])
@pytest.mark.parametrize('precision', SIXTEEN)
def test_kv_cached_stream(lab, precision, step):
    """The 300-frame item pushed `step` frames at a time through Stream, which packs its own copies of the
    parameters: the causal forward of the whole utterance, to the bound of the one-shot case."""
    net = lab.net(256, 2, True)
    item = net.valid.index(P.FRAMES)
    feats = net.feats[item].cuda()
    stream = engine_of(net, precision).stream(P.FRAMES)
    pieces = [stream.push(feats[:, at:at + step], softmax=False) for at in range(0, P.FRAMES, step)]
    pieces.append(stream.push(None, flush=True, softmax=False))
    torch.cuda.synchronize()
    out = torch.cat(pieces, dim=1).cpu().numpy()[None]
    check(out, net.ref[item:item + 1], [P.FRAMES], net.bound(precision), f'{precision} stream in steps of {step}')
