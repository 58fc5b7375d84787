"""The wav2vec 2.0 engines (feature encoder ppg_w2v2_*, transformer body ppg_w2v2_body_*) on a model whose biases,
norm affines and weight-norm gain are away from 0 and 1 (tests/w2v2_params.py: perturb), against the HF modules
themselves in float64 on the CPU.  Every other wav2vec2 test builds a freshly initialised HF model, in which those
parameters are exactly 0 / 1 / ||v||: a dropped, misplaced or swapped bias or affine computes the same numbers
there.  tests/test_w2v2_params_host.py shows that each of them moves the reference by > 10 x the bounds used here.
(Checked once on the MI355X from the engine's side as well: a W2v2Body / W2v2FeatureEncoder built from the model with
ONE tensor rolled by one element misses these bounds for each of the 25 + 2 tensors -- fp32 on the quiet model by
>= 60 x (a query bias: 6e-3 against 1e-4), bf16 on the loud model by >= 15 x (0.91 against 6e-2) -- and for a key
bias, which softmax cancels, it does not.)

Model: Wav2Vec2Config(num_hidden_layers=2), torch.manual_seed(5), perturb(model, 11) ("quiet", the amplitudes of
ppgs_amd.weights.seeded_state_dict) and perturb(model, 11, loud=True) (w2v2_params.LOUD).

BODY -- rows inside the frame mask, at the shapes of test_w2v2_body_shapes_vs_hf_modules / _16bit_kernels_at_odd_shapes
/ _two_pipelines_equal_one: (2, 33), (3, 257), (9, 77) and (9, 499) frames (the last: two pipelines).
  * fp32, fp16x2 against float64:  1e-4, the project's stated bar (HF's own fp32 on the CPU is 4e-6 from float64).
  * fp16 / bf16 against float64:   1e-2 / 6e-2, the bars of test_w2v2_body_vs_hf_fixture.
  * fp16 / bf16 against the same mode on the token-split kernels (PPGS_AMD_W2V2_GEMM32=0, _POSCONV=0, _QKV32=0:
    linear_kernel<EPI_QKV / EPI_GENERAL>, whose fp32 instantiation the first line holds to 1e-4):  2e-3 / 1.5e-2, the
    bounds of test_w2v2_body_16bit_kernels_at_odd_shapes.
  * loud model at (3, 257), fp16 / bf16 against float64:  1e-2 / 6e-2 (a misplaced entry costs >= 10 x that).
  * workspaces poisoned with 0xFF bytes: the same bits.
  emulated() (the float64 modules with matrices and GEMM inputs rounded to the format) is printed beside every
  16-bit error: the format's own cost.
  Measured on the MI355X (maximum over the four shapes; activations of magnitude 5 .. 8):
    fp32 1.1e-5, fp16x2 1.2e-5 (both largest at (9, 499));
    fp16 2.3e-3 (format cost 2.4e-3), against the token-split kernels 6.9e-4;
    bf16 1.9e-2 (format cost 1.9e-2), against the token-split kernels 5.0e-3;
    loud model (magnitude 9.2): fp16 3.2e-3 (format cost 3.4e-3), bf16 2.6e-2 (format cost 2.5e-2).
  The 16-bit errors ARE the format cost, on both kernel sets; no same-mode bound had to be derived from emulated().

FEATURE ENCODER -- sample counts 400 (one frame), 401..404 (the stride-5 remainder), 719 / 720 (one / two frames),
10000 (31 frames: 32 rows per item), 10249 (2048 layer-0 frames: the most that one block of the moments kernel
takes), 10320 and 10321 (32 frames: 64 rows per item; 2063 layer-0 frames: two blocks of the moments kernel and
their atomics); batches of 1, 3 and 17 with six kinds of signal mixed inside a batch (0.1 noise; noise + 0.5 DC;
zeros; 1e-4 noise, variance far below eps; full-scale +-1; zero-padded after 60 %).
  * frames(n) equals the reference's frame count.
  * fp32, fp16x2:  1e-4 x max(1, max|ref| / 3) -- the bar of test_w2v2_feature_encoder_vs_hf_fixture was stated for
    activations of magnitude ~3.
  * fp16 / bf16:   2e-2 / 1.5e-1, scaled the same way; also on the loud GroupNorm affine.
  * the all-zeros item equals gelu(beta) pushed through the six convolutions (computed here in float64).
  * repeat with the workspace poisoned: the same bits when layer 0 has <= 2048 frames; above that the two blocks'
    double atomicAdd order is not fixed, and the repeat is held to the bound only.
  Measured on the MI355X (maximum over all sample counts, batches and signals; magnitude 3.1 .. 3.7, loud 5.3):
    fp32 7.6e-6, fp16x2 7.6e-6 (7 % of the bound); fp16 3.3e-3, bf16 2.8e-2 (16 % of the bound);
    loud GroupNorm affine: fp16 5.7e-3, bf16 4.6e-2 (18 % of the scaled bound).
"""
import os

import pytest
import torch
import transformers

from ppgs_amd import engine as E

import w2v2_params as P

pytestmark = pytest.mark.gpu

transformers.utils.logging.set_verbosity_error()

BODY_CASES = {
    (2, 33): [33, 1],
    (3, 257): [257, 200, 129],
    (9, 77): [77, 1, 40, 77, 76, 33, 64, 65, 77],
    (9, 499): [499, 400, 499, 1, 257, 499, 33, 480, 499],          # >= 8 items, >= 4096 rows: two pipelines
}
BODY_TOL = {'fp32': 1e-4, 'fp16x2': 1e-4, 'fp16': 1e-2, 'bf16': 6e-2}
BODY_SAME_MODE_TOL = {'fp16': 2e-3, 'bf16': 1.5e-2}
ENCODER_TOL = {'fp32': 1e-4, 'fp16x2': 1e-4, 'fp16': 2e-2, 'bf16': 1.5e-1}
DTYPE = {'fp16': torch.float16, 'bf16': torch.bfloat16}
TOKEN_SPLIT = ('PPGS_AMD_W2V2_GEMM32', 'PPGS_AMD_W2V2_POSCONV', 'PPGS_AMD_W2V2_QKV32')
SAMPLES = (400, 401, 402, 403, 404, 719, 720, 10000, 10249, 10320, 10321)
KINDS = ('noise', 'noise + DC', 'zeros', 'tiny', 'full scale', 'padded')


class Lab:
    """Models, engines, inputs and float64 references, each built once for the module."""

    def __init__(self):
        self.models, self.bodies, self.encoders, self.body_refs, self.encoder_refs, self.costs = {}, {}, {}, {}, {}, {}

    def model(self, loud):
        if loud not in self.models:
            torch.manual_seed(5)
            model = transformers.Wav2Vec2Model(transformers.Wav2Vec2Config(num_hidden_layers=2)).eval()
            P.perturb(model, 11, loud=loud)
            self.models[loud] = (model, P.to64(model))
        return self.models[loud]

    def body(self, loud, precision, token_split=False):
        key = (loud, precision, token_split)
        if key not in self.bodies:
            saved = {name: os.environ.get(name) for name in TOKEN_SPLIT}
            try:
                for name in TOKEN_SPLIT:                 # (read when the engine is created)
                    if token_split:
                        os.environ[name] = '0'
                    else:
                        os.environ.pop(name, None)
                self.bodies[key] = E.W2v2Body(self.model(loud)[0], 0, precision)
            finally:
                for name, value in saved.items():
                    os.environ.pop(name, None)
                    if value is not None:
                        os.environ[name] = value
        return self.bodies[key]

    def encoder(self, loud, precision):
        key = (loud, precision)
        if key not in self.encoders:
            self.encoders[key] = E.W2v2FeatureEncoder(self.model(loud)[0].feature_extractor.state_dict(), 0, precision)
        return self.encoders[key]

    def body_case(self, loud, shape):
        """features, valid, float64 reference"""
        key = (loud, shape)
        if key not in self.body_refs:
            generator = torch.Generator().manual_seed(1000 * shape[0] + shape[1])
            features = torch.randn(*shape, 512, generator=generator)
            valid = BODY_CASES[shape]
            self.body_refs[key] = (features, valid, P.reference64(self.model(loud)[1], features, valid))
        return self.body_refs[key]

    def format_cost(self, loud, shape, precision):
        """emulated()'s distance from the float64 reference on this case: what the operand format alone costs"""
        key = (loud, shape, precision)
        if key not in self.costs:
            features, valid, ref = self.body_case(loud, shape)
            rounded = P.reference64(P.emulated(self.model(loud)[1], DTYPE[precision]), features, valid)
            self.costs[key] = inside_mask(rounded, ref, valid)
        return self.costs[key]

    def audio(self, samples):
        """(17, samples): item i of sample count number c is of kind (i + c) % 6"""
        index = SAMPLES.index(samples)
        generator = torch.Generator().manual_seed(77 + samples)
        noise = torch.randn(17, samples, generator=generator)
        audio = torch.empty(17, samples)
        for item in range(17):
            kind = KINDS[(item + index) % len(KINDS)]
            if kind == 'noise':
                audio[item] = 0.1 * noise[item]
            elif kind == 'noise + DC':
                audio[item] = 0.1 * noise[item] + 0.5
            elif kind == 'zeros':
                audio[item] = 0.
            elif kind == 'tiny':
                audio[item] = 1e-4 * noise[item]
            elif kind == 'full scale':
                audio[item] = torch.sign(noise[item])
            else:
                audio[item] = 0.1 * noise[item]
                audio[item, int(0.6 * samples):] = 0.
        return audio

    def encoder_case(self, loud, samples):
        key = (loud, samples)
        if key not in self.encoder_refs:
            audio = self.audio(samples)
            self.encoder_refs[key] = (audio, P.encoder64(self.model(loud)[1], audio))
        return self.encoder_refs[key]


@pytest.fixture(scope='module')
def lab():
    lab = Lab()
    yield lab
    lab.__dict__.clear()
    torch.cuda.empty_cache()


def inside_mask(out, ref, valid):
    out = out.detach().to('cpu', torch.float64)
    return max(float((out[item, :count] - ref[item, :count]).abs().max()) for item, count in enumerate(valid))


def run_poisoned(engine, *args):
    """The engine's output, and its output again after every workspace was filled with 0xFF bytes."""
    first = engine(*args).clone()
    for workspace in engine._workspaces.values():
        workspace.fill_(255)
    second = engine(*args).clone()
    torch.cuda.synchronize()
    return first, second


@pytest.mark.parametrize('shape', list(BODY_CASES), ids=lambda s: f'{s[0]}x{s[1]}')
@pytest.mark.parametrize('precision', ['fp32', 'fp16x2'])
def test_body_fp32_modes_vs_float64(lab, precision, shape):
    features, valid, ref = lab.body_case(False, shape)
    out, again = run_poisoned(lab.body(False, precision), features.cuda(), valid)
    assert out.shape == (*shape, 768) and bool(torch.isfinite(out).all())
    error = inside_mask(out, ref, valid)
    print(f'body {precision} {shape}: max error {error:.3g} (magnitude {float(ref.abs().max()):.2f})')
    assert error < BODY_TOL[precision]
    assert torch.equal(out, again)


@pytest.mark.parametrize('shape', list(BODY_CASES), ids=lambda s: f'{s[0]}x{s[1]}')
@pytest.mark.parametrize('precision', ['fp16', 'bf16'])
def test_body_16bit_modes_vs_float64_and_token_split(lab, precision, shape):
    features, valid, ref = lab.body_case(False, shape)
    out, again = run_poisoned(lab.body(False, precision), features.cuda(), valid)
    old = lab.body(False, precision, token_split=True)(features.cuda(), valid)
    assert bool(torch.isfinite(out).all())
    error, same_mode = inside_mask(out, ref, valid), inside_mask(out, old.to('cpu', torch.float64), valid)
    old_error = inside_mask(old, ref, valid)
    print(f'body {precision} {shape}: max error {error:.3g} (token-split kernels {old_error:.3g}; format cost '
          f'{lab.format_cost(False, shape, precision):.3g}), against the token-split kernels {same_mode:.3g}')
    assert error < BODY_TOL[precision]
    assert old_error < BODY_TOL[precision]
    assert same_mode < BODY_SAME_MODE_TOL[precision]
    assert torch.equal(out, again)


@pytest.mark.parametrize('precision', ['fp16', 'bf16'])
def test_body_16bit_modes_on_the_loud_model(lab, precision):
    shape = (3, 257)
    features, valid, ref = lab.body_case(True, shape)
    out, again = run_poisoned(lab.body(True, precision), features.cuda(), valid)
    error = inside_mask(out, ref, valid)
    print(f'body {precision} {shape} loud: max error {error:.3g} (format cost {lab.format_cost(True, shape, precision):.3g}, '
          f'magnitude {float(ref.abs().max()):.2f})')
    assert bool(torch.isfinite(out).all()) and error < BODY_TOL[precision]
    assert torch.equal(out, again)


def zeros_through_the_stack(extractor64):
    """All-zeros audio: the convolution gives 0, GroupNorm gives beta, and every later layer sees the same vector in
    each of its taps -- gelu(beta) pushed through the six convolutions, (512,) float64."""
    x = torch.nn.functional.gelu(extractor64.conv_layers[0].layer_norm.bias.detach())
    for layer in list(extractor64.conv_layers)[1:]:
        x = torch.nn.functional.gelu(layer.conv.weight.detach().sum(dim=2) @ x)
    return x


@pytest.mark.parametrize('samples', SAMPLES)
def test_feature_encoder_vs_float64(lab, samples):
    index = SAMPLES.index(samples)
    layer0_frames = (samples - 10) // 5 + 1
    runs = [(False, precision) for precision in ENCODER_TOL] + [(True, 'fp16'), (True, 'bf16')]
    for loud, precision in runs:
        audio, ref = lab.encoder_case(loud, samples)
        encoder = lab.encoder(loud, precision)
        assert encoder.frames(samples) == ref.shape[1]
        zero_row = zeros_through_the_stack(lab.model(loud)[1].feature_extractor)
        for items in ([0], [1, 2, 3], list(range(17))) if not loud else (list(range(17)),):
            want = ref[items]
            tol = ENCODER_TOL[precision] * max(1., float(want.abs().max()) / 3.)
            out, again = run_poisoned(encoder, audio[items].cuda())
            assert out.shape == want.shape and bool(torch.isfinite(out).all())
            error = float((out.to('cpu', torch.float64) - want).abs().max())
            repeat = float((again.to('cpu', torch.float64) - want).abs().max())
            print(f'encoder {precision}{" loud" if loud else ""} {samples} samples x {len(items)}: max error {error:.3g} '
                  f'(bound {tol:.3g}, magnitude {float(want.abs().max()):.2f})')
            assert error < tol and repeat < tol, (precision, loud, len(items))
            if layer0_frames <= 2048:
                assert torch.equal(out, again), (precision, loud, len(items))
            for row, item in enumerate(items):
                if KINDS[(item + index) % len(KINDS)] == 'zeros':
                    assert float((want[row] - zero_row).abs().max()) < 1e-12
                    assert float((out[row].to('cpu', torch.float64) - zero_row).abs().max()) < tol
