"""The GPU tests of tests/test_gpu_w2v2_params.py can fail: every parameter class that w2v2_params.perturb() moves
away from 0 / 1 is one the float64 reference reacts to, by far more than the bound the HIP engines are held to.  CPU
only.

Model: transformers.Wav2Vec2Model(Wav2Vec2Config(num_hidden_layers=2)), torch.manual_seed(5), perturb(model, 11) and
perturb(model, 11, loud=True).  Body input (3, 77, 512) N(0, 1), valid frames [77, 40, 1]; feature-encoder input
(2, 4000) 0.1 N(0, 1).

Mutation: ONE parameter tensor of the float64 reference rolled by one element -- what a bias read in the wrong order,
from the neighbouring slot, or a swapped gamma / beta amounts to at least.  The rows inside the mask must move by
  * quiet amplitudes (the rule of ppgs_amd.weights.seeded_state_dict):  > 10 x 1e-4, the fp32 / fp16x2 bar;
  * loud amplitudes (w2v2_params.LOUD):  > 10 x the bf16 bar of the engine, 6e-2 (body) / 1.5e-1 (feature encoder),
    the bars of test_w2v2_body_vs_hf_fixture and test_w2v2_feature_encoder_vs_hf_fixture.
Classes: projection LayerNorm weight / bias, projection bias, positional-convolution bias and weight-norm gain,
encoder LayerNorm weight / bias; in each of the two layers the q, v, out, ffn1, ffn2 biases and both LayerNorms'
weight / bias; the feature encoder's GroupNorm weight / bias.

Smallest observed movement / bar (all above the required 10):
  * quiet, body:     104   (layer 1 q bias: 1.04e-2 against 1e-4; every other class > 1700)
  * quiet, encoder:  3080  (GroupNorm bias: 0.308)
  * loud, body:      14.0  (layer 0 v bias: 0.842 against 6e-2; layer 1 q bias 15.0)
  * loud, encoder:   16.1  (GroupNorm weight: 2.42 against 1.5e-1)
The loud amplitudes are the smallest round figures that reach 10 with some margin: a query bias acts only through
the softmax, against keys of magnitude ~0.5, and needs U(-16, 16) (at U(-8, 8): 9.4).

Stated exception: a key bias adds the same constant q . b_k to every logit of a query, which softmax cancels --
rolling k_proj.bias changes nothing beyond float64 rounding (measured <= 4.9e-15; bound 1e-11 = 768-term sums of
magnitude-10 values at 2.2e-16, two layers, with two orders of margin).  The GPU tests cannot see a misplaced key
bias, and nobody should expect them to.

Oracle cross-check: oracle.ppg_oracle.w2v2_body / w2v2_feature_encoder (fp32 restatements, the CPU references of other
tests) on the perturbed state dict stay within 1e-4 of the float64 HF modules -- the first time the oracle's
weight-norm branch runs with g != ||v||.  Measured: body 3.7e-6 quiet / 4.5e-6 loud (magnitude 8.5), encoder 1.1e-6 / 2.4e-6.
"""
import pytest
import torch
import transformers

from oracle import ppg_oracle as O

import w2v2_params as P

transformers.utils.logging.set_verbosity_error()

VALID = [77, 40, 1]
BARS = {False: (1e-4, 1e-4), True: (6e-2, 1.5e-1)}       # loud -> (body, feature encoder)


class _Case:
    def __init__(self, loud):
        torch.manual_seed(5)
        model = transformers.Wav2Vec2Model(transformers.Wav2Vec2Config(num_hidden_layers=2)).eval()
        self.model = P.perturb(model, 11, loud=loud)
        self.model64 = P.to64(self.model)
        generator = torch.Generator().manual_seed(3)
        self.features = torch.randn(3, 77, 512, generator=generator)
        self.audio = 0.1 * torch.randn(2, 4000, generator=generator)
        self.body = P.reference64(self.model64, self.features, VALID)
        self.encoder = P.encoder64(self.model64, self.audio)


_cases = {}


def case(loud):
    if loud not in _cases:
        _cases[loud] = _Case(loud)
    return _cases[loud]


def moved_inside_mask(a, b):
    return max(float((a[item, :count] - b[item, :count]).abs().max()) for item, count in enumerate(VALID))


def _labels():
    layers = [f'layer {index} {what}' for index in range(2) for what in (
        'q bias', 'v bias', 'out bias', 'ffn1 bias', 'ffn2 bias', 'LayerNorm 1 weight', 'LayerNorm 1 bias',
        'LayerNorm 2 weight', 'LayerNorm 2 bias')]
    return ['projection LayerNorm weight', 'projection LayerNorm bias', 'projection bias',
            'positional convolution bias', 'positional convolution gain', 'encoder LayerNorm weight',
            'encoder LayerNorm bias'] + layers


class _Rolled:
    """`name` of the float64 model rolled by one element, and back."""
    def __init__(self, module, name):
        self.parameter = dict(module.named_parameters())[name]

    def __enter__(self):
        self.saved = self.parameter.detach().clone()
        with torch.no_grad():
            self.parameter.copy_(torch.roll(self.saved.flatten(), 1).view_as(self.saved))

    def __exit__(self, *_):
        with torch.no_grad():
            self.parameter.copy_(self.saved)


def test_perturb_leaves_no_bias_or_affine_at_its_initial_value():
    """What the helper promises: every bias and norm affine moved (none at 0 / 1), the gain away from ||v||, matrices
    and masked_spec_embed untouched, the same values from the same seed."""
    torch.manual_seed(5)
    fresh = transformers.Wav2Vec2Model(transformers.Wav2Vec2Config(num_hidden_layers=2)).eval()
    before = {name: value.clone() for name, value in fresh.state_dict().items()}
    model = case(False).model
    body, encoder = P.mutation_classes(model)
    moved = set(body.values()) | set(encoder.values()) | {f'encoder.layers.{i}.attention.k_proj.bias' for i in range(2)}
    for name, value in model.state_dict().items():
        if name in moved:
            assert not bool((value == 0).any()) and not bool((value == 1).any()), name
            assert not bool((value == before[name]).any()), name
        else:
            assert torch.equal(value, before[name]), name
    assert {name for name, _ in model.named_parameters() if name.endswith('bias') or 'layer_norm' in name} <= moved
    gain_key = P.gain_name(model)
    v = model.state_dict()[gain_key.replace('original0', 'original1').replace('weight_g', 'weight_v')]
    assert float((model.state_dict()[gain_key] / v.norm(dim=(0, 1), keepdim=True) - 1).abs().min()) > 1e-4
    again = P.perturb(fresh, 11)
    for name, value in model.state_dict().items():
        assert torch.equal(value, again.state_dict()[name]), name


@pytest.mark.parametrize('label', _labels())
@pytest.mark.parametrize('loud', [False, True], ids=['quiet', 'loud'])
def test_body_reference_reacts_to_a_misplaced_parameter(loud, label):
    c = case(loud)
    name = P.mutation_classes(c.model)[0][label]
    with _Rolled(c.model64, name):
        moved = moved_inside_mask(P.reference64(c.model64, c.features, VALID), c.body)
    bar = BARS[loud][0]
    print(f'{"loud" if loud else "quiet"} {label}: moved {moved:.4g} = {moved / bar:.1f} x the bar {bar:g}')
    assert moved > 10 * bar, (label, moved)
    assert torch.equal(P.reference64(c.model64, c.features, VALID), c.body)      # (rolled back)


@pytest.mark.parametrize('label', ['GroupNorm weight', 'GroupNorm bias'])
@pytest.mark.parametrize('loud', [False, True], ids=['quiet', 'loud'])
def test_encoder_reference_reacts_to_a_misplaced_parameter(loud, label):
    c = case(loud)
    name = P.mutation_classes(c.model)[1][label]
    with _Rolled(c.model64, name):
        moved = float((P.encoder64(c.model64, c.audio) - c.encoder).abs().max())
    bar = BARS[loud][1]
    print(f'{"loud" if loud else "quiet"} {label}: moved {moved:.4g} = {moved / bar:.1f} x the bar {bar:g}')
    assert moved > 10 * bar, (label, moved)


@pytest.mark.parametrize('layer', [0, 1])
@pytest.mark.parametrize('loud', [False, True], ids=['quiet', 'loud'])
def test_key_bias_is_cancelled_by_softmax(loud, layer):
    """The stated exception: a misplaced key bias is invisible to every output-level test."""
    c = case(loud)
    with _Rolled(c.model64, f'encoder.layers.{layer}.attention.k_proj.bias'):
        moved = moved_inside_mask(P.reference64(c.model64, c.features, VALID), c.body)
    print(f'{"loud" if loud else "quiet"} layer {layer} k bias: moved {moved:.3g}')
    assert moved < 1e-11


@pytest.mark.parametrize('loud', [False, True], ids=['quiet', 'loud'])
def test_oracle_restatements_agree_with_hf_on_the_perturbed_model(loud):
    c = case(loud)
    state = {key: value.detach().float() for key, value in c.model.state_dict().items()}
    assert not any(key.endswith('pos_conv_embed.conv.weight') for key in state)       # the weight-norm branch runs
    body = O.w2v2_body(state, c.features, VALID)
    error = moved_inside_mask(body.double(), c.body)
    extractor = {key: value.detach().float() for key, value in c.model.feature_extractor.state_dict().items()}
    encoder_error = float((O.w2v2_feature_encoder(extractor, c.audio).double() - c.encoder).abs().max())
    print(f'oracle against float64 HF: body {error:.3g} (magnitude {float(c.body.abs().max()):.2f}), feature encoder {encoder_error:.3g}')
    assert error < 1e-4 and encoder_error < 1e-4


@pytest.mark.parametrize('dtype', [torch.float16, torch.bfloat16])
def test_emulated_costs_one_operand_rounding(dtype):
    """emulated(): the float64 modules with matrices and GEMM inputs rounded -- its error is of the size of the format
    (eps x activation magnitude x a few layers), not zero and not the size of the activations; the float64 model it
    was copied from is left as it was."""
    c = case(False)
    eps = torch.finfo(dtype).eps
    body = moved_inside_mask(P.reference64(P.emulated(c.model64, dtype), c.features, VALID), c.body)
    encoder = float((P.encoder64(P.emulated(c.model64.feature_extractor, dtype), c.audio) - c.encoder).abs().max())
    print(f'{dtype}: format cost body {body:.3g}, feature encoder {encoder:.3g}')
    magnitude = float(c.body.abs().max())
    assert 0.1 * eps < body < 8 * eps * magnitude and 0.1 * eps < encoder < 8 * eps * magnitude
    assert torch.equal(P.reference64(c.model64, c.features, VALID), c.body)
