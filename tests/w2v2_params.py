"""Shared by tests/test_w2v2_params_host.py and tests/test_gpu_w2v2_params.py: a wav2vec 2.0 model whose biases,
norm affines and weight-norm gain are away from 0 and 1, and float64 references of its two halves.

A freshly initialised ``transformers.Wav2Vec2Model`` has every bias but the feature projection's at exactly 0, every
LayerNorm / GroupNorm affine at exactly (1, 0) and the positional convolution's weight-norm gain equal to ||v||: a
kernel that drops, misplaces or swaps one of them computes the same numbers.  :func:`perturb` applies the rule of
``ppgs_amd.weights.seeded_state_dict`` ("no parameter at a value, 0 or 1, that would hide an indexing bug") to such a
model.  No GPU is needed here; the HF modules themselves, deep-copied to float64 on the CPU, are the reference.
"""
import copy

import torch

# amplitudes of perturb(): (bias: U(-a, a), norm weight: 1 + a N, norm bias: a N, weight-norm gain: x (1 + a N)).
# QUIET is the rule of seeded_state_dict.  LOUD is chosen in tests/test_w2v2_params_host.py: the smallest round
# figures at which rolling any one tensor by one element moves the float64 output by more than 10 x the bf16 bar
# of its engine (the figures are in that module's docstring).
QUIET = {'bias': 0.1, 'norm_weight': 0.1, 'norm_bias': 0.1, 'gain': 0.1, 'group_norm_weight': 0.1, 'group_norm_bias': 0.1}
# A query bias reaches the output only through the softmax, and through keys of magnitude ~0.5: it needs 16.
# (an entry may be a dict {suffix of the parameter's name: amplitude, '': default})
LOUD = {'bias': {'q_proj.bias': 16., '': 0.5}, 'norm_weight': 0.3, 'norm_bias': 0.3, 'gain': 0.3,
        'group_norm_weight': 0.75, 'group_norm_bias': 0.75}

GAIN_NAMES = ('parametrizations.weight.original0', 'weight_g')


def _amplitude(table, kind, name):
    value = table[kind]
    if isinstance(value, dict):
        for suffix, amplitude in value.items():
            if suffix and name.endswith(suffix):
                return amplitude
        return value['']
    return value


def perturb(model, seed, loud=False):
    """Overwrite, in place and from one seeded generator, every parameter of an HF Wav2Vec2Model whose name ends in
    `bias` (U(-a, a)), every `layer_norm` / `final_layer_norm` weight (1 + a N) and bias (a N) -- the feature
    extractor's GroupNorm (`conv_layers.0.layer_norm`) included -- and multiply the positional convolution's
    weight-norm gain per tap by 1 + a N.  Matrices and `masked_spec_embed` stay.  Returns the model."""
    table = LOUD if loud else QUIET
    generator = torch.Generator(device='cpu').manual_seed(seed)
    with torch.no_grad():
        for name, parameter in model.named_parameters():
            shape = tuple(parameter.shape)

            def normal():
                return torch.randn(shape, generator=generator)
            if name == 'masked_spec_embed':
                continue
            if 'layer_norm' in name:
                group = 'group_' if name.startswith('feature_extractor.') else ''
                if name.endswith('weight'):
                    value = 1. + _amplitude(table, group + 'norm_weight', name) * normal()
                else:
                    value = _amplitude(table, group + 'norm_bias', name) * normal()
            elif name.endswith('bias'):
                value = _amplitude(table, 'bias', name) * (2. * torch.rand(shape, generator=generator) - 1.)
            elif name.endswith(GAIN_NAMES):
                value = parameter.detach().cpu().float() * (1. + _amplitude(table, 'gain', name) * normal())
            else:
                continue
            parameter.copy_(value.to(parameter.device, parameter.dtype))
    return model


def to64(module):
    """A float64 CPU copy of an HF module (the module itself when it already is one)."""
    first = next(module.parameters())
    if first.dtype == torch.float64 and first.device.type == 'cpu':
        return module
    return copy.deepcopy(module).to('cpu', torch.float64).eval()


def frame_mask(frames, valid):
    return torch.arange(frames)[None] < torch.as_tensor(list(valid)).reshape(-1, 1)


def reference64(model, features, valid):
    """HF's own feature_projection + encoder(..., attention_mask=mask) in float64 on the CPU:
    features (B, T, 512), valid frames per item -> last_hidden_state (B, T, hidden) float64."""
    model = to64(model)
    features = features.detach().to('cpu', torch.float64)
    with torch.no_grad():
        hidden, _ = model.feature_projection(features)
        return model.encoder(hidden, attention_mask=frame_mask(features.shape[1], valid)).last_hidden_state


def encoder64(model, audio):
    """HF's own feature_extractor in float64 on the CPU: audio (B, N) -> extract_features (B, frames, 512) float64.
    `model` is the Wav2Vec2Model or its feature_extractor."""
    extractor = to64(getattr(model, 'feature_extractor', model))
    with torch.no_grad():
        return extractor(audio.detach().to('cpu', torch.float64)).transpose(1, 2).contiguous()


class _Rounded(torch.nn.Module):
    def __init__(self, dtype):
        super().__init__()
        self.dtype = dtype

    def forward(self, weight):
        return weight.to(self.dtype).to(weight.dtype)


def _round_weight(layer, dtype):
    """Round a layer's weight to `dtype`: of a weight-normed convolution the EFFECTIVE weight g v / ||v||.  (A
    parametrized module's class is shared with the module it was deep-copied from, so the parametrization is not
    removed: the rounding is appended to the copy's own list.)"""
    parametrizations = getattr(layer, 'parametrizations', None)
    if parametrizations is not None and 'weight' in parametrizations:
        torch.nn.utils.parametrize.register_parametrization(layer, 'weight', _Rounded(dtype), unsafe=True)
        return
    if hasattr(layer, 'weight_g'):
        torch.nn.utils.remove_weight_norm(layer)
    layer.weight.copy_(layer.weight.to(dtype).to(layer.weight.dtype))


def emulated(module64, dtype):
    """The format cost of a 16-bit mode: a copy of the float64 module with every matrix (Linear / Conv1d weight, the
    effective weight of the weight-normed convolution) rounded to `dtype`, and a forward pre-hook on every nn.Linear
    and nn.Conv1d that rounds its input to `dtype`; everything else stays float64.  Its distance from the float64
    module is what rounding the GEMM operands alone costs (the spirit of the `quant=` hook of
    test_fused_layer_kernel_vs_oracle_and_unfused)."""
    module = copy.deepcopy(to64(module64))

    def rounded(x):
        return x.to(dtype).to(torch.float64)

    def hook(_, args):
        return (rounded(args[0]),) + tuple(args[1:])
    with torch.no_grad():
        for layer in module.modules():
            if isinstance(layer, (torch.nn.Linear, torch.nn.Conv1d)):
                _round_weight(layer, dtype)
                layer.register_forward_pre_hook(hook)
    return module


def roll_one(module, name):
    """The mutation a misplaced read amounts to: parameter `name` of `module` rolled by one element, in place."""
    parameter = dict(module.named_parameters())[name]
    with torch.no_grad():
        parameter.copy_(torch.roll(parameter.flatten(), 1).view_as(parameter))


def gain_name(model):
    for name, _ in model.named_parameters():
        if name.endswith(GAIN_NAMES):
            return name
    raise KeyError('no weight-norm gain in this model')


def mutation_classes(model):
    """{label: parameter name} of the 16 parameter classes (per layer: 9) a kernel can misplace, and the one
    exception ('k bias': softmax cancels it)."""
    body = {
        'projection LayerNorm weight': 'feature_projection.layer_norm.weight',
        'projection LayerNorm bias': 'feature_projection.layer_norm.bias',
        'projection bias': 'feature_projection.projection.bias',
        'positional convolution bias': 'encoder.pos_conv_embed.conv.bias',
        'positional convolution gain': gain_name(model),
        'encoder LayerNorm weight': 'encoder.layer_norm.weight',
        'encoder LayerNorm bias': 'encoder.layer_norm.bias',
    }
    for index in range(len(model.encoder.layers)):
        p = f'encoder.layers.{index}.'
        body.update({
            f'layer {index} q bias': p + 'attention.q_proj.bias',
            f'layer {index} v bias': p + 'attention.v_proj.bias',
            f'layer {index} out bias': p + 'attention.out_proj.bias',
            f'layer {index} ffn1 bias': p + 'feed_forward.intermediate_dense.bias',
            f'layer {index} ffn2 bias': p + 'feed_forward.output_dense.bias',
            f'layer {index} LayerNorm 1 weight': p + 'layer_norm.weight',
            f'layer {index} LayerNorm 1 bias': p + 'layer_norm.bias',
            f'layer {index} LayerNorm 2 weight': p + 'final_layer_norm.weight',
            f'layer {index} LayerNorm 2 bias': p + 'final_layer_norm.bias',
        })
    encoder = {
        'GroupNorm weight': 'feature_extractor.conv_layers.0.layer_norm.weight',
        'GroupNorm bias': 'feature_extractor.conv_layers.0.layer_norm.bias',
    }
    return body, encoder
