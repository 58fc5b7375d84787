"""Shared by tests/test_encoder_params_host.py and tests/test_gpu_encoder_params.py: PPG networks whose biases and
LayerNorm affines are loud, float64 references of them, and mutants of every per-channel parameter.

Five kernels exist only in the 16-bit modes (ppg_gemm32.hip, ppg_layer32.hip, ppg_ffn32x2.hip, ppg_head32.hip,
ppg_outconv.hip); each packs the biases, the LayerNorm affines and the positional rows into a tile layout of its
own.  With the parameters of ``ppgs_amd.weights.seeded_state_dict`` (biases in U(-0.1, 0.1), affines at 1 +- 0.1 and
0 +- 0.1) a 16-wide block of one of them read from the wrong offset moves the logits by about the 16-bit bound and the
posteriors by a fraction of their bar (tests/test_encoder_params_host.py::test_the_gap).  :func:`loud_state` keeps the
matrices and the position table of that checkpoint and draws every bias and affine an order of magnitude further from
0 and 1 -- they are applied in fp32 and are no MFMA operands, so the cost of the 16-bit formats stays where it was --
and the probe networks are TRUNCATED: behind a parameter of layer l every further layer normalises its fault away
again (5 layers deep, layer 0's norm1.weight fault is at the bound), so layer l is judged in the network of l + 1
layers, where it is the last one.

MUTANTS is the catalogue of faults a tile-layout error would make, each a function state -> state on the LAST layer
of the network it is given (or on the input / output layer, or the position table); the host test shows that each
moves the float64 logits by at least 4 x the 16-bit bound, the GPU test compares the kernels with float64.
"""
import numpy as np
import torch

import attention_probe as A
from oracle import ppg_oracle as O
from ppgs_amd import weights as W

GEOMETRY = A.GEOMETRY                # hidden -> input channels: (80, 256) and (768, 512)
DEPTHS = (1, 2, 3, 5)
SEED = 7
FRAMES = 300
# valid lengths of the probe batch: 0, 1 and the full length; on, before and behind 16-token boundaries (16, 32,
# 144, 288) and the 160-token boundary.  Items with an odd number of 16-token blocks (1, 15, 16, 33, 144, 161, 289,
# 300) put the window packed behind them at an odd block.
VALID = (0, 1, 15, 16, 17, 33, 144, 159, 160, 161, 289, 300)
# the items the mutants are judged on (the full window, and one that ends one frame behind the 160-token boundary):
# the effect on a part of the batch is a lower bound of the effect on all of it, at a sixth of the arithmetic
JUDGED = (VALID.index(300), VALID.index(161))
# T = 850: windows of 500 / 500 / 100 frames; the second window holds 500, 215, 116 and 51 valid frames
CHUNKED_FRAMES = 850
CHUNKED_VALID = (850, 565, 466, 401)
FP32_LOGITS_TOL = 2e-4               # the project's logits bound (test_gpu_parity.py::test_single_window_fp32) ...
FP32_LOGITS_SCALE = 4.4              # ... stated for logits of this magnitude
DTYPES = A.DTYPES

# The scales of loud_state().  Chosen on the CPU (tests/test_encoder_params_host.py prints the table): the smallest
# round figures at which every mutant of MUTANTS moves the float64 logits of the network that judges it by 4 x the
# 16-bit bound, while the logits stay finite and the format cost stays within 2 x of the seeded checkpoint's.
# Biases: the seeded U(-0.1, 0.1) x BIAS_SCALE.  A query bias reaches the logits through the softmax alone, against
# keys of magnitude about 1, so it has a scale of its own (as in tests/w2v2_params.py), and so has linear1.bias, which
# reaches them through the ReLU and 16 of linear2's 2048 columns.  Norm gains: U(1 - g, 1 + g); norm shifts: U(-s, s).
# At 10 / 10 / 10 / 0.5 / 1 (ten times the seeded biases) linear1.bias, norm1.weight and out_proj.bias blocks were at
# 2.6 .. 3.9 x in some networks and layer 0's query bias at 3.3 x.
BIAS_SCALE = 15.
QUERY_BIAS_SCALE = 40.
LINEAR1_BIAS_SCALE = 30.
NORM_GAIN = 0.75
NORM_SHIFT = 1.0


def loud_state(seed, input_channels, hidden_channels, num_layers):
    """seeded_state_dict(seed, ...) with every bias and every norm gain and shift replaced by loud values from a
    generator seeded with `seed`; matrices and `position.encoding` stay as they are."""
    state = W.seeded_state_dict(seed=seed, input_channels=input_channels, hidden_channels=hidden_channels,
                                num_layers=num_layers)
    generator = torch.Generator(device='cpu').manual_seed(seed + 1000003)
    loud = {}
    for key, value in state.items():
        def uniform():
            return 2. * torch.rand(value.shape, generator=generator) - 1.
        if 'norm' in key and key.endswith('weight'):
            loud[key] = 1. + NORM_GAIN * uniform()
        elif 'norm' in key:
            loud[key] = NORM_SHIFT * uniform()
        elif key.endswith('in_proj_bias'):
            bias = 0.1 * BIAS_SCALE * uniform()
            bias[:hidden_channels] *= QUERY_BIAS_SCALE / BIAS_SCALE
            loud[key] = bias
        elif key.endswith('linear1.bias'):
            loud[key] = 0.1 * LINEAR1_BIAS_SCALE * uniform()
        elif key.endswith('bias'):
            loud[key] = 0.1 * BIAS_SCALE * uniform()
        else:
            loud[key] = value
    return loud


def features(cin, batch, frames=FRAMES, seed=SEED):
    """(batch, cin, frames) fp16 N(0, 1)"""
    generator = torch.Generator(device='cpu').manual_seed(seed + 2)
    return torch.randn(batch, cin, frames, generator=generator).half()


def reference64(state, feats, lengths, causal, quant=None):
    """The oracle's float64 logits (B, 40, T), numpy; `quant` as in attention_probe.reference64."""
    return A.reference64(state, feats, lengths, causal, quant=quant)


def format_cost(state, feats, lengths, causal, precision, ref=None):
    """What the 16-bit format itself costs: max |float64 with every MFMA operand rounded to the format where the
    kernels round it - float64| inside the mask."""
    ref = reference64(state, feats, lengths, causal) if ref is None else ref
    rounded = reference64(state, feats, lengths, causal, quant=DTYPES[precision])
    return float((np.abs(rounded - ref) * A.inside(lengths, ref.shape[-1])).max())


bound16 = A.bound16


def bound32(ref):
    """The fp32 / fp16x2 bound: the project's logits bound, scaled to the magnitude of these logits."""
    return FP32_LOGITS_TOL * max(1., float(np.abs(ref).max()) / FP32_LOGITS_SCALE)


# ---- mutants ---------------------------------------------------------------------------------------------------------

def last_layer(state):
    return f'model.layers.{O.num_layers(state) - 1}.'


class Mutant:
    """One fault: `mutant(state)` returns the mutated copy of a state dict.  `where`: 'layer' (a parameter of the
    last layer: judged at every depth), 'input' (judged at depth 1), 'output' (judged at every depth) or 'chunked'
    (judged on the chunked batch at depth 1; this one is no function of the state alone: `hook(lengths)` gives the
    oracle's quant= argument that applies it)."""

    def __init__(self, name, where, key, change, hook=None, silent=False):
        self.name, self.where, self.key, self.change, self.hook, self.silent = name, where, key, change, hook, silent

    def __call__(self, state):
        state = dict(state)
        if self.change is not None:
            key = (last_layer(state) if self.where == 'layer' else '') + self.key
            state[key] = self.change(state[key].clone())
        return state

    def judged_at(self, depth):
        return depth == 1 if self.where in ('input', 'chunked') else True

    def __repr__(self):
        return self.name


def _copy_block(lo, width, source):
    """v[lo : lo + width] = v[source : source + width]"""
    def change(v):
        v[lo:lo + width] = v[source:source + width].clone()
        return v
    return change


def _last(width, hi=None):
    """the neighbouring block over the last block of `width` of v[:hi]"""
    def change(v):
        end = len(v) if hi is None else hi
        return _copy_block(end - width, width, end - 2 * width)(v)
    return change


def _first(width, lo=0):
    """the neighbouring block over the first block of `width` of v[lo:]"""
    return _copy_block(lo, width, lo + width)


def _shift_rows(table):
    """row t of the position table <- row t + 1"""
    return torch.roll(table, -1, dims=0)


def absolute_rows_hook(state, frames, lengths, window=1):
    """quant= hook of the oracle: the `window`-th window of a chunked batch adds the position rows at its ABSOLUTE
    frames (start .. start + Tc of the padded sequence) instead of rows 0 .. Tc.  ('x0' is the first stage the
    oracle calls per window, with the residual stream itself: changed in place.)"""
    table = state['position.encoding'].double()[:, 0]
    plan = O.plan_windows(frames, lengths)
    calls = [0]

    def hook(stage, x):
        if stage == 'x0':
            w = plan[calls[0]]
            if calls[0] == window:
                x.add_((table[w['start']:w['start'] + w['Tc']] - table[:w['Tc']])[None])
            calls[0] += 1
        return x
    return hook


def _catalogue():
    mutants = []
    for key in ('self_attn.out_proj.bias', 'norm1.weight', 'norm1.bias', 'linear1.bias', 'linear2.bias',
                'norm2.weight', 'norm2.bias'):
        mutants.append(Mutant(f'{key} last 16', 'layer', key, _last(16)))
        mutants.append(Mutant(f'{key} first 32', 'layer', key, _first(32)))
    for where, key in (('input', 'input_layer.bias'),):
        mutants.append(Mutant(f'{key} last 16', where, key, _last(16)))
        mutants.append(Mutant(f'{key} first 32', where, key, _first(32)))
    mutants.append(Mutant('output_layer.bias last 8', 'output', 'output_layer.bias', _last(8)))
    mutants.append(Mutant('output_layer.bias first 8', 'output', 'output_layer.bias', _first(8)))
    # in_proj_bias = [q; k; v], each third = [head 0; head 1]: blocks inside each head's half of the q and v thirds.
    # (the geometry is read off the vector: thirds of len / 3, halves of len / 6)
    for third, name in ((0, 'q'), (2, 'v'), (1, 'k')):
        for head in (0, 1):
            def last(v, third=third, head=head):
                d = len(v) // 6
                return _last(16, hi=(2 * third + head + 1) * d)(v)

            def first(v, third=third, head=head):
                d = len(v) // 6
                return _first(32, lo=(2 * third + head) * d)(v)
            # a k bias adds q . b_k to every score of a query's row: the softmax cancels it
            silent = name == 'k'
            mutants.append(Mutant(f'in_proj_bias {name} head {head} last 16', 'layer', 'self_attn.in_proj_bias', last,
                                  silent=silent))
            mutants.append(Mutant(f'in_proj_bias {name} head {head} first 32', 'layer', 'self_attn.in_proj_bias', first,
                                  silent=silent))
    mutants.append(Mutant('position.encoding rows shifted by one frame', 'input', 'position.encoding', _shift_rows))
    mutants.append(Mutant('position.encoding absolute rows in the second window', 'chunked', None, None,
                          hook=absolute_rows_hook))
    return {m.name: m for m in mutants}


MUTANTS = _catalogue()


# ---- the probe networks and their references, computed once ----------------------------------------------------------

class Net:
    """One probe network (hidden, depth, causal) on one batch: the loud state dict, the features, the float64
    logits and the format costs."""

    def __init__(self, hidden, depth, causal, valid=VALID, frames=FRAMES, state=None, feats=None):
        self.hidden, self.depth, self.causal = hidden, depth, bool(causal)
        self.valid, self.frames = tuple(valid), frames
        self.cin = GEOMETRY[hidden]
        self.state = loud_state(SEED, self.cin, hidden, depth) if state is None else state
        self.feats = features(self.cin, len(self.valid), frames) if feats is None else feats
        self.ref = reference64(self.state, self.feats, self.valid, self.causal)
        self.inside = A.inside(self.valid, frames)
        self._cost = {}

    def __repr__(self):
        return f'hidden {self.hidden} depth {self.depth} {"causal" if self.causal else "non-causal"}'

    def cost(self, precision):
        if precision not in self._cost:
            self._cost[precision] = format_cost(self.state, self.feats, self.valid, self.causal, precision, self.ref)
        return self._cost[precision]

    def bound(self, precision):
        return bound32(self.ref) if precision in ('fp32', 'fp16x2') else bound16(self.cost(precision))

    def error(self, logits):
        return float((np.abs(logits - self.ref) * self.inside).max())

    def effect(self, mutant, items=None):
        """max |reference64(mutant) - reference64| inside the mask, on `items` of the batch (default: all)."""
        items = list(range(len(self.valid))) if items is None else list(items)
        valid = [self.valid[i] for i in items]
        feats = self.feats[items]
        if mutant.hook is not None:
            mutated = reference64(self.state, feats, valid, self.causal,
                                  quant=mutant.hook(self.state, self.frames, valid))
        else:
            mutated = reference64(mutant(self.state), feats, valid, self.causal)
        return float((np.abs(mutated - self.ref[items]) * self.inside[items]).max())


class Lab:
    def __init__(self):
        self._nets = {}

    def net(self, hidden, depth, causal, valid=VALID, frames=FRAMES):
        key = (hidden, depth, bool(causal), tuple(valid), frames)
        if key not in self._nets:
            self._nets[key] = Net(hidden, depth, causal, valid, frames)
        return self._nets[key]


def tiled(net, times):
    """The probe batch `times` over: (feats, valid, reference)."""
    return net.feats.repeat(times, 1, 1), list(net.valid) * times, np.tile(net.ref, (times, 1, 1))
