"""Shared by tests/test_geometry_probe_host.py and tests/test_gpu_geometry.py: the model geometries `ppg_engine_create`
accepts beyond the two shipped ones, seeded checkpoints of them, float64 references with the geometry's head count,
and the faults a kernel that mishandles one axis of the geometry would make.

The engine takes input channels, hidden width, depth, F, output channels and the length of the position table from the
checkpoint, and the head count from the caller; packing, planner and launchers branch on every one of them (padded
K-groups, hidden chunks per split, feature passes, LDS budgets, the 48-row output tile).  The rule the two test files
establish: a geometry that `Engine(...)` constructs computes the reference's network within the project's bounds in
every precision and launch regime, and a geometry the kernels cannot do is refused at construction with a message
that names the field.

Conventions are the project's: attention_probe.inside / DTYPES for the mask and the format cost, encoder_params.bound32
/ bound16 for the bounds, encoder_params.VALID / FRAMES as the base batch and encoder_params.tiled to replicate it.
"""
import collections

import numpy as np
import torch

import attention_probe as A
import encoder_params as P
from oracle import ppg_oracle as O
from ppgs_amd import weights as W

SEED = 11
PRECISIONS = ('fp32', 'fp16x2', 'fp16', 'bf16')

Geometry = collections.namedtuple('Geometry', 'cin hidden heads layers ffn out max_len')

SHIPPED = {256: Geometry(80, 256, 2, 2, 2048, 40, 5000), 512: Geometry(768, 512, 2, 2, 2048, 40, 5000)}


class Row:
    """One geometry of the catalogue.  `axis`: the field it moves away from the shipped geometry ('cin', 'heads',
    'ffn', 'out', 'layers', 'max_len'); `why`: what that value reaches; `big`: also run in the whole-tile layer32 /
    head32 regime (the batch 7 x), for the rows whose packing those kernels hold images of; `refused`: the field the
    construction error must name (None: accepted), `refused_in`: the precisions that refuse it (default: all)."""

    def __init__(self, axis, why, big=False, refused=None, refused_in=PRECISIONS, **changes):
        hidden = changes.pop('hidden', 256)
        self.geometry = SHIPPED[hidden]._replace(**changes)
        self.axis, self.why, self.big, self.refused = axis, why, big, refused
        self.refused_in = tuple(refused_in) if refused else ()
        self.name = f'h{hidden}-' + '-'.join(f'{k}{v}' for k, v in changes.items())

    def accepted(self, precision):
        g = self.geometry
        if precision == 'fp16x2' and (g.hidden, g.hidden // g.heads) not in ((256, 128), (512, 256)):
            return False           # the mode covers these two head shapes (test_gpu_parity.py::test_fp16x2_mode_at_hidden_512)
        return precision not in self.refused_in

    def __repr__(self):
        return self.name


def _catalogue():
    """Each row changes one or two axes of a shipped geometry; depth is 2 unless stated.

    input channels (hidden 256; Cp = the channels rounded up to a K-group of 32 16-bit or 16 fp32 elements):
      1    one K-group that is all padding but one channel
      16   an odd count of fp32 K-groups per 5 taps (5, padded to 6)
      65   the lower end of head32's class Cp == 96, 31 pad channels
      96   the upper end of it, no pad channel
      97   the first count outside it (16-bit Cp 128; fp32 Cp 112, 35 groups padded to 36)
      128, 144   the reference's encodec and bottleneck widths
      100 at hidden 512   padding at the other hidden width
    heads: (80, 256, 1) runs attention at d 256 with hidden 256, (768, 512, 4) at d 128 with hidden 512; 1 and 4 heads
      deal the attention items into 8 and 2 XCD lanes instead of 4.  fp16x2 refuses both (its two head shapes).
    F at hidden 256:
      64    one hidden chunk in the 16-bit modes
      192   F % 128 != 0: no layer32; an odd F / 64
      640   10 chunks of 64: neither 4 nor 8 hidden splits divide them
      1152  18 chunks, and F / 128 = 9 is odd: layer32 without sub-tiles
      5888  the largest F at which the fused FFN holds the out-projection's parameters in LDS as well
      6656  the largest F of layer32 and of the fused FFN kernel at all
      6784  no route can run it: refused
    F at hidden 512:
      320   F % 256 != 0: the two-GEMM FFN (fp16x2's only route there) cannot write its last 64 features: refused in
            fp16x2, computed by the fused kernel in the other modes
      3584, 3840   either side of the fused out-projection's LDS limit at hidden 512
      5120  the largest F of the fused FFN kernel at hidden 512, above layer32's own limit there (4864): the 16-bit
            modes stay on the token-split kernels at every batch size
    output channels: 1 (a softmax over one channel), 41 (one more than shipped), 48 (the whole padded tile) at hidden
      256; 48 at hidden 512 -- the 48-row padding, the softmax width, the 1 / out fill, ppg_outconv.hip against
      EPI_OUTCONV.
    depth: 16 = PPG_MAX_LAYERS at F 256; 17 is refused.
    table: 500 rows = chunk_length must work (a full window uses rows 0 .. 499 exactly); 499 and 300 are refused (a
      500-frame window would read behind the table).
    """
    rows = [
        Row('cin', 'one channel: a K-group of padding', cin=1),
        Row('cin', 'odd count of fp32 K-groups', cin=16),
        Row('cin', 'lower end of the Cp == 96 class of head32', big=True, cin=65),
        Row('cin', 'upper end of the Cp == 96 class, no pad channel', big=True, cin=96),
        Row('cin', 'first count outside the Cp == 96 class', cin=97),
        Row('cin', 'encodec width', cin=128),
        Row('cin', 'bottleneck width', cin=144),
        Row('cin', 'padding at hidden 512', hidden=512, cin=100),
        Row('heads', 'd 256 at hidden 256, 8 XCD lanes', big=True, heads=1),
        Row('heads', 'd 128 at hidden 512, 2 XCD lanes', hidden=512, heads=4),
        Row('ffn', 'one hidden chunk', ffn=64),
        Row('ffn', 'F % 128, odd F / 64', ffn=192),
        Row('ffn', '10 chunks: 4 and 8 splits do not divide', ffn=640),
        Row('ffn', '18 chunks, odd F / 128', ffn=1152),
        Row('ffn', 'largest F with the out-projection fused into the FFN kernel', big=True, ffn=5888),
        Row('ffn', 'largest F of layer32 and of the fused FFN kernel', big=True, ffn=6656),
        Row('ffn', 'no route fits it in LDS', refused='ffn_channels', ffn=6784),
        Row('ffn', 'F % 256 on the two-GEMM route', hidden=512, ffn=320, refused='ffn_channels', refused_in=('fp16x2',)),
        Row('ffn', 'largest F with the out-projection fused at hidden 512', hidden=512, ffn=3584),
        Row('ffn', 'first F without it at hidden 512', hidden=512, ffn=3840),
        Row('ffn', 'largest F at hidden 512, above the limit of layer32 there', hidden=512, ffn=5120),
        Row('out', 'softmax over one channel', out=1),
        Row('out', 'one more row than shipped', out=41),
        Row('out', 'the whole 48-row tile', big=True, out=48),
        Row('out', 'the whole 48-row tile at hidden 512', hidden=512, out=48),
        Row('layers', 'PPG_MAX_LAYERS', big=True, layers=16, ffn=256),
        Row('layers', 'one layer too many', refused='num_layers', layers=17, ffn=256),
        Row('max_len', 'a table of exactly chunk_length rows', max_len=500),
        Row('max_len', 'one row short of a full window', refused='max_positions', max_len=499),
        Row('max_len', '300 rows: a 400-frame window reads 100 rows behind it', refused='max_positions', max_len=300),
    ]
    return {row.name: row for row in rows}


CATALOGUE = _catalogue()
ACCEPTED = [row for row in CATALOGUE.values() if row.refused is None or len(row.refused_in) < len(PRECISIONS)]
REFUSED = [(row, precision) for row in CATALOGUE.values() for precision in row.refused_in]


def state(geometry, seed=SEED):
    """The seeded checkpoint of `geometry` (ppgs_amd.weights.seeded_state_dict)."""
    g = geometry
    return W.seeded_state_dict(seed=seed, input_channels=g.cin, hidden_channels=g.hidden, num_layers=g.layers,
                               output_channels=g.out, ffn_channels=g.ffn, max_len=g.max_len)


def reference64(state_dict, feats, valid, causal, heads, quant=None):
    """The oracle's forward in float64 with `heads` heads -> logits (B, out, T) float64 numpy; `quant` as in
    attention_probe.reference64."""
    return O.from_features(
        A.state64(state_dict), feats.double(), torch.as_tensor(list(valid)), softmax=False, is_causal=causal,
        quant=A._rounding(quant), dtype=torch.float64, heads=heads).numpy()


# ---- the faults of one axis, as functions state -> state (or a misread head count) -------------------------------

def drop_chunk(state_dict, layer):
    """The last 64 hidden features of `layer`'s FFN never summed: their linear1 rows and biases zeroed (ReLU(0) = 0)."""
    mutated = dict(state_dict)
    for key in (f'model.layers.{layer}.linear1.weight', f'model.layers.{layer}.linear1.bias'):
        value = state_dict[key].clone()
        value[-64:] = 0
        mutated[key] = value
    return mutated


def drop_last_channel(state_dict):
    mutated = dict(state_dict)
    weight = state_dict['input_layer.weight'].clone()
    weight[:, -1] = 0
    mutated['input_layer.weight'] = weight
    return mutated


def swap_last_output_rows(state_dict):
    """Output row out - 1 <-> out - 2 (a single row has no neighbour: it is zeroed, weight and bias)."""
    mutated = dict(state_dict)
    for key in ('output_layer.weight', 'output_layer.bias'):
        value = state_dict[key].clone()
        if len(value) > 1:
            value[[-1, -2]] = value[[-2, -1]]
        else:
            value[-1] = 0
        mutated[key] = value
    return mutated


def shift_position_rows(state_dict):
    mutated = dict(state_dict)
    mutated['position.encoding'] = torch.roll(state_dict['position.encoding'], -1, dims=0)
    return mutated


def misread_heads(heads):
    """1 <-> 2, 4 -> 2"""
    return {1: 2, 2: 1, 4: 2}[heads]


# ---- a row on a batch, its reference and format costs, computed once ----------------------------------------------

class Case:
    """One catalogue row on one batch: the checkpoint, the features, the float64 logits and the format costs."""

    def __init__(self, row, causal=False, valid=P.VALID, frames=P.FRAMES):
        self.row, self.geometry, self.causal = row, row.geometry, bool(causal)
        self.valid, self.frames = tuple(valid), frames
        self.state = state(self.geometry)
        self.feats = P.features(self.geometry.cin, len(self.valid), frames, seed=SEED)
        self.ref = reference64(self.state, self.feats, self.valid, self.causal, self.geometry.heads)
        self.inside = A.inside(self.valid, frames)
        self._cost = {}

    def __repr__(self):
        return f'{self.row} {"causal" if self.causal else "non-causal"}'

    def cost(self, precision):
        """max |float64 with every MFMA operand rounded to the format - float64| inside the mask"""
        if precision not in self._cost:
            rounded = reference64(self.state, self.feats, self.valid, self.causal, self.geometry.heads,
                                  quant=A.DTYPES[precision])
            self._cost[precision] = float((np.abs(rounded - self.ref) * self.inside).max())
        return self._cost[precision]

    def bound(self, precision):
        """fp32 / fp16x2: the project's logits bound.  fp16 / bf16: 1.6 x the format's own cost on this geometry and
        batch, and never below the fp32 bound (cin 1 and F 64 cost the formats less than that)."""
        if precision in ('fp32', 'fp16x2'):
            return P.bound32(self.ref)
        return max(P.bound16(self.cost(precision)), P.bound32(self.ref))

    def effect(self, mutated_state=None, heads=None):
        """max |reference64(the fault) - reference64| inside the mask"""
        mutated = reference64(self.state if mutated_state is None else mutated_state, self.feats, self.valid,
                              self.causal, self.geometry.heads if heads is None else heads)
        return float((np.abs(mutated - self.ref) * self.inside).max())


class Lab:
    def __init__(self):
        self._cases = {}

    def case(self, row, causal=False, valid=P.VALID, frames=P.FRAMES):
        key = (row.name, bool(causal), tuple(valid), frames)
        if key not in self._cases:
            self._cases[key] = Case(row, causal, valid, frames)
        return self._cases[key]

    def release(self):
        self._cases.clear()


tiled = P.tiled
