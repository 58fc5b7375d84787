"""What stands behind tests/test_gpu_geometry.py, checked without a GPU:

* the oracle is right at every geometry of the catalogue (tests/test_oracle_golden.py pins it against the reference's
  modules at the shipped geometry only): its float64 forward against torch.nn.TransformerEncoder in float64 from the
  same state dict, with the same two convolutions, mask and position rows around it, causal and not, ragged batch;
* the probe would notice: the fault a kernel would make on each axis (a dropped hidden chunk, a dropped input channel,
  a misread head count, a misplaced output row, position rows one off) moves the float64 logits by at least 4 x the
  bf16 bound of that geometry;
* seeded_state_dict's new keywords give the shapes asked for and leave the default draws bit for bit;
* the refusals ppg_engine_create makes before it touches a device.

The batch here is small (5 items of 100 frames, valid 100, 61, 33, 16 and 1): the properties are those of the network,
not of the batch, and every row is checked.
"""
import ctypes

import numpy as np
import pytest
import torch

import encoder_params as P
import geometry_probe as G
from oracle import ppg_oracle as O
from ppgs_amd import engine as E
from ppgs_amd import weights as W

FRAMES = 100
VALID = (100, 61, 33, 16, 1)
FACTOR = 4.0


@pytest.fixture(scope='module')
def lab():
    lab = G.Lab()
    yield lab
    lab.release()


def torch_forward(state, geometry, feats, valid, causal):
    """The network out of torch.nn modules in float64: Conv1d, the position rows, TransformerEncoder (post-norm, ReLU,
    no dropout), Conv1d; masked before the encoder's position rows and behind the output convolution."""
    g = geometry
    layer = torch.nn.TransformerEncoderLayer(g.hidden, g.heads, g.ffn, dropout=0.)
    encoder = torch.nn.TransformerEncoder(layer, g.layers, enable_nested_tensor=False).double().eval()
    encoder.load_state_dict({key[len('model.'):]: value.double() for key, value in state.items()
                             if key.startswith('model.')})
    frames = feats.shape[-1]
    mask = torch.arange(frames)[None] < torch.as_tensor(valid)[:, None]
    with torch.inference_mode():
        x = torch.nn.functional.conv1d(feats.double(), state['input_layer.weight'].double(),
                                       state['input_layer.bias'].double(), padding='same') * mask[:, None]
        x = x.permute(2, 0, 1) + state['position.encoding'].double()[:frames]
        attn_mask = torch.nn.Transformer.generate_square_subsequent_mask(frames).double() if causal else None
        padding = torch.zeros(mask.shape, dtype=torch.float64).masked_fill(~mask, float('-inf'))
        if g.layers:
            x = encoder(x, mask=attn_mask, src_key_padding_mask=padding)
        y = torch.nn.functional.conv1d(x.permute(1, 2, 0), state['output_layer.weight'].double(),
                                       state['output_layer.bias'].double(), padding='same')
    return (y * mask[:, None]).numpy()


@pytest.mark.parametrize('causal', [False, True])
@pytest.mark.parametrize('row', list(G.CATALOGUE.values()), ids=repr)
def test_oracle_matches_torch_modules_at_every_geometry(row, causal):
    state = G.state(row.geometry)
    feats = P.features(row.geometry.cin, len(VALID), FRAMES, seed=G.SEED)
    ours = G.reference64(state, feats, VALID, causal, row.geometry.heads)
    theirs = torch_forward(state, row.geometry, feats, VALID, causal)
    difference = float((np.abs(ours - theirs) * G.A.inside(VALID, FRAMES)).max())
    print(f'{row} causal={causal}: oracle - torch modules {difference:.2e}')
    assert ours.shape == (len(VALID), row.geometry.out, FRAMES)
    assert difference < 1e-10


def shallower(row, layers):
    """The same geometry at `layers` layers (the rule of encoder_params.py: behind a fault every further layer
    normalises part of it away, so a layer is judged in the network where it is the last one)."""
    twin = G.Row(row.axis, row.why)
    twin.geometry = row.geometry._replace(layers=layers)
    twin.name = f'{row.name}-judged-at-{layers}'
    return twin


def faults_of(row, case):
    """(name, effect) of every fault on the row's own axis."""
    g = case.geometry
    if row.axis == 'ffn':
        return [(f'chunk dropped in layer {l}', case.effect(G.drop_chunk(case.state, l))) for l in range(g.layers)]
    if row.axis == 'cin':
        return [('last input channel dropped', case.effect(G.drop_last_channel(case.state)))]
    if row.axis == 'heads':
        return [(f'{g.heads} heads read as {G.misread_heads(g.heads)}', case.effect(heads=G.misread_heads(g.heads)))]
    if row.axis == 'out':
        return [('last output row misplaced', case.effect(G.swap_last_output_rows(case.state)))]
    if row.axis == 'max_len':
        return [('position rows one off', case.effect(G.shift_position_rows(case.state)))]
    raise AssertionError(row.axis)


@pytest.mark.parametrize('row', [r for r in G.ACCEPTED if r.axis != 'layers'], ids=repr)
def test_the_probe_would_notice(lab, row):
    case = lab.case(row, False, VALID, FRAMES)
    bound = P.bound16(case.cost('bf16'))
    for name, effect in faults_of(row, case):
        print(f'{row}: {name}: {effect:.3f} = {effect / bound:.1f} x the bf16 bound {bound:.4f}')
        assert effect >= FACTOR * bound, (row, name)


def test_the_probe_would_notice_at_full_depth(lab):
    """16 layers: a chunk dropped in layer l is judged in the network of l + 1 layers, where it is the last one (what
    the 15 layers behind layer 0 leave of its fault is not the measure of a probe of layer 0); the network of all 16
    judges its last layer."""
    row = G.CATALOGUE['h256-layers16-ffn256']
    for layers in (1, 2, 3, 5, 8, 12, 16):
        case = lab.case(shallower(row, layers), False, VALID, FRAMES)
        bound = P.bound16(case.cost('bf16'))
        effect = case.effect(G.drop_chunk(case.state, layers - 1))
        print(f'{row}: chunk dropped in layer {layers - 1} of {layers}: {effect:.3f} = {effect / bound:.1f} x {bound:.4f}')
        assert effect >= FACTOR * bound, layers


def test_every_axis_fault_on_the_shipped_geometries(lab):
    """The five faults on the two shipped geometries themselves (depth 2), as a baseline for the table above."""
    for hidden in (256, 512):
        row = G.Row('ffn', 'shipped', hidden=hidden)
        case = lab.case(row, False, VALID, FRAMES)
        bound = P.bound16(case.cost('bf16'))
        effects = dict(faults_of(row, case))
        for axis in ('cin', 'heads', 'out', 'max_len'):
            row.axis = axis
            effects.update(faults_of(row, case))
        for name, effect in effects.items():
            print(f'shipped hidden {hidden}: {name}: {effect:.3f} = {effect / bound:.1f} x {bound:.4f}')
            assert effect >= FACTOR * bound, (hidden, name)


def test_seeded_state_dict_keywords():
    default = W.seeded_state_dict(seed=3)
    spelled = W.seeded_state_dict(seed=3, output_channels=40, ffn_channels=2048, max_len=5000)
    assert list(default) == list(spelled)
    assert all(torch.equal(default[key], spelled[key]) for key in default)
    state = W.seeded_state_dict(seed=3, input_channels=7, hidden_channels=512, num_layers=3, output_channels=41,
                                ffn_channels=320, max_len=500)
    expected = W.state_dict_shapes(input_channels=7, hidden_channels=512, num_layers=3, output_channels=41,
                                   ffn_channels=320, max_len=500)
    assert {key: tuple(value.shape) for key, value in state.items()} == expected
    assert state['position.encoding'].shape == (500, 1, 512)
    assert state['model.layers.2.linear1.weight'].shape == (320, 512)
    assert state['model.layers.2.linear2.weight'].shape == (512, 320)
    assert state['output_layer.weight'].shape == (41, 512, 5) and state['output_layer.bias'].shape == (41,)
    assert torch.equal(state['position.encoding'], W.positional_encoding(512, 5000)[:500])
    for row in G.CATALOGUE.values():
        g = row.geometry
        shapes = {key: tuple(value.shape) for key, value in G.state(g).items()}
        assert shapes == W.state_dict_shapes(g.cin, g.hidden, g.layers, g.out, 5, g.ffn, g.max_len)


def create(geometry, precision):
    """ppg_engine_create through the C ABI with no weights behind the pointers: (code, message).  Geometry checks come
    before the device is used and before a weight is read, so a refusal needs neither -- an ACCEPTED geometry may only
    be passed where there is no device to go on to (the callers see to that)."""
    lib = E.library()
    g = geometry
    cfg = E.PpgConfig(input_channels=g.cin, hidden_channels=g.hidden, num_layers=g.layers, ffn_channels=g.ffn,
                      output_channels=g.out, kernel_size=5, heads=g.heads, is_causal=0, max_positions=g.max_len,
                      chunk_length=500, chunk_overlap=50, precision=E.PRECISIONS[precision])
    handle = ctypes.c_void_p()
    code = lib.ppg_engine_create(ctypes.byref(cfg), ctypes.byref(E.PpgWeights()), 0, ctypes.byref(handle))
    assert code != 0
    return code, lib.ppg_last_error().decode()


@pytest.mark.parametrize('row,precision', G.REFUSED, ids=lambda v: str(v))
def test_refusals_need_no_device(row, precision):
    code, message = create(row.geometry, precision)
    print(f'{row} {precision}: {message}')
    assert code == -1 and row.refused in message
    limit = {'h256-ffn6784': '6656', 'h256-layers17-ffn256': '16', 'h256-max_len499': '500', 'h256-max_len300': '500',
             'h512-ffn320': '256'}[row.name]
    assert limit in message


@pytest.mark.parametrize('row', G.ACCEPTED, ids=repr)
def test_accepted_rows_pass_the_geometry_checks(row):
    """Without a device an accepted geometry gets as far as the device: the error is the device's, not the geometry's.
    (With a device the call would go on to read weights: there tests/test_gpu_geometry.py constructs every one of
    these for real.)"""
    if torch.cuda.is_available():
        return
    for precision in G.PRECISIONS:
        if row.accepted(precision):
            code, message = create(row.geometry, precision)
            assert code != -1, (row, precision, message)


def test_hidden_512_limit_and_environment_switch(monkeypatch):
    """F above the fused kernel's LDS limit at hidden 512 (5120) is refused, except where the FFN runs as two GEMMs
    (fp16x2), which in turn needs whole passes of 256; PPGS_AMD_FFN_UNFUSED selects that route for every mode and
    refuses the same F."""
    wide = G.SHIPPED[512]
    code, message = create(wide._replace(ffn=5184), 'bf16')
    assert code == -1 and 'ffn_channels' in message and '5120' in message
    if not torch.cuda.is_available():
        assert create(wide._replace(ffn=5120), 'bf16')[0] != -1
    monkeypatch.setenv('PPGS_AMD_FFN_UNFUSED', '1')
    code, message = create(G.SHIPPED[256]._replace(ffn=320), 'bf16')
    assert code == -1 and 'ffn_channels' in message and 'PPGS_AMD_FFN_UNFUSED' in message
