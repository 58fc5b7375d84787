"""The loud probe networks of tests/encoder_params.py, checked on the CPU in float64: that they are a probe at all.

The gap they close (test_the_gap prints it).  The kernels that exist only in the 16-bit modes are checked end to end
on ``seeded_state_dict``, posteriors against 4e-3 (bf16) and 1e-3 (fp16).  On that checkpoint, 5 layers deep, copying
one block of a last-layer parameter over its neighbour -- what a wrong tile offset does -- moves the posteriors by
(seed 7, 3 items x 75 frames of lengths 75, 40 and 17; hidden 256 / 512)

    linear1.bias       1.6e-3 .. 1.9e-3 / 1.1e-3 .. 1.5e-3      out_proj.bias      3.0e-3 .. 6.5e-3 / 2.8e-3 .. 3.4e-3
    linear2.bias       2.4e-3 .. 3.7e-3 / 3.0e-3 .. 3.6e-3      in_proj_bias, v    3.3e-3 .. 5.5e-3 / 2.1e-3 .. 3.0e-3
    in_proj_bias, q    7.7e-5 .. 1.7e-4 / 7.2e-5 .. 1.9e-4      norm affines       5.2e-3 .. 2.4e-2
    output_layer.bias  5.1e-3 .. 1.9e-2

11 (hidden 256) and 14 (hidden 512) of the 24 are under the bar of bf16, the engine's default precision, 4 of them under
the fp16 bar too; the rest is 1.1 .. 6 x the bf16 bar, with nothing to spare for a fault half the size.

What makes the loud networks a probe (test_mutant_strength prints the table): every mutant of encoder_params.MUTANTS
moves the float64 logits of the network that judges it -- the one in which its layer is the last -- by at least 4 x
the 16-bit bound of the GPU test (1.6 x the format cost, bf16 and fp16) and 4 x the fp32 bound.  4 is a condition:
the GPU test still fails for a fault half the size of the modelled one with 2 x to spare over summation-order noise.
The mutants are judged on two items of the probe batch (encoder_params.JUDGED); the bound is that of the whole batch,
so the figures are lower bounds.

Smallest .. largest ratio effect / largest bound over the 16 networks (hidden 256 / 512, depth 1, 2, 3, 5, causal or
not; |logit| <= 4.7, bf16 format cost 0.015 .. 0.020, fp16 0.0019 .. 0.0025, fp32 oracle 2e-6 from float64):

    out_proj.bias    4.2 .. 15      norm1.weight   4.1 .. 18      norm1.bias    7.8 .. 20      linear1.bias   4.3 .. 11
    linear2.bias     6.3 .. 23      norm2.weight   8.2 .. 35      norm2.bias     11 .. 35      in_proj_bias v 4.9 .. 16
    input_layer.bias  14 .. 20      output_layer.bias 43 .. 100   in_proj_bias q, layer 0: 7.8 .. 22
    position rows shifted by one frame 11 .. 13; absolute rows in the second window of a chunked item 45 .. 50

The class that does not reach 4 x: the QUERY bias (`in_proj_bias`, q third) of layers 1 and deeper.  A query bias
reaches the logits only through the softmax, as b_q . k_j, and behind layer 0 the keys of a network with two heads
and near-uniform attention differ little from token to token (the spread of x over the tokens halves per layer), so
the bias moves every score of a row alike.  At QUERY_BIAS_SCALE 40 its ratios are 0.2 .. 3.3 at depth 2, 0.0 .. 1.0 at
depth 3 and 0.0 at depth 5.  Swept on hidden 256: at 160 the depth-2 ratios are 2.2 .. 7.3 but the bf16 format cost
is 0.032 -- 1.8 x the seeded one, which would halve every other ratio -- and at 640 (cost 0.11, past 2 x the seeded
cost) they fall again; at depth 5 the ratio is 0.0 .. 0.1 at every scale.  They are printed, not asserted.  Layer
0's query bias, which meets the position rows, clears 4 x and is judged at depth 1.  The KEY bias has exactly no
effect (q . b_k is the same for every key of a row): test_mutant_strength asserts that, as a note for the reader.

Soundness (test_soundness): loud_state is deterministic and changes biases and norm affines only; the fp32 oracle is
within 1e-5 x max |logit| of float64; no logit is non-finite; the format cost of every loud network is at most 2 x
that of the seeded network of the same shape (same features, the judged items).
"""
import numpy as np
import pytest
import torch

import encoder_params as P
from oracle import ppg_oracle as O
from ppgs_amd import weights as W
from test_gpu_parity import BF16_TOL, FP16_TOL

FACTOR = 4.
NETWORKS = [(hidden, depth, causal) for hidden in P.GEOMETRY for depth in P.DEPTHS for causal in (False, True)]


@pytest.fixture(scope='module')
def lab():
    return P.Lab()


def short_of_the_factor(mutant, depth):
    """The class reported in the module docstring: the query bias behind layer 0."""
    return ' q head' in mutant.name and depth > 1


def test_catalogue():
    """Two blocks of every parameter vector: the last 16 and the first 32 (output bias: 8 and 8, 40 is no tile
    multiple), each overwritten by its neighbour; q and v thirds of in_proj_bias per head; the position rows."""
    state = P.loud_state(P.SEED, 80, 256, 2)
    vectors = {key[len('model.layers.1.'):] for key, value in state.items()
               if key.startswith('model.layers.1.') and value.dim() == 1}
    covered = {m.key for m in P.MUTANTS.values() if m.where == 'layer'}
    assert covered == vectors
    assert {m.key for m in P.MUTANTS.values() if m.where in ('input', 'output')} == \
        {'input_layer.bias', 'output_layer.bias', 'position.encoding'}
    for mutant in P.MUTANTS.values():
        if mutant.change is None:
            continue
        mutated = mutant(state)
        changed = [key for key in state if not torch.equal(state[key], mutated[key])]
        assert len(changed) == 1 and changed[0].endswith(mutant.key), mutant
        if mutant.key == 'position.encoding':
            assert torch.equal(mutated[changed[0]][:-1], state[changed[0]][1:])
            continue
        where = torch.nonzero(state[changed[0]] != mutated[changed[0]]).flatten()
        width = int(mutant.name.split()[-1])
        lo = int(where.min()) // width * width
        assert int(where.max()) < lo + width, mutant                 # one aligned block
        source = lo + width if 'first' in mutant.name else lo - width
        assert torch.equal(mutated[changed[0]][lo:lo + width], state[changed[0]][source:source + width]), mutant
    d = 128
    blocks = {name: int(torch.nonzero(state['model.layers.1.self_attn.in_proj_bias'] !=
                                       m(state)['model.layers.1.self_attn.in_proj_bias']).min()) // 16 * 16
              for name, m in P.MUTANTS.items() if 'in_proj_bias' in name}
    assert blocks['in_proj_bias q head 0 last 16'] == d - 16 and blocks['in_proj_bias q head 1 first 32'] == d
    assert blocks['in_proj_bias k head 1 last 16'] == 4 * d - 16
    assert blocks['in_proj_bias v head 0 first 32'] == 4 * d and blocks['in_proj_bias v head 1 last 16'] == 6 * d - 16


def test_probe_batch():
    assert len(P.VALID) <= 24 and {0, 1, P.FRAMES} <= set(P.VALID)
    assert {15, 16, 17} <= set(P.VALID) and {159, 160, 161} <= set(P.VALID)
    windows = O.plan_windows(P.CHUNKED_FRAMES, P.CHUNKED_VALID)
    assert [w['Tc'] for w in windows] == [500, 500, 100]
    assert windows[1]['clens'] == [500, 215, 116, 51]


@pytest.mark.parametrize('hidden,depth,causal', NETWORKS)
def test_mutant_strength(lab, hidden, depth, causal):
    net = lab.net(hidden, depth, causal)
    bounds = {precision: net.bound(precision) for precision in ('bf16', 'fp16', 'fp32')}
    print(f'\n{net}: |logit| <= {np.abs(net.ref).max():.2f}; format cost bf16 {net.cost("bf16"):.4f} fp16 '
          f'{net.cost("fp16"):.5f}; bounds bf16 {bounds["bf16"]:.4f} fp16 {bounds["fp16"]:.5f} fp32 {bounds["fp32"]:.1e}')
    weak = []
    for mutant in P.MUTANTS.values():
        if mutant.where == 'chunked' or not mutant.judged_at(depth):
            continue
        effect = net.effect(mutant, P.JUDGED)
        if mutant.silent:
            assert effect < 1e-9 * np.abs(net.ref).max(), (mutant, effect)
            continue
        ratio = effect / max(bounds.values())
        note = '   (the reported class)' if short_of_the_factor(mutant, depth) else ''
        print(f'    {mutant.name:46s} {effect:.4f} = {ratio:5.1f} x the largest bound{note}')
        if not short_of_the_factor(mutant, depth) and ratio < FACTOR:
            weak.append((mutant.name, round(ratio, 2)))
    assert not weak, (str(net), weak)


@pytest.mark.parametrize('causal', [False, True])
def test_position_rows_of_a_chunked_batch(lab, causal):
    """T = 850: the second window with the position rows of its absolute frames (400 .. 900 of the padded sequence)
    in place of rows 0 .. 500."""
    net = lab.net(256, 1, causal, P.CHUNKED_VALID, P.CHUNKED_FRAMES)
    mutant = P.MUTANTS['position.encoding absolute rows in the second window']
    bound = max(net.bound(precision) for precision in ('bf16', 'fp16', 'fp32'))
    effect = net.effect(mutant)
    print(f'\n{net} chunked: {mutant.name}: {effect:.3f} = {effect / bound:.1f} x the largest bound {bound:.4f}')
    assert effect >= FACTOR * bound
    # ... and only in the frames the second window contributes (50 .. 450 of it = frames 400 .. 800)
    mutated = P.reference64(net.state, net.feats, net.valid, causal,
                            quant=mutant.hook(net.state, net.frames, net.valid))
    moved = np.abs(mutated - net.ref).max(axis=(0, 1))
    assert moved[:400].max() < 1e-9 and moved[800:].max() < 1e-9 and moved[400:800].min() > 0


@pytest.mark.parametrize('hidden', list(P.GEOMETRY))
def test_the_gap(hidden):
    """On the seeded checkpoint, 5 layers, posteriors (seed 7, 3 items x 75 frames of lengths 75, 40 and 17): the
    last layer's block mutants against the bars of test_gpu_parity.py."""
    cin = P.GEOMETRY[hidden]
    state = P.A.state64(W.seeded_state_dict(seed=P.SEED, input_channels=cin, hidden_channels=hidden, num_layers=5))
    lengths = torch.tensor([75, 40, 17])
    feats = P.features(cin, 3, 75).double()

    def posteriors(s):
        return O.from_features(s, feats, lengths, softmax=True, dtype=torch.float64).numpy()
    ref = posteriors(state)
    inside = P.A.inside(lengths.tolist(), 75)
    print()
    moved = {}
    for mutant in P.MUTANTS.values():
        if mutant.where in ('layer', 'output') and not mutant.silent:
            moved[mutant.name] = float((np.abs(posteriors(mutant(state)) - ref) * inside).max())
            print(f'    hidden {hidden} seeded, 5 layers: {mutant.name:46s} moves the posteriors by {moved[mutant.name]:.1e}')
    under_bf16 = [name for name, value in moved.items() if value < BF16_TOL]
    unseen = [name for name, value in moved.items() if value < min(BF16_TOL, FP16_TOL)]
    print(f'    of {len(moved)}: under the bf16 bar {BF16_TOL}: {len(under_bf16)}, under the fp16 bar {FP16_TOL} too: {len(unseen)}')
    assert unseen and len(under_bf16) > len(unseen)


def test_loud_state_is_deterministic_and_keeps_the_matrices():
    a, b = P.loud_state(3, 80, 256, 2), P.loud_state(3, 80, 256, 2)
    seeded = W.seeded_state_dict(seed=3, input_channels=80, hidden_channels=256, num_layers=2)
    assert list(a) == list(seeded)
    for key in a:
        assert torch.equal(a[key], b[key])
        if a[key].dim() == 1:
            assert not torch.equal(a[key], seeded[key]) and a[key].dtype == torch.float32
            assert float((a[key] - seeded[key]).abs().max()) > 0.3, key
        else:
            assert torch.equal(a[key], seeded[key]), key
    assert not torch.equal(a['input_layer.bias'], P.loud_state(4, 80, 256, 2)['input_layer.bias'])


@pytest.mark.parametrize('hidden,depth,causal', NETWORKS)
def test_soundness(lab, hidden, depth, causal):
    net = lab.net(hidden, depth, causal)
    assert np.isfinite(net.ref).all()
    assert np.all((net.ref == 0) | net.inside)                                         # frames >= valid: exactly 0
    items = list(P.JUDGED)
    valid = [net.valid[i] for i in items]
    fp32 = O.from_features(net.state, net.feats[items].float(), torch.tensor(valid), softmax=False,
                           is_causal=causal).numpy()
    oracle_error = float((np.abs(fp32 - net.ref[items]) * net.inside[items]).max())
    assert oracle_error < 1e-5 * np.abs(net.ref).max()
    seeded = W.seeded_state_dict(seed=P.SEED, input_channels=net.cin, hidden_channels=hidden, num_layers=depth)
    line = f'\n{net}: fp32 oracle {oracle_error:.1e};'
    for precision in ('bf16', 'fp16'):
        loud_cost = P.format_cost(net.state, net.feats[items], valid, causal, precision, net.ref[items])
        seeded_cost = P.format_cost(seeded, net.feats[items], valid, causal, precision)
        line += f' {precision} format cost {loud_cost:.5f}, seeded {seeded_cost:.5f};'
        assert loud_cost <= 2 * seeded_cost, (precision, loud_cost, seeded_cost)
        assert loud_cost <= net.cost(precision) * (1 + 1e-9)
    print(line)
