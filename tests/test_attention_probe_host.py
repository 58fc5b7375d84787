"""The staircase probe of tests/attention_probe.py, checked on the CPU in float64: that it is a probe at all.

The gap it closes.  Every encoder test compares posteriors of the seeded checkpoint, whose attention is close to
uniform: one key more or less is worth about 1 / valid of the attention output.  Mutating the oracle's mask on that
checkpoint (seed 1234, 5 layers, T = 500, lengths [500, 333]) changes the posteriors by at most

    mutant                      non-causal   causal
    last valid key dropped        1.3e-3     1.6e-4
    first padded key admitted     8.0e-4     large
    causal: key q + 1 visible       --       large

against a bf16 bar of 4e-3 and an fp16 bar of 1e-3: an off-by-one at `valid` in the bf16 / fp16 instantiations of the
attention kernel (the benchmarked modes, with tile sizes and a V^T permutation of their own) passes the whole suite,
and the fp32 bar of 1e-4 catches it only at valid of about 500 and below.

Two conditions make the staircase a probe, for hidden 256 (80 input channels) and hidden 512 (768), causal and not,
T = 300 and the 24 valid lengths of attention_probe.VALID:

* dominance: for every (item, head, query) the visible edge with the largest index holds a softmax weight >= 0.999.
* separation: each mask mutant moves the float64 logits of every item it targets by >= 5 x the bf16 bound of the GPU
  test (1.6 x the bf16 format cost) -- drop_last: items whose valid - 1 is an edge; extra_key: items whose valid is
  an edge; leak_future, hide_diagonal: items with valid >= 16.

Measured (18 edges, step = 16, c = 12): dominance >= 0.99985; smallest targeted change 0.18 (extra_key, causal,
valid 192, hidden 256) = 6.2 x the bf16 bound there, the non-causal mutants 0.36 .. 3.6, leak_future 1.3 .. 2.0,
hide_diagonal 0.87 .. 1.7; format cost 0.018 .. 0.020 at bf16 and 0.0021 .. 0.0036 at fp16; the fp32 oracle 2.5e-6
from float64; logits of magnitude 3.2 .. 4.0.
"""
import numpy as np
import pytest
import torch

import attention_probe as A
from oracle import ppg_oracle as O


@pytest.fixture(scope='module')
def lab():
    return A.Lab()


CASES = [(hidden, causal) for hidden in (256, 512) for causal in (False, True)]


def test_probe_sets():
    """The edges are the multiples of every key- and query-tile size and their neighbours; the valid lengths put
    `valid - 1` and `valid` on each of them in turn."""
    assert set(A.EDGES) == {0, 256} | {m + s for m in (16, 32, 64, 128, 192) for s in (-1, 0, 1)} | {255}
    assert len(A.VALID) == 24 and max(A.VALID) == A.FRAMES == 300
    assert {v for v in A.VALID if v in A.EDGES} == set(A.EDGES) - {0}            # extra_key: every edge that can be `valid`
    assert {v - 1 for v in A.VALID if v - 1 in A.EDGES} == set(A.EDGES) - {17}   # drop_last (17 is the last key of no item)


@pytest.mark.parametrize('hidden,causal', CASES)
def test_dominance(lab, hidden, causal):
    case = lab.case(hidden, causal)
    weights = A.attention_weights(case.state, case.feats, case.valid, causal)       # (B, heads, query, key)
    top = A.top_visible_edge(case.valid, causal)                                      # (B, query)
    held = torch.gather(weights, -1, top[:, None, :, None].expand(-1, weights.shape[1], -1, 1))[..., 0]
    print(f'hidden {hidden} causal {causal}: smallest weight of the top visible edge {float(held.min()):.6f}')
    assert float(held.min()) >= 0.999
    # and the edges really are visible as the test believes: the top edge lies inside the mask of its query
    assert bool((top < torch.tensor(case.valid)[:, None]).all())
    if causal:
        assert bool((top <= torch.arange(A.FRAMES)[None]).all())


MUTANTS = [(hidden, causal, mutant) for hidden, causal in CASES
           for mutant in (A.drop_last, A.extra_key) + ((A.leak_future, A.hide_diagonal) if causal else ())]


@pytest.mark.parametrize('hidden,causal,mutant', MUTANTS, ids=lambda v: getattr(v, '__name__', str(v)))
def test_mutant_separation(lab, hidden, causal, mutant):
    case = lab.case(hidden, causal)
    bound = A.bound16(case.cost('bf16'))
    mutated = A.reference64(case.state, case.feats, case.valid, causal, mask_mutant=mutant)
    moved = (np.abs(mutated - case.ref) * case.inside).max(axis=(1, 2))               # per item
    targeted = A.targets(mutant, case.valid)
    assert targeted
    smallest = min(moved[i] for i in targeted)
    print(f'hidden {hidden} causal {causal} {mutant.__name__}: smallest targeted change {smallest:.3f} = '
          f'{smallest / bound:.1f} x the bf16 bound {bound:.4f}; largest {max(moved[i] for i in targeted):.2f}')
    for i in targeted:
        assert moved[i] >= 5 * bound, (case.valid[i], moved[i], bound)
    if mutant in (A.drop_last, A.extra_key) and not causal:
        # ... and only there: an item whose boundary keys are unmarked barely notices (1 / valid of the softmax at most)
        others = [i for i in range(len(case.valid)) if i not in targeted and case.valid[i] < A.FRAMES]
        assert max(moved[i] for i in others) < bound


@pytest.mark.parametrize('hidden,causal', CASES)
def test_what_the_gpu_bounds_rest_on(lab, hidden, causal):
    """The fp32 / fp16x2 bound of the GPU test, 2e-4, is the project's logits bound, stated for logits of magnitude
    about 4.4 (test_single_window_fp32): the probe's logits are no larger, the fp32 oracle is 1e-5 from float64 at
    most, and fp16 costs less than bf16."""
    case = lab.case(hidden, causal)
    assert np.abs(case.ref).max() <= 4.4
    fp32 = O.from_features(case.state, case.feats.float(), torch.tensor(case.valid), softmax=False,
                           is_causal=causal).numpy()
    assert case.error(fp32) < 1e-5
    assert np.all((fp32 == 0) | case.inside) and np.all((case.ref == 0) | case.inside)      # frames >= valid: exactly 0
    assert 2e-4 < case.cost('fp16') < case.cost('bf16') < 0.05
    print(f'hidden {hidden} causal {causal}: |logit| <= {np.abs(case.ref).max():.2f}, fp32 oracle {case.error(fp32):.1e}, '
          f'format cost bf16 {case.cost("bf16"):.4f} fp16 {case.cost("fp16"):.5f}')
