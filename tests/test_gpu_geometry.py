"""Encoder parity at every geometry `ppg_engine_create` accepts, or a refusal: the catalogue of tests/geometry_probe.py
(input channels 1 .. 144, 1 / 2 / 4 heads, F 64 .. 6656, 1 .. 48 output channels, 16 layers, a position table of
exactly chunk_length rows) through Engine.encode in fp32, fp16x2, fp16 and bf16, in every launch regime the geometry
has, against the float64 oracle with the geometry's head count.  That the oracle is right at these geometries, and
that a fault on each axis is at least 4 x the bf16 bound: tests/test_geometry_probe_host.py.

Regimes, reached by replicating the base batch of encoder_params (12 items x 300 frames, valid 0, 1, 15, 16, 17, 33,
144, 159, 160, 161, 289, 300: 11 windows of 304 token rows), one float64 reference per row; the row counts that
select them are asserted:
* hidden 256: x 1 (3344 rows <= 6144: token-split kernels, the FFN in hidden splits); x 2 (6688 rows: 16-bit modes
  on sub-tile layer32 with the head kernel where F and the channels allow, fp32 without hidden splits); x 4 in fp16x2
  (13376 >= 128 x 96: ppg_ffn32x2.hip where F <= 3328 and F % 128 == 0); x 7 in the 16-bit modes (23408 >= 128 x 160:
  whole-tile layer32 and head32) for the rows those kernels hold packed images of (cin 65 / 96, 1 head, F 5888 /
  6656, 48 outputs, 16 layers);
* hidden 512: the two halves of the batch (<= 2048 rows each: hidden splits) and the whole batch (layer32 in the
  16-bit modes).

Every encode: logits (softmax=False) inside the mask within the bound, exactly 0 behind it, and the same bits again
after every workspace was filled with 0xFF (a feature or chunk the kernels never wrote shows as NaN there, not as a
small error).  Once per row and precision with softmax: padded frames exactly 1 / out, every frame sums to 1 within
1e-5, fp32 posteriors within 1e-4.  Bounds, all the project's: fp32 and fp16x2 encoder_params.bound32 (2e-4 at logits
of magnitude 4.4); fp16 / bf16 max(1.6 x the format cost of this geometry and batch, the fp32 bound).

Replicated copies of an item (every copy is held to the bound everywhere; the count of copies that differ from the
first in some bit is printed):
* 16-bit modes, hidden 256, F % 128 == 0, x 2 and x 7: the layers run on ppg_layer32.hip, which walks the hidden chunks
  in one order wherever a token lies -- the copies must agree bit for bit (measured: they do, in every such case);
* every route through the fused token-split FFN kernel (fp32 x 2; fp16x2 x 4 where F > 3328 or F % 128 != 0; the
  16-bit modes at F % 128 != 0): ffn_body starts its walk over the hidden chunks at a chunk that depends on the
  workgroup's index (`rot`), so two copies sum in different orders -- measured: all copies differ, by <= 3e-6;
* fp16x2 x 4 on ppg_ffn32x2.hip: not asserted.  Measured: 11 of 13 rows agree in every bit; at cin 65 and F 1152 the
  logits of 2 .. 5 frames around ONE token row of one item differ by <= 4.8e-7 (an ulp or two of the logits) between
  copies whose windows start at other offsets inside the 96-token tile.

Refusals (construction raises, naming the field; nothing is launched; the process then still constructs and runs a
good engine): tables of 499 and 300 rows, 17 layers, F 6784, F 320 at hidden 512 in fp16x2 (the two-GEMM FFN writes 256
features per pass), 1 head at hidden 256 and 4 at hidden 512 in fp16x2.

Measured on an MI355X (max over the regimes of a row; logits, inside the mask).  The file: 27 s of test time, 130
cases.  fp32 5.1e-6 .. 1.3e-5 and fp16x2 4.6e-6 .. 1.0e-5 on every row, against bounds of 2.0e-4 .. 2.3e-4; fp32
posteriors <= 3.1e-6.  16-bit modes, error (format cost), the bound being 1.6 x the cost:

    row                     fp16                  bf16
    cin 1                   2.9e-3 (2.8e-3)       2.1e-2 (2.2e-2)
    cin 16                  2.3e-3 (2.6e-3)       1.9e-2 (1.9e-2)
    cin 65                  2.5e-3 (2.4e-3)       2.2e-2 (2.4e-2)
    cin 96                  2.7e-3 (2.7e-3)       2.4e-2 (2.1e-2)
    cin 97                  2.4e-3 (2.4e-3)       2.0e-2 (1.8e-2)
    cin 128                 2.5e-3 (2.3e-3)       2.0e-2 (2.0e-2)
    cin 144                 2.5e-3 (2.6e-3)       2.4e-2 (1.9e-2)
    cin 100, hidden 512     2.5e-3 (2.4e-3)       2.0e-2 (1.9e-2)
    1 head                  2.5e-3 (2.5e-3)       2.0e-2 (2.0e-2)
    1 head, causal          2.4e-3 (2.5e-3)       2.1e-2 (2.1e-2)
    4 heads, hidden 512     2.4e-3 (2.5e-3)       2.0e-2 (2.0e-2)
    4 heads, 512, causal    2.7e-3 (2.4e-3)       2.4e-2 (2.2e-2)
    out 1                   1.6e-3 (1.7e-3)       1.7e-2 (1.7e-2)
    out 41                  2.6e-3 (2.5e-3)       1.9e-2 (2.1e-2)
    out 48                  2.6e-3 (2.5e-3)       1.9e-2 (2.1e-2)
    out 48, hidden 512      2.5e-3 (2.3e-3)       1.9e-2 (2.2e-2)
    F 64                    2.1e-3 (2.2e-3)       2.0e-2 (1.7e-2)
    F 192                   2.4e-3 (2.2e-3)       2.0e-2 (1.9e-2)
    F 640                   2.4e-3 (2.4e-3)       2.0e-2 (2.0e-2)
    F 1152                  2.4e-3 (2.4e-3)       1.9e-2 (1.7e-2)
    F 5888                  2.4e-3 (2.4e-3)       2.2e-2 (2.0e-2)
    F 6656                  2.1e-3 (2.1e-3)       2.1e-2 (1.9e-2)
    F 320, hidden 512       2.6e-3 (2.4e-3)       2.0e-2 (2.0e-2)
    F 3584, hidden 512      2.5e-3 (2.4e-3)       2.1e-2 (1.9e-2)
    F 3840, hidden 512      3.3e-3 (2.9e-3)       2.1e-2 (1.9e-2)
    16 layers, F 256        3.8e-3 (4.0e-3)       3.5e-2 (3.7e-2)
    table of 500 rows       2.6e-3 (2.5e-3)       1.9e-2 (2.1e-2)

On the kernels before the fixes that came with this file (the same cases, the library of the parent commit): F 640,
F 1152, F 5888 (16-bit) and F 320 at hidden 512 were 0.7 .. 1.4 off in every mode at x 1 (hidden chunks that no split
summed); F 6656 and F 3840 at hidden 512 failed in `encode` with a launch error in fp32; fp16x2 at hidden 512 with
F 320 was 1.6 off and all NaN over a poisoned workspace (64 hidden features never written).
"""
import time

import numpy as np
import pytest
import torch

import encoder_params as P
import geometry_probe as G
from ppgs_amd import engine as E

pytestmark = pytest.mark.gpu

FP32_TOL = 1e-4
SIXTEEN = ('fp16', 'bf16')


@pytest.fixture(scope='module')
def lab():
    started = time.time()
    lab = G.Lab()
    yield lab
    lab.release()
    print(f'\ntest_gpu_geometry.py: {time.time() - started:.0f} s wall')


def engine_of(case, precision):
    return E.Engine(case.state, 0, precision, case.causal, heads=case.geometry.heads)


def encode(engine, feats, valid, softmax):
    out = engine.encode(feats.cuda(), list(valid), softmax=softmax)
    torch.cuda.synchronize()
    return out.cpu().numpy()


def poison(engine):
    for workspace in engine._workspaces.values():
        workspace.view(torch.int16).fill_(-1)          # 0xffff.. = NaN as bf16, fp16 and fp32


def check_logits(engine, feats, valid, ref, bound, what):
    """max |logits - float64| inside the mask < bound, exactly 0 behind it, the same bits over a poisoned workspace."""
    out = encode(engine, feats, valid, False)
    inside = G.A.inside(valid, ref.shape[-1])
    assert out.shape == ref.shape, what
    assert np.isfinite(out).all(), f'{what}: non-finite logits'
    assert np.all(out[~np.broadcast_to(inside, out.shape)] == 0), f'{what}: frames >= valid are not exactly 0'
    err = np.abs(out - ref) * inside
    item, channel, frame = np.unravel_index(err.argmax(), err.shape)
    print(f'{what}: error {err.max():.3e} bound {bound:.3e}')
    assert err.max() < bound, (f'{what}: {err.max():.3e} >= {bound:.3e} at item {item} (valid {valid[item]}) '
                               f'frame {frame} output channel {channel}')
    poison(engine)
    again = encode(engine, feats, valid, False)
    assert np.array_equal(out, again), f'{what}: depends on what the workspace held'
    return out


def check_posteriors(engine, case, precision, what):
    out = encode(engine, case.feats, case.valid, True)
    channels = case.geometry.out
    inside = np.broadcast_to(case.inside, out.shape)
    assert np.isfinite(out).all(), what
    assert np.all(out[~inside] == np.float32(1) / np.float32(channels)), f'{what}: padded frames are not exactly 1 / {channels}'
    assert np.abs(out.sum(1) - 1).max() < 1e-5, f'{what}: posteriors do not sum to 1'
    exp = np.exp(case.ref - case.ref.max(1, keepdims=True))
    err = float((np.abs(out - exp / exp.sum(1, keepdims=True)) * case.inside).max())
    print(f'{what}: posteriors error {err:.3e}')
    if precision == 'fp32':
        assert err < FP32_TOL, what


def copies_differing(out, times):
    """how many of the replicated copies 1 .. times - 1 differ from copy 0 in any bit"""
    items = len(out) // times
    return sum(not np.array_equal(out[:items], out[k * items:(k + 1) * items]) for k in range(1, times))


def regimes(row, precision):
    """[(times or item slice, lowest row count, highest row count)] of a row in a precision"""
    if row.geometry.hidden == 512:
        return [(slice(0, 6), 1, 2048), (slice(6, 12), 1, 2048), (1, 2049, 1 << 30)]
    plan = [(1, 1, 6144)]
    if precision in SIXTEEN:
        plan.append((2, 6145, 128 * 160 - 1))
        if row.big:
            plan.append((7, 128 * 160, 1 << 30))
    elif precision == 'fp16x2':
        plan.append((4, 128 * 96, 1 << 30))
    else:
        plan.append((2, 6145, 1 << 30))
    return plan


def _cases():
    cases = []
    for row in G.ACCEPTED:
        for causal in ((False, True) if row.axis == 'heads' else (False,)):
            for precision in G.PRECISIONS:
                if row.accepted(precision):
                    cases.append(pytest.param(row, causal, precision,
                                              id=f'{row}-{"causal" if causal else "noncausal"}-{precision}'))
    return cases


@pytest.mark.parametrize('row,causal,precision', _cases())
def test_geometry(lab, row, causal, precision):
    case = lab.case(row, causal)
    engine = engine_of(case, precision)
    bound = case.bound(precision)
    cost = f' format cost {case.cost(precision):.3e}' if precision in SIXTEEN else ''
    for which, lowest, highest in regimes(row, precision):
        if isinstance(which, slice):
            feats, valid, ref, times = case.feats[which], case.valid[which], case.ref[which], 1
        else:
            (feats, valid, ref), times = G.tiled(case, which), which
        _, info = E.plan_windows(len(valid), case.frames, valid, engine=engine)
        assert lowest <= info.tokens <= highest, (which, info.tokens)
        what = f'{case} {precision} {which if isinstance(which, slice) else f"x {which}"} ({info.tokens} rows)'
        out = check_logits(engine, feats, list(valid), ref, bound, what + cost)
        if times > 1:
            differing = copies_differing(out, times)
            print(f'{what}: {differing} of {times - 1} copies differ from the first in some bit')
            if precision in SIXTEEN and row.geometry.ffn % 128 == 0:       # ppg_layer32.hip: one order of summation
                assert differing == 0, f'{what}: copies of one item differ on the feature-split layer kernel'
    check_posteriors(engine, case, precision, f'{case} {precision}')


@pytest.mark.parametrize('precision', G.PRECISIONS)
@pytest.mark.parametrize('frames,valid', [(500, (500, 257, 1)), (850, (850, 401, 400))], ids=['T500', 'T850'])
def test_table_of_chunk_length_rows(lab, precision, frames, valid):
    """A 500-row table: a full window (T = 500) and the windows of a chunked batch (T = 850: 500 / 500 / 100 frames)
    use rows 0 .. 499 exactly."""
    case = lab.case(G.CATALOGUE['h256-max_len500'], False, valid, frames)
    windows = G.O.plan_windows(frames, valid)
    assert max(w['Tc'] for w in windows) == 500 and max(max(w['clens']) for w in windows) == 500
    engine = engine_of(case, precision)
    check_logits(engine, case.feats, list(valid), case.ref, case.bound(precision), f'{case} {precision} T = {frames}')


FP16X2_HEADS = [(G.CATALOGUE['h256-heads1'], 'fp16x2', 'head dimension'), (G.CATALOGUE['h512-heads4'], 'fp16x2', 'head dimension')]


@pytest.mark.parametrize('row,precision,field', [(row, precision, row.refused) for row, precision in G.REFUSED] + FP16X2_HEADS,
                         ids=lambda v: str(v).replace(' ', '_'))
def test_refused_at_construction(lab, row, precision, field):
    state = G.state(row.geometry)
    with pytest.raises((ValueError, E.PpgError), match=field):
        E.Engine(state, 0, precision, heads=row.geometry.heads)
    # the process still constructs and runs a good engine
    good = lab.case(G.CATALOGUE['h256-ffn64'])
    check_logits(engine_of(good, 'bf16'), good.feats, list(good.valid), good.ref, good.bound('bf16'),
                 f'after the refusal of {row} {precision}: {good} bf16')
