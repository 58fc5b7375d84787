"""The KV-cached streams on the GPU (ppg_stream.hip: Stream, BatchedStream, LongStream) against the float64 probes
the one-shot encoder is held to -- the loud-parameter networks of tests/encoder_params.py and the attention staircase
of tests/attention_probe.py -- in fp32, fp16x2, fp16 and bf16, at hidden 256 and 512, and bit for bit against
themselves under another push cadence.  Schedules, the row-range rule and the drivers: tests/stream_probe.py; that the
schedules reach the row-block counts at which a step changes its launch shape: tests/test_stream_probe_host.py.

A batched step differs from a one-utterance step where kernels go wrong: the row map mixes 16-row blocks of several
items into one four-wave workgroup, the window is looked up per block, every item has its own tok_off / vt_off = b R
and its own `valid`, one attention launch carries the query tiles of all items, and the split-hidden FFN writes
slot-dense partial rows whose stride depends on the step's block count.  With the seeded checkpoint an error of one
block, one row or one key there stays below the bars (tests/test_encoder_params_host.py::test_the_gap); with these
probes it is O(1) or at least 4 x the bound.

Every comparison is on logits (softmax=False), per item against float64 of that utterance alone (`alone`: the batch's
reference inside the item's length, but for the last four frames, where the batch reads behind the length and a stream,
like the utterance alone, ends in the convolutions' zero padding); every chunk tensor is NaN behind counts[b]; every
step is held to the emission rule (stream_probe.drive).  Bounds, none of them new: Net.bound(precision) for the loud
networks (1.6 x the format cost in fp16 / bf16, the project's 2e-4 scaled to the logits' magnitude in fp32 / fp16x2),
attention_probe.bound16(case.cost(precision)) / 2e-4 for the staircase.  The cadence tests have no tolerance.
(The format cost behind a 16-bit bound is that of the probe BATCH, as the issue sets it, while an item's last four frames
are compared with the utterance alone; the cost is a maximum over 12 or 24 items x 300 frames of which those frames are
a fiftieth, and the measured errors are 60 % of the bounds.)

Forms: the default (four launches per layer, the FFN split over the hidden chunks) and PPGS_AMD_STREAM_FUSED=2 (one
fused launch per layer, no hidden splits), read when the stream is created; the switch does nothing in fp16x2, so that
pair is left out.  Hidden 512 runs in the default form.

Measured on an MI355X (max |logits - float64| over all items and schedules of a case; the bound):
    precision  hidden  loud, batched (depth 2 / 5)    bound (2 / 5)        staircase, batched    bound
    fp32        256     7.0e-6 / 6.0e-6                2.1e-4 / 2.0e-4      6.4e-6                2.0e-4
    fp16x2      256     6.4e-6 / 5.0e-6                2.1e-4 / 2.0e-4      4.3e-6                2.0e-4
    fp16        256     2.6e-3 / 2.0e-3                4.2e-3 / 3.1e-3      2.4e-3                3.8e-3
    bf16        256     1.9e-2 / 1.6e-2                3.2e-2 / 2.4e-2      1.8e-2                2.9e-2
    fp32        512     1.0e-5                         2.0e-4               7.6e-6                2.0e-4
    fp16        512     2.1e-3                         3.3e-3               3.6e-3                5.7e-3
    bf16        512     1.9e-2                         3.0e-2               2.0e-2                3.1e-2
the fused form at hidden 256: fp32 7.7e-6, fp16 2.4e-3, bf16 1.8e-2; 7 x 160 rows: the figures of the twelve items;
Stream at hidden 512 in steps of 37: 1.0e-5 / 1.8e-3 / 1.7e-2; LongStream of 850 / 565 frames: fp32 7.1e-6 / 7.9e-6 of
2.1e-4, fp16 2.5e-3 / 2.2e-3 of 3.7e-3, bf16 1.9e-2 / 1.8e-2 of 2.7e-2.  Every schedule of a case gives the same figure,
as it must once the bits do not depend on the cadence.  The whole file (88 cases): 11 s.

Scratch builds (not committed): with the V^T offset of the items b >= 1 one 16-column block off in the stream's window
records (shifted down, so that every store stays inside the caches) 68 of 85 cases failed; with norm2.bias read 16
channels off in the row-mapped reduce pass 50 failed.  test_gpu_parity.py's two batched-stream tests noticed both as
well (6 of their 8 cases each).

What the cadence tests found when they were first run (the split counts are those stream_probe.ffn_splits derives):
* BatchedStream, default form: `whole` against the rest in fp16 and bf16 (8 against 16 hidden splits of the FFN launch);
  `whole` | `sixteens` + `ragged2` | `ragged` in fp32, fp16x2 and at hidden 512 (8 | 32 | 32 and 16 splits): exactly the
  schedules whose steps chose the same split count paired up.  The split count was chosen per step; it is now the
  stream's (ppg_stream.hip: ffn_groups), and a big step sums the same groups in one workgroup that applies LayerNorm-2
  in the reduce pass's order itself (FfnArgs::groups, ffn_closed_kernel).
* LongStream in fp16 and fp16x2 (1e-3 and 2e-6 apart): attention re-based the softmax shift of a whole wave when one
  of its queries passed the ceiling (2^10 in these modes), so a final row's bits depended on the not yet final rows
  beside it in the frontier block.  It now re-bases the queries that are past the ceiling.
* the fused form, Stream, and LongStream in fp32 and bf16: equal from the start.
"""
import numpy as np
import pytest
import torch

import attention_probe as A
import encoder_params as P
import stream_probe as S
from ppgs_amd import engine as E

pytestmark = pytest.mark.gpu

PRECISIONS = ['fp32', 'fp16x2', 'fp16', 'bf16']
FORMS = ['default', 'fused']
PAIRS = [(p, f) for p in PRECISIONS for f in FORMS if not (p == 'fp16x2' and f == 'fused')]
FP32_LOGITS_TOL = 2e-4
SHORT = tuple(v for v in P.VALID if v <= 144)
LONG_TOTALS = P.CHUNKED_VALID[:2]                 # 850 and 565 frames: both above one window


class Labs:
    def __init__(self):
        self.loud, self.staircase, self._long = P.Lab(), A.Lab(), {}

    def long(self, total):
        """The causal depth-2 loud network on ONE utterance of the chunked probe batch, alone: reference64 over [T]."""
        if total not in self._long:
            item = P.CHUNKED_VALID.index(total)
            feats = P.features(P.GEOMETRY[256], len(P.CHUNKED_VALID), P.CHUNKED_FRAMES)[item:item + 1, :, :total]
            net = P.Net(256, 2, True, valid=(total,), frames=total, state=self.loud.net(256, 2, True).state,
                        feats=feats.contiguous())
            self._long[total] = net
        return self._long[total]


@pytest.fixture(scope='module')
def labs():
    return Labs()


_engines = {}


def engine_of(probe, precision):
    """One causal engine per (probe's state dict, precision)."""
    key = (id(probe.state), precision)
    if key not in _engines:
        _engines[key] = (E.Engine(probe.state, 0, precision, True), probe.state)
    return _engines[key][0]


def batched_stream(engine, batch, max_frames, form, monkeypatch):
    """A BatchedStream of `batch` items (None: a Stream) in the given form: PPGS_AMD_STREAM_FUSED is read when the
    stream is created and fixed for its life."""
    if form == 'fused':
        monkeypatch.setenv('PPGS_AMD_STREAM_FUSED', '2')
    try:
        return engine.stream(max_frames) if batch is None else engine.batched_stream(batch, max_frames)
    finally:
        if form == 'fused':
            monkeypatch.delenv('PPGS_AMD_STREAM_FUSED')


def utterances(probe, items=None):
    items = range(len(probe.valid)) if items is None else items
    return [probe.feats[b, :, :probe.valid[b]].contiguous() for b in items]


def alone(probe, items=None):
    """The float64 logits of every utterance of the probe batch ALONE, (40, total) each -- what a stream computes: the
    causal forward of the whole utterance.  Up to an item's last four frames that is the batch's reference inside the
    item's length (asserted); the last four differ, because in the batch the input convolution reads the features
    behind `total` and the output convolution the rows behind it, while an utterance alone -- and a flushed stream --
    ends in the convolutions' zero padding."""
    if not hasattr(probe, '_alone'):
        probe._alone = {}
    items = range(len(probe.valid)) if items is None else items
    for b in items:
        total = probe.valid[b]
        if b not in probe._alone:
            ref = np.zeros((probe.ref.shape[1], 0))
            if total:
                ref = A.reference64(probe.state, probe.feats[b:b + 1, :, :total], [total], True)[0]
                assert np.abs(ref[:, :max(total - 4, 0)] - probe.ref[b, :, :max(total - 4, 0)]).max(initial=0.) < 1e-9
            probe._alone[b] = ref
    return [probe._alone[b] for b in items]


def check(outs, refs, totals, bound, what):
    """Per item: (40, total) finite logits, max |out - float64| < bound; the message names item, total, frame and
    output channel of the worst element."""
    worst, at = 0., None
    for b, (out, ref, total) in enumerate(zip(outs, refs, totals)):
        assert out.shape == (ref.shape[0], total), f'{what}: item {b} has shape {out.shape}, {total} frames expected'
        assert np.isfinite(out).all(), f'{what}: item {b} (total {total}) is not finite'
        if total == 0:
            continue
        err = np.abs(out - ref)
        if err.max() >= worst:
            channel, frame = np.unravel_index(err.argmax(), err.shape)
            worst, at = float(err.max()), (b, total, frame, channel)
    print(f'{what}: error {worst:.3e} bound {bound:.3e}')
    assert worst < bound, (f'{what}: {worst:.3e} >= {bound:.3e} at item {at[0]} (total {at[1]}) frame {at[2]} '
                           f'output channel {at[3]}')
    return worst


def staircase_bound(case, precision):
    return FP32_LOGITS_TOL if precision in ('fp32', 'fp16x2') else A.bound16(case.cost(precision))


# ---- 1. loud parameters, batched -------------------------------------------------------------------------------------

@pytest.mark.parametrize('name', ['ragged', 'whole'])
@pytest.mark.parametrize('depth', [2, 5])
@pytest.mark.parametrize('precision,form', PAIRS)
def test_loud_parameters_batched(labs, monkeypatch, precision, form, depth, name):
    """The twelve items of the probe batch (0, 1, 15 .. 300 frames) as twelve streams of batched_stream(12, 300): every
    bias, LayerNorm affine and position row through the row-mapped launches, per item against float64."""
    net = labs.loud.net(256, depth, True)
    stream = batched_stream(engine_of(net, precision), len(net.valid), P.FRAMES, form, monkeypatch)
    assert stream.rows == 320
    outs = S.drive(stream, utterances(net), S.named(name, net.valid))
    check(outs, alone(net), net.valid, net.bound(precision), f'{precision} {form} {net} batched {name}')


# ---- 2. batch * R = 32 modulo 64 -------------------------------------------------------------------------------------

@pytest.mark.parametrize('name', ['whole', 'small_then_near_full'])
@pytest.mark.parametrize('precision', ['bf16', 'fp32'])
def test_loud_parameters_half_a_workgroup_of_rows(labs, monkeypatch, precision, name):
    """The items of at most 144 frames as batched_stream(7, 144): R = 160, 1120 rows = 32 modulo 64, so the slot-dense
    partial rows of a near-full step end past batch * R (test_stream_near_full_push_after_small_push) -- with
    parameters that show a row of the caches behind them overwritten."""
    net = labs.loud.net(256, 2, True)
    items = [net.valid.index(v) for v in SHORT]
    stream = batched_stream(engine_of(net, precision), len(SHORT), max(SHORT), 'default', monkeypatch)
    assert stream.rows == 160 and len(SHORT) * stream.rows % 64 == 32
    steps = S.named('whole', SHORT) if name == 'whole' else S.small_then_near_full(SHORT)
    outs = S.drive(stream, utterances(net, items), steps)
    check(outs, alone(net, items), SHORT, net.bound(precision), f'{precision} {net} 7 x 160 rows {name}')


# ---- 3. hidden 512 ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('precision', ['fp32', 'fp16', 'bf16'])
def test_hidden_512(labs, monkeypatch, precision):
    """The w2v2fb geometry (768 input channels, hidden 512, head_dim 256): ffn_reduce_ln_kernel's generic branch under a
    row map, the 256-wide attention items, max_splits of 64 / 128 hidden chunks.  Twelve streams with `ragged`, and
    stream(300) on the 300-frame item in steps of 37.  (fp16x2 has no stream at hidden 512:
    test_gpu_geometry.py holds the refusal.)"""
    net = labs.loud.net(512, 2, True)
    engine = engine_of(net, precision)
    stream = batched_stream(engine, len(net.valid), P.FRAMES, 'default', monkeypatch)
    outs = S.drive(stream, utterances(net), S.named('ragged', net.valid))
    check(outs, alone(net), net.valid, net.bound(precision), f'{precision} {net} batched ragged')
    item = net.valid.index(P.FRAMES)
    out = S.drive_one(engine.stream(P.FRAMES), net.feats[item], S.push_sizes(P.FRAMES, 37))
    check([out], alone(net, [item]), [P.FRAMES], net.bound(precision), f'{precision} {net} stream in steps of 37')


# ---- 4. the staircase, batched ---------------------------------------------------------------------------------------

@pytest.mark.parametrize('name', ['ones', 'sixteens', 'ragged'])
@pytest.mark.parametrize('precision,hidden', [(p, 256) for p in PRECISIONS] + [(p, 512) for p in ('fp32', 'fp16', 'bf16')])
def test_staircase_batched(labs, monkeypatch, precision, hidden, name):
    """The 24 items of the staircase batch as 24 streams of batched_stream(24, 300).  With one-frame pushes every
    x_new and every q0 occurs for every item, beside other items' query tiles in the same attention launch.  In a
    causal stream a key at `valid` is only ever seen by rows that a later step recomputes -- the frontier's rows are not
    final, and once they are the key is inside `valid` -- so what this judges is the DIAGONAL rule (key q visible to
    query q, key q + 1 not) at every position of the query tile and the key tile, and the end of the key loop at the
    tile's last query; the `valid` edge itself is judged by the one-shot cases of test_gpu_attention_probe.py."""
    case = labs.staircase.case(hidden, True)
    stream = batched_stream(engine_of(case, precision), len(case.valid), A.FRAMES, 'default', monkeypatch)
    outs = S.drive(stream, utterances(case), S.named(name, case.valid))
    check(outs, alone(case), case.valid, staircase_bound(case, precision),
          f'{precision} hidden {hidden} staircase batched {name}')


# ---- 5. push-cadence invariance, bit for bit -------------------------------------------------------------------------

CADENCES = ['whole', 'sixteens', 'ragged', 'ragged2']


def assert_same_bits(runs, totals, what):
    """runs: name -> per-item outputs.  All equal in every bit; the message says which runs pair up and names the first
    item, frame and channel that differ."""
    names = list(runs)
    groups = []
    for name in names:
        for group in groups:
            if all(S.same_bits(x, y) for x, y in zip(runs[name], runs[group[0]])):
                group.append(name)
                break
        else:
            groups.append([name])
    print(f'{what}: bit-equal groups {groups}')
    if len(groups) == 1:
        return
    first, other = runs[groups[0][0]], runs[groups[1][0]]
    for b, (x, y) in enumerate(zip(first, other)):
        if not S.same_bits(x, y):
            differ = x.view(np.int32) != y.view(np.int32)
            frame = int(np.argmax(differ.any(axis=0)))
            channel = int(np.argmax(differ[:, frame]))
            raise AssertionError(
                f'{what}: the bits depend on the push cadence; bit-equal groups {groups}; {groups[0][0]} against '
                f'{groups[1][0]}: item {b} (total {totals[b]}) frame {frame} output channel {channel}: '
                f'{x[channel, frame]!r} against {y[channel, frame]!r}, max difference {np.abs(x - y).max():.3e}')


@pytest.mark.parametrize('precision,form,probe', [(p, f, 'loud 256') for p, f in PAIRS] + [('bf16', 'default', 'loud 512')] +
                         [(p, 'default', 'staircase 256') for p in PRECISIONS])
def test_batched_stream_bits_do_not_depend_on_the_push_cadence(labs, monkeypatch, precision, form, probe):
    """ppg_stream.hip: "a recomputed row gives the same bits".  The twelve loud items pushed whole (one step of 86 row
    blocks), in 16-frame steps (<= 16 blocks), by `ragged` (steps of 40 and of 1 .. 16 blocks) and by `ragged2` (every
    item's own pushes as in `ragged`, its neighbours doing something else): the logits of every item are equal in every
    bit.  `ragged` against `ragged2` is "an item's bits do not depend on its neighbours' schedule".  The 24 staircase
    items as well: pushed whole (185 blocks) they take the one-workgroup form of the FFN launch in every precision, which
    the loud batch reaches in fp32 and fp16x2 only (tests/test_stream_probe_host.py)."""
    kind, hidden = probe.split()
    net = labs.loud.net(int(hidden), 2, True) if kind == 'loud' else labs.staircase.case(int(hidden), True)
    engine = engine_of(net, precision)
    runs = {}
    for name in CADENCES:
        stream = batched_stream(engine, len(net.valid), P.FRAMES, form, monkeypatch)
        runs[name] = S.drive(stream, utterances(net), S.named(name, net.valid))
    assert_same_bits(runs, net.valid, f'{precision} {form} {probe} batched')


@pytest.mark.parametrize('precision,form', PAIRS)
def test_stream_bits_do_not_depend_on_the_push_cadence(labs, monkeypatch, precision, form):
    """Stream: the 300-frame loud item in steps of 1, 16, 37 and whole."""
    net = labs.loud.net(256, 2, True)
    item = net.valid.index(P.FRAMES)
    engine = engine_of(net, precision)
    runs = {}
    for size in (1, 16, 37, P.FRAMES):
        stream = batched_stream(engine, None, P.FRAMES, form, monkeypatch)
        runs[f'steps of {size}'] = [S.drive_one(stream, net.feats[item], S.push_sizes(P.FRAMES, size))]
    assert_same_bits(runs, [P.FRAMES], f'{precision} {form} {net} stream')


@pytest.mark.parametrize('precision,form', PAIRS)
def test_long_stream_bits_do_not_depend_on_the_push_cadence(labs, monkeypatch, precision, form):
    """LongStream: the 850-frame utterance in two push patterns (the ragged size list from two offsets).  A LongStream
    creates its windows' Streams as the frames reach them, so the form's switch stays set for the whole drive."""
    net = labs.long(850)
    engine = engine_of(net, precision)
    if form == 'fused':
        monkeypatch.setenv('PPGS_AMD_STREAM_FUSED', '2')
    runs = {f'sizes from {offset}': [S.drive_one(engine.long_stream(), net.feats[0], S.cycle_sizes(850, offset=offset))]
            for offset in (0, 4)}
    assert_same_bits(runs, [850], f'{precision} {form} {net} long stream')


# ---- 6. LongStream with loud parameters ------------------------------------------------------------------------------

@pytest.mark.parametrize('total', LONG_TOTALS)
@pytest.mark.parametrize('precision', ['fp32', 'fp16', 'bf16'])
def test_long_stream_loud_parameters(labs, precision, total):
    """An utterance longer than a window, alone, in ragged pushes: the reference's chunk rule (windows of 500 rows every
    400 frames over the left-replicated sequence, each with window-relative position rows and the loud parameters)
    against float64 of that utterance alone."""
    net = labs.long(total)
    assert total > 500 and net.ref.shape == (1, 40, total)
    out = S.drive_one(engine_of(net, precision).long_stream(), net.feats[0], S.cycle_sizes(total))
    check([out], [net.ref[0]], [total], net.bound(precision), f'{precision} {net} long stream of {total} frames')
