"""Shared by tests/test_metrics_probe_host.py and tests/test_gpu_metrics_probe.py: seeded inputs for the frame metrics
(ppg_metrics.hip) that reach what the fixture's `3 randn` logits with frame-by-frame labels cannot, an fp32 restatement
of the kernel's arithmetic, criteria and mutants.  The float64 reference is restate() of tests/test_metrics_host.py.
No GPU is touched here; the similarity matrix, exponent and class weights are fixture g13_metrics (`g` below).

Families (each (logits fp32 (batch, 40, frames), labels int64, lengths or None); never modified by a caller):
  stride        (3, 40, 22000): 66000 frames = 516 tiles of 128 on 256 workgroups: workgroups 0..3 make three trips,
                the others two, the last tile holds 80 frames.  Labels in runs of 1..90 frames, logits
                2 randn + 6 onehot(c), c the label on about 80 % of the frames and another class otherwise (on a tenth
                of the runs for the whole run); -100 holes as single frames and as spans of 200+ frames that start off
                a multiple of 64; lengths (22000, 9001, 22000).
  ties          (5, 40, 333): logits round(1.5 randn) / 2; on a third of the frames the label's logit is the maximum,
                on a tenth all 40 are equal.  Judged without class weights only: tied logits then give bit-identical
                fp32 probabilities and the rule alone decides the distance row.
  single        (4097, 40, 1): every lane another batch item.  single_lengths: the same with lengths in {0, 1, 5}.
  edge_lengths  (7, 40, 45), lengths (45, 0, 1, 44, 45, 100, 7): batch boundaries inside a wave; labels in range
                everywhere, logits past each length NaN / +inf / 1e38.
  extreme       (1, 40, 197), read one frame at a time: confident and correct, confident and wrong, -inf in several
                other classes, and eight frames whose own label's logit is -inf.
Every family but `ties` is repaired after the draw: while the two largest softmax values of a frame, or the two
largest softmax * class weight, are closer than 1e-3 relative (float64), its largest logit goes up by 1.  So the
float64 reference and an fp32 kernel agree on every argmax and no frame is left out of the exact comparison.

Criteria.  Integers (count, true_positives, topk_correct, invalid_labels, class_total, class_count, frames per distance
row -- read off the row sums where there are no class weights) equal the reference.  A confusion row sums to its
class_count within count * 42 * 2^-24 + n * 2^-32 (a 40-term fp32 softmax, the fixed-point quantum), as does a distance
row without class weights; a row nobody used is exactly 0.  loss and JSD means within rtol 2e-5 / atol 2e-6 + 2^-32,
cells within 2e-6 * rows + n * 2^-32 + 2e-5 |cell| (the project's bound; the logits of stride, single and edge_lengths
are in the fixture's regime).  `extreme`, per frame: loss within 2^-33 + 8 * 2^-24 max(1, |ref|) of min(ref, 2^20);
JSD within E_t(kappa) + 2^-33 of postops_probe.distance64(softmax64, onehot, mix), E_t as there with unit_p enlarged by
DELTA a_p |ln a_p - ln m_p| / 2, DELTA = 8 * 2^-24: what one expf, a 40-term sum and a division leave unknown in a_p.
KAPPA_REF[mix] is the smallest kappa at which restate32 passes on every frame (measured by the host test); the kernel is
held to 4 max(KAPPA_REF, 1), the convention of postops_probe.kappa_gpu.
"""
import numpy as np
import torch

from postops_probe import U, distance64, distance_bound
from test_metrics_host import ATOL, FIXED, RTOL, restate

NP = 40
TILE, MAX_BLOCKS = 128, 256                     # ppg_metrics.hip: frames per workgroup and trip, workgroups
FIRST_TRIP = TILE * MAX_BLOCKS                  # 32768 frames
LOSS_CLAMP = 2.0 ** 20
DELTA = 8 * U
GAP = 1e-3
FAMILIES = ('stride', 'ties', 'single', 'single_lengths', 'edge_lengths', 'extreme')
SUMMED = ('stride', 'single', 'single_lengths', 'edge_lengths')      # loss, JSD and cells judged on the whole input
STRIDE_CUTS = (0, 1, 8191, 8192, 16385, 22000)
STRIDE_SPANS = ((0, 5003, 230), (1, 4037, 211), (2, 3011, 290), (2, 21601, 250))     # (item, first frame, frames)
EDGE_LENGTHS = (45, 0, 1, 44, 45, 100, 7)

# The smallest kappa at which restate32 is inside E_t + 2^-33 on every frame of `extreme`, rounded up to 0.05; measured
# and asserted by tests/test_metrics_probe_host.py::test_kappa_ref_is_a_measurement.  Keyed by mix.
KAPPA_REF = {True: 0.15, False: 0.20}
# (both are below 1, so the kernel's bound is kappa 4 with and without the mix: the table records what the restatement
# needs, it does not move the bound.)


def kappa_gpu(mix):
    return 4.0 * max(KAPPA_REF[bool(mix)], 1.0)


def tables(g):
    """(mix (40, 40), class weights (40,)) fp32 of the fixture"""
    return (torch.from_numpy(g['similarity']).float().T ** float(g['exponent'])).contiguous(), \
        torch.from_numpy(g['weights']).float()


# ---- families ------------------------------------------------------------------------------------------------------

def masked_labels(labels, lengths):
    labels = labels.to(torch.int64).clone()
    if lengths is not None:
        labels[torch.arange(labels.shape[1])[None, :] >= torch.as_tensor(lengths)[:, None]] = -100
    return labels


def weighted_gap(logits, weights=None):
    """(batch, frames) float64: relative gap of the two largest softmax [* weight] values of every frame"""
    probs = torch.softmax(logits.double(), dim=1)
    if weights is not None:
        probs = probs * weights.double()[None, :, None]
    top = probs.topk(2, dim=1).values
    return (top[:, 0] - top[:, 1]) / top[:, 0]


def repair(logits, weights):
    while True:
        near = (weighted_gap(logits) < GAP) | (weighted_gap(logits, weights) < GAP)
        if not near.any():
            return logits
        b, t = near.nonzero(as_tuple=True)
        logits[b, logits.argmax(dim=1)[b, t], t] += 1.0


def _other(generator, label, shape=()):
    return (label + 1 + torch.randint(0, NP - 1, shape, generator=generator)) % NP


def _stride(weights):
    generator = torch.Generator().manual_seed(1401)
    batch, frames = 3, 22000
    labels = torch.empty(batch, frames, dtype=torch.int64)
    boosted = torch.empty(batch, frames, dtype=torch.int64)
    for b in range(batch):
        t, previous = 0, -1
        while t < frames:
            end = min(t + int(torch.randint(1, 91, (), generator=generator)), frames)
            label = int(torch.randint(0, NP, (), generator=generator))
            if label == previous:
                label = (label + 1) % NP
            labels[b, t:end] = label
            if float(torch.rand((), generator=generator)) < 0.1:               # another class for the whole run
                boosted[b, t:end] = _other(generator, label)
            else:
                elsewhere = torch.rand(end - t, generator=generator) < 0.11
                boosted[b, t:end] = torch.where(elsewhere, _other(generator, label, (end - t,)), label)
            t, previous = end, label
    logits = 2 * torch.randn(batch, NP, frames, generator=generator)
    logits.scatter_add_(1, boosted[:, None, :], torch.full((batch, 1, frames), 6.0))
    labels[torch.rand(batch, frames, generator=generator) < 0.01] = -100
    for b, first, count in STRIDE_SPANS:
        labels[b, first:first + count] = -100
    return repair(logits, weights), labels, torch.tensor([22000, 9001, 22000])


def _ties(weights):
    generator = torch.Generator().manual_seed(1402)
    batch, frames = 5, 333
    logits = torch.round(1.5 * torch.randn(batch, NP, frames, generator=generator)) * 0.5
    labels = torch.randint(0, NP, (batch, frames), generator=generator)
    kind = torch.rand(batch, frames, generator=generator)
    level = torch.round(torch.randn(batch, frames, generator=generator)) * 0.5
    own_is_top, all_equal = kind < 1 / 3, kind > 0.9
    logits = torch.where(all_equal[:, None, :], level[:, None, :], logits)
    b, t = own_is_top.nonzero(as_tuple=True)
    logits[b, labels[b, t], t] = logits.max(dim=1).values[b, t]
    b, t = all_equal.nonzero(as_tuple=True)
    labels[b[0], t[0]], labels[b[1], t[1]] = 0, NP - 1
    holes = torch.rand(batch, frames, generator=generator) < 0.02
    labels[holes & ~all_equal] = -100
    return logits.contiguous(), labels, None


def _single(weights, with_lengths):
    generator = torch.Generator().manual_seed(1403)
    batch = 4097
    logits = 3 * torch.randn(batch, NP, 1, generator=generator)
    labels = torch.randint(0, NP, (batch, 1), generator=generator)
    labels[torch.rand(batch, 1, generator=generator) < 0.01] = -100
    lengths = torch.tensor([0, 1, 5])[torch.randint(0, 3, (batch,), generator=generator)]
    return repair(logits, weights), labels, lengths if with_lengths else None


def _edge_lengths(weights):
    generator = torch.Generator().manual_seed(1404)
    batch, frames = len(EDGE_LENGTHS), 45
    logits = repair(3 * torch.randn(batch, NP, frames, generator=generator), weights)
    labels = torch.randint(0, NP, (batch, frames), generator=generator)
    lengths = torch.tensor(EDGE_LENGTHS)
    padding = torch.arange(frames)[None, :] >= lengths[:, None]
    garbage = torch.tensor([float('nan'), float('inf'), 1e38])
    logits.transpose(1, 2)[padding] = garbage[torch.arange(int(padding.sum())) % 3][:, None]
    return logits, labels, lengths


def _extreme(weights):
    generator = torch.Generator().manual_seed(1405)
    frames = 197
    labels = torch.randint(0, NP, (1, frames), generator=generator)
    logits = 30 * torch.randn(1, NP, frames, generator=generator)
    soft = 3 * torch.randn(1, NP, frames, generator=generator)
    push = 20 + 70 * torch.rand(frames, generator=generator)
    wrong = _other(generator, labels[0], (frames,))
    lost = torch.rand(NP, frames, generator=generator) < 0.2
    for t in range(frames):
        label = int(labels[0, t])
        if t >= frames - 8:                                                 # the label's own logit is -inf
            logits[0, :, t] = soft[0, :, t]
            logits[0, label, t] = -float('inf')
        elif t % 3 == 2:                                                    # -inf in several other classes
            logits[0, :, t] = soft[0, :, t]
            lost[label, t] = False
            lost[(label + 1) % NP, t] = lost[(label + 7) % NP, t] = True
            logits[0, lost[:, t], t] = -float('inf')
        else:                                                               # confident: correct, or wrong
            winner = label if t % 3 == 0 else int(wrong[t])
            logits[0, winner, t] = -float('inf')
            logits[0, winner, t] = logits[0, :, t].max() + push[t]
    return repair(logits, weights), labels, None


_cache = {}


def family(name, g):
    if name not in _cache:
        weights = tables(g)[1]
        build = {'stride': _stride, 'ties': _ties, 'single': lambda w: _single(w, False),
                 'single_lengths': lambda w: _single(w, True), 'edge_lengths': _edge_lengths, 'extreme': _extreme}
        _cache[name] = build[name](weights)
    return _cache[name]


def poisoned(inputs, fill):
    """The logits of every frame that does not count (past its length, or label -100) replaced: fill = 'zero' or
    'garbage' (NaN, +inf, -inf, 1e38 in turn)."""
    logits, labels, lengths = inputs
    unread = masked_labels(labels, lengths) == -100
    out = logits.clone()
    count = int(unread.sum())
    values = torch.zeros(count) if fill == 'zero' else \
        torch.tensor([float('nan'), float('inf'), -float('inf'), 1e38])[torch.arange(count) % 4]
    out.transpose(1, 2)[unread] = values[:, None]
    return out


def runs(flat):
    """lengths of the runs of equal labels among the labelled frames of a flat label sequence (holes skipped)"""
    kept = flat[flat != -100]
    if not len(kept):
        return torch.zeros(0, dtype=torch.int64)
    change = torch.cat([torch.tensor([True]), kept[1:] != kept[:-1]]).nonzero()[:, 0]
    return torch.diff(torch.cat([change, torch.tensor([len(kept)])]))


# ---- the kernel's arithmetic in fp32 ---------------------------------------------------------------------------------

def to_fixed(v):
    """the header's rounding: [0, 2^20], NaN as 0, to the nearest multiple of 2^-32 -> int64"""
    v = torch.nan_to_num(v.float(), nan=0.0, posinf=float('inf'), neginf=-float('inf')).clamp(0.0, LOSS_CLAMP)
    return torch.round(v.double() * 2.0 ** 32).to(torch.int64)


def _sum40(x):
    total = torch.zeros_like(x[:, 0])
    for p in range(NP):
        total = total + x[:, p]
    return total


def restate32(logits, labels, lengths=None, k=3, mix=None, class_weights=None, loss_weights=None):
    """ppg_metrics.hip's formulas as fp32 CPU torch vector code -> the accumulators as real numbers.  It measures what
    a correct fp32 evaluation needs of a bound; it is never a reference for the kernel."""
    batch, classes, frames = logits.shape
    flat = masked_labels(labels, lengths).flatten()
    counted = flat != -100
    keep = counted & (flat >= 0) & (flat < classes)
    rows = logits.float().transpose(1, 2).flatten(0, 1)[keep]
    target = flat[keep]
    n = len(target)
    top = rows.max(dim=1).values if n else rows.new_zeros(0)
    own = rows.gather(1, target[:, None])[:, 0]
    order = torch.sort(rows, dim=1, descending=True, stable=True).indices
    correct = order[:, 0] == target
    e = torch.exp(rows - top[:, None])
    total = _sum40(e)
    loss = torch.log(total) - (own - top)
    weight_fixed = 0
    if loss_weights is not None:
        loss = loss * loss_weights.float()[target]
        weight_fixed = int(to_fixed(loss_weights.float()[target]).sum())
    probs = e / total[:, None]
    weighted = probs if class_weights is None else probs * class_weights.float()[None]
    predicted = weighted.argmax(dim=1) if n else torch.zeros(0, dtype=torch.int64)
    lo, hi = torch.tensor(1e-8), torch.tensor(1.0) - torch.tensor(1e-8)
    x = torch.minimum(torch.maximum(probs, lo), hi)
    y = torch.where(torch.nn.functional.one_hot(target, classes).bool(), hi, lo)
    if mix is not None:
        u, v = torch.zeros_like(x), torch.zeros_like(y)
        for q in range(NP):
            u = u + mix.float()[None, :, q] * x[:, q:q + 1]
            v = v + mix.float()[None, :, q] * y[:, q:q + 1]
    else:
        u, v = x, y
    log_m = torch.log((u + v) * 0.5)
    ku, kv = u * (torch.log(u) - log_m), v * (torch.log(v) - log_m)
    jsd = _sum40(torch.sqrt(((ku + kv) * 0.5).clamp(min=0)))

    def matrix(index, values):
        return (torch.zeros(classes, classes, dtype=torch.int64).index_add_(0, index, to_fixed(values)).numpy()
                / 2.0 ** 32)
    return dict(
        count=n, true_positives=int(correct.sum()), topk_correct=int((order[:, :k] == target[:, None]).sum()),
        invalid_labels=int((counted & ~keep).sum()),
        class_total=torch.bincount(target[correct], minlength=classes).numpy(),
        class_count=torch.bincount(target, minlength=classes).numpy(),
        loss_sum=int(to_fixed(loss).sum()) / 2.0 ** 32, jsd_sum=int(to_fixed(jsd).sum()) / 2.0 ** 32,
        loss_weight_sum=weight_fixed / 2.0 ** 32,
        distance_matrix=matrix(predicted, weighted), confusion=matrix(target, probs))


# ---- criteria --------------------------------------------------------------------------------------------------------

def _worst(error, bound):
    """(every error inside its bound, the largest error / bound); NaN fails, 0 / 0 is 0"""
    error, bound = np.broadcast_arrays(np.asarray(error, dtype=np.float64), np.asarray(bound, dtype=np.float64))
    ok = bool((error <= bound).all())
    ratio = np.where(error == 0, 0.0, error / np.where(bound > 0, bound, 1e-300))
    return ok, float(np.max(np.where(np.isnan(ratio), np.inf, ratio))) if ratio.size else 0.0


def judge(got, want, k, class_weighted, summed):
    """`got`: accumulators as real numbers of any evaluation, `want`: restate() of the same input.
    -> (names of the criteria that fail, {name: worst error / bound})"""
    failed, ratios = [], {}
    n = int(want['count'])
    for key in ('count', 'true_positives', 'invalid_labels'):
        if int(got[key]) != int(want[key]):
            failed.append(key)
    if int(got['topk_correct']) != int(want['topk_by_k'][k - 1]):
        failed.append('topk_correct')
    for key in ('class_total', 'class_count'):
        if not np.array_equal(np.asarray(got[key]), want[key]):
            failed.append(key)
    confusion = np.asarray(got['confusion'], dtype=np.float64)
    distance = np.asarray(got['distance_matrix'], dtype=np.float64)
    counts = want['class_count'].astype(np.float64)
    used = want['distance_rows'].astype(np.float64)

    def criterion(name, ok, ratio=None):
        if ratio is not None:
            ratios[name] = ratio
        if not ok:
            failed.append(name)
    criterion('confusion_row_sums', *_worst(np.abs(confusion.sum(axis=1) - counts), counts * 42 * U + n * FIXED))
    criterion('confusion_unused_rows', not confusion[counts == 0].any())
    criterion('distance_unused_rows', not distance[used == 0].any())
    if not class_weighted:
        with np.errstate(invalid='ignore'):
            criterion('distance_rows', np.array_equal(np.rint(distance.sum(axis=1)), used))
        criterion('distance_row_sums', *_worst(np.abs(distance.sum(axis=1) - used), used * 42 * U + n * FIXED))
    if summed:
        for key in ('loss_sum', 'jsd_sum'):
            if n == 0:
                criterion(key, got[key] == 0)
            else:
                criterion(key, *_worst(abs(got[key] - want[key]) / n, ATOL + RTOL * abs(want[key]) / n + FIXED))
        criterion('loss_weight_sum', *_worst(abs(got['loss_weight_sum'] - want['loss_weight_sum']), n * FIXED / 2))
        criterion('confusion', *_worst(np.abs(confusion - want['confusion']),
                                       ATOL * counts[:, None] + n * FIXED + RTOL * np.abs(want['confusion'])))
        criterion('distance_matrix', *_worst(np.abs(distance - want['distance_matrix']),
                                             ATOL * used[:, None] + n * FIXED + RTOL * np.abs(want['distance_matrix'])))
    return failed, ratios


def tables_for(g, mix=False, class_weights=False, loss_weights=False):
    """keyword arguments of an evaluation from three switches"""
    matrix, weights = tables(g)
    return dict(mix=matrix if mix else None, class_weights=weights if class_weights else None,
                loss_weights=weights if loss_weights else None)


_references = {}


def reference(name, g, k=3, mix=False, class_weights=False, loss_weights=False):
    """restate() of a family, computed once per set of switches (k does not enter: topk_by_k holds every k)"""
    key = (name, mix, class_weights, loss_weights)
    if key not in _references:
        _references[key] = restate(*family(name, g), **tables_for(g, mix, class_weights, loss_weights))
    return _references[key]


# ---- extreme: one frame at a time ------------------------------------------------------------------------------------

def only_frame(labels, t):
    out = torch.full_like(labels, -100)
    out[0, t] = labels[0, t]
    return out


def frame_by_frame(evaluate, g, mix, loss_weights):
    """(loss (197,), jsd (197,)) of any evaluation of `extreme`, every label but one masked"""
    logits, labels, _ = family('extreme', g)
    kwargs = tables_for(g, mix=mix, loss_weights=loss_weights)
    out = [evaluate(logits, only_frame(labels, t), **kwargs) for t in range(labels.shape[1])]
    return np.array([o['loss_sum'] for o in out]), np.array([o['jsd_sum'] for o in out])


def extreme_reference(g, mix, loss_weights):
    """-> (loss (197,) float64 with the clamp, jsd (197,), avg (40, 197), unit (40, 197)): unit enlarged by what the
    fp32 softmax leaves unknown"""
    key = ('extreme/frames', mix, loss_weights)
    if key not in _references:
        logits, labels, _ = family('extreme', g)
        kwargs = tables_for(g, mix=mix, loss_weights=loss_weights)
        loss = np.array([restate(logits, only_frame(labels, t), **kwargs)['loss_sum'] for t in range(labels.shape[1])])
        probs = torch.softmax(logits[0].double(), dim=0)
        onehot = torch.nn.functional.one_hot(labels[0], NP).double().T
        jsd, avg, unit = distance64(probs, onehot, kwargs['mix'])
        a = probs.float().clamp(1e-8, 1 - 1e-8).double()
        b = onehot.float().clamp(1e-8, 1 - 1e-8).double()
        if mix:
            a, b = kwargs['mix'].double() @ a, kwargs['mix'].double() @ b
        a, m = a.numpy(), ((a + b) / 2).numpy()
        _references[key] = (loss, jsd, avg, unit + DELTA * a * np.abs(np.log(a) - np.log(m)) / 2)
    return _references[key]


def extreme_loss_ratio(loss, g, mix, loss_weights):
    """worst |loss - min(ref, 2^20)| / (2^-33 + 8 * 2^-24 max(1, |ref|)); inf where a frame that must add exactly
    2^20 (its label's logit is -inf) does not"""
    want = extreme_reference(g, mix, loss_weights)[0]
    loss = np.asarray(loss, dtype=np.float64)
    capped = want == LOSS_CLAMP
    assert int(capped.sum()) == 8
    if not np.array_equal(loss[capped], want[capped]):
        return float('inf')
    return _worst(np.abs(loss - want), FIXED / 2 + DELTA * np.maximum(1.0, np.abs(want)))[1]


def extreme_jsd_kappa(jsd, g, mix, loss_weights=False, ceiling=4096.0):
    """the smallest kappa at which every frame is inside E_t(kappa) + 2^-33, to 1 %, from above"""
    _, want, avg, unit = extreme_reference(g, mix, loss_weights)
    error = np.abs(np.asarray(jsd, dtype=np.float64) - want)
    if not (error <= distance_bound(avg, unit, ceiling) + FIXED / 2).all():
        return ceiling
    lo, hi = np.zeros_like(error), np.full_like(error, ceiling)
    for _ in range(40):
        mid = 0.5 * (lo + hi)
        ok = error <= distance_bound(avg, unit, mid) + FIXED / 2
        lo, hi = np.where(ok, lo, mid), np.where(ok, mid, hi)
    return float(np.where(error <= FIXED / 2, 0.0, hi).max())


# ---- mutants ---------------------------------------------------------------------------------------------------------

MUTANTS = ('argmax_tie_highest', 'topk_tie_label_first', 'trip_dropped', 'trip_twice', 'run_tail_lost',
           'hole_breaks_row', 'batch_stride', 'length_inclusive', 'loss_unclamped')
ADDITIVE = ('count', 'true_positives', 'topk_correct', 'topk_by_k', 'invalid_labels', 'class_total', 'class_count',
            'loss_sum', 'jsd_sum', 'loss_weight_sum', 'distance_matrix', 'distance_rows', 'confusion')


def mutant(kind):
    """restate() with one fault, as an evaluation of the same signature.
    argmax_tie_highest    both argmaxes give a tie to the highest index
    topk_tie_label_first  the rank of the label counts only strictly larger logits
    trip_dropped          frames at or beyond 32768 (the first trip of the grid) are not counted
    trip_twice            tiles 256 .. 511 are added twice
    run_tail_lost         a run of two or more equal labels loses its last frame in `confusion`
    hole_breaks_row       the frame after a -100 frame adds its probabilities to the previous labelled frame's row
    batch_stride          frames == 1 read as if frames == 64: a wave's 64 lanes all take its first frame's batch item
    length_inclusive      t <= lengths[b] counts
    loss_unclamped        no [0, 2^20]"""
    assert kind in MUTANTS

    def evaluate(logits, labels, lengths=None, k=3, mix=None, class_weights=None, loss_weights=None):
        kwargs = dict(k=k, mix=mix, class_weights=class_weights, loss_weights=loss_weights)
        if kind == 'loss_unclamped':
            kwargs['loss_clamp'] = None
        if kind == 'length_inclusive' and lengths is not None:
            lengths = torch.as_tensor(lengths) + 1
        labels = masked_labels(labels, lengths)
        batch, classes, frames = logits.shape
        if kind == 'batch_stride' and frames == 1:
            logits = logits[torch.arange(batch) // 64 * 64]
        if kind == 'trip_dropped':
            labels.view(-1)[FIRST_TRIP:] = -100
        out = restate(logits, labels, **kwargs)
        flat = labels.flatten()
        if kind == 'argmax_tie_highest':
            mirrored = torch.where(flat >= 0, classes - 1 - flat, flat).view_as(labels)
            kwargs['class_weights'] = None if class_weights is None else class_weights.flip(0)
            other = restate(logits.flip(1), mirrored, **kwargs)
            out.update(true_positives=other['true_positives'], class_total=other['class_total'][::-1].copy(),
                       distance_matrix=other['distance_matrix'][::-1, ::-1].copy(),
                       distance_rows=other['distance_rows'][::-1].copy())
        if kind == 'topk_tie_label_first':
            keep = flat != -100
            rows = logits.float().transpose(1, 2).flatten(0, 1)[keep]
            ahead = (rows > rows.gather(1, flat[keep][:, None])).sum(dim=1)
            out['topk_by_k'] = np.array([int((ahead < j).sum()) for j in range(1, 9)])
            out['topk_correct'] = int(out['topk_by_k'][k - 1])
        if kind == 'trip_twice':
            again = torch.full_like(flat, -100)
            again[FIRST_TRIP:2 * FIRST_TRIP] = flat[FIRST_TRIP:2 * FIRST_TRIP]
            other = restate(logits, again.view_as(labels), **kwargs)
            out = {key: out[key] + other[key] for key in ADDITIVE}
        if kind in ('run_tail_lost', 'hole_breaks_row'):
            at = (flat != -100).nonzero()[:, 0]
            kept = flat[at]
            changed = torch.full_like(flat, -100)
            if kind == 'run_tail_lost' and len(at) > 1:
                first = torch.cat([torch.tensor([True]), kept[1:] != kept[:-1]])
                last = torch.cat([kept[1:] != kept[:-1], torch.tensor([True])])
                tails = at[last & ~first]
                changed[tails] = flat[tails]
                out['confusion'] = out['confusion'] - restate(logits, changed.view_as(labels), **kwargs)['confusion']
            if kind == 'hole_breaks_row' and len(at) > 1:
                changed[at] = kept
                after_hole = torch.cat([torch.tensor([False]), at[1:] - at[:-1] > 1])
                changed[at[after_hole]] = kept[:-1][after_hole[1:]]
                out['confusion'] = restate(logits, changed.view_as(labels), **kwargs)['confusion']
        return out
    return evaluate
