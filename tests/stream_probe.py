"""Shared by tests/test_stream_probe_host.py and tests/test_gpu_stream_probe.py: push schedules for the KV-cached
streams (Stream, BatchedStream, LongStream), the Python restatement of the row-range rule of ppg_stream_push_batch,
and drivers that push a schedule through a stream and hold it to the emission rule.

A schedule is a list of steps, each `(counts, flush)` with one entry per item: `counts[b]` new frames of item b (0 =
the item sits the step out, unless it is flushed) and `flush[b]`.  Item b's OWN pushes -- their sizes, in order -- are
a function of b and the size list alone; `seed` only moves them in time (a delay before the first push, other sit-out
steps), so that two schedules of different seeds give every item the same pushes beside neighbours that do something
else.  The float64 references are those of tests/encoder_params.py and tests/attention_probe.py: a causal item's
logits inside its length are those of its utterance alone.
"""
import numpy as np
import torch

from ppgs_amd import config

# the push sizes of test_gpu_parity.py::test_batched_kv_cached_streams_equal_causal_forward
SIZES = [16, 48, 7, 100, 1, 64, 33, 90, 2, 76, 130, 49, 5]
# Item b's k-th push takes SIZES[(k + offset(b)) % 13] frames.  The existing test's offset, 3 b, spreads the large
# pushes of the twelve-item probe batch so evenly that no step touches more than 30 of its 86 row blocks (every phase
# of it tried); with two offsets the large items' 130- and 90-frame pushes meet in one step (40 blocks, and 67 of the
# staircase batch's 185), beside steps of 1 .. 20 -- tests/test_stream_probe_host.py holds the schedules to that.
def offset(b):
    return 3 * (b % 2) + 7


# items of at least this many frames sit at least one step out before they end
SIT_OUT_FROM = 40
NAMES = ('whole', 'sixteens', 'ones', 'ragged', 'ragged2')


def _sits_out(seed, step, b):
    if seed is None:
        return False
    if seed == 0:
        return (step + b) % 5 == 4                      # as the existing batched test does
    return step < (b * seed) % 3 or (step + 2 * b + seed) % 7 == 3


def schedule(totals, sizes, seed=None):
    """The steps that push `totals[b]` frames of item b: its k-th push takes sizes[(k + offset(b)) % len(sizes)]
    frames (ragged, unaligned, an offset per item as in the existing batched test), the push that completes it carries its
    flush (an item of 0 frames is flushed with nothing received, an item of 1 frame pushed and flushed in one step).
    seed None: no item ever sits out (`whole`, `sixteens`, `ones`).  Otherwise item b sits out the steps the seed
    picks for it, and an item of >= SIT_OUT_FROM frames that would end without ever having sat out sits out first."""
    batch = len(totals)
    sent, pushes, sat, done, steps = [0] * batch, [0] * batch, [False] * batch, [False] * batch, []
    step = -1
    while not all(done):
        step += 1
        counts, flush = [], []
        for b in range(batch):
            n = min(sizes[(pushes[b] + offset(b)) % len(sizes)], totals[b] - sent[b])
            ends = sent[b] + n == totals[b]
            sit = done[b] or _sits_out(seed, step, b)
            if seed is not None and not done[b] and ends and totals[b] >= SIT_OUT_FROM and not sat[b]:
                sit = True
            if sit:
                counts.append(0)
                flush.append(False)
                sat[b] = sat[b] or not done[b]
                continue
            counts.append(n)
            flush.append(ends)
            sent[b] += n
            pushes[b] += 1
            done[b] = ends
        if any(counts) or any(flush):                   # (a step in which every item sits out is no step)
            steps.append((counts, flush))
        assert step <= 4 * (max(totals) + 8), 'the schedule does not end'
    return steps


def named(name, totals):
    if name == 'whole':
        return schedule(totals, [max(max(totals), 1)])
    if name == 'sixteens':
        return schedule(totals, [16])
    if name == 'ones':
        return schedule(totals, [1])
    if name == 'ragged':
        return schedule(totals, SIZES, seed=0)
    if name == 'ragged2':
        return schedule(totals, SIZES, seed=1)
    raise KeyError(name)


def small_then_near_full(totals, small=20):
    """Two steps: `small` frames of every item (rows 0 .. 15 cached), then the rest with the flush -- the cadence of
    test_gpu_parity.py::test_stream_near_full_push_after_small_push.  An item of at most `small` frames ends in the
    first step."""
    first = [min(small, n) for n in totals]
    return [(first, [n <= small for n in totals]),
            ([n - f for n, f in zip(totals, first)], [n > small for n in totals])]


def own_pushes(steps, b):
    """The sizes of item b's pushes, in order (a flush of nothing received counts as a push of 0)."""
    return [counts[b] for counts, flush in steps if counts[b] > 0 or flush[b]]


def round_up(n, m):
    return (n + m - 1) // m * m


def blocks_per_step(totals, steps):
    """The number of 16-row blocks of the residual stream each step touches -- ppg_stream_push_batch's row-range rule:
    an active item (new frames or a flush) has x_new = received - 2 (received at its flush) final residual rows and
    recomputes rows x_prev // 16 * 16 .. round_up(x_new, 16)."""
    received, x_valid = [0] * len(totals), [0] * len(totals)
    blocks = []
    for counts, flush in steps:
        touched = 0
        for b, (n, fl) in enumerate(zip(counts, flush)):
            if n == 0 and not fl:
                continue
            received[b] += n
            x_new = received[b] if fl else max(received[b] - 2, 0)
            touched += (round_up(x_new, 16) - x_valid[b] // 16 * 16) // 16
            x_valid[b] = x_new
        blocks.append(touched)
    return blocks


def ffn_splits(blocks, cap, num_cus=256):
    """The hidden splits the PER-STEP rule gave the FFN launch of a step of `blocks` row blocks (until the bitwise tests
    showed what it does to a recomputed row): doubled while the workgroups (one per four blocks, times the splits) still
    fit the chip, up to `cap` (half the hidden chunks: 16 in the 16-bit modes at hidden 256, 32 in fp32 and at hidden
    512).  Steps on different sides of a threshold of it summed the FFN in different orders."""
    wgs, splits = (blocks + 3) // 4, 1
    while splits * 2 <= cap and wgs * splits * 2 <= num_cus:
        splits *= 2
    return splits


def ffn_groups(batch, cap, num_cus=256):
    """The hidden groups of a stream of `batch` items (ppg_stream_create_batch): what the per-step rule gave a step of
    two row blocks per item, fixed for the life of the stream."""
    return ffn_splits(2 * batch, cap, num_cus)


def ffn_closed(blocks, groups, num_cus=256):
    """Whether a step of `blocks` row blocks walks the groups in ONE workgroup per token tile that closes its accumulator
    at the group boundaries and applies LayerNorm-2 itself (hidden 256: ffn_closed_kernel) instead of one workgroup per
    group and a reduce pass: more than two rounds of workgroups."""
    return groups > 1 and (blocks + 3) // 4 * groups > 2 * num_cus


# ---- drivers ---------------------------------------------------------------------------------------------------------

def drive(stream, feats, steps, softmax=False):
    """Push `steps` through a BatchedStream; feats[b] is item b's (channels, total) utterance on the host.  The chunk
    tensor of a step is NaN behind counts[b].  After every step every item has emitted `sent` frames once flushed and
    max(sent - 4, 0) before (both convolutions look two frames ahead).  -> per item the (40, total) outputs, numpy."""
    batch = len(feats)
    channels = feats[0].shape[0]
    sent, done, pieces = [0] * batch, [False] * batch, [[] for _ in range(batch)]
    for index, (counts, flush) in enumerate(steps):
        nmax = max(counts)
        chunk = torch.full((batch, channels, nmax), float('nan'), dtype=feats[0].dtype)
        for b in range(batch):
            chunk[b, :, :counts[b]] = feats[b][:, sent[b]:sent[b] + counts[b]]
        out = stream.push(chunk.cuda() if nmax else None, counts, flush, softmax=softmax)
        for b in range(batch):
            sent[b] += counts[b]
            done[b] = done[b] or flush[b]
            pieces[b].append(out[b])
            emitted = sum(p.shape[1] for p in pieces[b])
            expected = sent[b] if done[b] else max(sent[b] - 4, 0)
            assert emitted == expected, f'step {index} item {b}: {emitted} frames emitted, {expected} expected'
    assert all(done) and [int(f.shape[1]) for f in feats] == sent
    torch.cuda.synchronize()
    return [torch.cat(p, dim=1).cpu().numpy() for p in pieces]


def push_sizes(total, size):
    """`total` frames in pushes of `size` (the last one shorter)."""
    return [min(size, total - at) for at in range(0, total, size)]


def cycle_sizes(total, sizes=SIZES, offset=0):
    """`total` frames in pushes of sizes[offset], sizes[offset + 1], ... (cyclic, the last one cut)."""
    out, index = [], offset
    while sum(out) < total:
        out.append(min(sizes[index % len(sizes)], total - sum(out)))
        index += 1
    return out


def drive_one(stream, feats, sizes, softmax=False):
    """Push the (channels, total) utterance through a Stream or a LongStream in pushes of `sizes`, the flush as a push
    of its own.  Stream: max(sent - 4, 0) frames emitted after every push.  LongStream: never more than that (a
    window's kept rows start behind its first 50), and never more than two windows alive.  -> (40, total) numpy."""
    assert sum(sizes) == feats.shape[1]
    exact = not hasattr(stream, '_windows')
    pieces, sent = [], 0
    for n in sizes:
        pieces.append(stream.push(feats[:, sent:sent + n].cuda(), softmax=softmax))
        sent += n
        emitted = sum(p.shape[1] for p in pieces)
        if exact:
            assert emitted == max(sent - 4, 0), f'{emitted} frames emitted after {sent}'
        else:
            assert emitted <= max(sent - 4, 0) and len(stream._windows) <= 2
    pieces.append(stream.push(None, flush=True, softmax=softmax))
    torch.cuda.synchronize()
    out = torch.cat(pieces, dim=1).cpu().numpy()
    assert out.shape[1] == sent, f'{out.shape[1]} frames emitted of {sent}'
    return out


def rows_of(max_frames):
    """Rows per item of a stream of `max_frames` frames (R of ppg_stream_create_batch)."""
    assert 1 <= max_frames <= config.CHUNK_LENGTH
    return round_up(max_frames, 32)


def same_bits(a, b):
    """Equal in every bit (the int32 view: NaNs and signed zeros count)."""
    a, b = np.ascontiguousarray(a, dtype=np.float32), np.ascontiguousarray(b, dtype=np.float32)
    return a.shape == b.shape and torch.equal(torch.from_numpy(a).view(torch.int32), torch.from_numpy(b).view(torch.int32))
