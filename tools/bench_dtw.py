"""HIP-event time of ppgs_amd.dtw against the plain PyTorch formulation of the same thing on the same GPU: the cost
matrix by broadcasting, the dynamic programme as a loop over anti-diagonals.

    python tools/bench_dtw.py [--out profiles/dtw_bench.json] [--trace-only]

Four workloads: one 1000 x 1000 pair (distance only; with the path), 256 such pairs in one call, and 10 000 ragged
pairs of 50 to 600 frames.  Median of the timed calls after warm-up calls of the same shape; every timed window
ends in an event synchronise.  The torch formulation is timed on fewer pairs where it is slow (the record says how
many) and keeps its results on the device.  The record also holds the cell rate: cells of the cost table per
second, each cell 40 logs and 40 square roots.
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ppgs_amd import dtw  # noqa: E402


def torch_cost(x, y, mix):
    """(B, 40, Tx), (B, 40, Ty) -> (B, Tx, Ty), the per-frame term of ppgs_amd.distance for every frame pair"""
    x, y = x.clamp(1e-8, 1 - 1e-8), y.clamp(1e-8, 1 - 1e-8)
    if mix is not None:
        x, y = mix @ x, mix @ y
    a, b = x.transpose(1, 2)[:, :, None, :], y.transpose(1, 2)[:, None, :, :]
    log_m = torch.log((a + b) / 2)
    kl = (a * (torch.log(a) - log_m) + b * (torch.log(b) - log_m)) / 2
    return torch.sqrt(kl.clamp(min=0)).sum(-1)


def torch_dtw(x, y, lengths_x, lengths_y, mix=None, chunk_bytes=2 << 30):
    """total (B,) of the same recurrence with torch ops (no step count, no path)"""
    pairs, _, frames_x = x.shape
    frames_y = y.shape[2]
    group = max(1, chunk_bytes // (frames_x * frames_y * 40 * 4 * 4))
    cost = torch.cat([torch_cost(x[at:at + group], y[at:at + group], mix) for at in range(0, pairs, group)])
    table = torch.full((pairs, frames_x + 1, frames_y + 1), float('inf'), device=x.device)
    table[:, 0, 0] = 0
    rows = torch.arange(frames_x, device=x.device)
    for d in range(frames_x + frames_y - 1):
        i = rows[max(0, d - frames_y + 1):min(d, frames_x - 1) + 1]
        j = d - i
        best = torch.minimum(torch.minimum(table[:, i, j], table[:, i, j + 1]), table[:, i + 1, j])
        table[:, i + 1, j + 1] = cost[:, i, j] + best
    return table[torch.arange(pairs, device=x.device), lengths_x, lengths_y]


def timed(call, warmup, repeats):
    for _ in range(warmup):
        call()
    torch.cuda.synchronize()
    times = []
    for _ in range(repeats):
        start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        call()
        end.record()
        end.synchronize()
        times.append(start.elapsed_time(end))
    return statistics.median(times)


def ppgs(pairs, frames, generator):
    return torch.softmax(3 * torch.randn(pairs, 40, frames, generator=generator), dim=1).cuda()


def main():
    parser = argparse.ArgumentParser()
    parser.add_argument('--out', default=None)
    parser.add_argument('--trace-only', action='store_true', help='a few calls of each workload and nothing else')
    parser.add_argument('--ragged', type=int, default=10000)
    args = parser.parse_args()
    generator = torch.Generator().manual_seed(0)
    similarity = torch.rand(40, 40, generator=generator) * 0.5 + torch.eye(40)
    keywords = dict(similarity=similarity, reduction='sum')
    mix = (similarity.T ** 1.2).cuda()
    x, y = ppgs(256, 1000, generator), ppgs(256, 1000, generator)
    lengths_x = torch.randint(50, 601, (args.ragged,), generator=generator)
    lengths_y = torch.randint(50, 601, (args.ragged,), generator=generator)
    rx, ry = ppgs(args.ragged, 600, generator), ppgs(args.ragged, 600, generator)
    ragged = dict(lengths_x=lengths_x, lengths_y=lengths_y, **keywords)
    full = torch.full((256,), 1000)
    calls = {
        'single_distance': lambda: dtw.distance(x[0], y[0], **keywords),
        'single_path': lambda: dtw.align(x[0], y[0], similarity=similarity),
        'batch_256': lambda: dtw.distance(x, y, **keywords),
        'ragged': lambda: dtw.distance(rx, ry, **ragged),
    }
    if args.trace_only:
        for call in calls.values():
            for _ in range(3):
                call()
        torch.cuda.synchronize()
        return
    subset = min(256, args.ragged)
    baselines = {
        'single_distance': (1, lambda: torch_dtw(x[:1], y[:1], full[:1], full[:1], mix)),
        'batch_256': (16, lambda: torch_dtw(x[:16], y[:16], full[:16], full[:16], mix)),
        'ragged': (subset, lambda: torch_dtw(rx[:subset], ry[:subset], lengths_x[:subset].cuda(),
                                             lengths_y[:subset].cuda(), mix)),
    }
    # same numbers first: the torch formulation sums in another order, so to rounding only
    got = dtw.distance(x[:2], y[:2], **keywords)
    want = torch_dtw(x[:2], y[:2], full[:2], full[:2], mix)
    assert torch.allclose(got, want, rtol=1e-4), (got, want)
    got = dtw.distance(rx[:8], ry[:8], lengths_x=lengths_x[:8], lengths_y=lengths_y[:8], **keywords)
    want = torch_dtw(rx[:8], ry[:8], lengths_x[:8].cuda(), lengths_y[:8].cuda(), mix)
    assert torch.allclose(got, want, rtol=1e-4), (got, want)
    record = {'device': torch.cuda.get_device_name(0), 'unit': 'milliseconds, median (HIP events)'}
    cells = {'single_distance': 1e6, 'single_path': 1e6, 'batch_256': 256e6,
             'ragged': float((lengths_x * lengths_y).sum())}
    pairs = {'single_distance': 1, 'single_path': 1, 'batch_256': 256, 'ragged': args.ragged}
    for name, call in calls.items():
        heavy = name in ('batch_256', 'ragged')
        time = timed(call, 3 if heavy else 20, 10 if heavy else 100)
        entry = {'pairs': pairs[name], 'ms': round(time, 4), 'us_per_pair': round(1e3 * time / pairs[name], 3),
                 'cells_per_second': round(cells[name] / (time * 1e-3), -6)}
        if name in baselines:
            count, baseline = baselines[name]
            base = timed(baseline, 1, 3)
            entry.update(torch_pairs=count, torch_ms=round(base, 3), torch_us_per_pair=round(1e3 * base / count, 1),
                         ratio_per_pair=round((base / count) / (time / pairs[name]), 1))
        record[name] = entry
    print(json.dumps(record))
    if args.out:
        with open(args.out, 'w') as file:
            json.dump(record, file, indent=1)
            file.write('\n')


if __name__ == '__main__':
    main()
