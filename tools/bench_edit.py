"""HIP-event time of the edit distance (ppg_edit_distance through engine.edit_pairs) against the plain PyTorch
formulation of the same thing on the same GPU: the substitution costs by a broadcast compare, the dynamic programme as a
loop over anti-diagonals.

    python tools/bench_edit.py [--out profiles/edit_bench.json]

Three workloads under the unit costs, on token tables already on the device: one 4096 x 4096 pair, 256 pairs of
1000 x 1000, and 10 000 ragged pairs of 20 to 200 tokens, each without and with the operations.  Median of the timed
calls after warm-up calls of the same shape; every timed window ends in an event synchronise.  The torch formulation
gives totals only, is timed on fewer pairs where it is slow (the record says how many) and keeps its results on the
device.  The record also holds the time of one four-cell step of the programme: the single pair is 16 blocks of
4096 + 64 steps, one wave, nothing else on the device (DESIGN 4.9 has the same figure for dtw_programme).
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ppgs_amd import engine  # noqa: E402


def torch_edit(ref, hyp, lengths_ref, lengths_hyp):
    """total (B,) of the same recurrence under the unit costs with torch ops (no counts, no operations)"""
    pairs, rows = ref.shape
    columns = hyp.shape[1]
    device = ref.device
    cost = (ref[:, :, None] != hyp[:, None, :]).to(torch.float32)
    table = torch.empty((pairs, rows + 1, columns + 1), device=device)
    table[:, 0, :] = torch.arange(columns + 1, device=device)
    table[:, :, 0] = torch.arange(rows + 1, device=device)[None]
    index = torch.arange(rows, device=device)
    for d in range(rows + columns - 1):
        i = index[max(0, d - columns + 1):min(d, rows - 1) + 1]
        j = d - i
        best = torch.minimum(torch.minimum(table[:, i, j] + cost[:, i, j], table[:, i, j + 1] + 1),
                             table[:, i + 1, j] + 1)
        table[:, i + 1, j + 1] = best
    return table[torch.arange(pairs, device=device), lengths_ref.long(), lengths_hyp.long()]


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


def main():
    parser = argparse.ArgumentParser()
    parser.add_argument('--out', default=None)
    parser.add_argument('--ragged', type=int, default=10000)
    args = parser.parse_args()
    generator = torch.Generator().manual_seed(0)

    def table(pairs, width, low, high):
        tokens = torch.randint(0, 40, (pairs, width), generator=generator, dtype=torch.int32).cuda()
        lengths = torch.randint(low, high + 1, (pairs,), generator=generator, dtype=torch.int32).cuda()
        return tokens, lengths
    workloads = {
        'single_4096': table(1, 4096, 4096, 4096) + table(1, 4096, 4096, 4096),
        'batch_256x1000': table(256, 1000, 1000, 1000) + table(256, 1000, 1000, 1000),
        'ragged_20_200': table(args.ragged, 200, 20, 200) + table(args.ragged, 200, 20, 200),
    }
    torch_pairs = {'single_4096': 1, 'batch_256x1000': 16, 'ragged_20_200': min(1024, args.ragged)}
    record = {'device': torch.cuda.get_device_name(0), 'unit': 'milliseconds, median (HIP events)',
              'costs': 'unit', 'library': engine.library_sha16()}
    for name, (ref, lengths_ref, hyp, lengths_hyp) in workloads.items():
        pairs = ref.shape[0]
        cells = float((lengths_ref.long() * lengths_hyp.long()).sum())
        count = torch_pairs[name]
        part = (ref[:count], hyp[:count], lengths_ref[:count], lengths_hyp[:count])
        # same numbers first: under the unit costs every value is a small integer, so exactly
        got = engine.edit_pairs(part[0], part[1], part[2], part[3])[0]
        want = torch_edit(*part)
        assert torch.equal(got, want), (name, got, want)
        entry = {'pairs': pairs}
        for label, want_ops in (('distance', False), ('ops', True)):
            time = timed(lambda: engine.edit_pairs(ref, hyp, lengths_ref, lengths_hyp, want_ops=want_ops),
                         3 if pairs > 1 else 10, 10 if pairs > 1 else 30)
            entry[label] = {'ms': round(time, 4), 'us_per_pair': round(1e3 * time / pairs, 3),
                            'cells_per_second': round(cells / (time * 1e-3), -6)}
        base = timed(lambda: torch_edit(*part), 1, 3)
        entry['torch'] = {'pairs': count, 'ms': round(base, 3), 'us_per_pair': round(1e3 * base / count, 1)}
        entry['ratio_per_pair'] = round((base / count) / (entry['distance']['ms'] / pairs), 1)
        record[name] = entry
    steps = 16 * (4096 + 64)
    record['programme_step_ns'] = {
        'distance': round(1e6 * record['single_4096']['distance']['ms'] / steps, 1),
        'ops': round(1e6 * record['single_4096']['ops']['ms'] / steps, 1),
        'steps': steps, 'note': 'whole call of the single pair over its four-cell steps; with ops the trace-back is in it'}
    print(json.dumps(record))
    if args.out:
        with open(args.out, 'w') as file:
            json.dump(record, file, indent=1)
            file.write('\n')


if __name__ == '__main__':
    main()
