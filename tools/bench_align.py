"""HIP-event time of the alignment and search entries of ppg_align.hip at the shapes DESIGN quotes:

    python tools/bench_align.py [--label head] [--out profiles/align_bench.json]

Eight workloads through the package's Python calls, softmax scale 3:
    engine.align_items      64 x 1000 x 120 and 1 x 4096 x 1024 (utterances x frames x phonemes), each plain and with
                            every second phoneme optional
    engine.search_items     1 x 100 000 x 1 of 8 and 64 x 1000 x 8 of 8 (recordings x frames x queries of N), top = 1
    SearchStream.push       64 x 16 x 8 and 1 x 1000 x 64 (streams x frames x queries of 8), threshold -1, patience 25
Median of 20 timed calls after 5 warm-up calls of the same shape; every timed window ends in an event synchronise.

One run is one process and gives one median per workload.  With --out the run is appended to the runs of its --label in
that file, so that builds can be compared on one machine with their runs interleaved: the tool needs nothing but the
package's Python side, and PPGS_AMD_LIB selects the library (an earlier build's beside the current one).  A change is
held against the spread of the build it replaces: the largest minus the smallest of that build's medians.
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ppgs_amd import alignment, engine  # noqa: E402

WARMUP, REPEATS = 5, 20


def timed(call):
    for _ in range(WARMUP):
        call()
    torch.cuda.synchronize()
    times = []
    for _ in range(REPEATS):
        start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        call()
        end.record()
        end.synchronize()
        times.append(start.elapsed_time(end))
    return statistics.median(times)


def ppgs(items, frames, generator):
    return torch.softmax(3 * torch.randn(items, 40, frames, generator=generator), dim=1).cuda()


def align_calls(items, frames, count, generator):
    x = ppgs(items, frames, generator)
    table = torch.randint(0, 40, (items, count), generator=generator, dtype=torch.int32).cuda()
    flags = (torch.arange(count) % 2).to(torch.int32).repeat(items, 1).cuda()          # every second phoneme
    lengths, counts = [frames] * items, [count] * items
    return (lambda: engine.align_items(x, lengths, table, counts),
            lambda: engine.align_items(x, lengths, table, counts, optional=flags))


def search_call(items, frames, queries, count, generator):
    x = ppgs(items, frames, generator)
    table = torch.randint(0, 40, (queries, count), generator=generator, dtype=torch.int32).cuda()
    lengths, counts = [frames] * items, [count] * queries
    return lambda: engine.search_items(x, lengths, table, counts, top=1)


def push_call(streams, frames, queries, generator):
    x = ppgs(streams, frames, generator)
    table = torch.randint(0, 40, (queries, 8), generator=generator).tolist()
    spotter = alignment.SearchStream(table, threshold=-1., patience=25, batch=streams)
    return lambda: spotter.push(x)


def main():
    parser = argparse.ArgumentParser()
    parser.add_argument('--out', default=None)
    parser.add_argument('--label', default='head')
    args = parser.parse_args()
    generator = torch.Generator().manual_seed(0)
    calls = {}
    calls['align_64x1000x120'], calls['align_optional_64x1000x120'] = align_calls(64, 1000, 120, generator)
    calls['align_1x4096x1024'], calls['align_optional_1x4096x1024'] = align_calls(1, 4096, 1024, generator)
    calls['search_1x100000x1of8'] = search_call(1, 100000, 1, 8, generator)
    calls['search_64x1000x8of8'] = search_call(64, 1000, 8, 8, generator)
    calls['push_64x16x8'] = push_call(64, 16, 8, generator)
    calls['push_1x1000x64'] = push_call(1, 1000, 64, generator)
    run = {name: round(timed(call), 5) for name, call in calls.items()}
    print(json.dumps({'label': args.label, 'ms': run}))
    if args.out:
        record = {}
        if os.path.exists(args.out):
            with open(args.out) as file:
                record = json.load(file)
        record.setdefault('device', torch.cuda.get_device_name(0))
        record.setdefault('unit', f'milliseconds, median of {REPEATS} (HIP events), one entry per process')
        record.setdefault('runs', {}).setdefault(args.label, []).append(run)
        with open(args.out, 'w') as file:
            json.dump(record, file, indent=1)
            file.write('\n')


if __name__ == '__main__':
    main()
