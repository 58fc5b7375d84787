"""HIP-event time of a push of the live phrase search over a phoneme graph (ppg_search_graph_stream_push)
and of its yardsticks:

    python tools/bench_search_graph_stream.py [--label head] [--out profiles/search_graph_stream_bench.json]
    rocprofv3 --kernel-trace --output-format csv -d DIR -- python tools/bench_search_graph_stream.py --trace-only
    python tools/bench_search_graph_stream.py --split DIR/.../*_kernel_trace.csv [--out ...]

Workloads (streams x frames of one push x graphs), softmax scale 3: 1 x 16 x 1, 64 x 16 x 8 and 1 x 1000 x 64, each on
the `chain` (8 states) and the `phrase` (20 states) of tools/bench_search_graph.py:
    push           SearchGraphStream.push of that many frames into every stream, all graphs on every stream
beside, measured in the same process on the same device,
    search_graph   engine.search_graph_items over the pushed frames alone: the whole-recording call on the same frames
    history        engine.search_graph_items over a history of 100000 frames per stream: what a live user pays per
                   push without the live form
    search_stream  SearchStream.push on the same chain, as many queries as graphs: the live chain search
Median of 20 timed calls after 5 warm-up calls of the same shape; every timed window ends in an event synchronise.
With --out the run is appended to the runs of its --label in that file.  --trace-only makes three untimed calls of
every entry and nothing else: the run to put under a rocprofv3 kernel trace.  --split reads that trace: every call
launches exactly one *_programme kernel, so the k-th three of them in start order belong to the k-th entry; printed
and, with --out, stored under 'kernel_split': the median microseconds of the programme and its nanoseconds per frame
(one wave walks the frames of one pair; the pairs of a call run side by side).
"""
import argparse
import csv
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ppgs_amd import alignment, engine  # noqa: E402

from bench_search_graph import graphs, packed, timed  # noqa: E402

SHAPES = [(1, 16, 1), (64, 16, 8), (1, 1000, 64)]
HISTORY = 100000
WORKSPACE = 4 << 30                           # every yardstick is one call of the library: one programme kernel
NAMES = ('chain', 'phrase')


def plan():
    """The entries of a run in their fixed order, without a device: [(name, frames)]."""
    out = []
    for streams, frames, count in SHAPES:
        shape = f'{streams}x{frames}x{count}'
        for name in NAMES:
            out += [(f'push_{name}_{shape}', frames), (f'search_graph_{name}_{shape}', frames),
                    (f'history_{name}_{streams}x{HISTORY}x{count}', HISTORY)]
        out += [(f'search_stream_chain_{shape}', frames)]
    return out


def entries():
    """The calls of a run in the order of `plan`: {name: (call, frames)}."""
    generator = torch.Generator(device='cuda').manual_seed(0)
    sequence, named = graphs()
    calls = {}
    for streams, frames, count in SHAPES:
        history = torch.softmax(3 * torch.randn(streams, 40, HISTORY, generator=generator, device='cuda'), dim=1)
        x = history[:, :, :frames].contiguous()
        shape = f'{streams}x{frames}x{count}'
        for name in NAMES:
            spotter = alignment.SearchGraphStream([named[name]] * count, -1., batch=streams)
            given = packed(named[name], count)
            calls[f'push_{name}_{shape}'] = (lambda spotter=spotter, x=x: spotter.push(x), frames)
            calls[f'search_graph_{name}_{shape}'] = (
                lambda x=x, given=given, lengths=[frames] * streams: engine.search_graph_items(
                    x, lengths, **given, workspace_bytes=WORKSPACE), frames)
            calls[f'history_{name}_{streams}x{HISTORY}x{count}'] = (
                lambda x=history, given=given, lengths=[HISTORY] * streams: engine.search_graph_items(
                    x, lengths, **given, workspace_bytes=WORKSPACE), HISTORY)
        chain = alignment.SearchStream([sequence] * count, -1., batch=streams)
        calls[f'search_stream_chain_{shape}'] = (lambda chain=chain, x=x: chain.push(x), frames)
    assert [(name, frames) for name, (_, frames) in calls.items()] == plan()
    return named, calls


def split(trace, out):
    with open(trace) as file:
        rows = sorted(csv.DictReader(file), key=lambda row: int(row['Start_Timestamp']))
    spans = [int(row['End_Timestamp']) - int(row['Start_Timestamp']) for row in rows if 'programme' in row['Kernel_Name']]
    assert len(spans) == 3 * len(plan()), (len(spans), len(plan()))
    table = {}
    print('entry                                   programme us    ns per frame   (median of three calls)')
    for k, (name, frames) in enumerate(plan()):
        median = sorted(spans[3 * k:3 * k + 3])[1]
        table[name] = {'programme_us': round(median / 1000, 2), 'ns_per_frame': round(median / frames, 2)}
        print(f'{name:38s} {median / 1000:12.1f} {median / frames:14.1f}')
    if out:
        record = {}
        if os.path.exists(out):
            with open(out) as file:
                record = json.load(file)
        record['kernel_split'] = table
        with open(out, 'w') as file:
            json.dump(record, file, indent=1)
            file.write('\n')


def main():
    parser = argparse.ArgumentParser()
    parser.add_argument('--out', default=None)
    parser.add_argument('--label', default='head')
    parser.add_argument('--trace-only', action='store_true', help='three untimed calls per entry')
    parser.add_argument('--split', default=None, help='a rocprofv3 kernel trace (csv) of a --trace-only run')
    args = parser.parse_args()
    if args.split:
        return split(args.split, args.out)
    named, calls = entries()
    if args.trace_only:
        for call, _ in calls.values():
            for _ in range(3):
                call()
            torch.cuda.synchronize()
        return
    run = {}
    for name, (call, _) in calls.items():
        run[name] = round(timed(call), 5)
        print(name, run[name], flush=True)
    sizes = {name: {'states': int(named[name].phonemes.shape[0]), 'arcs': int(named[name].sources.shape[0])}
             for name in NAMES}
    print(json.dumps({'label': args.label, 'graphs': sizes, 'ms': run}))
    if args.out:
        record = {}
        if os.path.exists(args.out):
            with open(args.out) as file:
                record = json.load(file)
        record.setdefault('device', torch.cuda.get_device_name(0))
        record.setdefault('unit', 'milliseconds, median of 20 (HIP events)')
        record.setdefault('graphs', sizes)
        record.setdefault('runs', {}).setdefault(args.label, []).append(run)
        with open(args.out, 'w') as file:
            json.dump(record, file, indent=1)
            file.write('\n')


if __name__ == '__main__':
    main()
