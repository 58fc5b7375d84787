"""HIP-event time of the phrase search over a phoneme graph (ppg_search_graph) and of its yardsticks:

    python tools/bench_search_graph.py [--label head] [--out profiles/search_graph_bench.json]
    rocprofv3 --kernel-trace --output-format csv -d DIR -- python tools/bench_search_graph.py --trace-only
    python tools/bench_search_graph.py --split DIR/.../*_kernel_trace.csv [--out profiles/search_graph_bench.json]

Workloads (recordings x frames x graphs), softmax scale 3: 1 x 100000 x 1, 1 x 100000 x 64 and 64 x 1000 x 8, each with
    chain        chain_graph of 8 phonemes (one final state)
    chain2       the same chain with a second final state of weight -1000: the same recurrence, what a shortcut for
                 a single final state would have to beat
    phrase       phrase_graph of 3 words x 2 variants x 3 phonemes with pauses (20 states, two final states)
beside, measured in the same process on the same device,
    search       engine.search_items on the same chain, as many queries as graphs: ppg_search, the parent's kernel
    viterbi      engine.viterbi_items on the same graph, one path per recording (it has no axis of graphs)
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
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ppgs_amd import alignment, engine  # noqa: E402

SHAPES = [(1, 100000, 1), (1, 100000, 64), (64, 1000, 8)]
FIELDS = ('state_begin', 'phonemes', 'stay', 'initial', 'final', 'arc_begin', 'sources', 'weights')


def timed(call, warmup=5, repeats=20):
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


def packed(graph, copies):
    """What engine.search_graph_items and engine.viterbi_items take of `copies` copies of one Graph."""
    counts, state_begin, arc_begin, joined = alignment._joined_graphs([graph] * copies)
    given = {name: joined(name).cuda() for name in FIELDS if name not in ('state_begin', 'arc_begin')}
    given.update(state_begin=state_begin, arc_begin=arc_begin, max_states=max(counts))
    return given


def graphs():
    generator = torch.Generator().manual_seed(1)
    sequence = torch.randint(0, 39, (8,), generator=generator).tolist()

    def word():
        return torch.randint(0, 39, (3,), generator=generator).tolist()
    chain = alignment.chain_graph(sequence)
    final = chain.final.clone()
    final[0] = -1000.
    return sequence, {'chain': chain, 'chain2': chain._replace(final=final),
                      'phrase': alignment.phrase_graph([[word(), word()] for _ in range(3)])[0]}


def plan():
    """The entries of a run in their fixed order, without a device: [(name, frames)]."""
    out = []
    for items, frames, count in SHAPES:
        shape = f'{items}x{frames}x{count}'
        out += [(f'search_graph_{name}_{shape}', frames) for name in ('chain', 'chain2', 'phrase')]
        out += [(f'search_chain_{shape}', frames)]
        if count == 1 or items > 1:                            # (the recordings of 1 x 100000 once)
            out += [(f'viterbi_{name}_{items}x{frames}', frames) for name in ('chain', 'phrase')]
    return out


def entries():
    """The calls of a run in the order of `plan`: {name: (call, frames)}."""
    generator = torch.Generator().manual_seed(0)
    sequence, named = graphs()
    calls = {}
    for items, frames, count in SHAPES:
        x = torch.softmax(3 * torch.randn(items, 40, frames, generator=generator), dim=1).cuda()
        lengths = [frames] * items
        shape = f'{items}x{frames}x{count}'
        for name, graph in named.items():
            given = packed(graph, count)
            calls[f'search_graph_{name}_{shape}'] = (
                lambda x=x, lengths=lengths, given=given: engine.search_graph_items(x, lengths, **given), frames)
        table = torch.tensor([sequence] * count, dtype=torch.int32).cuda()
        calls[f'search_chain_{shape}'] = (
            lambda x=x, lengths=lengths, table=table, count=count: engine.search_items(x, lengths, table, [8] * count),
            frames)
        for name in ('chain', 'phrase') if count == 1 or items > 1 else ():
            given = {key: value.cuda() if torch.is_tensor(value) else value for key, value in packed(named[name], 1).items()}
            calls[f'viterbi_{name}_{items}x{frames}'] = (
                lambda x=x, lengths=lengths, given=given: engine.viterbi_items(x, lengths, **given, want_gop=False), frames)
    assert [(name, frames) for name, (_, frames) in calls.items()] == plan()
    return named, calls


def split(trace, out):
    calls = {name: (None, frames) for name, frames in plan()}
    with open(trace) as file:
        rows = sorted(csv.DictReader(file), key=lambda row: int(row['Start_Timestamp']))
    spans = [int(row['End_Timestamp']) - int(row['Start_Timestamp']) for row in rows if 'programme' in row['Kernel_Name']]
    assert len(spans) == 3 * len(calls), (len(spans), len(calls))
    table = {}
    print('entry                                   programme us    ns per frame   (median of three calls)')
    for k, (name, (_, frames)) in enumerate(calls.items()):
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
    sizes = {name: {'states': int(graph.phonemes.shape[0]), 'arcs': int(graph.sources.shape[0])}
             for name, graph in named.items()}
    print(json.dumps({'label': args.label, 'graphs': sizes, 'ms': run}))
    if args.out:
        record = {}
        if os.path.exists(args.out):
            with open(args.out) as file:
                record = json.load(file)
        record.setdefault('device', torch.cuda.get_device_name(0))
        record.setdefault('unit', 'milliseconds, median of 20 (HIP events), one entry per process')
        record.setdefault('graphs', sizes)
        record.setdefault('runs', {}).setdefault(args.label, []).append(run)
        with open(args.out, 'w') as file:
            json.dump(record, file, indent=1)
            file.write('\n')


if __name__ == '__main__':
    main()
