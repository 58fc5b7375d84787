"""HIP-event time of the Viterbi over a phoneme graph (ppg_viterbi) and of its yardsticks:

    python tools/bench_viterbi.py [--label head] [--out profiles/viterbi_bench.json] [--only viterbi]

Workloads, each at 1, 64 and 2048 utterances x 1000 frames, softmax scale 3:
    model        model_graph of a switch penalty of 2                       beside engine.recognize_items
    chain        chain_graph of 120 phonemes                                 beside engine.align_items
    optional     chain_graph of 120 phonemes, every fifth optional           beside engine.align_items(optional=)
    sausage      pronunciations of 100 words x 2 variants x 3 phonemes       beside the torch loop
    loop10       word_loop of 10 words x 3 phonemes                          beside the torch loop
    loop170      word_loop of 170 words x 2 phonemes: 29 410 arcs, the most  beside the torch loop
                 word ends the limit on arcs leaves room for
The torch loop is the forward recurrence alone (no trace-back, no runs, no scores) as torch operations on the device,
one frame at a time: a gather of D at the arcs' sources, an add, a segment maximum over the arcs' targets
(scatter_reduce amax), the stay candidate and the emission.  Median of 20 timed calls after 5 warm-up calls of the same
shape for the library's entries, of 3 after 1 for the torch loop (a call of it is a thousand sequential steps); every
timed window ends in an event synchronise.  --only viterbi leaves the yardsticks out.  With --out the run is appended
to the runs of its --label in that file.  --trace-only makes three untimed calls of every viterbi workload and nothing
else: the run to put under a rocprofv3 kernel trace.
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ppgs_amd import alignment, engine  # noqa: E402

SHAPES = [(1, 1000), (64, 1000), (2048, 1000)]


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


def ppgs(items, frames, generator):
    return torch.softmax(3 * torch.randn(items, 40, frames, generator=generator), dim=1).cuda()


def packed(graph):
    """What engine.viterbi_items takes of one Graph, on the device once."""
    count = graph.phonemes.shape[0]
    return dict(state_begin=torch.tensor([0, count], dtype=torch.int32).cuda(), phonemes=graph.phonemes.cuda(),
                stay=graph.stay.cuda(), initial=graph.initial.cuda(), final=graph.final.cuda(),
                arc_begin=graph.offsets.cuda(), sources=graph.sources.cuda(), weights=graph.weights.cuda(),
                max_states=count)


def torch_loop(logp, graph):
    """The forward recurrence as torch operations: logp (items, frames, 40) on the device -> total (items,)."""
    device = logp.device
    degrees = (graph.offsets[1:] - graph.offsets[:-1]).long()
    targets = torch.repeat_interleave(torch.arange(degrees.shape[0]), degrees).to(device)
    sources, weights = graph.sources.long().to(device), graph.weights.to(device)
    sym, stay = graph.phonemes.long().to(device), graph.stay.to(device)
    items, frames, _ = logp.shape
    index = targets[None].expand(items, -1)
    d = logp[:, 0][:, sym] + graph.initial.to(device)
    for t in range(1, frames):
        best = (d + stay).scatter_reduce(1, index, d[:, sources] + weights, 'amax')
        d = logp[:, t][:, sym] + best
    return (d + graph.final.to(device)).max(dim=1).values


def graphs():
    generator = torch.Generator().manual_seed(1)
    sequence = torch.randint(0, 39, (120,), generator=generator).tolist()
    flags = [n % 5 == 2 for n in range(120)]

    def word(length):
        return torch.randint(0, 39, (length,), generator=generator).tolist()
    return sequence, flags, {
        'model': alignment.model_graph(alignment.switch_penalty(2.)),
        'chain': alignment.chain_graph(sequence),
        'optional': alignment.chain_graph(sequence, flags),
        'sausage': alignment.pronunciations([[word(3), word(3)] for _ in range(100)])[0],
        'loop10': alignment.word_loop([(w, [word(3)]) for w in range(10)], penalty=2.)[0],
        'loop170': alignment.word_loop([(w, [word(2)]) for w in range(170)], penalty=2.)[0],
    }


def main():
    parser = argparse.ArgumentParser()
    parser.add_argument('--out', default=None)
    parser.add_argument('--label', default='head')
    parser.add_argument('--only', default=None, choices=['viterbi'])
    parser.add_argument('--trace-only', action='store_true', help='three untimed calls per viterbi workload')
    args = parser.parse_args()
    args.only = 'viterbi' if args.trace_only else args.only
    generator = torch.Generator().manual_seed(0)
    sequence, flags, named = graphs()
    model = alignment.switch_penalty(2.).cuda()
    calls, slow = {}, set()
    for items, frames in SHAPES:
        x, lengths = ppgs(items, frames, generator), [frames] * items
        for name, graph in named.items():
            given = packed(graph)
            calls[f'viterbi_{name}_{items}x{frames}'] = (
                lambda x=x, lengths=lengths, given=given: engine.viterbi_items(x, lengths, **given))
        if args.only:
            continue
        table = torch.tensor([sequence] * items, dtype=torch.int32).cuda()
        optional = torch.tensor([flags] * items, dtype=torch.int32).cuda()
        counts = [120] * items
        logp = x.clamp(1e-8, 1 - 1e-8).log().transpose(1, 2).contiguous()
        calls[f'recognize_{items}x{frames}'] = lambda x=x, lengths=lengths: engine.recognize_items(x, lengths, model)
        calls[f'align_{items}x{frames}x120'] = (
            lambda x=x, lengths=lengths, table=table, counts=counts: engine.align_items(x, lengths, table, counts))
        calls[f'align_optional_{items}x{frames}x120'] = (
            lambda x=x, lengths=lengths, table=table, counts=counts, optional=optional: engine.align_items(
                x, lengths, table, counts, optional=optional))
        for name in ('sausage', 'loop10', 'loop170'):
            calls[f'torch_loop_{name}_{items}x{frames}'] = lambda logp=logp, graph=named[name]: torch_loop(logp, graph)
            slow.add(f'torch_loop_{name}_{items}x{frames}')
    if args.trace_only:
        for call in calls.values():
            for _ in range(3):
                call()
            torch.cuda.synchronize()
        return
    run = {}
    for name, call in calls.items():
        run[name] = round(timed(call, 1, 3) if name in slow else timed(call), 5)
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
        record.setdefault('unit', 'milliseconds, median of 20 (HIP events; the torch loops of 3), one entry per process')
        record.setdefault('graphs', sizes)
        record.setdefault('runs', {}).setdefault(args.label, []).append(run)
        with open(args.out, 'w') as file:
            json.dump(record, file, indent=1)
            file.write('\n')


if __name__ == '__main__':
    main()
