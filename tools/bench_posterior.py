"""HIP-event time of posterior decoding over a phoneme graph (ppg_posterior) and of its yardsticks:

    python tools/bench_posterior.py [--label head] [--out profiles/posterior_bench.json] [--only posterior]

The six graphs and the batch sizes of tools/bench_viterbi.py (1, 64 and 2048 utterances x 1000 frames, softmax scale 3).
Beside every posterior, in the same process: engine.viterbi_items on the same graph, and a torch loop, the forward and
the backward recurrence as torch operations on the device, one frame at a time: a gather at the arcs' far ends, an add,
a segment logsumexp over the arcs' near ends (scatter_reduce amax, then scatter_add of the exponentials), the stay
candidate and the emission; no occupancy and no phoneme sums.  The torch loop, and the posterior with the state
occupancy as an output, run at 1 and 64 utterances only (at 2048 either moves gigabytes).  Median of 20 timed calls
after 5 warm-up calls of the same shape for the library's entries, of 3 after 1 for the torch loop; every timed window
ends in an event synchronise.  --only posterior leaves the yardsticks out.  With --out the run is appended to the runs
of its --label in that file.  --trace-only makes three untimed calls of every posterior workload (without the occupancy
output) and nothing else: the run to put under a rocprofv3 kernel trace.
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from bench_viterbi import SHAPES, graphs, packed, ppgs, timed  # noqa: E402
from ppgs_amd import alignment, engine  # noqa: E402


def packed_both(graph):
    """What engine.posterior_items takes of one Graph, on the device once."""
    offsets, targets, weights = alignment._transposed(graph)
    return dict(packed(graph), out_begin=offsets.to(torch.int32).cuda(), targets=targets.to(torch.int32).cuda(),
                out_weights=weights.cuda())


def segment_lse(own, index, candidates):
    """Per row and state n: LSE(own[:, n], candidates[:, i] for index[i] == n)."""
    top = own.scatter_reduce(1, index, candidates, 'amax')
    safe = torch.where(torch.isinf(top), torch.zeros_like(top), top)
    total = (own - safe).exp().scatter_add(1, index, (candidates - safe.gather(1, index)).exp())
    return top + total.log()


def torch_loop(logp, graph):
    """Forward and backward as torch operations: logp (items, frames, 40) on the device -> (total (items,), the last
    row of alpha + beta)."""
    device = logp.device
    degrees = (graph.offsets[1:] - graph.offsets[:-1]).long()
    targets = torch.repeat_interleave(torch.arange(degrees.shape[0]), degrees).to(device)
    sources, weights = graph.sources.long().to(device), graph.weights.to(device)
    sym, stay = graph.phonemes.long().to(device), graph.stay.to(device)
    items, frames, _ = logp.shape
    into, out_of = targets[None].expand(items, -1), sources[None].expand(items, -1)
    rows = [logp[:, 0][:, sym] + graph.initial.to(device)]
    for t in range(1, frames):
        a = rows[-1]
        rows.append(logp[:, t][:, sym] + segment_lse(a + stay, into, a[:, sources] + weights))
    b = graph.final.to(device)[None].expand(items, -1)
    total = torch.logsumexp(rows[-1] + b, dim=1)
    for t in range(frames - 2, -1, -1):
        inner = logp[:, t + 1][:, sym] + b
        b = segment_lse(inner + stay, out_of, inner[:, targets] + weights)
    return total, rows[0] + b


def main():
    parser = argparse.ArgumentParser()
    parser.add_argument('--out', default=None)
    parser.add_argument('--label', default='head')
    parser.add_argument('--only', default=None, choices=['posterior'])
    parser.add_argument('--trace-only', action='store_true', help='three untimed calls per posterior workload')
    args = parser.parse_args()
    args.only = 'posterior' if args.trace_only else args.only
    generator = torch.Generator().manual_seed(0)
    _, _, named = graphs()
    calls, slow = {}, set()
    for items, frames in SHAPES:
        x, lengths = ppgs(items, frames, generator), [frames] * items
        for name, graph in named.items():
            both = packed_both(graph)
            calls[f'posterior_{name}_{items}x{frames}'] = (
                lambda x=x, lengths=lengths, both=both: engine.posterior_items(x, lengths, **both))
            if items <= 64:                                    # (at 2048 the occupancy alone is gigabytes)
                calls[f'posterior_states_{name}_{items}x{frames}'] = (
                    lambda x=x, lengths=lengths, both=both: engine.posterior_items(x, lengths, want_states=True,
                                                                                   **both))
            if args.only:
                continue
            given = packed(graph)
            calls[f'viterbi_{name}_{items}x{frames}'] = (
                lambda x=x, lengths=lengths, given=given: engine.viterbi_items(x, lengths, **given))
            if items <= 64:
                logp = x.clamp(1e-8, 1 - 1e-8).log().transpose(1, 2).contiguous()
                calls[f'torch_loop_{name}_{items}x{frames}'] = lambda logp=logp, graph=graph: torch_loop(logp, graph)
                slow.add(f'torch_loop_{name}_{items}x{frames}')
    if args.trace_only:
        for name, call in calls.items():
            if not name.startswith('posterior_states_'):
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
