"""HIP-event time of the live posterior over a graph (ppg_posterior_stream_*) and of its yardsticks:

    python tools/bench_posterior_stream.py [--label head] [--out profiles/posterior_stream_bench.json]

The six graphs of tools/bench_viterbi.py at softmax scale 3.  Per graph, 1 and 64 streams, window 1024, on streams that
have already received 1024 frames (the ring has wrapped, the schedule is in its steady state):
    PosteriorStream.push    16 frames a push at (block, lag) = (1, 0), (16, 16) and (16, 64): every push gives out 16
                            frames per stream
    engine.posterior_items  1000 frames of the same graph and as many utterances, divided by 1000: what a frame costs in
                            the whole-recording call
    ViterbiStream.push      the same 16 frames on the same graph, max_lag 512, as tools/bench_viterbi_stream.py times it
all from one process and one build.  Median of 20 timed calls after 5 warm-up calls of the same shape; every timed
window ends in an event synchronise.  With --out the run is appended to the runs of its --label in that file.
--trace-only makes three untimed pushes of every PosteriorStream workload and nothing else: the run to put under a
rocprofv3 kernel trace.
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from bench_posterior import packed_both  # noqa: E402
from bench_viterbi import graphs, ppgs, timed  # noqa: E402
from ppgs_amd import alignment, engine  # noqa: E402

GEOMETRIES = ((1, 0), (16, 16), (16, 64))
HISTORY, PUSH = 1024, 16


def live(stream, recording):
    """A push of PUSH frames on streams that have a history of HISTORY frames."""
    for at in range(0, HISTORY, 64):
        stream.push(recording[:, :, at:at + 64])
    x = recording[:, :, HISTORY:HISTORY + PUSH].contiguous()
    return lambda: stream.push(x)


def main():
    parser = argparse.ArgumentParser()
    parser.add_argument('--out', default=None)
    parser.add_argument('--label', default='head')
    parser.add_argument('--trace-only', action='store_true', help='three untimed pushes per PosteriorStream workload')
    args = parser.parse_args()
    generator = torch.Generator().manual_seed(0)
    _, _, named = graphs()
    calls, objects = {}, {}
    for streams in (1, 64):
        recording = ppgs(streams, HISTORY + PUSH, generator)
        whole = ppgs(streams, 1000, generator)
        for name, graph in named.items():
            for block, lag in GEOMETRIES:
                key = f'push_{streams}x{PUSH}_{name}_block{block}_lag{lag}'
                objects[key] = alignment.PosteriorStream(graph, block=block, lag=lag, window=1024, batch=streams)
                calls[key] = live(objects[key], recording)
            if args.trace_only:
                continue
            both = packed_both(graph)
            calls[f'posterior_{streams}x1000_{name}'] = (
                lambda whole=whole, both=both: engine.posterior_items(whole, [1000] * whole.shape[0], **both))
            calls[f'viterbi_stream_push_{streams}x{PUSH}_{name}'] = live(
                alignment.ViterbiStream(graph, window=1024, max_lag=512, batch=streams), recording)
    if args.trace_only:
        for call in calls.values():
            for _ in range(3):
                call()
            torch.cuda.synchronize()
        return
    run = {}
    for name, call in calls.items():
        run[name] = round(timed(call), 5)
        print(name, run[name], flush=True)
    # what the timed pushes met: every one must have given out its 16 frames, on streams that are alive
    met = {}
    for name, stream in objects.items():
        last = stream.push(torch.full((stream.batch, 40, PUSH), 1. / 40, device='cuda'))
        met[name] = {'count': sorted(set(last.count.tolist())), 'alive': bool(torch.isfinite(last.evidence).all())}
    sizes = {name: {'states': int(graph.phonemes.shape[0]), 'arcs': int(graph.sources.shape[0])}
             for name, graph in named.items()}
    print(json.dumps({'label': args.label, 'graphs': sizes, 'ms': run, 'streams': met}))
    if args.out:
        record = {}
        if os.path.exists(args.out):
            with open(args.out) as file:
                record = json.load(file)
        record.setdefault('device', torch.cuda.get_device_name(0))
        record.setdefault('unit', 'milliseconds per call, median of 20 (HIP events), one entry per process')
        record.setdefault('graphs', sizes)
        record.setdefault('runs', {}).setdefault(args.label, []).append({'ms': run, 'streams': met})
        with open(args.out, 'w') as file:
            json.dump(record, file, indent=1)
            file.write('\n')


if __name__ == '__main__':
    main()
