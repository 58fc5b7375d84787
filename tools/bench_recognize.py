"""HIP-event time of the phoneme recogniser (ppg_recognize) and of its yardsticks:

    python tools/bench_recognize.py [--label head] [--out profiles/recognize_bench.json] [--only recognize]

Workloads (utterances x frames), softmax scale 3, a switch penalty of 2 as the model:
    engine.recognize_items  1 x 1000, 64 x 1000, 2048 x 1000 and 1 x 262144 with gop; 64 x 1000 also without
    engine.decode_items     1 x 1000, 64 x 1000, 2048 x 1000: the same question without a model
    engine.align_items      the same three, 120 phonemes each: the same frame walk with two predecessors per state
    torch loop              the same recurrence as one broadcast add, one max over the predecessor axis and one
                            gather of the path per frame, on log-posteriors already on the GPU, at the same three (the
                            quarter of a million sequential steps of 1 x 262144 are left out)
Median of 20 timed calls after 5 warm-up calls of the same shape; every timed window ends in an event synchronise.
--only recognize leaves the yardsticks out (to compare two builds of the library: PPGS_AMD_LIB selects it).  With --out
the run is appended to the runs of its --label in that file.  --trace-only makes three untimed calls of every recognize
workload and nothing else: the run to put under a rocprofv3 kernel trace, whose dispatches tell the workloads apart by
their grids.
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
SHAPES = [(1, 1000), (64, 1000), (2048, 1000)]


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


def torch_loop(logp, transitions):
    """The recurrence as torch operations, one frame at a time: logp (items, frames, 40) -> labels (items, frames)."""
    items, frames, _ = logp.shape
    back = torch.empty((items, frames, 40), dtype=torch.int64, device=logp.device)
    d = logp[:, 0]
    for t in range(1, frames):
        best, back[:, t] = (d[:, :, None] + transitions[None]).max(dim=1)
        d = logp[:, t] + best
    labels = torch.empty((items, frames), dtype=torch.int64, device=logp.device)
    last = d.argmax(dim=1)
    labels[:, frames - 1] = last
    for t in range(frames - 1, 0, -1):
        last = back[:, t].gather(1, last[:, None])[:, 0]
        labels[:, t - 1] = last
    return labels


def main():
    parser = argparse.ArgumentParser()
    parser.add_argument('--out', default=None)
    parser.add_argument('--label', default='head')
    parser.add_argument('--only', default=None, choices=['recognize'])
    parser.add_argument('--trace-only', action='store_true', help='three untimed calls per recognize workload')
    args = parser.parse_args()
    args.only = 'recognize' if args.trace_only else args.only
    generator = torch.Generator().manual_seed(0)
    model = alignment.switch_penalty(2.).cuda()
    calls = {}
    for items, frames in SHAPES + [(1, 262144)]:
        x, lengths = ppgs(items, frames, generator), [frames] * items
        calls[f'recognize_{items}x{frames}'] = lambda x=x, lengths=lengths: engine.recognize_items(x, lengths, model)
        if (items, frames) == (64, 1000):
            calls['recognize_64x1000_no_gop'] = (
                lambda x=x, lengths=lengths: engine.recognize_items(x, lengths, model, want_gop=False))
        if args.only or frames > 1000:
            continue
        table = torch.randint(0, 40, (items, 120), generator=generator, dtype=torch.int32).cuda()
        counts = [120] * items
        logp = x.clamp(1e-8, 1 - 1e-8).log().transpose(1, 2).contiguous()
        calls[f'decode_{items}x{frames}'] = lambda x=x, lengths=lengths: engine.decode_items(x, lengths)
        calls[f'align_{items}x{frames}x120'] = (
            lambda x=x, lengths=lengths, table=table, counts=counts: engine.align_items(x, lengths, table, counts))
        calls[f'torch_loop_{items}x{frames}'] = lambda logp=logp: torch_loop(logp, model)
    if args.trace_only:
        for call in calls.values():
            for _ in range(3):
                call()
            torch.cuda.synchronize()
        return
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
