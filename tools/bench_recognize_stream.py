"""HIP-event time of the live phoneme recogniser (ppg_recognize_stream_*) and of its yardsticks:

    python tools/bench_recognize_stream.py [--label head] [--out profiles/recognize_stream_bench.json]

Workloads (streams x frames per push), softmax scale 3, a switch penalty of 4, window 1024, max_lag 512:
    RecognizeStream.push    1 x 16, 64 x 16 and 1 x 1000 (fed as pieces of window - max_lag frames), on streams that have
                            already received 1024 frames, so the ring has wrapped and the lag is the recording's own
    the commit's walk       the same 1 x 16 push at softmax scale 0.3 under a switch penalty of 40 (nearly flat posteriors
                            and switches that never pay: the paths of the alive states stay apart, so the lag is
                            whatever max_lag allows and every push is forced) with max_lag 16 and with max_lag 1000:
                            the walk of the commit over 32 and over 1016 frames
    a growing lag           the same flat stream from frame 0 with max_lag 1000: the 25 pushes of a measurement are the
                            first 25 of the stream, nothing can be committed and nothing is forced, the lag grows from
                            16 to 400 frames (the median push meets about 250)
    alignment.recognize     over the pushed frames alone, and over a 100 000-frame history: what a live caller pays
                            without the stream
Median of 20 timed calls after 5 warm-up calls of the same shape; every timed window ends in an event synchronise.  With
--out the run is appended to the runs of its --label in that file.  --only-stream leaves the yardsticks out (to compare
two builds of the library: PPGS_AMD_LIB selects it).  --trace-only makes three untimed pushes of every
stream workload and nothing else: the run to put under a rocprofv3 kernel trace.
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ppgs_amd import alignment  # noqa: E402

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


def ppgs(items, frames, generator, scale=3.):
    return torch.softmax(scale * torch.randn(items, 40, frames, generator=generator), dim=1).cuda()


def live(streams, frames, generator, scale=3., window=1024, max_lag=512, history=1024, penalty=4.):
    """A push of `frames` frames on `streams` streams that have a history of 1024 frames: (call, the object)."""
    said = alignment.RecognizeStream(penalty=penalty, window=window, max_lag=max_lag, batch=streams)
    past = ppgs(streams, max(history, 1), generator, scale)
    for at in range(0, history, 64):
        said.push(past[:, :, at:at + 64])
    x = ppgs(streams, frames, generator, scale)
    return (lambda: said.push(x)), said


def main():
    parser = argparse.ArgumentParser()
    parser.add_argument('--out', default=None)
    parser.add_argument('--label', default='head')
    parser.add_argument('--only-stream', action='store_true', help='no yardsticks')
    parser.add_argument('--trace-only', action='store_true', help='three untimed pushes per stream workload')
    args = parser.parse_args()
    generator = torch.Generator().manual_seed(0)
    calls, objects = {}, {}
    for streams, frames in ((1, 16), (64, 16), (1, 1000)):
        name = f'push_{streams}x{frames}'
        calls[name], objects[name] = live(streams, frames, generator)
    for max_lag in (16, 1000):
        name = f'push_1x16_flat_max_lag_{max_lag}'
        calls[name], objects[name] = live(1, 16, generator, scale=0.3, max_lag=max_lag, penalty=40.)
    name = 'push_1x16_flat_growing_lag'
    calls[name], objects[name] = live(1, 16, generator, scale=0.3, max_lag=1000, history=0, penalty=40.)
    if args.trace_only:
        for call in calls.values():
            for _ in range(3):
                call()
            torch.cuda.synchronize()
        return
    for streams, frames in () if args.only_stream else ((1, 16), (64, 16), (1, 1000)):
        x = ppgs(streams, frames, generator)
        calls[f'recognize_{streams}x{frames}'] = lambda x=x: alignment.recognize(x, penalty=4.)
    if not args.only_stream:
        history = ppgs(1, 100000, generator)
        calls['recognize_1x100000'] = lambda: alignment.recognize(history, penalty=4.)
    run = {name: round(timed(call), 5) for name, call in calls.items()}
    # the lag the timed pushes of the flat streams met: frames forced per push say how far the walk went
    lags = {}
    for name, said in objects.items():
        last = said.flush()
        lags[name] = {'window': said.window, 'forced_per_stream': last.forced.tolist(), 'max_lag': said.max_lag}
    print(json.dumps({'label': args.label, 'ms': run, 'streams': lags}))
    if args.out:
        record = {}
        if os.path.exists(args.out):
            with open(args.out) as file:
                record = json.load(file)
        record.setdefault('device', torch.cuda.get_device_name(0))
        record.setdefault('unit', f'milliseconds, median of {REPEATS} (HIP events), one entry per process')
        record.setdefault('runs', {}).setdefault(args.label, []).append({'ms': run, 'streams': lags})
        with open(args.out, 'w') as file:
            json.dump(record, file, indent=1)
            file.write('\n')


if __name__ == '__main__':
    main()
