"""HIP-event time of the live Viterbi over a graph (ppg_viterbi_stream_*) and of its yardsticks:

    python tools/bench_viterbi_stream.py [--label head] [--out profiles/viterbi_stream_bench.json]

Workloads (streams x frames per push), window 1024, on streams that have already received 1024 frames, so the ring
has wrapped and the lag is the recording's own:
    ViterbiStream.push      1 x 16 and 64 x 16 under model_graph(switch penalty 4) at softmax scale 3, max_lag 512,
                            beside RecognizeStream.push of the same frames from the same process;
                            1 x 16 on the ten-word loop and on the 170-word loop (29 410 arcs: they come from memory)
                            over a clearly said word string, max_lag 512;
                            1 x 16 on a sausage of 100 words with two variants each over flat posteriors, max_lag 50:
                            every push is forced
    a stalled stream        1 x 16 under model_graph(switch penalty 40) at softmax scale 0.3 with max_lag 1000, from
                            frame 0: switches never pay, the paths of the alive states stay apart, nothing commits and
                            nothing is forced while the lag grows from 16 to 400 frames; only the ancestor ballot saves
                            the walk
    alignment.viterbi       over the pushed frames alone (1 x 16, the ten-word loop), and over a 10 000-frame history:
                            what a live caller pays without the stream
Median of 20 timed calls after 5 warm-up calls of the same shape; every timed window ends in an event synchronise.  With
--out the run is appended to the runs of its --label in that file.  --trace-only makes three untimed pushes of every
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


def loop(words, generator):
    """(graph, lexicon): `words` words of two different phonemes each, no two alike."""
    pairs = [(a, b) for a in range(39) for b in range(39) if a != b]
    chosen = torch.randperm(len(pairs), generator=generator)[:words].tolist()
    lexicon = [(f'word{w}', [list(pairs[index])]) for w, index in enumerate(chosen)]
    return alignment.word_loop(lexicon, penalty=1.5)[0], lexicon


def spoken(lexicon, frames, generator):
    """(1, 40, frames): words of the lexicon said clearly one after the other, four frames a phoneme."""
    labels = []
    while len(labels) < frames:
        word = int(torch.randint(0, len(lexicon), (), generator=generator))
        labels += [p for p in lexicon[word][1][0] for _ in range(4)] + [39] * 2
    labels = labels[:frames]
    logits = torch.randn(40, frames, generator=generator)
    logits[torch.tensor(labels), torch.arange(frames)] += 12.
    return torch.softmax(logits, dim=0)[None].cuda()


def live(make, recording, frames, history=1024):
    """A push of `frames` frames on streams that have a history of 1024: (call, the object)."""
    stream = make()
    for at in range(0, history, 64):
        stream.push(recording[:, :, at:at + 64])
    x = recording[:, :, history:history + frames].contiguous()
    return (lambda: stream.push(x)), stream


def main():
    parser = argparse.ArgumentParser()
    parser.add_argument('--out', default=None)
    parser.add_argument('--label', default='head')
    parser.add_argument('--trace-only', action='store_true', help='three untimed pushes per stream workload')
    args = parser.parse_args()
    generator = torch.Generator().manual_seed(0)
    calls, objects = {}, {}
    model = alignment.model_graph(alignment.switch_penalty(4.))
    for streams in (1, 64):
        recording = ppgs(streams, 1024 + 16, generator)
        name = f'push_{streams}x16_model_graph'
        calls[name], objects[name] = live(
            lambda: alignment.ViterbiStream(model, window=1024, max_lag=512, batch=streams), recording, 16)
        name = f'recognize_stream_push_{streams}x16'
        calls[name], objects[name] = live(
            lambda: alignment.RecognizeStream(penalty=4., window=1024, max_lag=512, batch=streams), recording, 16)
    ten, ten_lexicon = loop(10, generator)
    large, large_lexicon = loop(170, generator)
    for name, graph, lexicon in (('push_1x16_loop_10', ten, ten_lexicon), ('push_1x16_loop_170', large, large_lexicon)):
        calls[name], objects[name] = live(
            lambda: alignment.ViterbiStream(graph, window=1024, max_lag=512, batch=1),
            spoken(lexicon, 1024 + 16, generator), 16)
    pairs = [(a, b) for a in range(39) for b in range(39) if a != b]
    words = [[list(pairs[2 * w]), list(pairs[2 * w + 1])] for w in range(100)]
    sausage = alignment.pronunciations(words)[0]
    name = 'push_1x16_sausage_100_max_lag_50'
    calls[name], objects[name] = live(
        lambda: alignment.ViterbiStream(sausage, window=1024, max_lag=50, batch=1),
        ppgs(1, 1024 + 16, generator, 0.3), 16)
    name = 'push_1x16_model_graph_stalled_max_lag_1000'
    apart = alignment.model_graph(alignment.switch_penalty(40.))
    calls[name], objects[name] = live(
        lambda: alignment.ViterbiStream(apart, window=1024, max_lag=1000, batch=1), ppgs(1, 16, generator, 0.3), 16,
        history=0)
    if args.trace_only:
        for call in calls.values():
            for _ in range(3):
                call()
            torch.cuda.synchronize()
        return
    short = spoken(ten_lexicon, 16, generator)[0]
    history = spoken(ten_lexicon, 10000, generator)[0]
    calls['viterbi_1x16_loop_10'] = lambda: alignment.viterbi(short, ten)
    calls['viterbi_1x10000_loop_10'] = lambda: alignment.viterbi(history, ten)
    run = {name: round(timed(call), 5) for name, call in calls.items()}
    # what the timed pushes met: the frames forced per stream say whether the walks ran
    met = {}
    for name, stream in objects.items():
        last = stream.flush()
        met[name] = {'window': stream.window, 'max_lag': stream.max_lag, 'forced_per_stream': last.forced.tolist()[:4],
                     'refused': bool((last.count < 0).any())}
    print(json.dumps({'label': args.label, 'ms': run, 'streams': met}))
    if args.out:
        record = {}
        if os.path.exists(args.out):
            with open(args.out) as file:
                record = json.load(file)
        record.setdefault('device', torch.cuda.get_device_name(0))
        record.setdefault('unit', f'milliseconds, median of {REPEATS} (HIP events), one entry per process')
        record.setdefault('runs', {}).setdefault(args.label, []).append({'ms': run, 'streams': met})
        with open(args.out, 'w') as file:
            json.dump(record, file, indent=1)
            file.write('\n')


if __name__ == '__main__':
    main()
