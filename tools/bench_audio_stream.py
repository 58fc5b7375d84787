"""Audio-in streaming step: 64 live recordings, 16 new frames (2 560 samples) per item per step, causal model.

    python tools/bench_audio_stream.py [--rounds 15] [--steps 25] [--precision bf16]

Four variants of one step, microseconds per step (wall clock over `steps` enqueued steps + one synchronise):
  a  the incremental frontend alone            FrontendStream.push
  b  audio in, posteriors out                   BatchedAudioStream.push  (= a + c)
  c  the feature-in step                        BatchedStream.push on mel frames that already exist
  d  what could be written before FrontendStream existed, with public calls only: keep the carried samples in a
     torch buffer, torch.cat the new ones, engine.frontend() on it, slice off the frames whose window reaches past
     either edge, BatchedStream.push
The variants alternate inside one process (a b c d, a b c d, ...) and every round times each once on a fresh
utterance (the steady state of frames 32 .. 432 of a 500-frame window); the result is the median over rounds and the
spread (min .. max) of every variant -- (d)'s spread is the margin (b) is judged against.
Writes profiles/audio_stream_step.json.
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch                                              # noqa: E402

import ppgs_amd                                           # noqa: E402
from ppgs_amd import engine as E                          # noqa: E402

BATCH, STEP = 64, 2560
WARM = 2            # steps of every utterance that are not timed (the first frames: left reflection, short pushes)


class Emulation:
    """Variant d.  Frame t of a recording reads samples 160 t - 432 .. 160 t + 591.  engine.frontend() reflect-pads
    whatever it is given, so of the frames it returns for a buffer that starts at sample 160 g, the first 3 (their
    windows reach the left reflection) and every one whose window passes the buffer's end are wrong and are
    sliced off.  The buffer starts 4 hops before the first frame wanted: 3 would do for the padding, an even number
    keeps the kernel's frame pairs those of the whole recording (the same bits)."""

    def __init__(self, engine):
        self.stream = engine.batched_stream(BATCH, 500)
        self.buffer = None          # samples from 160 * self.start on
        self.start = 0              # (in frames)
        self.frontier = 0

    def push(self, samples):
        self.buffer = samples if self.buffer is None else torch.cat([self.buffer, samples], dim=1)
        received = 160 * self.start + self.buffer.shape[1]
        frontier = E.audio_stream_frames(received)
        if frontier == self.frontier:
            return None
        _, mel = E.frontend(self.buffer)
        new = mel[:, :, self.frontier - self.start:frontier - self.start].contiguous()
        out = self.stream.push(new)
        self.frontier = frontier
        start = max(frontier - 4, 0)
        self.buffer = self.buffer[:, 160 * (start - self.start):]
        self.start = start
        return out


def main():
    parser = argparse.ArgumentParser()
    parser.add_argument('--rounds', type=int, default=15)
    parser.add_argument('--steps', type=int, default=25)
    parser.add_argument('--precision', default='bf16')
    parser.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'audio_stream_step.json'))
    args = parser.parse_args()
    state = ppgs_amd.weights.seeded_state_dict(seed=1234)
    engine = E.Engine(state, 0, args.precision, is_causal=True)
    generator = torch.Generator().manual_seed(1234)
    steps = WARM + args.steps
    assert steps * 16 <= 496
    audio = (0.1 * torch.randn(BATCH, steps * STEP, generator=generator)).cuda()
    _, mel = E.frontend(audio)
    chunks = [audio[:, i * STEP:(i + 1) * STEP].contiguous() for i in range(steps)]
    # the frames step i of the audio-in variants hands the model: what the feature-in variant is fed
    bounds = [E.audio_stream_frames((i + 1) * STEP) for i in range(steps)]
    features = [mel[:, :, (bounds[i - 1] if i else 0):bounds[i]].contiguous() for i in range(steps)]

    def run(make, step):
        obj = make()
        for i in range(WARM):
            step(obj, i)
        torch.cuda.synchronize()
        start = time.perf_counter()
        for i in range(WARM, steps):
            step(obj, i)
        torch.cuda.synchronize()
        return (time.perf_counter() - start) / args.steps * 1e6

    variants = {
        'a_frontend_stream': (lambda: E.FrontendStream(BATCH, STEP, 0), lambda o, i: o.push(chunks[i])),
        'b_audio_in_step': (lambda: engine.batched_audio_stream(BATCH, 500, STEP), lambda o, i: o.push(chunks[i])),
        'c_feature_in_step': (lambda: engine.batched_stream(BATCH, 500), lambda o, i: o.push(features[i])),
        'd_emulation_public_calls': (lambda: Emulation(engine), lambda o, i: o.push(chunks[i])),
    }
    # the emulation computes the same posteriors (compared once, outside the timing)
    ours, theirs = engine.batched_audio_stream(BATCH, 500, STEP), Emulation(engine)
    same = True
    for i in range(6):
        x, y = ours.push(chunks[i]), theirs.push(chunks[i])
        same = same and all(torch.equal(p, q) for p, q in zip(x, y))
    for name, (make, step) in variants.items():          # one untimed pass: allocations, plans, code objects
        run(make, step)
    times = {name: [] for name in variants}
    for _ in range(args.rounds):
        for name, (make, step) in variants.items():
            times[name].append(run(make, step))
    result = {
        'what': 'us per step: 64 items x 2560 new samples (16 frames), causal, ' + args.precision,
        'rounds': args.rounds, 'steps_per_round': args.steps,
        'device': torch.cuda.get_device_name(0),
        'emulation_equals_audio_in': bool(same),
    }
    for name, values in times.items():
        result[name] = {'median_us': round(statistics.median(values), 1), 'min_us': round(min(values), 1),
                        'max_us': round(max(values), 1)}
    result['a_plus_c_us'] = round(result['a_frontend_stream']['median_us'] + result['c_feature_in_step']['median_us'], 1)
    result['b_not_slower_than_d'] = result['b_audio_in_step']['median_us'] <= result['d_emulation_public_calls']['max_us']
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, 'w') as f:
        json.dump(result, f, indent=1)
        f.write('\n')
    print(json.dumps(result))


if __name__ == '__main__':
    main()
