"""HIP-event time of one metrics update (engine.MetricsState.update: one kernel launch) against the same seven
accumulators computed with plain torch ops on the device, at 32 x 1000 and 1 x 1000 frames.

    python tools/bench_metrics.py [--out profiles/metrics_update.json]

Median of 200 timed calls after 20 warm-up calls.  The torch-op path leaves every result on the device and then
makes the .item() calls the reference's metric objects make per batch (ppgs/evaluate/metrics.py).
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ppgs_amd import engine  # noqa: E402


class TorchOps:
    """the seven accumulators with torch ops (no similarity mix, unit weights)"""

    def __init__(self, device):
        self.count = torch.zeros((), dtype=torch.int64, device=device)
        self.true_positives = torch.zeros_like(self.count)
        self.topk_correct = torch.zeros_like(self.count)
        self.class_total = torch.zeros(40, dtype=torch.int64, device=device)
        self.class_count = torch.zeros(40, dtype=torch.int64, device=device)
        self.distance = torch.zeros(40, 40, device=device)
        self.confusion = torch.zeros(40, 40, device=device)
        self.loss = 0.
        self.jsd = 0.

    def update(self, logits, labels):
        rows = logits.transpose(1, 2).flatten(0, 1)
        target = labels.flatten()
        keep = target != -100
        rows, target = rows[keep], target[keep]
        predicted = rows.argmax(dim=1)
        correct = predicted == target
        self.count += target.numel()
        self.true_positives += correct.sum()
        self.topk_correct += (rows.topk(3, dim=1).indices == target[:, None]).sum()
        self.class_total += torch.bincount(target[correct], minlength=40)
        self.class_count += torch.bincount(target, minlength=40)
        probs = torch.softmax(rows, dim=1)
        self.distance.index_add_(0, probs.argmax(dim=1), probs)
        self.confusion.index_add_(0, target, probs)
        loss = torch.nn.functional.cross_entropy(rows, target, reduction='sum')
        x = probs.clamp(1e-8, 1 - 1e-8)
        y = torch.nn.functional.one_hot(target, 40).float().clamp(1e-8, 1 - 1e-8)
        log_m = torch.log((x + y) / 2)
        kl = (x * (torch.log(x) - log_m) + y * (torch.log(y) - log_m)) / 2
        jsd = torch.sqrt(kl.clamp(min=0)).sum()
        self.loss += loss.item()          # Loss.update and JensenShannon.update read their sums every batch
        self.jsd += jsd.item()


def timed(call, warmup=20, repeats=200):
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
        times.append(start.elapsed_time(end) * 1e3)
    return statistics.median(times)


def main():
    parser = argparse.ArgumentParser()
    parser.add_argument('--out', default=None)
    parser.add_argument('--trace-only', action='store_true', help='ten updates and nothing else (for a kernel trace)')
    args = parser.parse_args()
    generator = torch.Generator().manual_seed(0)
    record = {'device': torch.cuda.get_device_name(0), 'unit': 'microseconds, median of 200 (HIP events)'}
    for batch, frames in ((32, 1000), (1, 1000)):
        logits = (3 * torch.randn(batch, 40, frames, generator=generator)).cuda()
        labels = torch.randint(0, 40, (batch, frames), generator=generator).repeat_interleave(8, dim=1)[:, :frames]
        labels[torch.rand(batch, frames, generator=generator) < 0.01] = -100
        labels = labels.cuda()
        state = engine.MetricsState(0)
        if args.trace_only:
            for _ in range(10):
                state.update(logits, labels)
            torch.cuda.synchronize()
            continue
        ops = TorchOps('cuda')
        kernel = timed(lambda: state.update(logits, labels))
        torch_ops = timed(lambda: ops.update(logits, labels))
        got = state.read()
        assert got['count'] == int(ops.count) * 1 and got['true_positives'] == int(ops.true_positives)
        record[f'{batch}x{frames}'] = {
            'update_us': round(kernel, 2), 'torch_ops_us': round(torch_ops, 2), 'ratio': round(torch_ops / kernel, 1)}
    if not args.trace_only:
        print(json.dumps(record))
        if args.out:
            with open(args.out, 'w') as file:
                json.dump(record, file, indent=1)
                file.write('\n')


if __name__ == '__main__':
    main()
