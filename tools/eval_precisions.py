"""What the operand precisions cost in the metrics the reference reports (ppgs_amd.evaluate.across_precisions) on
the seeded checkpoint at 32 x 1000 frames: labels are the fp32 engine's own argmax.

    python tools/eval_precisions.py [--out profiles/eval_precisions.json]
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import ppgs_amd  # noqa: E402


def main():
    parser = argparse.ArgumentParser()
    parser.add_argument('--out', default=None)
    args = parser.parse_args()
    checkpoint = ppgs_amd.weights.seeded_state_dict(seed=1234)
    audio = 0.1 * torch.randn(32, 1, 160000, generator=torch.Generator().manual_seed(1))
    features = ppgs_amd.preprocess.mel.from_audios(audio.cuda())
    results = ppgs_amd.evaluate.across_precisions(features, [1000] * 32, checkpoint)
    record = {'checkpoint': 'seeded_state_dict(seed=1234)', 'shape': [32, 1000], 'labels': 'argmax of the fp32 logits'}
    for precision, result in results.items():
        record[precision] = {key: result[key] for key in ('Accuracy', 'Top-3 Accuracy/', 'JSD', 'loss')}
    print(json.dumps(record))
    if args.out:
        with open(args.out, 'w') as file:
            json.dump(record, file, indent=1)
            file.write('\n')


if __name__ == '__main__':
    main()
