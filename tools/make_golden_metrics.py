"""Golden vectors for the frame metrics (ppgs_amd.evaluate): the reference's own ppgs/evaluate/metrics.py, loaded
under the stub namespace of oracle/make_golden.py and run on seeded logits and labels.

    python tools/make_golden_metrics.py         # writes tests/golden/g13_metrics.npz

Needs the reference checkout (it runs where the other fixtures are made); the tests only import build_inputs()
from here, which needs nothing but torch.  The fixture holds data: logits, labels, lengths, the reference's
similarity matrix and phoneme weights as inputs; its accumulators and result dicts as expected outputs.

Cases (logits = 3 * randn, label = argmax with probability 0.7 else uniform, ragged tails and 1 % scattered -100):
  A  4 x 300, stored in full          B  32 x 1000, stored as seed + float64 checksums of the logits
  C  1 x 7, every label -100          D  one frame
C and D run Metrics() without figures (the reference's DistanceMatrix needs label 39 to occur: its bincount has no
minlength); their two matrices come from the float64 restatement below.
"""
import json
import os
import sys
import types

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = {'A': (4, 300), 'B': (32, 1000), 'C': (1, 7), 'D': (1, 1)}
SEED_B = 1302


def build_inputs(seed, batch, frames, empty=False):
    """(logits (batch, 40, frames) fp32, labels (batch, frames) int64 with -100 holes, lengths (batch,))"""
    g = torch.Generator().manual_seed(seed)
    logits = 3. * torch.randn(batch, 40, frames, generator=g)
    pick = torch.rand(batch, frames, generator=g) < 0.7
    uniform = torch.randint(0, 40, (batch, frames), generator=g)
    labels = torch.where(pick, logits.argmax(dim=1), uniform)
    lengths = torch.randint(frames // 2 + 1, frames + 1, (batch,), generator=g)
    lengths[0] = frames
    holes = torch.rand(batch, frames, generator=g) < 0.01
    labels[torch.arange(frames)[None, :] >= lengths[:, None]] = -100
    if frames > 1:
        labels[holes] = -100
    if empty:
        labels[:] = -100
    return logits, labels, lengths


def checksums(logits):
    """float64 checksums that do not depend on the order of summation: the fp32 bit patterns summed as integers
    (of the values, and of their magnitudes); both stay below 2^53"""
    bits = logits.contiguous().view(torch.int32).to(torch.int64)
    return float(bits.sum().item()), float((bits & 0x7fffffff).sum().item())


def gaps(logits, labels, weights):
    """(smallest gap between neighbours among the four largest logits, smallest relative gap between the two
    largest softmax * weight) over the labelled frames"""
    keep = labels.flatten() != -100
    rows = logits.transpose(1, 2).flatten(0, 1)[keep].double()
    top = rows.topk(4, dim=1).values
    logit_gap = (top[:, :-1] - top[:, 1:]).min().item()
    weighted = (torch.softmax(rows, dim=1) * weights.double()[None]).topk(2, dim=1).values
    weighted_gap = ((weighted[:, 0] - weighted[:, 1]) / weighted[:, 0]).min().item()
    return logit_gap, weighted_gap


def restate_matrices(logits, labels, weights):
    """float64: (distance matrix, accumulated confusion matrix) for the cases the reference cannot run"""
    keep = labels.flatten() != -100
    probs = torch.softmax(logits.transpose(1, 2).flatten(0, 1)[keep].double(), dim=1)
    target = labels.flatten()[keep]
    weighted = probs * weights.double()[None]
    distance = torch.zeros(40, 40, dtype=torch.float64).index_add_(0, weighted.argmax(dim=1), weighted)
    confusion = torch.zeros(40, 40, dtype=torch.float64).index_add_(0, target, probs)
    return distance, confusion


def main():
    os.environ['MPLBACKEND'] = 'Agg'
    sys.path.insert(0, ROOT)
    from oracle import make_golden as G
    ppgs = G.import_reference()
    sys.modules['torchaudio'] = types.ModuleType('torchaudio')
    torchutil = types.ModuleType('torchutil')
    torchutil.notify = lambda *a, **k: (lambda f: f)
    sys.modules['torchutil'] = torchutil
    core = G._load('ppgs.core', os.path.join(G.REF, 'ppgs', 'core.py'))
    ppgs.distance = core.distance
    from ppgs_amd.phonemes import PHONEMES
    ppgs.PHONEMES = list(PHONEMES)
    weights = torch.load(ppgs.CLASS_WEIGHT_FILE).float()
    ppgs.load = types.ModuleType('ppgs.load')
    ppgs.load.phoneme_weights = lambda device='cpu': weights.to(device)
    ppgs.loss = lambda input, target, reduction='mean': torch.nn.functional.cross_entropy(
        input, target, reduction=reduction)
    metrics = G._load('ppgs.evaluate.metrics', os.path.join(G.REF, 'ppgs', 'evaluate', 'metrics.py'))
    similarity = torch.load(ppgs.SIMILARITY_MATRIX_PATH)

    # case A's seed: the first whose weighted argmax is nowhere nearer a tie than 1e-3 (relative)
    seed_a = next(seed for seed in range(1300, 4000)
                  if gaps(*build_inputs(seed, *CASES['A'])[:2], weights)[1] >= 1e-3)
    seeds = {'A': seed_a, 'B': SEED_B, 'C': 1303, 'D': 1304}
    out = dict(similarity=similarity, exponent=ppgs.SIMILARITY_EXPONENT, weights=weights)
    meta = {}
    for case, (batch, frames) in CASES.items():
        logits, labels, lengths = build_inputs(seeds[case], batch, frames, empty=case == 'C')
        figures = case in 'AB'
        m = metrics.Metrics(include_figures=figures)
        m.update(logits, labels)
        accuracy, categorical, jsd, topk, loss = m.metrics[:5]
        keep = labels.flatten() != -100
        rows = logits.transpose(1, 2).flatten(0, 1)[keep]
        target = labels.flatten()[keep]
        probs = torch.softmax(rows, dim=-1)
        onehot = torch.nn.functional.one_hot(target, num_classes=40).float()
        out.update({
            f'{case}_count': int(accuracy.count), f'{case}_true_positives': int(accuracy.true_positives),
            f'{case}_topk_correct': int(topk.correct_in_top_k),
            f'{case}_class_total': categorical.totals, f'{case}_class_count': categorical.counts,
            f'{case}_jsd_total': float(jsd.total), f'{case}_loss_total': float(loss.total),
            # what the reference's calls give with normalize=False / CLASS_BALANCED=True
            f'{case}_jsd_plain_total': float(core.distance(probs.T, onehot.T, reduction='sum', normalize=False)),
            f'{case}_loss_balanced_total': float(torch.nn.functional.cross_entropy(
                logits, labels, weights, reduction='sum')),
            f'{case}_lengths': lengths,
        })
        results = {}                      # (not m(): the DistanceMatrix would render its figure)
        for metric in m.metrics[:5]:
            results.update(metric())
        if figures:
            distance = m.metrics[5]
            assert (labels == 39).any(), case
            assert torch.equal(distance.count, categorical.counts)
            out[f'{case}_distance_matrix'] = distance.matrix
            out[f'{case}_confusion'] = restate_matrices(logits, labels, weights)[1]
        else:
            out[f'{case}_distance_matrix'], out[f'{case}_confusion'] = restate_matrices(logits, labels, weights)
        out[f'{case}_results'] = json.dumps(results)
        if keep.any():
            logit_gap, weighted_gap = gaps(logits, labels, weights)
            assert logit_gap > 0, (case, logit_gap)          # distinct fp32 values: the integer results are exact
            meta[case] = dict(seed=seeds[case], logit_gap=logit_gap, weighted_gap=weighted_gap)
        else:
            meta[case] = dict(seed=seeds[case])
        if case == 'A':
            assert weighted_gap >= 1e-3, weighted_gap
        if case == 'B':
            out['B_checksum'], out['B_abs_checksum'] = checksums(logits)
        else:
            out[f'{case}_logits'] = logits
            out[f'{case}_labels'] = labels
        out[f'{case}_seed'] = seeds[case]
    out['cases'] = json.dumps(meta)
    print(json.dumps(meta, indent=1))
    G.save('g13_metrics', **out)


if __name__ == '__main__':
    main()
