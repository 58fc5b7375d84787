"""ppgs.evaluate.Metrics (reference ppgs/evaluate/metrics.py) on engine.MetricsState."""
import os

import numpy as np
import torch

from .. import config, core, engine
from ..phonemes import PHONEMES

_weights_cache = {}


def phoneme_weights():
    """The reference's 40 phoneme class weights (ppgs.load.phoneme_weights, a data asset of the reference package,
    not of this one): read from the .pt file PPGS_AMD_PHONEME_WEIGHTS names (a bare tensor, loaded with
    weights_only=True) and cached per path, as core.similarity_matrix does for its matrix."""
    path = os.environ.get('PPGS_AMD_PHONEME_WEIGHTS')
    if path is None:
        raise ValueError(
            'the weighted distance matrix and the class-balanced loss need the phoneme class weights: pass '
            'weights=<(40,) tensor> or set PPGS_AMD_PHONEME_WEIGHTS to the reference\'s phoneme_weights.pt')
    if path not in _weights_cache:
        weights = torch.load(path, map_location='cpu', weights_only=True)
        if not torch.is_tensor(weights) or tuple(weights.shape) != (config.OUTPUT_CHANNELS,):
            raise ValueError(f'{path}: expected a ({config.OUTPUT_CHANNELS},) tensor')
        _weights_cache[path] = weights
    return _weights_cache[path]


def format_results(state, include_figures=False):
    """The reference's result dict (Metrics.__call__) from a MetricsState.read() dict.  Zero counts give NaN,
    as the reference's 0 / 0 tensor divisions do.  With `include_figures`: 'DistanceMatrix' (rows normalised
    to sum 1, DistanceMatrix._normalized) and 'ConfusionMatrix' (rows = label, accumulated softmax) as
    (40, 40) float64 tensors where the reference renders figures."""
    if state['invalid_labels']:
        raise ValueError(
            f'{state["invalid_labels"]} frames have a label that is neither -100 nor in [0, {len(PHONEMES)})')
    scale = engine.METRICS_FIXED_POINT
    count = state['count']

    def ratio(numerator, denominator):
        return float(numerator) / float(denominator) if denominator else float('nan')
    results = {'Accuracy': ratio(state['true_positives'], count)}
    for index, phoneme in enumerate(PHONEMES):
        total, frames = int(state['class_total'][index]), int(state['class_count'][index])
        results[f'Accuracy/{phoneme}'] = ratio(total, frames)
        results[f'Total/{phoneme}'] = total
        results[f'Count/{phoneme}'] = frames
    results['JSD'] = ratio(state['jsd_sum'] / scale, count)
    results[f'Top-{state["k"]} Accuracy/'] = ratio(state['topk_correct'], count)
    results['loss'] = ratio(state['loss_sum'] / scale, count)
    if include_figures:
        distance = torch.from_numpy(np.asarray(state['distance_matrix'], dtype=np.float64) / scale)
        results['DistanceMatrix'] = distance / distance.sum(dim=1)[:, None]
        results['ConfusionMatrix'] = torch.from_numpy(np.asarray(state['confusion'], dtype=np.float64) / scale)
    return results


class Metrics:
    """Drop-in for the reference's ppgs.evaluate.Metrics: update(logits, labels) per batch, __call__() for the
    result dict with the reference's keys.  update() is one kernel launch and does not synchronise.

    normalize / similarity: the similarity-normalised JSD of ppgs.distance (the matrix from `similarity` or
    PPGS_AMD_SIMILARITY_MATRIX); weights: the phoneme class weights of the distance matrix and of the
    class-balanced loss (`weights` or PPGS_AMD_PHONEME_WEIGHTS; needed with include_figures or class_balanced)."""

    def __init__(self, include_figures=False, k=3, normalize=True, similarity=None, weights=None,
                 class_balanced=False, gpu=None):
        self.include_figures = include_figures
        device = core.device_for(gpu)
        mix = None
        if normalize:
            if similarity is None:
                similarity = core.similarity_matrix()
            mix = core._similarity_mix(similarity, config.SIMILARITY_EXPONENT, device)
        if weights is None and (include_figures or class_balanced):
            weights = phoneme_weights()
        self.state = engine.MetricsState(
            device.index, k=k, similarity_mix=mix, class_weights=weights,
            loss_weights=weights if class_balanced else None)

    def update(self, predicted_logits, target_indices, lengths=None):
        self.state.update(predicted_logits, target_indices, lengths)

    def reset(self):
        self.state.reset()

    def read(self):
        return self.state.read()

    def __call__(self):
        return format_results(self.state.read(), self.include_figures)
