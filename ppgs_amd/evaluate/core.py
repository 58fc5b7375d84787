"""ppgs.evaluate.datasets' inner loop and save (reference ppgs/evaluate/core.py) on the engine."""
import json
import os

import torch

from .. import config, core
from .metrics import Metrics


def from_dataloader(dataloader, checkpoint=None, representation=config.REPRESENTATION, gpu=None, precision=None,
                    metrics=None):
    """Score a checkpoint over batches of (features, indices, lengths) -- the loop of the reference's
    evaluate.datasets (ppgs/evaluate/core.py:44-60): logits from the engine, then one metrics launch, both on
    the current stream; nothing is read back until the loader is exhausted.  Returns the result dict."""
    device = core.device_for(gpu)
    model = core.engine_for(representation, checkpoint, device.index, precision)
    if metrics is None:
        metrics = Metrics(gpu=device.index)
    with torch.cuda.device(device):
        for features, indices, lengths in dataloader:
            logits = model.encode(features.to(device, non_blocking=True), lengths, softmax=False)
            metrics.update(logits, indices, lengths)
    return metrics()


def save(results, name, directory, save_json=True):
    """Write <directory>/<name>.json, tensors to <directory>/<name>/<metric>.pt ('/' in a metric's name becomes
    '-'), nested dicts flattened the same way: the reference's file naming (ppgs/evaluate/core.py:77-107)."""
    directory = os.fspath(directory)
    tensor_directory = os.path.join(directory, name)
    os.makedirs(tensor_directory, exist_ok=True)
    for metric, value in list(results.items()):
        if isinstance(value, dict):
            save(value, name, directory, save_json=False)
        elif isinstance(value, torch.Tensor) and value.dim() >= 1:
            torch.save(value, os.path.join(tensor_directory, f'{metric.replace("/", "-")}.pt'))
            del results[metric]
    if save_json:
        with open(os.path.join(directory, f'{name}.json'), 'w') as file:
            json.dump(results, file, indent=4)


def across_precisions(features, lengths, checkpoint=None, precisions=('fp32', 'fp16x2', 'fp16', 'bf16'),
                      representation=config.REPRESENTATION, gpu=None):
    """What the operand precisions cost in the reported metrics, without labelled data: labels := argmax of the
    fp32 engine's logits, then every precision's logits scored against them.  {precision: result dict}."""
    device = core.device_for(gpu, features)
    features = features.to(device)
    reference = core.engine_for(representation, checkpoint, device.index, 'fp32')
    labels = reference.encode(features, lengths, softmax=False).argmax(dim=1)
    results = {}
    for precision in precisions:
        model = core.engine_for(representation, checkpoint, device.index, precision)
        metrics = Metrics(normalize=False, gpu=device.index)
        metrics.update(model.encode(features, lengths, softmax=False), labels, lengths)
        results[precision] = metrics()
    return results
