"""Pronunciation distance and alignment for PPGs of different lengths.

`ppgs_amd.distance` compares two PPGs frame for frame, so they must already be
aligned.  This module aligns them: dynamic time warping over that same
per-frame term, on the GPU (ppg_dtw, ppgs_amd/csrc/ppg_dtw.hip).

    C[i, j]  the per-frame term of `distance` for frame i of X and frame j of Y
    D[0, 0] = C[0, 0]
    D[i, j] = C[i, j] + min(D[i-1, j-1], D[i-1, j], D[i, j-1])        (fp32)

Ties go to the diagonal first, then (i-1, j), then (i, j-1).  The path runs
from (0, 0) to (Tx-1, Ty-1) in K cells, max(Tx, Ty) <= K <= Tx + Ty - 1;
total = D[Tx-1, Ty-1].  Equal frames cost exactly 0.

    path, total, K = ppgs_amd.dtw.align(x, y)
    y_on_x = ppgs_amd.edit.grid.sample(y, ppgs_amd.dtw.grid(path, x.shape[-1]))
    ppgs_amd.distance(x, y_on_x)          # the aligned distance, frame for frame
"""
import torch

from . import config, core, engine

MAX_FRAMES = engine.DTW_MAX_FRAMES      # per side


def _lengths(lengths, batch, frames, side):
    if lengths is None:
        return [frames] * batch
    if torch.is_tensor(lengths):
        lengths = lengths.detach().cpu().reshape(-1).tolist()
    elif isinstance(lengths, int):
        lengths = [lengths]
    lengths = [int(v) for v in lengths]
    if len(lengths) != batch:
        raise ValueError(f'lengths_{side} has {len(lengths)} entries for a batch of {batch}')
    for value in lengths:
        if not 1 <= value <= frames:
            raise ValueError(f'lengths_{side}: {value} is outside [1, {frames}]')
    return lengths


def _run(ppgX, ppgY, reduction, normalize, exponent, similarity, lengths_x, lengths_y, want_path, want_cost):
    """Every check that needs no device, then the device call: (batched, total, K, paths, costs)."""
    if reduction not in ('mean', 'sum', 'none', None):
        raise ValueError(f'Reduction method {reduction} not defined')
    if ppgX.dim() != ppgY.dim() or ppgX.dim() not in (2, 3):
        raise ValueError(
            f'PPGs must both be (40, frames) or both (batch, 40, frames), got {tuple(ppgX.shape)} and {tuple(ppgY.shape)}')
    batched = ppgX.dim() == 3
    if ppgX.shape[-2] != config.OUTPUT_CHANNELS or ppgY.shape[-2] != config.OUTPUT_CHANNELS:
        raise ValueError(
            f'PPGs must have {config.OUTPUT_CHANNELS} channels, got {tuple(ppgX.shape)} and {tuple(ppgY.shape)}')
    frames_x, frames_y = ppgX.shape[-1], ppgY.shape[-1]
    if frames_x < 1 or frames_y < 1:
        raise ValueError(f'PPGs must have at least one frame, got {tuple(ppgX.shape)} and {tuple(ppgY.shape)}')
    if batched and ppgX.shape[0] != ppgY.shape[0]:
        raise ValueError(f'batch sizes differ: {ppgX.shape[0]} and {ppgY.shape[0]}')
    if batched and ppgX.shape[0] < 1:
        raise ValueError('empty batch')
    if batched and reduction in ('none', None):
        raise ValueError("reduction 'none' returns one path's costs: it takes one pair, not a batch")
    if frames_x > MAX_FRAMES or frames_y > MAX_FRAMES:
        raise ValueError(f'dtw takes at most {MAX_FRAMES} frames per side, got {frames_x} and {frames_y}')
    batch = ppgX.shape[0] if batched else 1
    if not batched and (lengths_x is not None or lengths_y is not None):
        raise ValueError('lengths go with a batch: slice a single PPG instead')
    lengths_x = _lengths(lengths_x, batch, frames_x, 'x')
    lengths_y = _lengths(lengths_y, batch, frames_y, 'y')
    device = core.device_for(None, ppgX)
    mix = None
    if normalize:
        if similarity is None:
            similarity = core.similarity_matrix()
        mix = core._similarity_mix(similarity, exponent, device)
    x, y = ppgX.to(device), ppgY.to(device)
    if not batched:
        x, y = x[None], y[None]
    total, steps, paths, costs = engine.dtw_pairs(x, y, lengths_x, lengths_y, mix, want_path, want_cost)
    return batched, total, steps, paths, costs


def distance(ppgX, ppgY, reduction='mean', normalize=True, exponent=config.SIMILARITY_EXPONENT, similarity=None,
             lengths_x=None, lengths_y=None):
    """Pronunciation distance between PPGs of different lengths: the cost of the best monotone alignment.

    (40, Tx) and (40, Ty), or batches (B, 40, Tx) and (B, 40, Ty) padded to the longest item with `lengths_x` /
    `lengths_y` per item (pair b compares item b of each side; the padding is never read).  'sum' is the total cost
    of the path, 'mean' that divided by its number of cells K: a scalar, or (B,) for a batch.  'none' is the K
    cell costs along the path, for a single pair.  `normalize`, `exponent` and `similarity` as in
    `ppgs_amd.distance`.  'mean' and 'sum' build no path: the dynamic programme carries K beside the cost."""
    none = reduction in ('none', None)
    batched, total, steps, _, costs = _run(
        ppgX, ppgY, reduction, normalize, exponent, similarity, lengths_x, lengths_y, none, none)
    if none:
        return costs[0, :int(steps[0])]
    out = total / steps.to(torch.float32) if reduction == 'mean' else total
    return out if batched else out[0]


def align(ppgX, ppgY, normalize=True, exponent=config.SIMILARITY_EXPONENT, similarity=None,
          lengths_x=None, lengths_y=None):
    """The best alignment itself: (path, total, K).

    One pair: path (K, 2) int32 on the device, rows (i, j) = (frame of X, frame of Y) from (0, 0) to (Tx-1, Ty-1);
    total a 0-d device tensor; K an int.  A batch: a list of B paths, total (B,) on the device, K a list of ints."""
    batched, total, steps, paths, _ = _run(
        ppgX, ppgY, 'sum', normalize, exponent, similarity, lengths_x, lengths_y, True, False)
    counts = steps.tolist()
    if not batched:
        return paths[0, :counts[0]], total[0], counts[0]
    return [paths[b, :k] for b, k in enumerate(counts)], total, counts


def grid(path, frames_x):
    """A path as a time-stretch grid for `edit.grid.sample`: for every frame i of X the mean of the frames of Y
    matched to it, (frames_x,) float, non-decreasing.  `edit.grid.sample(ppgY, grid(path, Tx))` is Y on X's time
    line.  Plain tensor arithmetic: works on CPU and device paths alike."""
    if path.dim() != 2 or path.shape[1] != 2 or path.shape[0] < 1:
        raise ValueError(f'path must be (K >= 1, 2), got {tuple(path.shape)}')
    rows = path[:, 0].long()
    sums = torch.zeros(frames_x, dtype=torch.float64, device=path.device).index_add_(0, rows, path[:, 1].double())
    counts = torch.zeros(frames_x, dtype=torch.float64, device=path.device).index_add_(0, rows, torch.ones_like(sums[rows]))
    if bool((counts == 0).any()):
        raise ValueError(f'path does not visit every one of the {frames_x} frames of X')
    return (sums / counts).to(torch.float32)
