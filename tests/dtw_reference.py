"""CPU restatement of ppgs_amd.dtw for the tests (tests/test_dtw_host.py, tests/test_gpu_dtw.py; tests/dtw_probe.py
restates the programme in fp32 and is held against this one): the cost matrix
from the oracle's per-frame distance, a float64 dynamic programme with the documented tie-break (diagonal, then
(i-1, j), then (i, j-1)) vectorised over anti-diagonals, and its own trace-back."""
import numpy as np
import torch

from oracle import ppg_oracle as O


def cost_matrix(x, y, similarity=None, exponent=1.2):
    """(Tx, Ty) float64: row i is oracle.distance(frame i of x repeated, y, reduction='none')."""
    frames_x, frames_y = x.shape[1], y.shape[1]
    out = np.empty((frames_x, frames_y), dtype=np.float64)
    for i in range(frames_x):
        row = O.distance(x[:, i:i + 1].expand(-1, frames_y), y, similarity, exponent, 'none')
        out[i] = row.double().numpy()
    return out


def dtw(cost):
    """(total, path) of the float64 programme over `cost` (Tx, Ty); path is (K, 2) int64, forward order."""
    cost = np.asarray(cost, dtype=np.float64)
    frames_x, frames_y = cost.shape
    table = np.full((frames_x + 1, frames_y + 1), np.inf)
    table[0, 0] = 0.                                   # the virtual origin: D[0, 0] = C[0, 0]
    moves = np.zeros((frames_x, frames_y), dtype=np.int8)
    for d in range(frames_x + frames_y - 1):
        i = np.arange(max(0, d - frames_y + 1), min(d, frames_x - 1) + 1)
        j = d - i
        best = table[i, j].copy()                      # diagonal
        move = np.zeros(len(i), dtype=np.int8)
        up = table[i, j + 1]
        take = up < best
        best[take], move[take] = up[take], 1
        left = table[i + 1, j]
        take = left < best
        best[take], move[take] = left[take], 2
        table[i + 1, j + 1] = cost[i, j] + best
        moves[i, j] = move
    i, j = frames_x - 1, frames_y - 1
    path = [(i, j)]
    while (i, j) != (0, 0):
        move = moves[i, j]
        i, j = i - (move != 2), j - (move != 1)
        path.append((i, j))
    return float(table[frames_x, frames_y]), np.asarray(path[::-1], dtype=np.int64)


def check_path(path, frames_x, frames_y):
    """A valid warping path: corner to corner, every step one of the three unit moves."""
    path = np.asarray(path)
    assert path.ndim == 2 and path.shape[1] == 2
    assert tuple(path[0]) == (0, 0) and tuple(path[-1]) == (frames_x - 1, frames_y - 1)
    steps = np.diff(path, axis=0)
    assert ((steps >= 0) & (steps <= 1)).all() and (steps.sum(axis=1) >= 1).all()
    assert max(frames_x, frames_y) <= len(path) <= frames_x + frames_y - 1


def random_ppg(frames, scale, generator):
    return torch.softmax(scale * torch.randn(40, frames, generator=generator), dim=0)
