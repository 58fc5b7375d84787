"""ppgs_amd.dtw without a GPU: the C ABI is declared and exported, the workspace helper is host-only and monotone,
the compute entry fails loudly without a device, every argument error is raised before a device is needed,
dtw.grid is plain tensor arithmetic, and the tests' own float64 programme is right on a table worked by hand."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import ppgs_amd
from ppgs_amd import dtw, engine as E

import dtw_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_declares_and_library_exports_the_entry_points():
    text = open(os.path.join(ROOT, 'include', 'ppgs_amd.h')).read()
    code = re.sub(r'/\*.*?\*/', '', text, flags=re.S)
    for name in ('ppg_dtw', 'ppg_dtw_workspace_bytes'):
        assert re.search(r'\b%s\s*\(' % name, code), name
        assert name in E.SYMBOLS and hasattr(E.library(), name)
    limit = int(re.search(r'#define\s+PPG_DTW_MAX_FRAMES\s+(\d+)', code).group(1))
    assert limit >= 4096 and limit == E.DTW_MAX_FRAMES == dtw.MAX_FRAMES
    assert int(re.search(r'#define\s+PPG_DTW_MAX_PAIRS\s+(\d+)', code).group(1)) == E.DTW_MAX_PAIRS
    assert ppgs_amd.dtw is dtw


def test_workspace_helper_is_sensible_and_monotone():
    size = E.library().ppg_dtw_workspace_bytes
    one = size(1, 1, 1, 0)
    assert 0 < one < 1 << 20
    for pairs, fx, fy in ((1, 57, 43), (3, 300, 1), (2, 1000, 1000), (1, 4096, 4096)):
        plain, path = size(pairs, fx, fy, 0), size(pairs, fx, fy, 1)
        cells = pairs * fx * fy
        assert plain >= 4 * cells + 320 * pairs * (fx + fy)         # fp32 cost table + prepared frames
        assert path >= plain + cells                                # + a direction byte per cell
        assert size(pairs + 1, fx, fy, 0) > plain
        assert size(pairs, min(fx + 300, 4096), fy, 0) >= plain and size(pairs, fx, min(fy + 300, 4096), 0) >= plain
        # no more than the documented padding: rows to a multiple of 256, columns + 63 to a multiple of 64
        rows, columns = -(-fx // 256) * 256, fy + 126
        assert path <= pairs * (5 * rows * columns + 320 * (fx + fy)) + 4096
    assert size(1, 4096, 4096, 1) < 1 << 28
    # out of range: 0, never a wrapped number
    for bad in ((0, 10, 10, 0), (1, 0, 10, 0), (1, 10, 0, 0), (1, E.DTW_MAX_FRAMES + 1, 10, 0),
                (1, 10, E.DTW_MAX_FRAMES + 1, 1), (E.DTW_MAX_PAIRS + 1, 10, 10, 0), (-1, 10, 10, 0)):
        assert size(*bad) == 0, bad


def test_compute_entry_fails_loudly_without_gpu():
    if torch.cuda.is_available():
        pytest.skip('GPU present')
    lib = E.library()
    dummy = ctypes.c_void_p(256)
    need = lib.ppg_dtw_workspace_bytes(1, 10, 12, 1)
    rc = lib.ppg_dtw(0, dummy, 10, dummy, 12, 1, dummy, dummy, None, dummy, dummy, dummy, dummy, None, dummy, need, None)
    assert rc == -2 and b'no HIP device' in lib.ppg_last_error()
    with pytest.raises(E.PpgError):
        dtw.distance(torch.rand(40, 5), torch.rand(40, 7), normalize=False)
    with pytest.raises(E.PpgError):
        dtw.align(torch.rand(40, 5), torch.rand(40, 7), normalize=False)


def test_bad_arguments_return_einval():
    lib = E.library()
    dummy = ctypes.c_void_p(256)
    need = lib.ppg_dtw_workspace_bytes(1, 10, 12, 1)

    def call(x=dummy, fx=10, fy=12, pairs=1, path=dummy, length=dummy, cost=None, ws=dummy, size=need):
        return lib.ppg_dtw(0, x, fx, dummy, fy, pairs, dummy, dummy, None, dummy, dummy, path, length, cost, ws, size, None)
    assert call(x=None) == -1
    assert call(fx=0) == -1 and call(fy=-3) == -1 and call(pairs=0) == -1
    assert call(fx=E.DTW_MAX_FRAMES + 1, size=1 << 40) == -1 and b'at most' in lib.ppg_last_error()
    assert call(pairs=E.DTW_MAX_PAIRS + 1, size=1 << 40) == -1
    assert call(size=need - 1) == -1 and b'workspace' in lib.ppg_last_error()
    assert call(ws=None) == -1
    assert call(path=None, length=dummy) == -1 and call(path=None, length=None, cost=dummy) == -1
    assert call(path=dummy, length=None) == -1
    assert call(ws=ctypes.c_void_p(260)) == -1


def test_value_errors_come_before_any_device_call():
    x, y = torch.rand(40, 5), torch.rand(40, 7)
    bx, by = torch.rand(3, 40, 5), torch.rand(3, 40, 7)
    cases = [
        (torch.rand(39, 5), y, {}),                                      # channels
        (x, torch.rand(41, 7), {}),
        (torch.rand(3, 39, 5), by, {}),
        (torch.rand(40, 0), y, {}),                                      # zero frames
        (x, torch.rand(40, 0), {}),
        (bx, by, {'lengths_x': [5, 0, 1]}),                              # a length outside [1, padded frames]
        (bx, by, {'lengths_y': [7, 8, 1]}),
        (bx, by, {'lengths_x': torch.tensor([5, -1, 1])}),
        (bx, by, {'lengths_x': [5, 5]}),                                 # one length per item
        (bx, torch.rand(2, 40, 7), {}),                                  # batch sizes
        (bx, y, {}),                                                     # batch against single
        (torch.rand(40, dtw.MAX_FRAMES + 1), y, {}),                     # longer than the documented maximum
        (x, torch.rand(40, dtw.MAX_FRAMES + 1), {}),
        (x, y, {'reduction': 'median'}),                                 # unknown reduction
        (bx, by, {'reduction': 'none'}),                                 # 'none' with a batch
    ]
    for ppg_x, ppg_y, keywords in cases:
        with pytest.raises(ValueError):
            dtw.distance(ppg_x, ppg_y, normalize=False, **keywords)
        keywords = {k: v for k, v in keywords.items() if k != 'reduction'}
        if keywords or ppg_x.shape[-2:] != x.shape or ppg_y.shape[-2:] != y.shape:
            with pytest.raises(ValueError):
                dtw.align(ppg_x, ppg_y, normalize=False, **keywords)
    with pytest.raises(ValueError, match='Reduction method median not defined'):       # the reference's wording
        dtw.distance(x, y, reduction='median')


def test_grid_on_hand_written_paths():
    diagonal = torch.arange(9, dtype=torch.int32)[:, None].expand(-1, 2)
    out = dtw.grid(diagonal, 9)
    assert out.dtype == torch.float32 and torch.equal(out, torch.arange(9, dtype=torch.float32))
    # X's frame 3 held against Y's frames 3, 4 and 5; then frames 5 and 6 of X both on Y's frame 8
    path = torch.tensor([[0, 0], [1, 1], [2, 2], [3, 3], [3, 4], [3, 5], [4, 6], [4, 7], [5, 8], [6, 8], [7, 9]],
                        dtype=torch.int32)
    out = dtw.grid(path, 8)
    assert out.shape == (8,) and not out.is_cuda
    assert out.tolist() == [0., 1., 2., 4., 6.5, 8., 8., 9.]
    assert bool((out[1:] >= out[:-1]).all())
    # every path of the reference programme gives a monotone grid of the asked length
    rng = np.random.default_rng(3)
    for frames_x, frames_y in ((1, 1), (1, 9), (9, 1), (17, 30), (30, 17)):
        _, path = R.dtw(rng.random((frames_x, frames_y)))
        out = dtw.grid(torch.from_numpy(path), frames_x)
        assert out.shape == (frames_x,) and bool((out[1:] >= out[:-1]).all())
        assert out[0] >= 0 and out[-1] <= frames_y - 1
    with pytest.raises(ValueError):
        dtw.grid(torch.tensor([[0, 0], [2, 1]]), 3)              # frame 1 of X is on no cell
    with pytest.raises(ValueError):
        dtw.grid(torch.zeros(4, 3), 4)


def test_reference_programme_on_a_table_worked_by_hand():
    cost = [[1, 2, 3, 4],
            [2, 1, 2, 3],
            [3, 2, 1, 1]]
    # D = [[1, 3, 6, 10], [3, 2, 4, 7], [6, 4, 3, 4]]
    total, path = R.dtw(cost)
    assert total == 4.0
    assert path.tolist() == [[0, 0], [1, 1], [2, 2], [2, 3]]
    R.check_path(path, 3, 4)
    # ties: the diagonal first ...
    total, path = R.dtw(np.zeros((2, 2)))
    assert total == 0.0 and path.tolist() == [[0, 0], [1, 1]]
    # ... then (i-1, j) before (i, j-1): D[0, 1] = D[1, 0] = -1 < D[0, 0] = 0
    total, path = R.dtw([[0, -1], [-1, 5]])
    assert total == 4.0 and path.tolist() == [[0, 0], [0, 1], [1, 1]]
    # a single row and a single column have one path each
    total, path = R.dtw([[1, 2, 3]])
    assert total == 6.0 and path.tolist() == [[0, 0], [0, 1], [0, 2]]
    total, path = R.dtw([[1], [2], [3]])
    assert total == 6.0 and path.tolist() == [[0, 0], [1, 0], [2, 0]]
    # the cost matrix is the oracle's per-frame distance: its diagonal is distance(..., 'none')
    generator = torch.Generator().manual_seed(0)
    x, y = R.random_ppg(6, 3., generator), R.random_ppg(6, 3., generator)
    from oracle import ppg_oracle as O
    assert np.array_equal(np.diag(R.cost_matrix(x, y)), O.distance(x, y, None, 1.2, 'none').double().numpy())
