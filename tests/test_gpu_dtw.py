"""ppgs_amd.dtw on the GPU against the CPU restatement of tests/dtw_reference.py (the oracle's per-frame distance,
a float64 dynamic programme with the same tie-break).

The per-cell bound is the one test_postops_match_reference_fixture uses for the same arithmetic (rtol 2e-5,
atol 2e-6); a total accumulates it over the K cells of a path: rtol 2e-5 of the total plus K x 2e-6.  Paths are
compared by cost, never by identity, except where the margin between the best and every other path is orders of
magnitude above that bound."""
import numpy as np
import pytest
import torch

import ppgs_amd
from ppgs_amd import dtw
from ppgs_amd.edit import grid

import dtw_reference as R

pytestmark = pytest.mark.gpu

RTOL, ATOL = 2e-5, 2e-6


def fixture(golden):
    g = golden('g9_postops')
    return (torch.from_numpy(g['x']), torch.from_numpy(g['y']), torch.from_numpy(g['similarity']),
            float(g['exponent']), g)


def test_cell_cost_matches_reference_fixture(golden):
    x, y, sim, exponent, g = fixture(golden)
    assert x.shape == (40, 57)
    for normalize in (True, False):
        keywords = dict(normalize=normalize, similarity=sim, exponent=exponent)
        same = dtw.distance(x.cuda(), x.cuda(), reduction='none', **keywords)
        assert same.shape == (57,) and same.dtype == torch.float32 and bool((same == 0).all())
        path, total, count = dtw.align(x.cuda(), x.cuda(), **keywords)
        assert count == 57 and float(total) == 0.0
        assert path.dtype == torch.int32 and path.is_cuda
        assert path.cpu().tolist() == [[i, i] for i in range(57)]
        # every frame pair as a 1 x 1 problem: the device cost of cell (i, i), one value per pair
        cells = dtw.distance(x.T[:, :, None].cuda(), y.T[:, :, None].cuda(), reduction='sum', **keywords)
        ref = np.asarray(g[f'distance_{int(normalize)}_none'])
        error = np.abs(cells.cpu().numpy() - ref).max()
        print(f'dtw cell cost normalize={normalize}: max abs error {error:.3e} against the reference fixture')
        assert cells.shape == (57,) and np.allclose(cells.cpu().numpy(), ref, rtol=RTOL, atol=ATOL)
        mean = dtw.distance(x.T[:, :, None].cuda(), y.T[:, :, None].cuda(), **keywords)
        assert torch.equal(mean, cells)                       # K = 1


SIZES = [(1, 1), (1, 300), (300, 1), (57, 43), (500, 731), (1000, 1000), (dtw.MAX_FRAMES, 37), (29, dtw.MAX_FRAMES)]


@pytest.mark.parametrize('normalize', [True, False])
def test_optimum_and_path_against_float64_programme(golden, normalize):
    _, _, sim, exponent, _ = fixture(golden)
    generator = torch.Generator().manual_seed(20)
    worst = 0.
    for frames_x, frames_y in SIZES:
        for scale in (1., 3., 8.):
            x, y = R.random_ppg(frames_x, scale, generator), R.random_ppg(frames_y, scale, generator)
            cost = R.cost_matrix(x, y, sim if normalize else None, exponent)
            ref_total, ref_path = R.dtw(cost)
            keywords = dict(normalize=normalize, similarity=sim, exponent=exponent)
            xd, yd = x.cuda(), y.cuda()
            path, total, count = dtw.align(xd, yd, **keywords)
            total, path = float(total), path.cpu().numpy()
            # distance-only and alignment runs are the same programme
            assert float(dtw.distance(xd, yd, reduction='sum', **keywords)) == total
            mean = float(dtw.distance(xd, yd, **keywords))
            assert mean == float(torch.tensor(total, dtype=torch.float32) / torch.tensor(count, dtype=torch.float32))
            # the optimum: two-sided, each side over the cells of the path that bounds it
            worst = max(worst, abs(total - ref_total) / max(ref_total, 1e-30))
            assert total - ref_total <= RTOL * ref_total + len(ref_path) * ATOL, (frames_x, frames_y, scale)
            assert ref_total - total <= RTOL * ref_total + count * ATOL, (frames_x, frames_y, scale)
            # the path: valid, as good as the optimum on the oracle's costs, and consistent with the device total
            assert len(path) == count
            R.check_path(path, frames_x, frames_y)
            on_oracle = cost[path[:, 0], path[:, 1]].sum()
            assert on_oracle - ref_total <= RTOL * ref_total + count * ATOL, (frames_x, frames_y, scale)
            cells = dtw.distance(xd, yd, reduction='none', **keywords)
            assert cells.shape == (count,)
            assert abs(cells.double().sum().item() - total) <= 1e-5 * total
    print(f'dtw optimum normalize={normalize}: largest relative error of total {worst:.3e}')


def repeated_pair():
    generator = torch.Generator().manual_seed(5)
    frames = 300
    peak = torch.zeros(40, frames)
    peak[(7 * torch.arange(frames)) % 40, torch.arange(frames)] = 10.
    x = torch.softmax(torch.randn(40, frames, generator=generator) + peak, dim=0)
    repeats = torch.randint(1, 4, (frames,), generator=generator)
    y = torch.repeat_interleave(x, repeats, dim=1)
    expected = np.stack([np.repeat(np.arange(frames), repeats.numpy()), np.arange(y.shape[1])], axis=1)
    return x, y, expected


def test_exact_path_where_the_margin_allows_it(golden):
    _, _, sim, exponent, _ = fixture(golden)
    x, y, expected = repeated_pair()
    cost = R.cost_matrix(x, y)
    on_path = np.zeros(cost.shape, dtype=bool)
    on_path[expected[:, 0], expected[:, 1]] = True
    assert (cost[on_path] == 0).all()
    margin = cost[~on_path].min()
    print(f'dtw exact path: Ty = {y.shape[1]}, smallest cost off the expected path {margin:.4f}')
    assert margin >= 0.03
    xd, yd = x.cuda(), y.cuda()
    path, total, count = dtw.align(xd, yd, normalize=False)
    assert count == len(expected) and float(total) == 0.0
    assert np.array_equal(path.cpu().numpy(), expected)
    warp = dtw.grid(path, x.shape[1])
    assert warp.is_cuda and warp.shape == (300,)
    assert torch.equal(grid.sample(yd, warp), xd)
    # the other way round: X's frames held against their copies
    back, total, count = dtw.align(yd, xd, normalize=False)
    assert float(total) == 0.0 and np.array_equal(back.cpu().numpy(), expected[:, ::-1])
    # with the similarity mix the margin is too small to pin the path; the distance is still exactly 0
    keywords = dict(similarity=sim, exponent=exponent)
    assert float(dtw.distance(xd, yd, **keywords)) == 0.0
    path, _, _ = dtw.align(xd, yd, **keywords)
    assert float(ppgs_amd.distance(xd, grid.sample(yd, dtw.grid(path, 300)), **keywords)) == 0.0


def ragged_batch(pairs, longest, seed):
    generator = torch.Generator().manual_seed(seed)
    lengths_x = torch.randint(1, longest + 1, (pairs,), generator=generator)
    lengths_y = torch.randint(1, longest + 1, (pairs,), generator=generator)
    lengths_x[0], lengths_y[0], lengths_x[1], lengths_y[1] = 1, longest, longest, 1
    x = torch.full((pairs, 40, int(lengths_x.max())), float('nan'))
    y = torch.full((pairs, 40, int(lengths_y.max())), float('nan'))
    for b in range(pairs):
        x[b, :, :lengths_x[b]] = R.random_ppg(int(lengths_x[b]), 3., generator)
        y[b, :, :lengths_y[b]] = R.random_ppg(int(lengths_y[b]), 3., generator)
    return x, y, lengths_x, lengths_y


def test_batch_equals_singles_also_from_two_streams(golden):
    _, _, sim, exponent, _ = fixture(golden)
    x, y, lengths_x, lengths_y = ragged_batch(64, 700, 9)
    xd, yd = x.cuda(), y.cuda()
    keywords = dict(similarity=sim, exponent=exponent, lengths_x=lengths_x, lengths_y=lengths_y)
    paths, total, counts = dtw.align(xd, yd, **keywords)
    assert total.shape == (64,) and bool(torch.isfinite(total).all())
    assert torch.equal(dtw.distance(xd, yd, reduction='sum', **keywords), total)
    assert torch.equal(dtw.distance(xd, yd, **keywords), total / torch.tensor(counts, device='cuda', dtype=torch.float32))
    single = dict(similarity=sim, exponent=exponent)
    for b in range(64):
        one_x, one_y = xd[b, :, :lengths_x[b]], yd[b, :, :lengths_y[b]]
        path, one_total, one_count = dtw.align(one_x, one_y, **single)
        assert one_count == counts[b] and torch.equal(one_total, total[b]), b
        assert torch.equal(path, paths[b]), b
        assert torch.equal(dtw.distance(one_x, one_y, reduction='sum', **single), total[b]), b
    # two streams at once: X against Y on one, Y against X on the other
    swapped = dict(similarity=sim, exponent=exponent, lengths_x=lengths_y, lengths_y=lengths_x)
    expected_swapped = dtw.distance(yd, xd, reduction='sum', **swapped)
    torch.cuda.synchronize()
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    results = [[], []]
    for _ in range(3):
        with torch.cuda.stream(streams[0]):
            results[0].append(dtw.distance(xd, yd, reduction='sum', **keywords))
        with torch.cuda.stream(streams[1]):
            results[1].append(dtw.distance(yd, xd, reduction='sum', **swapped))
    torch.cuda.synchronize()
    assert all(torch.equal(r, total) for r in results[0])
    assert all(torch.equal(r, expected_swapped) for r in results[1])


def test_relations_to_the_aligned_distance(golden):
    x, y, sim, exponent, _ = fixture(golden)
    xd, yd = x.cuda(), y.cuda()
    for normalize in (True, False):
        keywords = dict(normalize=normalize, similarity=sim, exponent=exponent)
        aligned = float(ppgs_amd.distance(xd, yd, reduction='sum', **keywords))
        warped = float(dtw.distance(xd, yd, reduction='sum', **keywords))
        assert warped <= aligned + RTOL * aligned + 57 * ATOL          # the diagonal is one of the paths
        assert warped > 0
    # fp16 inputs are promoted as distance_frames promotes them
    half = dtw.distance(xd.half(), yd.half(), reduction='sum', similarity=sim, exponent=exponent)
    assert half.dtype == torch.float32
    assert torch.equal(half, dtw.distance(xd.half().float(), yd.half().float(), reduction='sum', similarity=sim,
                                          exponent=exponent))
    # CPU tensors are moved to the device, as in the other post-ops
    assert torch.equal(dtw.distance(x, y, reduction='sum', similarity=sim, exponent=exponent).cpu(),
                       dtw.distance(xd, yd, reduction='sum', similarity=sim, exponent=exponent).cpu())
    # ppgs_amd.distance still wants aligned PPGs
    with pytest.raises(ValueError):
        ppgs_amd.distance(xd, yd[:, :50], normalize=False)
