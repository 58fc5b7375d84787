"""ppg_dtw on the GPU, bit for bit: tests/dtw_probe.py's inputs against its fp32 programme over the DEVICE's own cell
costs, the cell cost itself against the float64 criterion ppgs_amd.distance is held to, and the raw C entry point with
poisoned workspaces, sentinels in every output, refusals, impossible lengths and grouped calls.

The cell costs of an alphabet of S frames are measured once, as S x S problems of 1 x 1 frames; the table of a probe is
C[i, j] = cell[sx[i], sy[j]].  The device's total (bits), K and path must equal programme32(C): the inputs are full of
exact ties, so nothing but the documented tie rule, a correct hand-over between the 256-row blocks, the 4-row strips
and the packed direction bytes gives that (tests/test_dtw_probe_host.py: which mutant each probe catches).  That a
cell's bits depend on its two frames and not on its place is checked as it goes: the 'none' costs along the path must
equal the table look-ups bit for bit.  If a probe fails and that check holds, the fault is in dtw_programme or
dtw_traceback; if that check fails, it is in dtw_cost.

The cell cost's own kappa per family (the smallest at which every cell passes): see DESIGN 4.9; every case prints it
beside its bound and records it as a test property."""
import numpy as np
import pytest
import torch

import dtw_probe as D
import postops_probe as P
from ppgs_amd import core, dtw, engine as E

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def sim(golden):
    g = golden('g9_postops')
    return torch.from_numpy(g['similarity']), float(g['exponent'])


def bits(x):
    if torch.is_tensor(x):
        x = x.detach().cpu().contiguous().numpy()
    return np.asarray(x, dtype=np.float32).view(np.int32)


def keywords(sim, normalize):
    return dict(normalize=normalize, similarity=sim[0], exponent=sim[1])


@pytest.fixture(scope='module')
def cells(sim):
    """kind -> the (S, S) fp32 table of the device's cell costs, [frame of X, frame of Y].  Never modified."""
    out = {}
    for kind, (_, symbols, normalize, _) in D.KINDS.items():
        x, y = D.all_pairs(D.frames_of(kind))
        got = dtw.distance(x.cuda(), y.cuda(), reduction='sum', **keywords(sim, normalize))
        assert got.shape == (symbols * symbols,) and got.dtype == torch.float32
        out[kind] = got.cpu().numpy().reshape(symbols, symbols)
        out[kind].setflags(write=False)
    return out


def test_cells_of_the_alphabets(cells):
    for kind, table in cells.items():
        assert np.isfinite(table).all() and (table >= 0).all()
        assert (bits(np.diag(table)) == 0).all(), kind                      # equal frames cost exactly +0
    # the precondition of the equal-cost probes: one value c off the diagonal, hence symmetric, bit for bit
    table = cells['equal_cost']
    c = table[0, 1]
    print(f'equal-cost alphabet: c = {c!r}')
    assert c > 0 and bits(table[0, 1]) == bits(table[1, 0])
    assert (bits(table[~np.eye(3, dtype=bool)]) == bits(c)).all()
    # sixteen distinct frames: no two cost 0 without the mix (with it, only finite and >= 0 is promised)
    assert (cells['alphabet_plain'][~np.eye(16, dtype=bool)] > 0).all()


def run_probe(x, y, table, kw, name):
    """One pair on the device against programme32(table): align, 'sum', 'mean' and 'none'."""
    expected = D.programme32(table)
    path, total, count = dtw.align(x, y, **kw)
    got = (total.cpu().numpy(), count, path.cpu().numpy())
    if not D.same(got, expected):
        along = dtw.distance(x, y, reduction='none', **kw).cpu().numpy()
        cells_hold = along.shape == (len(got[2]),) and (bits(along) == bits(table[got[2][:, 0], got[2][:, 1]])).all()
        same_path = np.array_equal(got[2], expected[2])
        first = -1 if same_path else int(np.argmax([tuple(a) != tuple(b) for a, b in zip(got[2], expected[2])] + [True]))
        pytest.fail(f'{name}: total {got[0]!r} K {got[1]} for {expected[0]!r} K {expected[1]}; path '
                    f"{'equal' if same_path else f'differs from cell {first}'}; the cells along the device's path "
                    f"{'equal' if cells_hold else 'DIFFER from'} the table")
    assert path.dtype == torch.int32 and path.shape == (expected[1], 2)
    summed = dtw.distance(x, y, reduction='sum', **kw)
    assert bits(summed) == bits(expected[0]), name
    mean = dtw.distance(x, y, **kw)
    assert bits(mean) == bits(np.float32(expected[0]) / np.float32(expected[1])), name
    along = dtw.distance(x, y, reduction='none', **kw)
    assert along.shape == (expected[1],), name
    assert (bits(along) == bits(table[expected[2][:, 0], expected[2][:, 1]])).all(), name
    return total, count, path


def ragged(items, device='cuda'):
    """[(40, T)] -> ((B, 40, longest) padded with NaN, lengths)."""
    lengths = [item.shape[1] for item in items]
    out = torch.full((len(items), D.NP, max(lengths)), float('nan'))
    for b, item in enumerate(items):
        out[b, :, :lengths[b]] = item
    return out.to(device), lengths


@pytest.mark.parametrize('kind', list(D.KINDS))
def test_probes_equal_the_fp32_programme(sim, cells, kind):
    kw = keywords(sim, D.KINDS[kind][2])
    frames = D.frames_of(kind)
    singles = {}
    for frames_x, frames_y in D.SHAPES:
        sx, sy = D.probe(kind, frames_x, frames_y)
        x, y = D.ppg_of(sx, frames).cuda(), D.ppg_of(sy, frames).cuda()
        name = D.probe_name(kind, frames_x, frames_y)
        singles[frames_x, frames_y] = (x, y) + run_probe(x, y, D.cost_table(cells[kind], sx, sy), kw, name)
        run_probe(y, x, D.cost_table(cells[kind], sy, sx), kw, name + ' transposed')
    # the same probes as ragged batches, NaN beyond every item's length: the long ones apart, to keep the padding small
    long = [shape for shape in D.SHAPES if max(shape) > 769]
    for shapes in ([shape for shape in D.SHAPES if shape not in long], long + [(1, 1), (5, 3)]):
        x, lengths_x = ragged([singles[shape][0].cpu() for shape in shapes])
        y, lengths_y = ragged([singles[shape][1].cpu() for shape in shapes])
        paths, total, counts = dtw.align(x, y, lengths_x=lengths_x, lengths_y=lengths_y, **kw)
        summed = dtw.distance(x, y, reduction='sum', lengths_x=lengths_x, lengths_y=lengths_y, **kw)
        mean = dtw.distance(x, y, lengths_x=lengths_x, lengths_y=lengths_y, **kw)
        assert torch.equal(summed.view(torch.int32), total.view(torch.int32))
        assert torch.equal(mean, total / torch.tensor(counts, device='cuda', dtype=torch.float32))
        for b, shape in enumerate(shapes):
            _, _, one_total, one_count, one_path = singles[shape]
            assert bits(total[b]) == bits(one_total) and counts[b] == one_count, (kind, shape)
            assert torch.equal(paths[b], one_path), (kind, shape)


@pytest.mark.parametrize('normalize', [True, False])
def test_constant_tables_follow_the_closed_form(sim, cells, normalize):
    kind = 'alphabet_mix' if normalize else 'alphabet_plain'
    kw = keywords(sim, normalize)
    frames = D.frames_of(kind)
    for at, (frames_x, frames_y) in enumerate(D.CONSTANT_SHAPES):
        s, t = (3 * at) % 16, (5 * at + 7) % 16
        assert s != t
        x = D.ppg_of(np.full(frames_x, s), frames).cuda()
        y = D.ppg_of(np.full(frames_y, t), frames).cuda()
        expected = D.constant_closed_form(frames_x, frames_y, cells[kind][s, t])
        path, total, count = dtw.align(x, y, **kw)
        assert D.same((total.cpu().numpy(), count, path.cpu().numpy()), expected), (frames_x, frames_y, s, t)
        along = dtw.distance(x, y, reduction='none', **kw)
        assert (bits(along) == bits(cells[kind][s, t])).all() and along.shape == (max(frames_x, frames_y),)


# ---- the cell cost against float64 -----------------------------------------------------------------------------------------

@pytest.mark.parametrize('family', P.FAMILIES)
def test_cell_cost_probe(sim, family, record_property):
    """dtw_prepare / dtw_cost restate distance_kernel's chain (log a prepared once, a (log a - log m)): the same
    criterion, the same bound, 4 max(KAPPA_REF, 1), as tests/test_gpu_postops_probe.py::test_distance_probe."""
    x, y = P.pair(family)
    for normalize in (True, False):
        mix = P.mix_matrix(*sim) if normalize else None
        bound = P.kappa_gpu(family, normalize)
        kw = keywords(sim, normalize)
        # 197 frame pairs as 1 x 1 problems: cell (0, 0) of 197 pairs
        out = dtw.distance(x.T[:, :, None].contiguous().cuda(), y.T[:, :, None].contiguous().cuda(), reduction='sum', **kw)
        assert out.shape == (P.FULL,) and out.dtype == torch.float32
        # one 65 x 197 pair: the cells along its path, away from (0, 0)
        xs, ys = x[:, :65].contiguous(), y
        path, _, count = dtw.align(xs.cuda(), ys.cuda(), **kw)
        along = dtw.distance(xs.cuda(), ys.cuda(), reduction='none', **kw)
        path = path.cpu().long()
        assert along.shape == (count,) and count >= P.FULL
        for where, got, a, b in (('1x1', out, x, y), ('path', along, xs[:, path[:, 0]], ys[:, path[:, 1]])):
            got = got.cpu().numpy()
            needed = P.distance_kappa(got, a, b, mix)
            print(f'dtw cell {family} mix={normalize} {where}: the kernel needs kappa {needed:.3f} (bound {bound}, oracle '
                  f'{P.KAPPA_REF[family, normalize]})')
            record_property(f"kappa_{'mix' if normalize else 'plain'}_{where}", round(needed, 3))
            bad = P.distance_violations(got, a, b, mix, bound)
            if bad.any():
                t = int(np.argmax(bad))
                ref, avg, unit = P.distance64(a, b, mix)
                pytest.fail(f'{family} mix={normalize} {where}: {bad.sum()} cells outside kappa {bound} (the kernel needs '
                            f'{needed:.2f}); the first is cell {t}: {got[t]!r} for {ref[t]:.9g}, allowance '
                            f'{P.distance_bound(avg, unit, bound)[t]:.3g}')


# ---- the raw entry point ---------------------------------------------------------------------------------------------------

SENTINEL = -7
RAW_SHAPES = ((1, 1), (1, 300), (300, 1), (257, 65), (5, 3))


def raw_dtw(x, y, lengths_x, lengths_y, workspace, mix=None, want_path=True, want_length=True, want_cost=True,
            frames_x=None, frames_y=None, pairs=None, size=None, offset=0):
    """ppg_dtw through ctypes with the caller's workspace; every output starts as a sentinel:
    (rc, (total, steps, path, path_length, path_cost))."""
    lib = E.library()
    count, longest = x.shape[0], x.shape[2] + y.shape[2] - 1
    both = torch.tensor([lengths_x, lengths_y], dtype=torch.int32).cuda()
    total = torch.full((count,), float(SENTINEL), device='cuda')
    steps = torch.full((count,), SENTINEL, dtype=torch.int32, device='cuda')
    path = torch.full((count, longest, 2), SENTINEL, dtype=torch.int32, device='cuda')
    path_length = torch.full((count,), SENTINEL, dtype=torch.int32, device='cuda')
    path_cost = torch.full((count, longest), float(SENTINEL), device='cuda')
    torch.cuda.synchronize()
    rc = lib.ppg_dtw(
        0, x.data_ptr(), x.shape[2] if frames_x is None else frames_x, y.data_ptr(),
        y.shape[2] if frames_y is None else frames_y, count if pairs is None else pairs, both[0].data_ptr(),
        both[1].data_ptr(), mix.data_ptr() if mix is not None else None, total.data_ptr(), steps.data_ptr(),
        path.data_ptr() if want_path else None, path_length.data_ptr() if want_length else None,
        path_cost.data_ptr() if want_cost else None, workspace.data_ptr() + offset,
        workspace.numel() - offset if size is None else size, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return rc, (total, steps, path, path_length, path_cost)


def identical(a, b):
    return all(torch.equal(p.view(torch.int32), q.view(torch.int32)) for p, q in zip(a, b))


@pytest.fixture(scope='module')
def raw_problem(sim, cells):
    """The ragged batch of the raw tests, (5, 40, 300) x (5, 40, 300) with NaN padding (most of its tiles hold no cell and
    are skipped by dtw_cost), and what programme32 makes of each item."""
    frames = D.frames_of('alphabet_mix')
    items_x, items_y, expected = [], [], []
    for frames_x, frames_y in RAW_SHAPES:
        sx, sy = D.sequences(frames_x, frames_y, 16, 11, 0)
        items_x.append(D.ppg_of(sx, frames))
        items_y.append(D.ppg_of(sy, frames))
        table = D.cost_table(cells['alphabet_mix'], sx, sy)
        expected.append(D.programme32(table) + (table,))
    x, lengths_x = ragged(items_x)
    y, lengths_y = ragged(items_y)
    assert x.shape == y.shape == (5, 40, 300)
    mix = core._similarity_mix(sim[0], sim[1], x.device)
    return x, y, lengths_x, lengths_y, mix, expected


def workspace_bytes(x, y, want_path=1):
    return E.library().ppg_dtw_workspace_bytes(x.shape[0], x.shape[2], y.shape[2], want_path)


def test_workspace_contents_do_not_matter(raw_problem):
    x, y, lengths_x, lengths_y, mix, expected = raw_problem
    need = workspace_bytes(x, y)
    fresh = raw_dtw(x, y, lengths_x, lengths_y, torch.zeros(need, dtype=torch.uint8, device='cuda'), mix)
    # 0xFF bytes are NaN costs and direction 3: what the programme prefetches from skipped tiles must stay unused
    poisoned = raw_dtw(x, y, lengths_x, lengths_y, torch.full((need,), 255, dtype=torch.uint8, device='cuda'), mix)
    # left behind by a larger problem
    generator = torch.Generator().manual_seed(4)
    large_x = torch.softmax(3 * torch.randn(1, 40, 4096, generator=generator), 1).cuda()
    large_y = torch.softmax(3 * torch.randn(1, 40, 700, generator=generator), 1).cuda()
    used = torch.zeros(max(workspace_bytes(large_x, large_y), need), dtype=torch.uint8, device='cuda')
    rc, (total, steps, _, _, _) = raw_dtw(large_x, large_y, [4096], [700], used, mix)
    assert rc == 0 and bool(torch.isfinite(total).all()) and 4096 <= int(steps[0]) <= 4795
    reused = raw_dtw(x, y, lengths_x, lengths_y, used, mix)
    # with and without a path in one workspace: the layouts differ
    shared = torch.zeros(need, dtype=torch.uint8, device='cuda')
    without = raw_dtw(x, y, lengths_x, lengths_y, shared, mix, want_path=False, want_length=False, want_cost=False)
    with_path = raw_dtw(x, y, lengths_x, lengths_y, shared, mix)
    again = raw_dtw(x, y, lengths_x, lengths_y, shared, mix, want_path=False, want_length=False, want_cost=False)
    assert fresh[0] == poisoned[0] == reused[0] == without[0] == with_path[0] == again[0] == 0
    for other in (poisoned, reused, with_path):
        assert identical(fresh[1], other[1])
    for other in (without, again):
        assert identical(fresh[1][:2], other[1][:2])
        assert all(bool((out == SENTINEL).all()) for out in other[1][2:])
    # and they are right: the fp32 programme over the device's cells; rows K and beyond keep the sentinel
    total, steps, path, path_length, path_cost = (out.cpu().numpy() for out in fresh[1])
    for b, (ref_total, ref_count, ref_path, table) in enumerate(expected):
        assert bits(total[b]) == bits(ref_total) and steps[b] == path_length[b] == ref_count, RAW_SHAPES[b]
        assert np.array_equal(path[b, :ref_count], ref_path), RAW_SHAPES[b]
        assert (bits(path_cost[b, :ref_count]) == bits(table[ref_path[:, 0], ref_path[:, 1]])).all(), RAW_SHAPES[b]
        assert (path[b, ref_count:] == SENTINEL).all() and (path_cost[b, ref_count:] == SENTINEL).all()
    # path_cost is optional
    no_cost = raw_dtw(x, y, lengths_x, lengths_y, shared, mix, want_cost=False)
    assert no_cost[0] == 0 and identical(fresh[1][:4], no_cost[1][:4]) and bool((no_cost[1][4] == SENTINEL).all())


def test_refusals_touch_nothing(raw_problem):
    x, y, lengths_x, lengths_y, mix, _ = raw_problem
    lib = E.library()
    need = workspace_bytes(x, y)
    workspace = torch.full((need + 16,), 0xA5, dtype=torch.uint8, device='cuda')
    huge = 1 << 40
    refusals = {
        'workspace one byte short': (dict(size=need - 1), b'workspace'),
        'workspace offset by 8 bytes': (dict(offset=8), b'aligned'),
        'frames_x above the limit': (dict(frames_x=E.DTW_MAX_FRAMES + 1, size=huge), b'at most'),
        'frames_y above the limit': (dict(frames_y=E.DTW_MAX_FRAMES + 1, size=huge), b'at most'),
        'pairs above the limit': (dict(pairs=E.DTW_MAX_PAIRS + 1, size=huge), b'at most'),
        'path_length without path': (dict(want_path=False, want_cost=False), b'need path'),
        'path_cost without path': (dict(want_path=False, want_length=False), b'need path'),
        'path without path_length': (dict(want_length=False), b'path_length'),
        'no pairs': (dict(pairs=0), b'dtw'),
    }
    for name, (arguments, message) in refusals.items():
        assert raw_dtw(x, y, lengths_x, lengths_y, workspace, mix)[0] == 0           # a good call: the error is stale
        workspace.fill_(0xA5)
        rc, outputs = raw_dtw(x, y, lengths_x, lengths_y, workspace, mix, **arguments)
        assert rc == -1 and message in lib.ppg_last_error(), (name, lib.ppg_last_error())
        assert all(bool((out == SENTINEL).all()) for out in outputs), name
        assert bool((workspace == 0xA5).all()), name


def test_impossible_lengths_on_the_device(raw_problem):
    x, y, lengths_x, lengths_y, mix, _ = raw_problem
    x = torch.nan_to_num(x, nan=0.025)                      # item 2 (300 x 1) is read to the full 300 frames below
    y = torch.nan_to_num(y, nan=0.025)
    workspace = torch.full((workspace_bytes(x, y),), 255, dtype=torch.uint8, device='cuda')
    clean = raw_dtw(x, y, lengths_x, lengths_y, workspace, mix)
    assert clean[0] == 0
    # no frames at all: total NaN, K 0, path and path_cost left alone; the neighbours as in the clean run
    for bad_x, bad_y in ((0, None), (None, 0), (-3, None), (None, -1), (0, 0), (-2 ** 31, 5)):
        lx, ly = list(lengths_x), list(lengths_y)
        lx[3] = lx[3] if bad_x is None else bad_x
        ly[3] = ly[3] if bad_y is None else bad_y
        rc, (total, steps, path, path_length, path_cost) = raw_dtw(x, y, lx, ly, workspace, mix)
        assert rc == 0, (bad_x, bad_y)
        assert bool(torch.isnan(total[3])) and int(steps[3]) == 0 and int(path_length[3]) == 0, (bad_x, bad_y)
        assert bool((path[3] == SENTINEL).all()) and bool((path_cost[3] == SENTINEL).all()), (bad_x, bad_y)
        keep = [0, 1, 2, 4]
        assert identical([out[keep] for out in clean[1]], [out[keep] for out in (total, steps, path, path_length, path_cost)])
    # more frames than there are: the result of `frames` frames, here 300 x 300 for 257 x 65 and 300 x 1
    full = list(lengths_x)
    full[3], full[2] = 300, 300
    full_y = list(lengths_y)
    full_y[3] = 300
    expected = raw_dtw(x, y, full, full_y, workspace, mix)
    for over_x, over_y in ((301, 300), (300, 4097), (2 ** 31 - 1, 2 ** 31 - 1)):
        lx, ly = list(full), list(full_y)
        lx[3], ly[3], lx[2] = over_x, over_y, over_x
        got = raw_dtw(x, y, lx, ly, workspace, mix)
        assert got[0] == expected[0] == 0 and identical(expected[1], got[1]), (over_x, over_y)
    keep = [0, 1, 4]
    assert identical([out[keep] for out in clean[1]], [out[keep] for out in expected[1]])
    assert int(expected[1][1][3]) >= 300 and bool(torch.isfinite(expected[1][0]).all())


# ---- grouped calls ---------------------------------------------------------------------------------------------------------

class CountingLibrary:
    """The library, with the pairs of every ppg_dtw call written down."""

    def __init__(self, library):
        self.library, self.calls = library, []

    def __getattr__(self, name):
        function = getattr(self.library, name)
        if name != 'ppg_dtw':
            return function

        def counted(*arguments):
            self.calls.append(arguments[5])
            return function(*arguments)
        return counted


def test_grouped_calls_equal_one_call(sim, monkeypatch):
    kw = keywords(sim, True)
    frames = D.frames_of('alphabet_mix')
    shapes = ((257, 65), (1, 1), (30, 300), (300, 30), (5, 3), (256, 64), (64, 257))
    pairs = [D.sequences(frames_x, frames_y, 16, 13, 1) for frames_x, frames_y in shapes]
    x, lengths_x = ragged([D.ppg_of(sx, frames) for sx, _ in pairs])
    y, lengths_y = ragged([D.ppg_of(sy, frames) for _, sy in pairs])
    kw.update(lengths_x=lengths_x, lengths_y=lengths_y)
    paths, total, counts = dtw.align(x, y, **kw)
    assert torch.equal(dtw.distance(x, y, reduction='sum', **kw).view(torch.int32), total.view(torch.int32))
    spy = CountingLibrary(E.library())
    monkeypatch.setattr(E, 'library', lambda: spy)
    for group, calls in ((3, [3, 3, 1]), (1, [1] * 7), (7, [7]), (6, [6, 1])):
        for want_path in (1, 0):
            per_pair = spy.ppg_dtw_workspace_bytes(1, x.shape[2], y.shape[2], want_path)
            monkeypatch.setattr(E, 'DTW_WORKSPACE_BYTES', group * per_pair + per_pair // 2)
            spy.calls.clear()
            if want_path:
                got_paths, got_total, got_counts = dtw.align(x, y, **kw)
                assert got_counts == counts and all(torch.equal(p, q) for p, q in zip(paths, got_paths)), group
            else:
                got_total = dtw.distance(x, y, reduction='sum', **kw)
            assert spy.calls == calls, (group, want_path)
            assert torch.equal(got_total.view(torch.int32), total.view(torch.int32)), (group, want_path)
