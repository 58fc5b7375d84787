"""ppgs_amd.alignment.PosteriorStream on the GPU (ppg_posterior_stream_*).

The definition is bitwise: with open(g) = g with final = 0, block k of a stream with block H and lag L is columns
[kH, (k+1)H) of alignment.posterior(ppg[:, :(k+1)H + L], open(g)), a push's evidence is that call's total over the frames
received so far, and the flush is alignment.posterior of the whole recording under g.  The prefixes of a case run as ONE
batched alignment.posterior (a batch equals its singles bit for bit, tests/test_gpu_posterior.py) and are shared by the
tests of that case.  Against the float64 reference (tests/posterior_stream_reference.py) the tolerance is
tests/test_gpu_posterior.py's B, taken at the length of the prefix that a block was smoothed over: |gamma - gamma64| <=
3 B(h + 1) gamma64 + 1e-6, the same for post plus S * 2**-24, |evidence - ref| <= B(p), |total - ref| <= B(T).
tests/test_posterior_stream_host.py shows that this tolerance cannot hide a horizon that is off by one frame at
(H, L) = (1, 2) and (4, 3); at (16, 16) only the bitwise tests guard the horizon."""
import ctypes
import functools
import math

import numpy as np
import pytest
import torch

from ppgs_amd import alignment, engine as E

import posterior_cases as C
import posterior_reference as R
import posterior_stream_reference as L

pytestmark = pytest.mark.gpu

HL = ((1, 0), (1, 2), (4, 3), (16, 16))


def bits(tensor):
    return tensor.contiguous().view(torch.int64 if tensor.dtype == torch.float64 else torch.int32)


def opened(graph):
    return graph._replace(final=torch.zeros_like(graph.final))


class Prefixes:
    """alignment.posterior of the prefixes ppg[:, :n], n in `lengths`, under the open graph, as one batch; and of the
    whole recording under the graph itself."""

    def __init__(self, ppg, graph, lengths=None):
        frames = ppg.shape[1]
        self.lengths = list(range(1, frames + 1)) if lengths is None else sorted(set(lengths))
        self.row = {n: i for i, n in enumerate(self.lengths)}
        longest = max(self.lengths)
        batch = ppg[None, :, :longest].repeat(len(self.lengths), 1, 1).cuda()
        got = alignment.posterior(batch, [opened(graph)] * len(self.lengths), self.lengths, states=True)
        self.total, self.phonemes, self.states = got.total.cpu(), got.phonemes.cpu(), got.states.cpu()
        whole = alignment.posterior(ppg.cuda(), graph, states=True)
        self.whole = (whole.total.cpu(), whole.phonemes.cpu(), whole.states.cpu())

    def block(self, k, block, lag):
        i = self.row[(k + 1) * block + lag]
        return self.phonemes[i][:, k * block:(k + 1) * block], self.states[i][k * block:(k + 1) * block]


@functools.lru_cache(maxsize=None)
def case(count, frames, seed):
    graph, ppg = C.random_graph(seed, count), C.random_ppg(seed, frames)
    return graph, ppg, Prefixes(ppg, graph)


@functools.lru_cache(maxsize=None)
def case64(count, frames, seed):
    graph, ppg, _ = case(count, frames, seed)
    g = R.lists(graph)
    return g, R.emissions(R.prepared(ppg.numpy()), g.sym)


def feed(stream, ppg, pushes):
    """The PosteriorFrames of pushes of these many frames and of the flush, on the CPU."""
    out, at = [], 0
    for frames in pushes:
        out.append(stream.push(ppg[:, at:at + frames].cuda()))
        at += frames
    out.append(stream.flush())
    return [alignment.PosteriorFrames(*[None if value is None else value.cpu() for value in piece]) for piece in out]


def steps(frames, size):
    return [min(size, frames - at) for at in range(0, frames, size)]


def assert_definition(pieces, pushes, prefixes, block, lag, frames, label):
    """Every push and the flush against the bitwise definition."""
    position = 0
    for index, (piece, pushed) in enumerate(zip(pieces[:-1], pushes)):
        before = L.emitted(position, block, lag)
        position += pushed
        after = L.emitted(position, block, lag)
        where = f'{label} push {index}'
        assert int(piece.begin) == before and int(piece.count) == after - before, where
        assert torch.equal(bits(piece.evidence), bits(prefixes.total[prefixes.row[position]])), where
        for k in range(before // block, after // block):
            phonemes, states = prefixes.block(k, block, lag)
            j = k * block - before
            assert torch.equal(bits(piece.phonemes[:, j:j + block]), bits(phonemes)), (where, k)
            assert torch.equal(bits(piece.states[j:j + block]), bits(states)), (where, k)
        assert bool((piece.phonemes[:, after - before:] == 0).all()) and bool((piece.states[after - before:] == 0).all())
    last, c = pieces[-1], L.emitted(position, block, lag)
    total, phonemes, states = prefixes.whole
    assert position == frames and int(last.begin) == c and int(last.count) == frames - c, label
    assert last.evidence is None and torch.equal(bits(last.total), bits(total)), label
    assert torch.equal(bits(last.phonemes[:, :frames - c]), bits(phonemes[:, c:])), label
    assert torch.equal(bits(last.states[:frames - c]), bits(states[c:])), label


# ---- 1. the definition, bit for bit ----

@pytest.mark.parametrize('block,lag', HL)
@pytest.mark.parametrize('count,frames,seed', C.RANDOM_CASES)
def test_every_block_is_posterior_of_its_prefix_under_the_open_graph(count, frames, seed, block, lag):
    graph, ppg, prefixes = case(count, frames, seed)
    stream = alignment.PosteriorStream(graph, block=block, lag=lag, window=256, states=True)
    pushes = steps(frames, 6)
    pieces = feed(stream, ppg, pushes)
    assert_definition(pieces, pushes, prefixes, block, lag, frames, f'{count} x {frames} ({block}, {lag})')
    assert stream.position == [0] and stream.emitted == [0]


# ---- 2. against float64 ----

@pytest.mark.parametrize('block,lag', HL)
@pytest.mark.parametrize('count,frames,seed', C.RANDOM_CASES)
def test_blocks_evidence_and_total_against_the_float64_reference(count, frames, seed, block, lag):
    graph, ppg, _ = case(count, frames, seed)
    g, e = case64(count, frames, seed)
    stream = alignment.PosteriorStream(graph, block=block, lag=lag, window=256, states=True)
    pushes = steps(frames, 6)
    pieces = feed(stream, ppg, pushes)
    expected = L.stream(e, g, pushes, block, lag)
    position, worst = 0, [0., 0., 0.]
    for piece, want, pushed in zip(pieces, expected, pushes + [0]):
        position += pushed
        assert int(piece.begin) == want['begin'] and int(piece.count) == want['count']
        flush = piece.evidence is None
        b = C.bound(graph, position)
        number = float(piece.total if flush else piece.evidence)
        worst[0] = max(worst[0], abs(number - want['total' if flush else 'evidence']) / b)
        assert abs(number - want['total' if flush else 'evidence']) <= b
        for j in range(want['count']):
            t = want['begin'] + j
            b = C.bound(graph, frames if flush else L.horizon(t // block, block, lag) + 1)
            gamma, post = want['gamma'][j], want['post'][:, j]
            ours, mine = piece.states[j, :count].double().numpy(), piece.phonemes[:, j].double().numpy()
            worst[1] = max(worst[1], np.abs(ours - gamma).max())
            worst[2] = max(worst[2], np.abs(mine - post).max())
            assert bool((np.abs(ours - gamma) <= 3. * b * gamma + 1e-6).all()), t
            assert bool((np.abs(mine - post) <= 3. * b * post + 1e-6 + count * 2. ** -24).all()), t
            assert abs(ours.sum() - 1.) <= 64 * 2. ** -23 + count * 2. ** -24, t
    print(f'{count} x {frames} ({block}, {lag}): evidence / B {worst[0]:.3e}, gamma {worst[1]:.3e}, post {worst[2]:.3e}')


# ---- 3. cadence ----

@pytest.mark.parametrize('block,lag', ((4, 3), (16, 16)))
def test_the_output_does_not_depend_on_the_pushes(block, lag):
    count, frames, seed = C.RANDOM_CASES[2]
    graph, ppg, _ = case(count, frames, seed)
    ragged = [1, 0, 5, 31, 2, 64, 0, 7, 19]
    assert sum(ragged) == frames
    joined = []
    for pushes in (steps(frames, 1), steps(frames, 16), steps(frames, 37), [frames], ragged):
        stream = alignment.PosteriorStream(graph, block=block, lag=lag, window=256, states=True)
        pieces = feed(stream, ppg, pushes)
        counts = [int(piece.count) for piece in pieces]
        assert sum(counts) == frames
        assert [int(piece.begin) for piece in pieces] == [sum(counts[:i]) for i in range(len(counts))]
        joined.append((alignment.joined_frames(pieces),
                       torch.cat([piece.states[:n] for piece, n in zip(pieces, counts)]), pieces[-1].total))
        assert joined[-1][0].shape == (40, frames)
    for phonemes, states, total in joined[1:]:
        assert torch.equal(bits(phonemes), bits(joined[0][0]))
        assert torch.equal(bits(states), bits(joined[0][1]))
        assert torch.equal(bits(total), bits(joined[0][2]))


# ---- 4. the ring wraps; a long push goes in pieces ----

def test_a_wrapping_ring_and_a_push_in_pieces_keep_the_definition():
    count, _, seed = C.RANDOM_CASES[2]
    frames, block, lag = 300, 16, 16
    graph, ppg = C.random_graph(seed, count), C.random_ppg(400, frames)
    horizons = [(k + 1) * block + lag for k in range(frames // block) if (k + 1) * block + lag <= frames]
    prefixes = Prefixes(ppg, graph, horizons + steps_ends(frames, 5) + [frames])
    stream = alignment.PosteriorStream(graph, block=block, lag=lag, window=64, states=True)
    pushes = steps(frames, 5)
    assert_definition(feed(stream, ppg, pushes), pushes, prefixes, block, lag, frames, 'pushes of 5')
    assert_definition(feed(stream, ppg, [frames]), [frames], prefixes, block, lag, frames, 'pieces of 33')


def steps_ends(frames, size):
    return [min(at + size, frames) for at in range(0, frames, size)]


# ---- 5. arcs from memory ----

def test_arcs_from_memory_keep_the_definition():
    heavy = C.random_graph(41, 700, big=False, most=20)
    assert int(heavy.offsets[-1]) == 6993
    frames, block, lag = 40, 8, 8
    ppg = C.random_ppg(41, frames)
    prefixes = Prefixes(ppg, heavy)
    stream = alignment.PosteriorStream(heavy, block=block, lag=lag, window=64, states=True)
    pushes = steps(frames, 7)
    assert_definition(feed(stream, ppg, pushes), pushes, prefixes, block, lag, frames, 'heavy 700')


# ---- 6. a batch equals its streams alone ----

BATCH = 33


def batch_inputs():
    rng = np.random.default_rng(6)
    counts = [3, 64, 65, 300] + [int(n) for n in rng.integers(3, 301, BATCH - 4)]
    graphs = [C.random_graph(600 + b, n, big=False) for b, n in enumerate(counts)]
    lengths = [[int(n) for n in rng.integers(0, 14, BATCH)] for _ in range(6)]
    lengths[2] = [0 if b % 2 else n for b, n in enumerate(lengths[2])]
    lengths[0][0] = 13
    ppgs = [C.random_ppg(660 + b, 6 * 13) for b in range(BATCH)]
    return graphs, lengths, ppgs


def padded(ppgs, position, lengths):
    most = max(max(lengths), 1)
    x = torch.full((len(ppgs), 40, most), float('nan'))
    for b, (ppg, at, n) in enumerate(zip(ppgs, position, lengths)):
        x[b, :, :n] = ppg[:, at:at + n]
    return x.cuda()


def test_a_batch_of_ragged_streams_equals_every_stream_alone():
    graphs, lengths, ppgs = batch_inputs()
    block, lag = 4, 3
    batch = alignment.PosteriorStream(graphs, block=block, lag=lag, window=64, batch=BATCH, states=True)
    position, outputs = [0] * BATCH, []
    for step in lengths:
        outputs.append(batch.push(padded(ppgs, position, step), step))
        position = [at + n for at, n in zip(position, step)]
    assert batch.position == position
    assert batch.emitted == [L.emitted(at, block, lag) for at in position]
    outputs.append(batch.flush())
    for b in range(BATCH):
        alone = alignment.PosteriorStream(graphs[b], block=block, lag=lag, window=64, states=True)
        at, count = 0, graphs[b].phonemes.shape[0]
        for step, got in zip(lengths + [None], outputs):
            if step is None:
                one = alone.flush()
                assert torch.equal(bits(got.total[b]), bits(one.total)), b
            elif step[b] == 0:
                assert int(got.count[b]) == 0 and int(got.begin[b]) == L.emitted(at, block, lag), b
                continue
            else:
                one = alone.push(ppgs[b][:, at:at + step[b]].cuda())
                at += step[b]
                assert torch.equal(bits(got.evidence[b]), bits(one.evidence)), b
            n = int(one.count)
            assert int(got.count[b]) == n and int(got.begin[b]) == int(one.begin), b
            assert torch.equal(bits(got.phonemes[b, :, :n]), bits(one.phonemes[:, :n])), b
            assert torch.equal(bits(got.states[b, :n, :count]), bits(one.states[:n])), b
            assert bool((got.phonemes[b, :, n:] == 0).all()) and bool((got.states[b, n:] == 0).all()), b
            assert bool((got.states[b, :, count:] == 0).all()), b


def test_flush_and_reset_of_one_stream_leave_the_neighbours_alone():
    graphs = [C.random_graph(700 + b, n, big=False) for b, n in enumerate((5, 70, 33))]
    ppgs = [C.random_ppg(710 + b, 40) for b in range(3)]
    block, lag = 4, 3
    for action in ('flush', 'reset'):
        batch = alignment.PosteriorStream(graphs, block=block, lag=lag, window=64, batch=3, states=True)
        alone = [alignment.PosteriorStream(graphs[b], block=block, lag=lag, window=64, states=True) for b in range(3)]
        first = batch.push(torch.stack([ppg[:, :17] for ppg in ppgs]).cuda())
        for b in range(3):
            alone[b].push(ppgs[b][:, :17].cuda())
        if action == 'flush':
            got, one = batch.flush(1), alone[1].flush()
            assert got.count.tolist() == [0, int(one.count), 0] and int(got.begin[1]) == int(one.begin)
            assert torch.equal(bits(got.total[1]), bits(one.total)) and bool(torch.isnan(got.total[[0, 2]]).all())
            assert torch.equal(bits(got.phonemes[1]), bits(one.phonemes))
        else:
            batch.reset(1)
            alone[1].reset()
        assert batch.position == [17, 0, 17] and first.count.tolist() == [12, 12, 12]
        second = batch.push(torch.stack([ppg[:, 17:40] for ppg in ppgs]).cuda(), [23, 17, 23])
        for b in range(3):
            piece = ppgs[b][:, 17:40] if b != 1 else ppgs[b][:, 17:34]
            one = alone[b].push(piece.cuda())
            n = int(one.count)
            assert int(second.count[b]) == n and int(second.begin[b]) == int(one.begin), (action, b)
            assert torch.equal(bits(second.evidence[b]), bits(one.evidence)), (action, b)
            assert torch.equal(bits(second.phonemes[b, :, :n]), bits(one.phonemes[:, :n])), (action, b)


def test_two_streams_on_two_hip_streams_equal_each_alone():
    count, frames, seed = C.RANDOM_CASES[2]
    graph, ppg, _ = case(count, frames, seed)
    heavy, other = C.random_graph(41, 700, big=False, most=20), C.random_ppg(41, frames)
    pushes = steps(frames, 16)
    expected = [feed(alignment.PosteriorStream(g, block=4, lag=3, window=256, states=True), x, pushes)
                for g, x in ((graph, ppg), (heavy, other))]
    objects = [alignment.PosteriorStream(g, block=4, lag=3, window=256, states=True) for g in (graph, heavy)]
    side = [torch.cuda.Stream(), torch.cuda.Stream()]
    inputs = [ppg.cuda(), other.cuda()]
    torch.cuda.synchronize()
    got, at = [[], []], 0
    for pushed in pushes:
        for i in range(2):
            with torch.cuda.stream(side[i]):
                got[i].append(objects[i].push(inputs[i][:, at:at + pushed]))
        at += pushed
    for i in range(2):
        with torch.cuda.stream(side[i]):
            got[i].append(objects[i].flush())
    torch.cuda.synchronize()
    for i in range(2):
        for mine, want in zip(got[i], expected[i]):
            for name in ('phonemes', 'states', 'begin', 'count'):
                assert torch.equal(bits(getattr(mine, name).cpu()), bits(getattr(want, name))), (i, name)
            number = 'total' if want.evidence is None else 'evidence'
            assert torch.equal(bits(getattr(mine, number).cpu()), bits(getattr(want, number))), i


# ---- 7. closed forms ----

@pytest.mark.parametrize('block,lag', HL)
def test_a_free_model_renormalises_the_clamped_input_whatever_the_lag(block, lag):
    frames = 45
    ppg = C.random_ppg(77, frames)
    ppg[:, 0] = 0.
    ppg[3, 0] = 1.
    graph = alignment.model_graph(torch.zeros(40, 40))
    stream = alignment.PosteriorStream(graph, block=block, lag=lag, window=64)
    pieces = feed(stream, ppg, steps(frames, 11))
    assert all(piece.states is None for piece in pieces)
    clamped = ppg.clamp(1e-8, 1. - 1e-8).double()
    expected = clamped / clamped.sum(dim=0)
    b = C.bound(graph, frames)
    error = (alignment.joined_frames(pieces).double() - expected).abs()
    assert bool((error <= 3. * b * expected + 1e-6 + 40 * 2. ** -24).all())
    assert abs(float(pieces[-1].total) - float(clamped.sum(dim=0).log().sum())) <= b
    at = 0
    for piece, pushed in zip(pieces[:-1], steps(frames, 11)):
        at += pushed
        assert abs(float(piece.evidence) - float(clamped[:, :at].sum(dim=0).log().sum())) <= C.bound(graph, at)


def test_a_chain_as_long_as_the_recording_gives_the_one_hot():
    sequence = [3, 3, 17, 0, 39, 8, 8, 8, 21, 5, 30, 12]
    ppg = C.random_ppg(78, len(sequence))
    stream = alignment.PosteriorStream(alignment.chain_graph(sequence), block=4, lag=3, window=64, states=True)
    pieces = feed(stream, ppg, steps(len(sequence), 5))
    # under the open end a prefix has more than one path, so only the flush, which reads `final`, is the one-hot
    last, c = pieces[-1], L.emitted(len(sequence), 4, 3)
    assert int(last.begin) == c and int(last.count) == len(sequence) - c
    assert torch.equal(last.states[:len(sequence) - c], torch.eye(len(sequence))[c:])
    one_hot = torch.zeros(40, len(sequence))
    one_hot[sequence, torch.arange(len(sequence))] = 1.
    assert torch.equal(last.phonemes[:, :len(sequence) - c], one_hot[:, c:])
    whole = feed(alignment.PosteriorStream(alignment.chain_graph(sequence), block=16, lag=16, window=64, states=True),
                 ppg, [len(sequence)])
    assert int(whole[0].count) == 0 and int(whole[1].count) == len(sequence)
    assert torch.equal(whole[1].states[:len(sequence)], torch.eye(len(sequence)))
    assert torch.equal(whole[1].phonemes[:, :len(sequence)], one_hot)


# ---- 8. dead and refused streams ----

def dying_graph():
    """Three states in a row that cannot be stayed in: every path has left the graph after frame 2."""
    return alignment.graph([1, 2, 3], [(0, 1, 0.), (1, 2, 0.)], stay=[-math.inf] * 3, initial=[0., -math.inf, -math.inf],
                           final=[0., 0., 0.])


def test_a_stream_whose_only_path_dies_at_frame_3():
    graph, ppg = dying_graph(), C.random_ppg(80, 8)
    stream = alignment.PosteriorStream(graph, block=1, lag=0, window=64, states=True)
    pieces = [stream.push(ppg[:, t:t + 1].cuda()) for t in range(6)]
    prefixes = Prefixes(ppg[:, :3], graph)
    for t in range(3):
        assert int(pieces[t].count) == 1 and int(pieces[t].begin) == t
        assert torch.equal(bits(pieces[t].phonemes[:, 0].cpu()), bits(prefixes.block(t, 1, 0)[0][:, 0]))
        assert torch.equal(bits(pieces[t].evidence.cpu()), bits(prefixes.total[t]))
    for t in range(3, 6):
        assert int(pieces[t].count) == 0 and float(pieces[t].evidence) == -math.inf
        assert bool((pieces[t].phonemes == 0).all())
    last = stream.flush()
    assert int(last.count) == 0 and float(last.total) == -math.inf
    again = stream.push(ppg[:, :1].cuda())                     # the flush started the stream again
    assert int(again.count) == 1 and torch.equal(bits(again.phonemes.cpu()), bits(pieces[0].phonemes.cpu()))


def test_a_flush_in_which_no_state_may_end():
    graph = alignment.graph([1, 2], [(0, 1, -1.)], stay=[-.5, -.5], initial=[0., -math.inf], final=[-math.inf, -math.inf])
    stream = alignment.PosteriorStream(graph, block=2, lag=1, window=64)
    piece = stream.push(C.random_ppg(81, 6).cuda())
    assert int(piece.count) == 4 and math.isfinite(float(piece.evidence))
    last = stream.flush()
    assert int(last.count) == 0 and float(last.total) == -math.inf and bool((last.phonemes == 0).all())
    assert stream.position == [0]


def packed_on_device(graphs):
    several = len(graphs) > 1
    stream = alignment.PosteriorStream(graphs if several else graphs[0], batch=len(graphs) if several else None)
    stream._ensure()
    return stream._graphs


def pointer(tensor):
    return None if tensor is None else ctypes.c_void_p(tensor.data_ptr())


class Raw:
    """The C entries on hand-made arrays: a state whose tail, a workspace and outputs that are poisoned."""

    POISON = -7.

    def __init__(self, packed, streams, window, block, lag, which=None):
        self.packed, self.streams, self.window = packed, streams, window
        lib = E.library()
        size = lib.ppg_posterior_stream_state_bytes(streams, window, packed.max_states)
        self.memory = torch.full((size + 256,), 0xA5, dtype=torch.uint8, device='cuda')
        self.state = self.memory[:size]
        self.which = None if which is None else torch.tensor(which, dtype=torch.int32).cuda()
        rc = lib.ppg_posterior_stream_open(0, pointer(self.state), streams, window, *E._out_graph_arguments(packed),
                                           pointer(self.which), block, lag, None)
        assert rc == 0

    def outputs(self, cap):
        most = self.packed.max_states
        return (torch.full((self.streams, 40, cap), self.POISON, device='cuda'),
                torch.full((self.streams, cap, most), self.POISON, device='cuda'),
                torch.full((self.streams,), -7, dtype=torch.int32, device='cuda'),
                torch.full((self.streams,), -7, dtype=torch.int32, device='cuda'),
                torch.full((self.streams,), self.POISON, dtype=torch.float64, device='cuda'))

    def push(self, ppg, lengths, cap):
        lib = E.library()
        frames = ppg.shape[2]
        workspace = torch.full((lib.ppg_posterior_stream_workspace_bytes(self.streams, frames),), 0xA5, dtype=torch.uint8,
                               device='cuda')
        lengths = torch.tensor(lengths, dtype=torch.int32).cuda()
        post, states, begin, count, evidence = self.outputs(cap)
        rc = lib.ppg_posterior_stream_push(
            0, pointer(self.state), self.streams, self.window, pointer(ppg), frames, pointer(lengths),
            *E._out_graph_arguments(self.packed), cap, pointer(post), pointer(states), self.packed.max_states,
            pointer(begin), pointer(count), pointer(evidence), pointer(workspace), workspace.numel(), None)
        torch.cuda.synchronize()
        assert bool((self.memory[self.state.numel():] == 0xA5).all())
        return rc, post.cpu(), states.cpu(), begin.cpu(), count.cpu(), evidence.cpu()

    def flush(self, cap):
        post, states, begin, count, total = self.outputs(cap)
        rc = E.library().ppg_posterior_stream_flush(
            0, pointer(self.state), self.streams, self.window, *E._out_graph_arguments(self.packed), None, cap,
            pointer(post), pointer(states), self.packed.max_states, pointer(begin), pointer(count), pointer(total), None)
        torch.cuda.synchronize()
        assert bool((self.memory[self.state.numel():] == 0xA5).all())
        return rc, post.cpu(), states.cpu(), begin.cpu(), count.cpu(), total.cpu()


def test_a_ragged_batch_from_poisoned_buffers_at_the_c_level():
    """The 33 ragged streams through the C entries, from a state whose bytes, a workspace and outputs that are poisoned:
    what a stream gives out is what the class gives out, and everything past it keeps its poison."""
    graphs, lengths, ppgs = batch_inputs()
    block, lag = 4, 3
    raw = Raw(packed_on_device(graphs), BATCH, 64, block, lag, which=list(range(BATCH)))
    batch = alignment.PosteriorStream(graphs, block=block, lag=lag, window=64, batch=BATCH, states=True)
    sizes = [graph.phonemes.shape[0] for graph in graphs]

    def same(got, want, number):
        rc, post, states, begin, count, float64 = got
        assert rc == 0 and torch.equal(count, want.count.cpu()) and torch.equal(begin, want.begin.cpu())
        assert torch.equal(bits(float64), bits(number.cpu()))
        for b in range(BATCH):
            n = int(count[b])
            assert torch.equal(bits(post[b, :, :n]), bits(want.phonemes[b, :, :n].cpu())), b
            assert torch.equal(bits(states[b, :n, :sizes[b]]), bits(want.states[b, :n, :sizes[b]].cpu())), b
            assert bool((post[b, :, n:] == Raw.POISON).all()) and bool((states[b, n:] == Raw.POISON).all()), b
            assert bool((states[b, :, sizes[b]:] == Raw.POISON).all()), b
    position = [0] * BATCH
    for step in lengths:
        x = padded(ppgs, position, step)
        want = batch.push(x, step)
        same(raw.push(x, step, x.shape[2] + block - 1), want, want.evidence)
        position = [at + n for at, n in zip(position, step)]
    want = batch.flush()
    same(raw.flush(block + lag - 1), want, want.total)


def test_a_block_as_long_as_the_largest_window_in_one_push_at_the_c_level():
    """block = window = 65536 and one push of 65536 frames: 65536 workgroups of which one has a block, and index * block
    passes 2^31 for half of them (ppg_posterior_stream_block is the rule; tests/test_posterior_stream_host.py)."""
    frames = 65536
    arcs = [(0, 1, -1.), (1, 2, -.5), (2, 3, -2.), (3, 4, -1.), (4, 0, -1.), (1, 3, -3.)]
    graph = alignment.graph([3, 17, 3, 8, 30], arcs, stay=[-.2] * 5, initial=[0., -1., -math.inf, -math.inf, -2.],
                            final=[-1., -math.inf, 0., 0., -.5])
    ppg = C.random_ppg(65, frames).cuda()
    raw = Raw(packed_on_device([graph]), 1, frames, frames, 0)
    rc, post, states, begin, count, evidence = raw.push(ppg[None].contiguous(), [frames], frames)
    want = alignment.posterior(ppg, opened(graph), states=True)
    assert rc == 0 and count.tolist() == [frames] and begin.tolist() == [0]
    assert torch.equal(bits(evidence[0]), bits(want.total.cpu()))
    assert torch.equal(bits(post[0]), bits(want.phonemes.cpu()))
    assert torch.equal(bits(states[0]), bits(want.states.cpu()))


def test_poisoned_buffers_refused_graphs_and_an_overfull_push_at_the_c_level():
    good, other = C.random_graph(90, 9, big=False), C.random_graph(91, 70, big=False)
    packed = packed_on_device([good, other])
    ppg = torch.stack([C.random_ppg(92, 80), C.random_ppg(93, 80)]).cuda()
    block, lag = 4, 3
    alone = alignment.PosteriorStream(good, block=block, lag=lag, window=64, states=True)
    want = [alone.push(ppg[0, :, :21]), alone.push(ppg[0, :, 21:40]), alone.flush()]
    # (a) stream 1's target out of range: its graph is refused, stream 0 is untouched
    broken = packed._replace(targets=packed.targets.clone())
    broken.targets[int(packed.arc_begin[packed.state_begin[1]])] = 70
    # (b) which_graph out of range for stream 1
    for raw in (Raw(broken, 2, 64, block, lag, which=[0, 1]), Raw(packed, 2, 64, block, lag, which=[0, 2])):
        at = 0
        for expected, pushed in zip(want[:2], (21, 19)):
            rc, post, states, begin, count, evidence = raw.push(ppg[:, :, at:at + pushed].contiguous(), [pushed, pushed],
                                                                pushed + block - 1)
            at += pushed
            n = int(expected.count)
            assert rc == 0 and count.tolist() == [n, -1] and int(begin[0]) == int(expected.begin)
            assert torch.equal(bits(evidence[0]), bits(expected.evidence.cpu())) and math.isnan(float(evidence[1]))
            assert torch.equal(bits(post[0, :, :n]), bits(expected.phonemes[:, :n].cpu()))
            assert torch.equal(bits(states[0, :n, :9]), bits(expected.states[:n].cpu()))
            assert bool((post[0, :, n:] == Raw.POISON).all()) and bool((states[0, n:] == Raw.POISON).all())
            assert bool((states[0, :, 9:] == Raw.POISON).all())
            assert bool((post[1] == Raw.POISON).all()) and bool((states[1] == Raw.POISON).all())
        rc, post, states, begin, count, total = raw.flush(block + lag - 1)
        n = int(want[2].count)
        assert rc == 0 and count.tolist() == [n, 0] and math.isnan(float(total[1]))
        assert torch.equal(bits(total[0]), bits(want[2].total.cpu()))
        assert torch.equal(bits(post[0, :, :n]), bits(want[2].phonemes[:, :n].cpu()))
        assert bool((post[0, :, n:] == Raw.POISON).all()) and bool((post[1] == Raw.POISON).all())
    # (c) an overfull push: (p - c) + frames > window keeps the state; the next legal push is what it would have been
    raw = Raw(packed, 2, 64, 16, 16, which=[0, 1])
    alone = alignment.PosteriorStream(good, block=16, lag=16, window=64, states=True)
    first, second = alone.push(ppg[0, :, :40]), alone.push(ppg[0, :, 40:50])
    rc, post, _, begin, count, evidence = raw.push(ppg[:, :, :40].contiguous(), [40, 40], 55)
    assert rc == 0 and count.tolist() == [int(first.count)] * 2 == [16, 16]
    rc, post, _, begin, count, evidence = raw.push(ppg[:, :, :64].contiguous(), [64, 10], 79)      # 24 + 64 > 64
    assert rc == 0 and int(count[0]) == -1 and math.isnan(float(evidence[0])) and bool((post[0] == Raw.POISON).all())
    rc, post, _, begin, count, evidence = raw.push(ppg[:, :, 40:50].contiguous(), [10, 0], 25)
    n = int(second.count)
    assert rc == 0 and int(count[0]) == n == 16 and int(begin[0]) == 16 and int(count[1]) == 0
    assert torch.equal(bits(evidence[0]), bits(second.evidence.cpu()))
    assert torch.equal(bits(post[0, :, :n]), bits(second.phonemes[:, :n].cpu()))
