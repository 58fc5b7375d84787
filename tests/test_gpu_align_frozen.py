"""The outputs of ppg_align, ppg_align_optional, ppg_search and a ppg_search_stream_push sequence, frozen: every array
the library gives for the inputs of tests/golden/g14_align_frozen.npz equals the array recorded there, bit for bit.
The fixture holds the seeded inputs themselves and the raw outputs of the build it was recorded from; nothing here has
a tolerance or a reference computation.  This is the check for changes to ppgs_amd/csrc/ppg_align.hip that must not
move a bit; what the numbers mean is the business of the alignment and search tests beside this one.

    python tests/test_gpu_align_frozen.py          records the fixture again from the current build (on the GPU)

Shapes: alignment, plain and with optional phonemes, at T in {1, 31, 32, 33, 63, 64, 65, 97} x N in {1, 2, 64, 65, 256,
257} wherever the utterance can be aligned (N <= T; with optional phonemes, the mandatory ones <= T, so N may exceed
T): the chunk, refill and strip-length edges of DESIGN 4.11.  No T of that grid takes N = 256 or 257, so two
utterances of 260 frames are added for them: the longest 4-state strips and the 16-state strips.  One ragged batch per
kind holds refused items (N > T, a phoneme index out of range).  Search: T = 97, queries of 1, 8, 64, 65 and 256
phonemes, top = 3, with the curve; the stream: the same recording pushed as 1 + 31 + 33 + 32 frames, then a flush."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, 'tests', 'golden', 'g14_align_frozen.npz')

FRAMES = (1, 31, 32, 33, 63, 64, 65, 97)
COUNTS = (1, 2, 64, 65, 256, 257)
LONG = 260                                    # frames of the two added utterances
SEARCH_FRAMES = 97
QUERY_COUNTS = (1, 8, 64, 65, 256)
PUSHES = (1, 31, 33, 32)
TOP = 3
STREAM_THRESHOLD, STREAM_PATIENCE = -4., 4
# the ragged batches: (T, N) per item in a batch padded to 97 frames; N = 257 does not fit, and the last item's second
# phoneme is replaced by index 40
RAGGED = ((97, 65), (33, 2), (64, 64), (97, 257), (1, 1), (31, 2))

pytestmark = pytest.mark.gpu


def flags(count):
    """Optional flags on the first, the last and an inner phoneme, as far as `count` phonemes allow them: no two
    adjacent, one mandatory."""
    out = [False] * count
    if count >= 2:
        out[0] = True
    if count >= 3:
        out[-1] = True
    if count >= 5:
        out[count // 2] = True
    return out


def cases(optional):
    """The (T, N) of the single-utterance calls."""
    grid = [(frames, count) for frames in FRAMES for count in COUNTS
            if (flags(count).count(False) if optional else count) <= frames]
    return grid + [(LONG, 256), (LONG, 257)]


def inputs(seed=14):
    """The seeded inputs: a recording (40, 260), 257 phoneme indices (an utterance of N phonemes takes the first N) and
    the five queries, cut from what the recording says (the per-frame argmax from frame 10 on) but for the longest."""
    import torch
    generator = torch.Generator().manual_seed(seed)
    ppg = torch.softmax(3 * torch.randn(40, LONG, generator=generator), dim=0).numpy()
    phonemes = torch.randint(0, 40, (257,), generator=generator).numpy().astype(np.int32)
    said = ppg.argmax(0).astype(np.int32)
    queries = np.full((len(QUERY_COUNTS), max(QUERY_COUNTS)), -1, dtype=np.int32)
    for q, count in enumerate(QUERY_COUNTS):
        queries[q, :count] = said[10:10 + count] if count <= 65 else phonemes[:count]
    return {'ppg': ppg, 'phonemes': phonemes, 'queries': queries}


def outputs(given):
    """Every output array of the four entries for the inputs `given`, as numpy arrays by name."""
    import torch
    from ppgs_amd import alignment, engine
    ppg = torch.from_numpy(given['ppg']).cuda()
    phonemes = given['phonemes'].tolist()
    out = {}

    def keep(name, tensors):
        for field, tensor in tensors.items():
            if isinstance(tensor, (list, tuple)):
                tensor = torch.cat([part.reshape(-1) for part in tensor])
            out[f'{name}_{field}'] = tensor.cpu().numpy()

    for kind in ('align', 'optional'):
        optional = kind == 'optional'
        results = [alignment.forced(ppg[:, :frames], phonemes[:count], optional=flags(count) if optional else None)
                   for frames, count in cases(optional)]
        keep(kind, {field: [getattr(result, field) for result in results]
                    for field in ('total', 'starts', 'score', 'gop')})
        # the ragged batch, through the engine: alignment.forced refuses on the host what the kernels must refuse here
        most = max(count for _, count in RAGGED)
        table = torch.full((len(RAGGED), most), -1, dtype=torch.int32)
        marks = torch.zeros((len(RAGGED), most), dtype=torch.int32)
        for item, (_, count) in enumerate(RAGGED):
            table[item, :count] = torch.tensor(phonemes[:count], dtype=torch.int32)
            marks[item, :count] = torch.tensor(flags(count), dtype=torch.int32)
        table[-1, 1] = 40
        batch = ppg[None, :, :max(frames for frames, _ in RAGGED)].repeat(len(RAGGED), 1, 1)
        total, starts, score, gop = engine.align_items(
            batch, [frames for frames, _ in RAGGED], table.cuda(), [count for _, count in RAGGED], True,
            optional=marks.cuda() if optional else None)
        keep(kind + '_ragged', {'total': total, 'starts': starts, 'score': score, 'gop': gop})

    recording = ppg[:, :SEARCH_FRAMES]
    queries = [given['queries'][q, :count].tolist() for q, count in enumerate(QUERY_COUNTS)]
    hits = alignment.search(recording, queries, top=TOP, curve=True)
    keep('search', {'begin': hits.begin, 'end': hits.end, 'total': hits.total, 'mean': hits.mean, 'count': hits.count,
                    'curve_total': hits.curve[0], 'curve_begin': hits.curve[1]})
    spotter = alignment.SearchStream(queries, STREAM_THRESHOLD, patience=STREAM_PATIENCE, curve=True)
    pushed, at = [], 0
    for frames in PUSHES:
        pushed.append(spotter.push(recording[:, at:at + frames]))
        at += frames
    pushed.append(spotter.flush())
    keep('stream', {field: [getattr(hits, field) for hits in pushed]
                    for field in ('begin', 'end', 'total', 'mean', 'count')})
    keep('stream', {'curve_total': [hits.curve[0] for hits in pushed[:-1]],
                    'curve_begin': [hits.curve[1] for hits in pushed[:-1]]})
    return out


def record(path=FIXTURE):
    """The recipe of the fixture: the inputs and what the current build makes of them."""
    given = inputs()
    made = outputs(given)
    assert not set(given) & set(made)
    np.savez_compressed(path, **given, **made)
    return given, made


def bits(array):
    """An integer view of the same bytes, so that NaN sentinels compare."""
    return array.view({4: np.int32, 8: np.int64}[array.dtype.itemsize])


def test_every_output_equals_the_frozen_fixture_bit_for_bit(golden):
    frozen = golden('g14_align_frozen')
    given = {name: frozen[name] for name in ('ppg', 'phonemes', 'queries')}
    made = outputs(given)
    assert set(made) == set(frozen) - set(given)
    for name, array in made.items():
        want = frozen[name]
        assert array.dtype == want.dtype and array.shape == want.shape, name
        assert np.array_equal(bits(array), bits(want)), name
    # the fixture is not vacuous: aligned and refused utterances, hits, stream events and a pending hit at the flush
    assert np.isnan(frozen['align_ragged_total']).sum() == 2 and np.isfinite(frozen['align_total']).all()
    assert np.isnan(frozen['optional_ragged_total']).sum() == 2 and np.isfinite(frozen['optional_total']).all()
    assert frozen['search_count'].max() == TOP and frozen['stream_count'].sum() > 0


if __name__ == '__main__':
    sys.path.insert(0, ROOT)
    target = sys.argv[1] if len(sys.argv) > 1 else FIXTURE
    given, made = record(target)
    for name, array in sorted(made.items()):
        print(f'{name:28s} {array.dtype} {array.shape}')
    print('totals', made['align_total'][:6], made['optional_total'][:6], made['align_ragged_total'],
          made['optional_ragged_total'])
    print('search count', made['search_count'], 'stream count', made['stream_count'])
    print(os.path.getsize(target), 'bytes')
