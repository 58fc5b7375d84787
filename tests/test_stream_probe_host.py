"""What tests/test_gpu_stream_probe.py relies on, without a GPU: the schedules of tests/stream_probe.py deliver every
frame once, flush every item once, let the long items sit steps out and end at different steps -- and their steps lie
on both sides of the row-block counts at which ppg_stream_push_batch changes the shape of its FFN launch, so that a
schedule edited later cannot quietly stop reaching that edge.

The edge the tests were written for: the hidden splits of the FFN launch were chosen per step
(stream_probe.ffn_splits, 256 CUs) -- 16-bit modes at hidden 256, cap 16: 16 up to 64 blocks, 8 up to 128, 4 up to 256;
fp32, cap 32: 32 up to 32 blocks, 16 up to 64, 8 up to 128 -- so 32 was the first threshold of the fp32 mode and 64 that
of the 16-bit modes, and steps on different sides of one summed in different orders.  The edge there is now: the number
of groups is the stream's (stream_probe.ffn_groups), and a step of more than two rounds of workgroups walks them in one
workgroup per token tile (stream_probe.ffn_closed) -- another kernel path that must give the same bits.

The twelve-item loud batch: `whole` 86 blocks, `sixteens` <= 16, `ones` <= 10, `ragged` 40 and 1 .. 16.  The 24-item
staircase batch: `whole` 185, `ones` <= 23, `ragged` 67 and 1 .. 51.  Its `sixteens` cannot stay below 32: twenty of
its items are longer than 32 frames and a 16-frame push behind the first touches two blocks of each (rows
x_prev // 16 * 16 .. round_up(x_prev + 16, 16) with x_prev = 14 mod 16), 42 at the most; it stays below 64, the
threshold of the 16-bit modes, and that is what is asserted for it.
"""
import pytest

import attention_probe as A
import encoder_params as P
import stream_probe as S

LOUD = P.VALID
STAIRCASE = A.VALID
SHORT = tuple(v for v in P.VALID if v <= 144)
BATCHES = {'loud': LOUD, 'staircase': STAIRCASE, 'short': SHORT}


@pytest.mark.parametrize('totals', list(BATCHES.values()), ids=list(BATCHES))
@pytest.mark.parametrize('name', S.NAMES)
def test_every_frame_once_every_item_flushed_once(name, totals):
    steps = S.named(name, totals)
    batch = len(totals)
    sent, flushed = [0] * batch, [0] * batch
    for counts, flush in steps:
        assert len(counts) == len(flush) == batch
        assert any(counts) or any(flush)
        for b in range(batch):
            assert counts[b] >= 0
            assert not flushed[b] or (counts[b] == 0 and not flush[b]), 'nothing follows an item\'s flush'
            sent[b] += counts[b]
            flushed[b] += bool(flush[b])
            assert not flush[b] or sent[b] == totals[b], 'the flush comes with the last frames'
    assert sent == list(totals) and flushed == [1] * batch


@pytest.mark.parametrize('totals', [LOUD, STAIRCASE], ids=['loud', 'staircase'])
@pytest.mark.parametrize('name', ['ragged', 'ragged2'])
def test_ragged_schedules_are_ragged(name, totals):
    steps = S.named(name, totals)
    batch = len(totals)
    ends = [max(i for i, (_, flush) in enumerate(steps) if flush[b]) for b in range(batch)]
    assert len(set(ends)) >= 6, 'items end at different steps'
    for b, total in enumerate(totals):
        mine = [(counts[b], flush[b]) for counts, flush in steps[:ends[b] + 1]]
        if total >= S.SIT_OUT_FROM:
            assert (0, False) in mine, f'item {b} ({total} frames) never sits a step out before it ends'
        if total == 0:
            assert mine[-1] == (0, True) and sum(n for n, _ in mine) == 0
        if total == 1:
            assert mine[-1] == (1, True)
    pushes = [n for counts, _ in steps for n in counts if n > 0]
    assert any(n % 16 for n in pushes) and len(set(pushes)) >= 8
    # frontiers before, on and behind block boundaries: the items' received counts modulo 16 take many values
    received, seen = [0] * batch, set()
    for counts, _ in steps:
        for b in range(batch):
            received[b] += counts[b]
            seen.add(received[b] % 16)
    assert 0 in seen and len(seen) >= 6


@pytest.mark.parametrize('totals', [LOUD, STAIRCASE, SHORT], ids=['loud', 'staircase', 'short'])
def test_ragged2_gives_every_item_the_pushes_of_ragged_beside_other_neighbours(totals):
    one, two = S.named('ragged', totals), S.named('ragged2', totals)
    for b in range(len(totals)):
        assert S.own_pushes(one, b) == S.own_pushes(two, b)
    assert S.blocks_per_step(totals, one) != S.blocks_per_step(totals, two)
    # who is pushed together differs: most steps of one are no steps of the other
    shared = set(tuple(counts) for counts, _ in one) & set(tuple(counts) for counts, _ in two)
    assert len(shared) <= len(one) // 2


def test_block_counts_of_the_loud_batch_straddle_the_split_thresholds():
    assert len(LOUD) == 12 and max(LOUD) == P.FRAMES == 300 and S.rows_of(300) == 320
    blocks = {name: S.blocks_per_step(LOUD, S.named(name, LOUD)) for name in S.NAMES}
    print(blocks['whole'], blocks['ragged'], blocks['ragged2'], max(blocks['sixteens']), max(blocks['ones']))
    assert blocks['whole'] == [sum((v + 15) // 16 for v in LOUD)] and blocks['whole'][0] > 64
    assert max(blocks['sixteens']) <= 32 and max(blocks['ones']) <= 32
    assert max(blocks['ragged']) > 32 and 0 < min(blocks['ragged']) < 32
    # the split counts the rule gives these steps: `whole` differs from the others in every mode, `ragged` in fp32
    for cap in (16, 32):
        assert S.ffn_splits(blocks['whole'][0], cap) == 8
        assert {S.ffn_splits(n, cap) for n in blocks['sixteens'] + blocks['ones'] if n} == {cap}
    assert {S.ffn_splits(n, 32) for n in blocks['ragged']} == {16, 32}


def test_block_counts_of_the_staircase_batch_straddle_the_split_thresholds():
    assert len(STAIRCASE) == 24 and max(STAIRCASE) == A.FRAMES == 300
    blocks = {name: S.blocks_per_step(STAIRCASE, S.named(name, STAIRCASE)) for name in S.NAMES}
    print(blocks['whole'], blocks['ragged'], blocks['ragged2'], max(blocks['sixteens']), max(blocks['ones']))
    assert blocks['whole'][0] > 64
    assert max(blocks['ones']) <= 32
    assert 32 < max(blocks['sixteens']) <= 64 and min(n for n in blocks['sixteens'] if n) < 32      # (module docstring)
    assert max(blocks['ragged']) > 64 and 0 < min(blocks['ragged']) < 32
    assert {S.ffn_splits(n, 16) for n in blocks['ragged']} == {8, 16}
    assert {S.ffn_splits(n, 32) for n in blocks['ragged']} == {8, 16, 32}
    assert {S.ffn_splits(n, 16) for n in blocks['sixteens'] + blocks['ones'] if n} == {16}


def test_whole_pushes_reach_the_closed_groups_and_small_pushes_the_split_ones():
    """The two shapes of the FFN launch of a stream whose groups are fixed: the loud batch pushed whole reaches the
    one-workgroup form in fp32 and fp16x2 (32 groups), the staircase batch pushed whole in every mode (16 groups); the
    16-frame and one-frame steps never do -- the bitwise tests compare the two."""
    assert [S.ffn_groups(12, cap) for cap in (16, 32)] == [16, 32]
    assert [S.ffn_groups(24, cap) for cap in (16, 32)] == [16, 16]
    assert [S.ffn_groups(1, cap) for cap in (16, 32)] == [16, 32] and S.ffn_groups(64, 16) == 8
    loud = {name: S.blocks_per_step(LOUD, S.named(name, LOUD)) for name in S.NAMES}
    stair = {name: S.blocks_per_step(STAIRCASE, S.named(name, STAIRCASE)) for name in S.NAMES}
    assert S.ffn_closed(loud['whole'][0], 32) and not S.ffn_closed(loud['whole'][0], 16)
    assert S.ffn_closed(stair['whole'][0], 16)
    for blocks, groups in ((loud, 16), (loud, 32), (stair, 16)):
        for name in ('sixteens', 'ones', 'ragged', 'ragged2'):
            assert not any(S.ffn_closed(n, groups) for n in blocks[name]), name
    # one utterance (at most 32 blocks of a 500-frame window) never leaves the split form
    assert not S.ffn_closed(32, 16) and not S.ffn_closed(32, 32)


def test_row_range_rule():
    """blocks_per_step against the rule worked by hand: one item of 40 frames in pushes of 20, 17 and 3 + flush."""
    steps = [([20], [False]), ([17], [False]), ([3], [True])]
    # received 20: x 0 -> 18, rows 0 .. 32; received 37: x 18 -> 35, rows 16 .. 48; flush at 40: x 35 -> 40, rows 32 .. 48
    assert S.blocks_per_step([40], steps) == [2, 2, 1]
    # a flush of nothing received touches nothing, a one-frame item one block
    assert S.blocks_per_step([0, 1], [([0, 1], [True, True])]) == [1]
    assert [S.ffn_splits(n, 16) for n in (1, 32, 64, 65, 128, 129, 256, 257)] == [16, 16, 16, 8, 8, 4, 4, 2]
    assert [S.ffn_splits(n, 32) for n in (1, 32, 33, 64, 65, 128, 129)] == [32, 32, 16, 16, 8, 8, 4]


def test_the_short_batch_leaves_half_a_workgroup_of_rows():
    """The items of at most 144 frames as streams of 144: R = 160, 7 x 160 rows = 32 modulo 64 -- the partial rows of a
    near-full step then end past batch * R (test_gpu_parity.py::test_stream_near_full_push_after_small_push)."""
    assert SHORT == (0, 1, 15, 16, 17, 33, 144)
    rows = S.rows_of(max(SHORT))
    assert rows == 160 and len(SHORT) * rows == 1120 and len(SHORT) * rows % 64 == 32
    steps = S.small_then_near_full(SHORT)
    assert [sum(counts) for counts, _ in steps] == [sum(min(20, v) for v in SHORT), sum(max(v - 20, 0) for v in SHORT)]
    assert [flush for _, flush in steps] == [[v <= 20 for v in SHORT], [v > 20 for v in SHORT]]
    # the second step recomputes from row 16 of the items still open
    first = sum((v + 15) // 16 for v in SHORT if v <= 20) + 2 * sum(1 for v in SHORT if v > 20)
    assert S.blocks_per_step(SHORT, steps) == [first, (48 - 16) // 16 + (144 - 16) // 16]


def test_push_lists():
    assert S.push_sizes(300, 37) == [37] * 8 + [4] and S.push_sizes(300, 300) == [300]
    assert sum(S.cycle_sizes(850)) == 850 and sum(S.cycle_sizes(565, offset=4)) == 565
    assert S.cycle_sizes(850)[:3] == S.SIZES[:3] and S.cycle_sizes(850) != S.cycle_sizes(850, offset=4)
