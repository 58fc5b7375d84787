"""Host side of the incremental frontend (ppg_frontend_stream_*, engine.FrontendStream): the frame
arithmetic that callers and the library share, pinned to the reference's padding with the oracle, and
the exported symbols.  No GPU."""
import ctypes

import numpy as np
import torch

from oracle import ppg_oracle as O
from ppgs_amd import engine as E


def brute_force_frames(received, flushed):
    """The rule as a sentence: a recording that goes on emits frame t once its last sample
    160 t + 591 has arrived, and only in whole pairs (2 j, 2 j + 1); one that ended has
    received // 160 frames."""
    if flushed:
        return received // 160
    frames = 0
    while 160 * (frames + 1) + 591 < received:        # both frames of the pair (frames, frames + 1)
        frames += 2
    return frames


def test_audio_stream_frames_rule():
    previous = 0
    for received in range(0, 4001):
        frames = E.audio_stream_frames(received, False)
        assert frames == brute_force_frames(received, False), received
        assert frames % 2 == 0 and frames >= previous
        # never a frame whose last sample has not arrived
        assert frames == 0 or 160 * (frames - 1) + 591 < received
        # and never more than one pair behind what is computable
        assert 160 * (frames + 1) + 591 >= received
        previous = frames
    for total in range(433, 4001):
        assert E.audio_stream_frames(total, True) == total // 160 == brute_force_frames(total, True)
        assert E.audio_stream_frames(total, True) >= E.audio_stream_frames(total, False)
    assert E.audio_stream_frames(2 ** 40, False) == ((2 ** 40 - 592) // 160 + 1) & ~1


def test_prefix_frames_equal_whole_recording_frames_in_the_oracle():
    """The 592-sample look-ahead is the reference's own: the frames audio_stream_frames calls computable
    after R samples do not change when more samples follow."""
    generator = torch.Generator().manual_seed(11)
    audio = 0.1 * torch.randn(2, 1, 6000, generator=generator)
    whole = O.mel_from_audios(audio).numpy()
    for received in (592, 751, 752, 911, 912, 1072, 2560, 3333, 4000, 5999):
        frames = E.audio_stream_frames(received, False)
        prefix = O.mel_from_audios(audio[..., :received]).numpy()
        assert frames <= prefix.shape[2]
        assert np.array_equal(prefix[:, :, :frames].view(np.int16), whole[:, :, :frames].view(np.int16)), received
    # one sample fewer and the pair's second frame does differ (the rule is tight)
    prefix = O.mel_from_audios(audio[..., :751]).numpy()
    assert not np.array_equal(prefix[:, :, :2], whole[:, :, :2])


def test_library_exports_the_frontend_stream():
    lib = E.library()
    for name in ('ppg_audio_stream_frames', 'ppg_frontend_stream_create', 'ppg_frontend_stream_destroy',
                 'ppg_frontend_stream_batch', 'ppg_frontend_stream_state', 'ppg_frontend_stream_reset',
                 'ppg_frontend_stream_push'):
        assert hasattr(lib, name) and name in E.SYMBOLS, name
    assert lib.ppg_audio_stream_frames(-1, 0) == -1
    # bad arguments are refused before any device is touched
    handle = ctypes.c_void_p()
    assert lib.ppg_frontend_stream_create(0, 0, 2560, ctypes.byref(handle)) == -1
    assert lib.ppg_frontend_stream_create(0, 4, 0, ctypes.byref(handle)) == -1
    assert lib.ppg_frontend_stream_push(None, None, 0, 0, None, None, None, 0, 0, None, None, None) == -1
    if not torch.cuda.is_available():
        assert lib.ppg_frontend_stream_create(0, 4, 2560, ctypes.byref(handle)) == -2
        assert b'no HIP device' in lib.ppg_last_error()
