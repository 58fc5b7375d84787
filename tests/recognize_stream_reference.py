"""CPU restatement of ppgs_amd.alignment.RecognizeStream for the tests (tests/test_recognize_stream_host.py,
tests/test_gpu_recognize_stream.py): DESIGN 4.16 word for word in numpy -- forward, natural and forced commit, runs,
flush.  It takes prepared frames, e (T, K) and top (T,) (the frame's maximum), so it can be run on the device's own
bits: `dtype` is the arithmetic, float32 restates the device's additions and divisions one for one, float64 is the
variant of the host tests.  It keeps every frame (no ring); `window` only decides what is refused.

A run is (phoneme, begin, end, score, gop); the weights are finite or -inf."""
import numpy as np


class Stream:
    def __init__(self, A, initial=None, max_lag=None, window=None, dtype=np.float32):
        self.dtype = dtype
        self.A = np.asarray(A, dtype=dtype)
        self.states = self.A.shape[0]
        assert self.A.shape == (self.states, self.states)
        self.initial = np.zeros(self.states, dtype=dtype) if initial is None else np.asarray(initial, dtype=dtype)
        self.max_lag, self.window = max_lag, window            # None: never forced; nothing refused
        self.commits = []                                      # c after every push
        self.reset()

    def reset(self):
        self.p = self.c = self.forced = 0
        self.d = np.full(self.states, -np.inf, dtype=self.dtype)
        self.origin, self.e, self.top = [], [], []             # per frame since the reset
        self.run = None                                        # the open run: [label, start, sum, below]

    # ---- forward: the recurrence of recognize, one frame ----
    def _frame(self, e):
        index = np.arange(self.states)
        with np.errstate(invalid='ignore'):
            if self.p == 0:
                self.d = (e + self.initial).astype(self.dtype)
                origin = index.copy()
            else:
                c = (self.d[:, None] + self.A).astype(self.dtype)          # c[p, q]: one addition per candidate
                best = c.max(axis=0)
                # staying wherever it is among the best, else the lowest of the best (argmax takes the first)
                origin = np.where(c[index, index] == best, index, c.argmax(axis=0))
                self.d = (e + best).astype(self.dtype)
        self.origin.append(origin)
        self.p += 1

    def _paths(self, low):
        """states[u - low][q] = path(q, u) for u in [low, p - 1]."""
        t = self.p - 1
        states = [None] * (t - low + 1)
        path = np.arange(self.states)
        for u in range(t, low - 1, -1):
            states[u - low] = path
            if u > 0:
                path = self.origin[u][path]
        return states

    # ---- runs: every newly committed frame in order ----
    def _give(self, labels, out):
        for label in labels:
            t = self.c
            if self.run is None or self.run[0] != label:
                self._close(t, out)
                self.run = [int(label), t, self.dtype(0.), self.dtype(0.)]
            e = self.e[t][label]
            self.run[2] = self.dtype(self.run[2] + e)
            self.run[3] = self.dtype(self.run[3] + self.dtype(e - self.top[t]))
            self.c += 1

    def _close(self, end, out):
        if self.run is not None:
            label, start, total, below = self.run
            count = self.dtype(end - start)
            out.append((label, start, end, self.dtype(total / count), self.dtype(below / count)))
        self.run = None

    def push(self, e, top):
        """The runs this push closes, or None if the stream refuses it (an overfull window): nothing changes then."""
        e, top = np.asarray(e, dtype=self.dtype), np.asarray(top, dtype=self.dtype)
        assert e.shape == (len(top), self.states)
        if self.window is not None and (self.p - self.c) + len(top) > self.window:
            return None
        for t in range(len(top)):
            self.e.append(e[t])
            self.top.append(top[t])
            self._frame(e[t])
        out = []
        p, t = self.p, self.p - 1
        alive = self.d > -np.inf
        if alive.any() and p > self.c:
            low = self.c
            states = self._paths(low)
            # 1. natural: the largest u at which every alive path is in the same state
            v = low - 1
            for u in range(t, low - 1, -1):
                here = states[u - low][alive]
                if (here == here[0]).all():
                    v = u
                    break
            self._give([states[u - low][alive][0] for u in range(low, v + 1)], out)
            # 2. forced
            if self.max_lag is not None and p - self.c > self.max_lag:
                best = int(np.argmax(np.where(alive, self.d, -np.inf)))    # the first of the largest
                last = p - self.max_lag - 1
                self.forced += last + 1 - self.c
                goal = states[last - low][best]
                self.d[states[last - low] != goal] = -np.inf
                self._give([states[u - low][best] for u in range(self.c, last + 1)], out)
                assert self.c == p - self.max_lag
        self.commits.append(self.c)
        return out

    def flush(self, final=None):
        """(runs, total, forced); the stream is reset."""
        final = np.zeros(self.states, dtype=self.dtype) if final is None else np.asarray(final, dtype=self.dtype)
        out = []
        with np.errstate(invalid='ignore'):
            f = (self.d + final).astype(self.dtype)
        last = 0
        for q in range(1, self.states):
            if f[q] > f[last]:
                last = q
        total = f[last]
        if total > -np.inf and self.p > self.c:
            states = self._paths(self.c)
            low = self.c
            self._give([states[u - low][last] for u in range(low, self.p)], out)
        self._close(self.c, out)
        forced = self.forced
        self.reset()
        return out, self.dtype(total), forced


def feed(stream, e, top, pushes):
    """Push e (T, K), top (T,) in pieces of `pushes` frames: the list of run lists, one per push."""
    out, at = [], 0
    for frames in pushes:
        out.append(stream.push(e[at:at + frames], top[at:at + frames]))
        at += frames
    assert at == len(top)
    return out


def flat(lists):
    return [run for runs in lists for run in runs]


def labels_of(runs):
    """The label row of a list of contiguous runs, and whether they are contiguous from their first frame on."""
    labels, at = [], runs[0][1] if runs else 0
    for label, begin, end, _, _ in runs:
        assert begin == at and end > begin, (begin, at, end)
        labels.extend([label] * (end - begin))
        at = end
    return np.asarray(labels, dtype=np.int64)


# The recordings of the ring test of tests/test_gpu_recognize_stream.py: the host test measures the reference's lag on
# these very seeds and shapes, which is what lets the GPU test ask for forced == 0 with a lag of 32 frames.
WRAP_FRAMES, WRAP_WINDOW, WRAP_LAG = 300, 64, 32
WRAP_SCALES, WRAP_PENALTIES = (3., 8.), (1., 4.)


def wrap_ppg(scale):
    """(40, WRAP_FRAMES) fp32 torch: the recording of the ring test at this softmax scale."""
    import torch

    import alignment_reference
    return alignment_reference.random_ppg(WRAP_FRAMES, scale, torch.Generator().manual_seed(31600 + int(scale)))


def switch(penalty, states=40):
    A = np.full((states, states), -float(penalty), dtype=np.float32)
    np.fill_diagonal(A, 0.)
    return A


def prepared(ppg):
    """e (T, 40), top (T,) float32 from a (40, T) torch PPG: the clamp and the log in fp32, as the device prepares them
    (up to the last bit of logf)."""
    e = np.log(np.clip(ppg.float().numpy().T, np.float32(1e-8), np.float32(1 - 1e-8))).astype(np.float32)
    return e, e.max(axis=1)
