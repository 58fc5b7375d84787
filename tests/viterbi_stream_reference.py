"""CPU restatement of ppgs_amd.alignment.ViterbiStream for the tests (tests/test_viterbi_stream_host.py,
tests/test_gpu_viterbi_stream.py): DESIGN 4.18 word for word in numpy -- forward, natural and forced commit, runs,
flush -- over prepared frames and a graph's arc lists (`Lists` of tests/viterbi_reference.py).  It takes logp (T, 40)
and top (T,) (the frame's maximum), so it can be run on the device's own bits: `dtype` is the arithmetic, float32
restates the device's additions and divisions one for one, float64 is the variant of the host tests.  It keeps every
frame (no ring); `window` only decides what is refused.

A run is (state, phoneme, begin, end, score, gop); the weights are finite or -inf."""
import numpy as np


class Stream:
    def __init__(self, graph, max_lag=None, window=None, dtype=np.float32):
        self.dtype = dtype
        self.sym = np.asarray(graph.sym, dtype=np.int64)
        self.states = len(self.sym)
        self.stay, self.initial, self.final = (np.asarray(v, dtype=dtype) for v in
                                               (graph.stay, graph.initial, graph.final))
        self.into = [[(int(source), dtype(weight)) for source, weight in arcs] for arcs in graph.into]
        self.max_lag, self.window = max_lag, window            # None: never forced; nothing refused
        self.commits = []                                      # c after every push
        self.reset()

    def reset(self):
        self.p = self.c = self.forced = 0
        self.d = np.full(self.states, -np.inf, dtype=self.dtype)
        self.origin, self.before, self.e, self.top = [], [], [], []    # per frame since the reset
        self.run = None                                        # the open run: [state, start, sum, below]

    # ---- forward: the recurrence of viterbi, one frame ----
    def _frame(self, e):
        origin = np.zeros(self.states, dtype=np.int64)         # the ordinal `from`
        before = np.arange(self.states)                        # the state it stands for
        with np.errstate(invalid='ignore'):
            if self.p == 0:
                self.d = (e + self.initial).astype(self.dtype)
            else:
                now = np.empty(self.states, dtype=self.dtype)
                for n in range(self.states):
                    best, chosen = self.dtype(self.d[n] + self.stay[n]), 0
                    for j, (source, weight) in enumerate(self.into[n]):
                        c = self.dtype(self.d[source] + weight)
                        if c > best:
                            best, chosen = c, j + 1
                    now[n] = self.dtype(e[n] + best)
                    origin[n] = chosen
                    if chosen:
                        before[n] = self.into[n][chosen - 1][0]
                self.d = now
        self.origin.append(origin)
        self.before.append(before)
        self.p += 1

    def _paths(self, low):
        """states[u - low][n] = path(n, u) for u in [low, p - 1]."""
        t = self.p - 1
        states = [None] * (t - low + 1)
        path = np.arange(self.states)
        for u in range(t, low - 1, -1):
            states[u - low] = path
            if u > 0:
                path = self.before[u][path]
        return states

    # ---- runs: every newly committed frame in order ----
    def _give(self, states, out):
        for state in states:
            t = self.c
            if t == 0 or self.origin[t][state] != 0:           # the frame opens a run
                self._close(t, out)
                self.run = [int(state), t, self.dtype(0.), self.dtype(0.)]
            e = self.e[t][state]
            self.run[2] = self.dtype(self.run[2] + e)
            self.run[3] = self.dtype(self.run[3] + self.dtype(e - self.top[t]))
            self.c += 1

    def _close(self, end, out):
        if self.run is not None:
            state, start, total, below = self.run
            count = self.dtype(end - start)
            out.append((state, int(self.sym[state]), start, end, self.dtype(total / count), self.dtype(below / count)))
        self.run = None

    def push(self, logp, top):
        """The runs this push closes, or None if the stream refuses it (an overfull window): nothing changes then."""
        logp, top = np.asarray(logp, dtype=self.dtype), np.asarray(top, dtype=self.dtype)
        assert logp.shape == (len(top), 40)
        if self.window is not None and (self.p - self.c) + len(top) > self.window:
            return None
        for t in range(len(top)):
            e = logp[t][self.sym]
            self.e.append(e)
            self.top.append(top[t])
            self._frame(e)
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

    def flush(self):
        """(runs, total, forced); the stream starts again at frame 0."""
        out = []
        with np.errstate(invalid='ignore'):
            f = (self.d + self.final).astype(self.dtype)
        last = 0
        for n in range(1, self.states):
            if f[n] > f[last]:
                last = n
        total = f[last]
        if total > -np.inf and self.p > self.c:
            low = self.c
            states = self._paths(low)
            self._give([states[u - low][last] for u in range(low, self.p)], out)
        self._close(self.c, out)
        forced = self.forced
        self.reset()
        return out, self.dtype(total), forced


def feed(stream, logp, top, pushes):
    """Push logp (T, 40), top (T,) in pieces of `pushes` frames: the list of run lists, one per push."""
    out, at = [], 0
    for frames in pushes:
        out.append(stream.push(logp[at:at + frames], top[at:at + frames]))
        at += frames
    assert at == len(top)
    return out


def flat(lists):
    return [run for runs in lists for run in runs]


def frames_of(runs):
    """The state of every frame of a list of contiguous runs, from their first frame on."""
    states, at = [], runs[0][2] if runs else 0
    for state, _, begin, end, _, _ in runs:
        assert begin == at and end > begin, (begin, at, end)
        states.extend([state] * (end - begin))
        at = end
    return np.asarray(states, dtype=np.int64)


def prepared(ppg):
    """logp (T, 40), top (T,) float32 from a (40, T) torch PPG: the clamp and the log in fp32, as the device prepares
    them (up to the last bit of logf)."""
    logp = np.log(np.clip(ppg.float().numpy().T, np.float32(1e-8), np.float32(1 - 1e-8))).astype(np.float32)
    return logp, logp.max(axis=1)
