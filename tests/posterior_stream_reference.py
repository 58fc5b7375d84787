"""CPU restatement of ppgs_amd.alignment.PosteriorStream for the tests (tests/test_posterior_stream_host.py,
tests/test_gpu_posterior_stream.py): DESIGN 4.20 in float64, built from posterior_reference.forward_backward.

With open(g) = g with final = 0 everywhere, a block H and a lag L: block k = frames [kH, (k+1)H) is given out by the
first push after which p >= (k+1)H + L, as columns [kH, (k+1)H) of forward_backward(e[:h + 1], open(g)), h = (k+1)H +
L - 1; every push reports evidence = the total of forward_backward(e[:p], open(g)); the flush gives out [c, p) and the
total of forward_backward(e[:p], g).  The emission schedule is plain integer arithmetic."""
import math

import numpy as np

import posterior_reference as reference


def emitted(received, block, lag):
    """c after `received` frames: H * max(0, floor((p - L) / H))."""
    return block * max(0, (received - lag) // block)


def schedule(pushes, block, lag):
    """[(begin, count)] of pushes of these many frames, from frame 0, and the flush's last."""
    out, position = [], 0
    for frames in pushes:
        before = emitted(position, block, lag)
        position += frames
        out.append((before, emitted(position, block, lag) - before))
    c = emitted(position, block, lag)
    return out + [(c, position - c)]


def open_graph(g):
    """`g` (Lists) with an open end: every state may end at no cost."""
    return g._replace(final=[0.] * len(g.final))


def horizon(block_index, block, lag):
    """The last frame block `block_index` is smoothed by."""
    return (block_index + 1) * block + lag - 1


class Prefixes:
    """forward_backward of the prefixes of one recording under the open graph, each computed once."""

    def __init__(self, e, g, dtype=np.float64):
        self.e, self.g, self.open, self.dtype, self.kept = np.asarray(e), g, open_graph(g), dtype, {}

    def upto(self, frames):
        """(total, gamma, post) of e[:frames] under the open graph."""
        if frames not in self.kept:
            self.kept[frames] = reference.forward_backward(self.e[:frames], self.open, self.dtype)
        return self.kept[frames]

    def block(self, block_index, block, lag):
        """(gamma (H, S), post (40, H)) of a block, None for a prefix without a path."""
        total, gamma, post = self.upto(horizon(block_index, block, lag) + 1)
        if gamma is None:
            return None
        first, end = block_index * block, (block_index + 1) * block
        return gamma[first:end], post[:, first:end]


def stream(e, g, pushes, block, lag, dtype=np.float64):
    """The stream over e (T, S) fed in pushes of these many frames (their sum may stay below T) and then flushed:
    a list of dicts begin, count, gamma (count, S), post (40, count), evidence per push, and the flush's with total in
    the place of evidence.  A dead stream reports count = 0 and evidence = -inf from the push in which it dies on, and
    its flush count = 0 and total = -inf."""
    prefixes = Prefixes(e, g, dtype)
    count_states = np.asarray(e).shape[1]
    out, position, dead = [], 0, False

    def nothing(begin, **more):
        return dict(begin=begin, count=0, gamma=np.zeros((0, count_states)), post=np.zeros((40, 0)), **more)
    for frames in pushes:
        before = emitted(position, block, lag)
        if dead or frames == 0:
            out.append(nothing(before, evidence=-math.inf if dead else
                               (prefixes.upto(position)[0] if position else 0.)))
            continue
        after = emitted(position + frames, block, lag)
        evidence = prefixes.upto(position + frames)[0]
        if evidence == -math.inf:
            dead = True
            out.append(nothing(before, evidence=-math.inf))
            continue
        position += frames
        blocks = [prefixes.block(k, block, lag) for k in range(before // block, after // block)]
        gamma = np.concatenate([b[0] for b in blocks]) if blocks else np.zeros((0, count_states))
        post = np.concatenate([b[1] for b in blocks], axis=1) if blocks else np.zeros((40, 0))
        out.append(dict(begin=before, count=after - before, gamma=gamma, post=post, evidence=evidence))
    c = emitted(position, block, lag)
    if dead or position == 0:
        out.append(nothing(c, total=-math.inf if dead else math.nan))
        return out
    total, gamma, post = reference.forward_backward(np.asarray(e)[:position], g, dtype)
    if gamma is None:
        out.append(nothing(c, total=-math.inf))
    else:
        out.append(dict(begin=c, count=position - c, gamma=gamma[c:], post=post[:, c:], total=total))
    return out
