"""CPU restatement of the online detector of ppgs_amd.alignment.SearchStream for the tests
(tests/test_search_stream_host.py, tests/test_gpu_search_stream.py): the rule of DESIGN 4.14 word for word over a float32
curve, frame by frame, with the events grouped by the push that gave them out; and the planted input of
tests/test_gpu_search.py, by the same recipe."""
import numpy as np
import torch


class Detector:
    """One pair's detector.  frame() and flush() return the hits they emit, each (begin, end, total, mean) with total
    and mean numpy float32."""

    def __init__(self, threshold, patience):
        self.threshold, self.patience = np.float32(threshold), int(patience)
        self.taken, self.pending = 0, None

    def _emit(self):
        hit, self.pending = self.pending, None
        self.taken = hit[1]
        return hit

    def frame(self, t, total, begin):
        """Frame t (absolute) with its curve values."""
        out = []
        # 1. a pending hit whose last frame lies more than `patience` frames back is emitted
        if self.pending is not None and t - (self.pending[1] - 1) > self.patience:
            out.append(self._emit())
        # 2. the match ending here, if it begins at or after `taken` and its mean reaches the threshold
        begin = int(begin)
        if begin >= 0 and begin >= self.taken:
            total = np.float32(total)
            mean = total / np.float32(t - begin + 1)                     # one fp32 division
            if mean >= self.threshold:
                candidate = (begin, t + 1, total, mean)
                if self.pending is None:
                    self.pending = candidate
                elif begin < self.pending[1]:                            # the spans overlap
                    if mean >= self.pending[3]:                          # ties go to the later end frame
                        self.pending = candidate
                else:                                                    # disjoint
                    out.append(self._emit())
                    self.pending = candidate
        return out

    def flush(self):
        return [self._emit()] if self.pending is not None else []


def detect(curve_total, curve_begin, threshold, patience, pushes=None, flush=True):
    """The events of a whole curve as a list per push (`pushes`: the frames of each; None: one push of everything) and,
    with `flush`, one more list for the flush at the end."""
    curve_total = np.asarray(curve_total, dtype=np.float32)
    pushes = [len(curve_total)] if pushes is None else list(pushes)
    assert sum(pushes) == len(curve_total)
    detector = Detector(threshold, patience)
    out, t = [], 0
    for frames in pushes:
        events = []
        for _ in range(frames):
            events += detector.frame(t, curve_total[t], curve_begin[t])
            t += 1
        out.append(events)
    if flush:
        out.append(detector.flush())
    return out


def flat(per_push):
    return [hit for events in per_push for hit in events]


def planted():
    """The planted input of tests/test_gpu_search.py, by its recipe: a PPG (target logit +10) in which the query stands
    at three known places; the frames between carry labels that are neither the query's first nor its last phoneme.
    (ppg, query, places, labels); places[i] are the starts of the five phonemes and the end."""
    generator = torch.Generator().manual_seed(19)
    query = [3, 11, 22, 11, 30]
    others = [p for p in range(40) if p not in (query[0], query[-1])]

    def filler(frames):
        picks = torch.randint(0, len(others), (frames,), generator=generator).tolist()
        return [others[p] for p in picks]
    labels, places = [], []
    for gap in (23, 40, 17, 31):
        labels += filler(gap)
        if len(places) < 3:
            durations = torch.randint(1, 7, (len(query),), generator=generator).tolist()
            starts = [len(labels)]
            for phoneme, duration in zip(query, durations):
                labels += [phoneme] * duration
                starts.append(len(labels))
            places.append(starts)
    labels = torch.tensor(labels)
    frames = labels.shape[0]
    logits = torch.randn(40, frames, generator=generator)
    logits[labels, torch.arange(frames)] += 10.
    return torch.softmax(logits, dim=0), query, places, labels
