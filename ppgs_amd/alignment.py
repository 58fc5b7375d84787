"""Forced alignment of a PPG to a phoneme sequence, with goodness-of-pronunciation scores.

`ppgs_amd.distance` and `ppgs_amd.dtw` say how far apart two pronunciations are.  This module answers the other
question of pronunciation work: given the PPG and the phonemes the speaker was meant to say, where does each phoneme
start, and how well was it said?  It runs on the GPU (ppg_align, ppg_decode and ppg_recognize,
ppgs_amd/csrc/ppg_align.hip).

For one utterance, PPG P (40, T) and phoneme indices s of length N, 1 <= N <= T:

    e[t, n] = logf(min(max(P[s[n], t], 1e-8), 1 - 1e-8))              (the clamp of `distance`)
    D[0, 0] = e[0, 0];  D[0, n > 0] = -inf
    D[t, n] = e[t, n] + max(D[t-1, n], D[t-1, n-1])                    (fp32, added in order of t)

The path advances to the next phoneme only if D[t-1, n-1] > D[t-1, n]; a tie stays.  total = D[T-1, N-1], and the
trace-back from (T-1, N-1) gives

    starts (N + 1,) int32   starts[n] is the first frame of phoneme n; starts[0] = 0, starts[N] = T, strictly increasing
    score  (N,) fp32        the mean of e[t, n] over the phoneme's frames, summed in frame order
    gop    (N,) fp32        the mean over those frames of e[t, n] - max_q logf(clamp(P[q, t])): <= 0, and exactly 0
                            where the target is every frame's most likely phoneme (goodness of pronunciation)

Repeated adjacent phonemes are legal; their boundary is decided by the tie rule and the data.  Without `optional`
every phoneme of the sequence gets at least one frame.

    alignment = ppgs_amd.alignment.forced(ppg, ['hh', 'ah', 'l', 'ow'])
    for name, start, end, score, gop in ppgs_amd.alignment.segments(alignment): ...
    free = ppgs_amd.alignment.decode(ppg)            # what the PPG says by itself: runs of the per-frame argmax

Recognition (`recognize`, ppg_recognize): what was said, under a transition model.  `decode` is the per-frame argmax
cut into runs, and one frame that flips to a neighbouring vowel splits a phoneme into three; `recognize` finds the best
path through the 40 phonemes given transitions A (40, 40) -- A[p, q] weighs going from p to q, the diagonal staying --
and weights `initial` and `final` (40,) on the first and the last frame's phoneme, every entry finite or -inf:

    e[t, q] = the log-posterior above, of phoneme q itself
    D[0, q] = e[0, q] + initial[q]
    c[p]    = D[t-1, p] + A[p, q]                                one fp32 addition per candidate
    best = c[q], from = q;  for p = 0 .. 39, p != q:  if c[p] > best: best = c[p], from = p
    D[t, q] = e[t, q] + best                                     fp32, in order of t
    F[q] = D[T-1, q] + final[q];  last = the first q with the largest F;  total = F[last]

Comparisons only: on ties staying beats switching and the lowest predecessor wins.  The trace-back from `last` labels
every frame; the result is the runs of those labels with `forced`'s score and gop per run, up to 262144 frames.  `forced`
and `decode` are the two corners of it: under `chain(s)`, the left-to-right topology of a transcript of distinct
phonemes, it is `forced(ppg, s)` bit for bit, and with A = 0 it is `decode` wherever every frame's winner is clear.

    said = ppgs_amd.alignment.recognize(ppg, penalty=4.)                     # a switch has to pay for itself
    A, initial, final = ppgs_amd.alignment.bigram(lexicon_sequences)         # or a phone bigram
    said = ppgs_amd.alignment.recognize(ppg, transitions=A, initial=initial, final=final)
    for name, start, end, score, gop in ppgs_amd.alignment.segments(said): ...

Graphs (`viterbi`, ppg_viterbi): `forced` takes one sequence and `recognize` the 40 phonemes themselves; pronunciation
variants ("either" is iy dh er or ay dh er), substitution networks, a loop over the words of a lexicon and a chain with
a phoneme twice are all the best path through a graph whose states each carry a phoneme.  A Graph has S <= 1024 states;
state n has a phoneme sym[n], a weight stay[n], an ordered list of at most 255 in-arcs (src[j], w[j]) and weights
initial[n] and final[n], every weight finite or -inf:

    e[t, n] = the log-posterior above, of phoneme sym[n]
    D[0, n] = e[0, n] + initial[n]
    best = D[t-1, n] + stay[n], from = 0
    for j in list order:  c = D[t-1, src[j]] + w[j];  if c > best: best = c, from = j + 1
    D[t, n] = e[t, n] + best                                     fp32, one addition per candidate, in order of t
    F[n] = D[T-1, n] + final[n];  last = the first n with the largest F;  total = F[last]

Comparisons only: staying wins ties, then the arc listed first.  The trace-back from `last` gives a state per frame; a
run opens at frame 0 and wherever `from` != 0, so an arc n -> n opens a second run of n.  The result is a Path: per run
its state, its phoneme, its first frame, and `forced`'s score and gop.  `forced`, `forced(optional=)` and `recognize`
are special graphs (`chain_graph`, `model_graph`) and `viterbi` equals them bit for bit there.

    graph, word_of, variant_of = ppgs_amd.alignment.pronunciations([[['dh', 'ah'], ['dh', 'iy']], [['k', 'ae', 't']]])
    path = ppgs_amd.alignment.viterbi(ppg, graph)
    said = [variant_of[n] for n in path.states.tolist()]                       # which variant each run belongs to
    graph, word_of = ppgs_amd.alignment.word_loop({'yes': [['y', 'eh', 's']], 'no': [['n', 'ow']]}, penalty=2.)
Not here: states that emit nothing, N-best lists, minimum durations, more than 1024 states.  The live form is
`ViterbiStream` (ppg_viterbi_stream_*): `RecognizeStream`'s rules with a state of the graph in the place of a phoneme.

Posterior decoding (`posterior`, ppg_posterior): `viterbi` says which single path is best; `posterior` sums over ALL
paths of the same graph (forward-backward) and so says how sure that is.  With LSE = log sum exp:

    alpha[0, n] = e[0, n] + initial[n];  alpha[t, n] = e[t, n] + LSE(alpha[t-1, n] + stay[n], alpha[t-1, src[j]] + w[j])
    total = LSE over n of (alpha[T-1, n] + final[n])                  the log-likelihood of the graph, float64
    beta[T-1, n] = final[n];  beta[t, n] = LSE(stay[n] + e[t+1, n] + beta[t+1, n], w + e[t+1, m] + beta[t+1, m], n -> m)
    gamma[t, n] = exp(alpha[t, n] + beta[t, n] - Z_t), Z_t = LSE over n: the probability of state n at frame t
    phonemes[p, t] = the sum of gamma[t, n] over the states with sym[n] = p

fp32 in the log domain with every row shifted by its maximum and the shifts added up in float64; up to 65536 frames.
`phonemes` is a PPG in the library's own layout, cleaned by the transcript or the lexicon of the graph.

    graph, word_of = ppgs_amd.alignment.word_loop(lexicon, penalty=2.)
    path = ppgs_amd.alignment.viterbi(ppg, graph)
    posterior = ppgs_amd.alignment.posterior(ppg, graph, states=True)
    sure = ppgs_amd.alignment.run_confidence(path, posterior)                # one number in [0, 1] per run of the path
Not here: training losses or gradients.  The live form is `PosteriorStream` (ppg_posterior_stream_*): the forward pass
carried across pushes, and every block of `block` frames given out once `lag` more frames have been received, smoothed
by a backward pass from that horizon with an open end: block k = frames [kH, (k+1)H) is columns [kH, (k+1)H) of
`posterior(ppg[:, :(k+1)H + L], the graph with final = 0)`, bit for bit, whatever the pushes were.

Optional phonemes (`forced(..., optional=flags)`, ppg_align_optional): a speaker pauses between words wherever they
like, and drops a final consonant or a schwa.  flags[n] lets the path leave phoneme n out:

    state -1, a virtual origin, holds 0 before frame 0; every real state holds -inf
    D[t, n] = e[t, n] + the best of   stay D[t-1, n],   advance D[t-1, n-1],   skip D[t-1, n-2] if flags[n-1]

taken in that order by strict comparisons, so stay beats advance beats skip on ties.  The end is state N-1, or N-2
if flags[N-1] and D[T-1, N-2] > D[T-1, N-1].  A phoneme that was left out has starts[n] == starts[n+1] (starts is
non-decreasing then) and NaN for its score and gop; the others are scored as before.  No two adjacent phonemes may be
optional, at least one must be mandatory, and the mandatory ones must fit the frames; N may exceed T within that.
With every flag False the results are those of the plain alignment bit for bit.

    phonemes, optional, word_of = ppgs_amd.alignment.transcript([['hh', 'ah'], ['l', 'ow']])   # <silent> around words
    alignment = ppgs_amd.alignment.forced(ppg, phonemes, optional=optional)
    for word, start, end, gop in ppgs_amd.alignment.word_segments(alignment, word_of): ...

Phrase search (`search`, ppg_search): where in a recording is a phoneme sequence said, and how well?  `forced` pins
its transcript to frame 0 and frame T-1 and stops at 4096 frames; `search` lets the match start and end anywhere in up
to 262144 frames.  For a recording P (40, T) and a query s of 1 <= N <= 256 phonemes:

    r[t, n] = logp[t][s[n]] - max_q logp[t][q]     the GOP term of `forced`: <= 0, exactly 0 at the frame's maximum
    before frame 0 every state holds -inf
    D[t, 0] = r[t, 0] + (0 > D[t-1, 0] ? 0 : D[t-1, 0])      a fresh start, b[t, 0] = t, only if strictly better
    D[t, n] = r[t, n] + max(D[t-1, n], D[t-1, n-1])           advance only if D[t-1, n-1] > D[t-1, n]; b follows the path

The curve is, per end frame t, curve_total[t] = D[t, N-1] and curve_begin[t] = b[t, N-1] (-inf and -1 for t < N-1): the
best match ending at t covers frames curve_begin[t] .. t, and mean[t] = curve_total[t] / (t - curve_begin[t] + 1).  Hits
are taken in at most `top` rounds: of the end frames whose span meets no hit already taken, the largest mean, ties to
the largest t; the rounds stop when nothing is left or the best mean < threshold.  A hit is (begin, end = t + 1, total,
mean); hits are disjoint and listed in the order taken.  Entries past `count` are -1, -1, NaN, NaN.

    hits = ppgs_amd.alignment.search(ppg, ['hh', 'ah', 'l', 'ow'], top=5, threshold=-1.)
    for start, end, total, mean in ppgs_amd.alignment.hit_segments(hits): ...
    b, e = int(hits.begin[0]), int(hits.end[0])
    inside = ppgs_amd.alignment.forced(ppg[:, b:e], ['hh', 'ah', 'l', 'ow'])     # the phoneme boundaries inside a hit

Phrase search over a graph (`search_graph`, ppg_search_graph): a real keyword is not one chain.  "either" has two
pronunciations, a phrase of several words may or may not have a pause between them, and a final consonant may be
dropped.  `search_graph` takes a Graph of at most 256 states and 4096 arcs as the query, with a free start and a free
end.  Every state carries D and a begin b; before frame 0 every D is -inf, and for every t >= 0:

    r[t, n] = logp[t][sym[n]] - max_q logp[t][q]                       the emission of `search`
    best = D[t-1, n] + stay[n], bb = b[t-1, n]
    for j in list order:  c = D[t-1, src[j]] + w[j];  if c > best: best = c, bb = b[t-1, src[j]]
    if initial[n] > best: best = initial[n], bb = t                    a fresh start: last, and only if strictly better
    D[t, n] = r[t, n] + best;  b[t, n] = bb                            fp32, one addition per candidate, in order of t

curve_total[t] is the largest D[t, n] + final[n] (the lowest n on ties), curve_begin[t] that state's b, -1 where the
total is -inf; the hits are picked as `search` picks them.  `search_graph(ppg, chain_graph(s))` is `search(ppg, s)` bit
for bit.  The path and the variants inside a hit are `viterbi(ppg[:, b:e], graph)`: the two emissions differ by the
frame's maximum, which no path through a fixed span can change.

    graph, word_of, variant_of = ppgs_amd.alignment.phrase_graph([[['iy', 'dh', 'er'], ['ay', 'dh', 'er']], [['w', 'ey']]])
    hits = ppgs_amd.alignment.search_graph(ppg, graph, top=5, threshold=-1.)
    b, e = int(hits.begin[0]), int(hits.end[0])
    said = [variant_of[n] for n in ppgs_amd.alignment.viterbi(ppg[:, b:e], graph).states.tolist()]
Not here: graphs over 256 states (a word loop belongs to `viterbi`).

Live phrase search (`SearchStream`, ppg_search_stream_*): the same curve carried across the pushes of a stream, bit for
bit whatever the push sizes, with an online rule that gives a hit out once nothing later can overlap and beat it.

    spotter = ppgs_amd.alignment.SearchStream(['hh', 'ah', 'l', 'ow'], threshold=-1., patience=25)
    hits = spotter.push(frames)          # (40, k) as a stream emits them, k >= 0; Hits of this push
    last = spotter.flush()

Live phrase search over a graph (`SearchGraphStream`, ppg_search_graph_stream_*): `search_graph`'s curve carried across
the pushes in the same way (a fresh start at frame t of a push at position p begins at p + t), under the same online
rule; on `chain_graph(s)` every output is `SearchStream(s)`'s bit for bit.

    spotter = ppgs_amd.alignment.SearchGraphStream(graph, threshold=-1.)
    hits = spotter.push(frames)          # GraphHits of this push

Live phoneme recognition (`RecognizeStream`, ppg_recognize_stream_*): `recognize` carried across the pushes of a stream.
One stream has a position p, the frames received since the last reset (frame indices are absolute); a commit point c,
0 <= c <= p: frames below c have had their label given out for good; D[0 .. 39] of frame p-1; a ring of `window` = W
frames that holds the back-pointers and the prepared frames (the 40 log-posteriors and their maximum) of the frames in
[c, p); one open run (label, start frame, fp32 sum and below); and a counter `forced`.

    Forward.  The recurrence of `recognize`, unchanged: the same prepared frame, D[0, q] = e[0, q] + initial[q] at
    absolute frame 0, one fp32 addition per candidate, staying first, then ascending p with strict >, D[t, q] =
    e[t, q] + best.  For any split of a recording into pushes, D and the back-pointers of every frame are the bits
    `recognize` computes for the whole recording: it is one body of code.
    Commit, once per stream and push, after the push's frames, with t = p-1.  alive(q) means D[q] > -inf; path(q, u)
    is the state at frame u of the trace-back from q at t.
      1. Natural.  v = the largest u in [c, t] at which path(q, u) is the same for every alive q; if there is none,
         v = c-1.  Frames c .. v get that path's labels and c = v+1.  If no state is alive nothing is committed, now or
         later.  Whatever comes later, the best path ends in a state that is alive now, so these labels are final; c
         after a push depends only on the frames received so far, not on how they were split.
      2. Forced (max_lag = L, 0 <= L < W), only if p - c > L after step 1.  best = the first alive q with the largest
         D[q] (strict >, ascending, no `final`).  Frames c .. p-L-1 get path(best, .); with g = path(best, p-L-1),
         every q with path(q, p-L-1) != g gets D[q] = -inf, so the later path stays consistent with what was given
         out; `forced` grows by the number of frames committed this way and c = p-L.  A forced commit depends on
         where pushes end; natural commits do not.
      3. Runs.  Each newly committed frame, in order, either extends the open run (sum += e[t, label], below +=
         e[t, label] - max[t], fp32, from 0.f: the order of `forced`'s score) or closes it and opens a new one.  A
         closed run is emitted as (phoneme, begin, end, sum / float(end - begin), below / float(end - begin)).
    A stream with (p - c) + its frames > W cannot take them: count = -1 and its state stays untouched (the check is
    made on the device; the host does not know c).  flush(final): F[q] = D[q] + final[q]; last = the first q with the
    largest F; total = F[last]; if total > -inf everything up to p is committed along path(last, .); the open run is
    closed and emitted, total and forced are reported, and the stream is reset: a flush ends an utterance.  reset puts
    p = c = 0, every D to -inf, no open run and forced = 0.
    If forced == 0 and `recognize` finds a path, the runs of all pushes and of the flush, concatenated, are
    `recognize(recording, ...)`'s phonemes, starts, score and gop, and flush's total is its total, bit for bit, for every
    split, pushes of 0 and 1 frames included.
Not here: a provisional hypothesis for the uncommitted tail, N-best lists, a matrix per stream, state spaces beyond the
40 phonemes.

    said = ppgs_amd.alignment.RecognizeStream(penalty=4.)
    runs = said.push(frames)             # (40, k) as a stream emits them, k >= 0; Runs this push has made final
    for name, start, end, score, gop in ppgs_amd.alignment.run_segments(runs): ...
    last = said.flush()                  # the rest, with total and forced; the stream starts again at frame 0
"""
import collections
import math

import torch

from . import config, core, engine
from .phonemes import PHONEMES, PHONEME_TO_INDEX_MAPPING

MAX_FRAMES = engine.ALIGN_MAX_FRAMES
MAX_PHONEMES = engine.ALIGN_MAX_PHONEMES
RECOGNIZE_MAX_FRAMES = engine.RECOGNIZE_MAX_FRAMES
SEARCH_MAX_FRAMES = engine.SEARCH_MAX_FRAMES
SEARCH_MAX_PHONEMES = engine.SEARCH_MAX_PHONEMES
SEARCH_MAX_HITS = engine.SEARCH_MAX_HITS
SEARCH_GRAPH_MAX_STATES = engine.SEARCH_GRAPH_MAX_STATES
SEARCH_GRAPH_MAX_ARCS = engine.SEARCH_GRAPH_MAX_ARCS
SEARCH_GRAPH_MAX_GRAPHS = engine.SEARCH_GRAPH_MAX_GRAPHS
VITERBI_MAX_FRAMES = engine.VITERBI_MAX_FRAMES
VITERBI_MAX_STATES = engine.VITERBI_MAX_STATES
VITERBI_MAX_ARCS = engine.VITERBI_MAX_ARCS
VITERBI_MAX_DEGREE = engine.VITERBI_MAX_DEGREE
POSTERIOR_MAX_FRAMES = engine.POSTERIOR_MAX_FRAMES
EDIT_MAX_TOKENS = engine.EDIT_MAX_TOKENS

Alignment = collections.namedtuple('Alignment', ['phonemes', 'starts', 'total', 'score', 'gop'])
Decoding = collections.namedtuple('Decoding', ['phonemes', 'starts'])
Recognition = collections.namedtuple('Recognition', Alignment._fields)
Graph = collections.namedtuple('Graph', ['phonemes', 'stay', 'offsets', 'sources', 'weights', 'initial', 'final'])
Path = collections.namedtuple('Path', ['states', 'phonemes', 'starts', 'total', 'score', 'gop'])
Hits = collections.namedtuple('Hits', ['phonemes', 'begin', 'end', 'total', 'mean', 'count', 'curve'])
GraphHits = collections.namedtuple('GraphHits', ['begin', 'end', 'total', 'mean', 'count', 'curve'])
Runs = collections.namedtuple('Runs', ['phonemes', 'begin', 'end', 'score', 'gop', 'count', 'total', 'forced'])
Posterior = collections.namedtuple('Posterior', ['total', 'phonemes', 'states'])
StateRuns = collections.namedtuple('StateRuns', ('states',) + Runs._fields)
EditDistance = collections.namedtuple('EditDistance', ['total', 'hits', 'substitutions', 'deletions', 'insertions', 'ops'])
PosteriorFrames = collections.namedtuple('PosteriorFrames', ['phonemes', 'states', 'begin', 'count', 'evidence', 'total'])


def _ppg(ppg, most=MAX_FRAMES, what='alignment'):
    """Shape checks of a PPG or a batch of them: (batched, batch, frames)."""
    if not torch.is_tensor(ppg) or ppg.dim() not in (2, 3):
        raise ValueError(f'PPG must be (40, frames) or (batch, 40, frames), got {tuple(getattr(ppg, "shape", ()))}')
    if ppg.shape[-2] != config.OUTPUT_CHANNELS:
        raise ValueError(f'PPG must have {config.OUTPUT_CHANNELS} channels, got {tuple(ppg.shape)}')
    batched = ppg.dim() == 3
    if batched and ppg.shape[0] < 1:
        raise ValueError('empty batch')
    frames = ppg.shape[-1]
    if frames < 1:
        raise ValueError(f'PPG must have at least one frame, got {tuple(ppg.shape)}')
    if frames > most:
        raise ValueError(f'{what} takes at most {most} frames, got {frames}')
    return batched, ppg.shape[0] if batched else 1, frames


def _lengths(lengths, batch, frames):
    if lengths is None:
        return [frames] * batch
    if torch.is_tensor(lengths):
        lengths = lengths.detach().cpu().reshape(-1).tolist()
    elif isinstance(lengths, int):
        lengths = [lengths]
    lengths = [int(v) for v in lengths]
    if len(lengths) != batch:
        raise ValueError(f'lengths has {len(lengths)} entries for a batch of {batch}')
    for value in lengths:
        if not 1 <= value <= frames:
            raise ValueError(f'lengths: {value} is outside [1, {frames}]')
    return lengths


def _sequence(phonemes):
    """One phoneme sequence, as names or indices, as a list of checked indices."""
    if torch.is_tensor(phonemes):
        if phonemes.dim() != 1 or phonemes.is_floating_point() or phonemes.is_complex() or phonemes.dtype == torch.bool:
            raise ValueError(f'a phoneme sequence must be a one-dimensional integer tensor, got {tuple(phonemes.shape)} '
                             f'{phonemes.dtype}')
        phonemes = phonemes.detach().cpu().tolist()
    if isinstance(phonemes, (str, bytes)) or not isinstance(phonemes, (list, tuple)):
        raise ValueError(f'a phoneme sequence must be a list of names or indices, got {type(phonemes).__name__}')
    out = []
    for value in phonemes:
        if isinstance(value, str):
            if value not in PHONEME_TO_INDEX_MAPPING:
                raise ValueError(f'unknown phoneme {value!r}: the names are ppgs_amd.PHONEMES')
            value = PHONEME_TO_INDEX_MAPPING[value]
        elif isinstance(value, bool) or not isinstance(value, int):
            raise ValueError(f'a phoneme must be a name or an index, got {value!r}')
        if not 0 <= value < len(PHONEMES):
            raise ValueError(f'phoneme index {value} is outside [0, {len(PHONEMES) - 1}]')
        out.append(value)
    return out


def _sequences(phonemes, phoneme_lengths, batched, batch, lengths, fit=True):
    """The transcripts of a call as a list of index lists, one per item, each within its item's frames (`fit`)."""
    if not batched:
        if phoneme_lengths is not None:
            raise ValueError('phoneme_lengths go with a batch: slice a single sequence instead')
        sequences = [_sequence(phonemes)]
    elif torch.is_tensor(phonemes) and phonemes.dim() == 2:
        if phonemes.shape[0] != batch:
            raise ValueError(f'phonemes has {phonemes.shape[0]} rows for a batch of {batch}')
        if phonemes.is_floating_point() or phonemes.is_complex() or phonemes.dtype == torch.bool:
            raise ValueError(f'a phoneme table must be an integer tensor, got {phonemes.dtype}')
        if phoneme_lengths is None:
            counts = [phonemes.shape[1]] * batch
        else:
            if torch.is_tensor(phoneme_lengths):
                phoneme_lengths = phoneme_lengths.detach().cpu().reshape(-1).tolist()
            counts = [int(v) for v in phoneme_lengths]
            if len(counts) != batch:
                raise ValueError(f'phoneme_lengths has {len(counts)} entries for a batch of {batch}')
            for value in counts:
                if not 0 <= value <= phonemes.shape[1]:
                    raise ValueError(f'phoneme_lengths: {value} is outside [1, {phonemes.shape[1]}]')
        # one copy to the host and one comparison for the whole table, not one per row
        host = phonemes.detach().cpu().to(torch.int64)
        used = torch.arange(host.shape[1])[None, :] < torch.tensor(counts)[:, None]
        if bool(((host < 0) | (host >= len(PHONEMES)))[used].any()):
            raise ValueError(f'a phoneme index is outside [0, {len(PHONEMES) - 1}]')
        sequences = [row[:count] for row, count in zip(host.tolist(), counts)]
    else:
        if phoneme_lengths is not None:
            raise ValueError('phoneme_lengths go with a padded (batch, N) tensor of phonemes')
        if isinstance(phonemes, (str, bytes)) or not isinstance(phonemes, (list, tuple)) or len(phonemes) != batch:
            raise ValueError(f'a batch of {batch} takes a list of {batch} phoneme sequences or a (batch, N) tensor')
        sequences = [_sequence(item) for item in phonemes]
    for sequence, frames in zip(sequences, lengths):
        if len(sequence) < 1:
            raise ValueError('an empty phoneme sequence cannot be aligned')
        if len(sequence) > MAX_PHONEMES:
            raise ValueError(f'alignment takes at most {MAX_PHONEMES} phonemes, got {len(sequence)}')
        if fit and len(sequence) > frames:
            raise ValueError(f'{len(sequence)} phonemes do not fit {frames} frames: every phoneme takes a frame')
    return sequences


def _flags(optional, sequences, batched, lengths):
    """The `optional` of a call as a list of bool lists, one per item, each a legal companion of its transcript."""
    if torch.is_tensor(optional):
        if optional.is_floating_point() or optional.is_complex() or optional.dim() != (2 if batched else 1):
            raise ValueError(f'optional must be a bool or integer tensor with the shape of the phonemes, got '
                             f'{tuple(optional.shape)} {optional.dtype}')
        rows = optional.detach().cpu().tolist()
        rows = rows if batched else [rows]
        if len(rows) != len(sequences):
            raise ValueError(f'optional has {len(rows)} rows for a batch of {len(sequences)}')
        for row, sequence in zip(rows, sequences):
            if len(row) < len(sequence):
                raise ValueError(f'optional has {len(row)} flags for {len(sequence)} phonemes')
        # (a padded table's entries past an item's own phonemes are padding, as in the phoneme table)
        rows = [row[:len(sequence)] if batched else row for row, sequence in zip(rows, sequences)]
    else:
        if not isinstance(optional, (list, tuple)):
            raise ValueError(f'optional must be a list of bools per sequence, got {type(optional).__name__}')
        rows = list(optional) if batched else [optional]
        if len(rows) != len(sequences):
            raise ValueError(f'optional has {len(rows)} entries for a batch of {len(sequences)}')
        for row in rows:
            if torch.is_tensor(row):
                if row.dim() != 1 or row.is_floating_point() or row.is_complex():
                    raise ValueError('the optional flags of a sequence must be one-dimensional bools or integers')
            elif not isinstance(row, (list, tuple)):
                raise ValueError(f'the optional flags of a sequence must be a list of bools, got {type(row).__name__}')
        rows = [row.detach().cpu().tolist() if torch.is_tensor(row) else list(row) for row in rows]
    out = []
    for row, sequence, frames in zip(rows, sequences, lengths):
        if len(row) != len(sequence):
            raise ValueError(f'optional has {len(row)} flags for {len(sequence)} phonemes')
        for value in row:
            if not isinstance(value, (bool, int)):
                raise ValueError(f'an optional flag must be a bool, got {value!r}')
        row = [bool(value) for value in row]
        if any(a and b for a, b in zip(row, row[1:])):
            raise ValueError('two adjacent phonemes are optional: a skip passes over one phoneme only')
        mandatory = row.count(False)
        if mandatory < 1:
            raise ValueError('every phoneme is optional: at least one must be mandatory')
        if mandatory > frames:
            raise ValueError(f'{mandatory} mandatory phonemes do not fit {frames} frames: each takes a frame')
        out.append(row)
    return out


def forced(ppg, phonemes, lengths=None, phoneme_lengths=None, gop=True, optional=None):
    """Align `ppg` to the phonemes the speaker was meant to say: Alignment(phonemes, starts, total, score, gop).

    `ppg` is (40, T) with `phonemes` a list of names from `ppgs_amd.PHONEMES` or of indices, or an integer tensor; or a
    batch (B, 40, T) padded to the longest item with `lengths` per item (the padding is never read) and `phonemes` a
    list of B such sequences, or a padded (B, Nmax) integer tensor with `phoneme_lengths`.  One utterance returns
    device tensors: phonemes (N,) int32, starts (N + 1,) int32, total 0-d, score and gop (N,) fp32.  A batch returns
    lists of B such tensors for the ragged fields and total (B,).  gop=False skips that sum and returns None for it.
    A batch equals its single calls bit for bit.

    `optional` marks phonemes the speaker may leave out (see the module's text): a list of bools per sequence, for a
    batch a list of such lists or a (B, Nmax) bool or integer tensor.  A phoneme that was left out has
    starts[n] == starts[n + 1] and NaN for its score and gop.  A sequence may then be longer than its frames, as long
    as its mandatory phonemes fit.  With None the call is the plain alignment."""
    batched, batch, frames = _ppg(ppg)
    if not batched and lengths is not None:
        raise ValueError('lengths go with a batch: slice a single PPG instead')
    lengths = _lengths(lengths, batch, frames)
    sequences = _sequences(phonemes, phoneme_lengths, batched, batch, lengths, fit=optional is None)
    counts = [len(sequence) for sequence in sequences]
    most = max(counts)
    flags = None
    if optional is not None:
        flags = _flags(optional, sequences, batched, lengths)
        flags = torch.tensor([row + [False] * (most - len(row)) for row in flags], dtype=torch.int32)
    device = core.device_for(None, ppg)
    table = torch.tensor([sequence + [-1] * (most - len(sequence)) for sequence in sequences], dtype=torch.int32)
    table = table.to(device)
    x = ppg.to(device)
    total, starts, score, below = engine.align_items(x if batched else x[None], lengths, table, counts, gop,
                                                     optional=None if flags is None else flags.to(device))
    if not batched:
        return Alignment(table[0], starts[0], total[0], score[0], below[0] if gop else None)
    return Alignment(
        [table[b, :n] for b, n in enumerate(counts)], [starts[b, :n + 1] for b, n in enumerate(counts)], total,
        [score[b, :n] for b, n in enumerate(counts)], [below[b, :n] for b, n in enumerate(counts)] if gop else None)


def transcript(words, silence=True):
    """A transcript of words for `forced`: (phonemes, optional, word_of), three lists of one length.

    `words` is a list of words, each a non-empty list of phoneme names (or indices).  With `silence` an optional
    '<silent>' stands before the first word, between words and after the last: the pauses a speaker may or may not
    make.  phonemes holds names, optional the flags for `forced(..., optional=)`, and word_of[n] the index in `words`
    of the word phoneme n belongs to, -1 for the inserted silences.  Host only."""
    if isinstance(words, (str, bytes)) or not isinstance(words, (list, tuple)) or len(words) < 1:
        raise ValueError('a transcript takes a non-empty list of words, each a list of phonemes')
    phonemes, optional, word_of = [], [], []

    def pause():
        phonemes.append('<silent>')
        optional.append(True)
        word_of.append(-1)
    for index, word in enumerate(words):
        names = [PHONEMES[value] for value in _sequence(word)]
        if not names:
            raise ValueError(f'word {index} has no phonemes')
        if silence:
            pause()
        phonemes.extend(names)
        optional.extend([False] * len(names))
        word_of.extend([index] * len(names))
    if silence:
        pause()
    return phonemes, optional, word_of


def word_segments(alignment, word_of, sample_rate=config.SAMPLE_RATE, hopsize=config.HOPSIZE):
    """The words of an alignment of one utterance as a host list of (word index, start seconds, end seconds, gop), one
    per word of `word_of` (as `transcript` returns it; phonemes with -1 belong to no word).  A word lasts from the
    start of its first phoneme to the end of its last; its gop is the mean of its present phonemes' gop (those that
    were given frames), NaN if none is present, None if the alignment has no gop.  A batch (lists in the alignment)
    takes a list of `word_of` lists and gives a list of such lists.  Host only."""
    phonemes, starts, gop = alignment.phonemes, alignment.starts, getattr(alignment, 'gop', None)
    if isinstance(phonemes, (list, tuple)):
        if not isinstance(word_of, (list, tuple)) or len(word_of) != len(phonemes):
            raise ValueError(f'a batch of {len(phonemes)} alignments takes {len(phonemes)} word_of lists')
        return [word_segments(Alignment(phonemes[b], starts[b], None, None, None if gop is None else gop[b]),
                              word_of[b], sample_rate, hopsize) for b in range(len(phonemes))]
    frames = starts.tolist()
    word_of = [int(value) for value in word_of]
    if len(frames) != len(word_of) + 1 or len(word_of) != phonemes.shape[0]:
        raise ValueError(f'{phonemes.shape[0]} phonemes take as many word_of entries and one more start, got '
                         f'{len(word_of)} and {len(frames)}')
    values = None if gop is None else gop.tolist()
    out = []
    for index in sorted(set(word_of) - {-1}):
        if index < 0:
            raise ValueError(f'word_of: {index} is neither a word index nor -1')
        members = [n for n, value in enumerate(word_of) if value == index]
        if members != list(range(members[0], members[-1] + 1)):
            raise ValueError(f'the phonemes of word {index} are not adjacent')
        mean = None
        if values is not None:
            present = [values[n] for n in members if frames[n] < frames[n + 1]]
            mean = sum(present) / len(present) if present else math.nan
        out.append((index, frames[members[0]] * hopsize / sample_rate, frames[members[-1] + 1] * hopsize / sample_rate,
                    mean))
    return out


def decode(ppg, lengths=None):
    """What the PPG says by itself: Decoding(phonemes, starts), the runs of the per-frame most likely phoneme (the
    lowest index on ties, as torch.argmax) -- `torch.unique_consecutive(ppg.argmax(0))` with the runs' first frames.

    (40, T) returns device tensors phonemes (R,) int32 and starts (R + 1,) int32 with starts[R] = T; a batch
    (B, 40, T) with `lengths` returns lists of B such tensors.  `forced(ppg, decode(ppg).phonemes)` reproduces these
    starts wherever every frame's best phoneme is clear of the others."""
    batched, batch, frames = _ppg(ppg)
    if not batched and lengths is not None:
        raise ValueError('lengths go with a batch: slice a single PPG instead')
    lengths = _lengths(lengths, batch, frames)
    device = core.device_for(None, ppg)
    x = ppg.to(device)
    phonemes, starts, runs = engine.decode_items(x if batched else x[None], lengths)
    runs = runs.tolist()
    if not batched:
        return Decoding(phonemes[0, :runs[0]], starts[0, :runs[0] + 1])
    return Decoding([phonemes[b, :r] for b, r in enumerate(runs)], [starts[b, :r + 1] for b, r in enumerate(runs)])


def switch_penalty(penalty):
    """The simplest transition model: (40, 40) fp32, 0 for staying in a phoneme and -penalty for every switch.
    `penalty` >= 0 and finite; in units of log-posterior, it is what a phoneme has to gain over its run's frames to be
    worth two switches.  Host only."""
    if isinstance(penalty, bool) or not isinstance(penalty, (int, float)) or not 0 <= penalty < math.inf:
        raise ValueError(f'a switch penalty must be a finite number >= 0, got {penalty!r}')
    count = len(PHONEMES)
    matrix = torch.full((count, count), -float(penalty), dtype=torch.float32)
    matrix.fill_diagonal_(0.)
    return matrix


def bigram(sequences, smoothing=1.0, scale=1.0):
    """A phone bigram from phoneme sequences (names or indices, e.g. what `decode` or a lexicon gives):
    (transitions (40, 40), initial (40,), final (40,)), fp32.  With count[p, q] the number of times q follows p in a
    sequence, row p of transitions holds scale * log((count[p, q] + smoothing) / (sum_q count[p, q] + 40 * smoothing));
    initial and final are the same from the counts of first and of last phonemes.  smoothing = 0 gives -inf for what
    was never seen; a row without counts is then an error.  Computed in float64, rounded once.  Host only."""
    for name, value in (('smoothing', smoothing), ('scale', scale)):
        if isinstance(value, bool) or not isinstance(value, (int, float)) or not 0 <= value < math.inf:
            raise ValueError(f'{name} must be a finite number >= 0, got {value!r}')
    if scale == 0:
        raise ValueError('scale must be positive: 0 would weigh nothing (and 0 * -inf is NaN)')
    if isinstance(sequences, (str, bytes)) or not isinstance(sequences, (list, tuple)) or len(sequences) < 1:
        raise ValueError('a bigram takes a non-empty list of phoneme sequences')
    count = len(PHONEMES)
    pairs = torch.zeros((count, count), dtype=torch.float64)
    first, last = torch.zeros(count, dtype=torch.float64), torch.zeros(count, dtype=torch.float64)
    for sequence in sequences:
        sequence = _sequence(sequence)
        if not sequence:
            raise ValueError('an empty phoneme sequence has no first or last phoneme')
        first[sequence[0]] += 1
        last[sequence[-1]] += 1
        for p, q in zip(sequence, sequence[1:]):
            pairs[p, q] += 1

    def weights(counts, what):
        sums = counts.sum(-1, keepdim=True) + count * smoothing
        if bool((sums == 0).any()):
            empty = [PHONEMES[p] for p in torch.nonzero(sums.reshape(-1) == 0).reshape(-1).tolist()]
            raise ValueError(f'{what} without counts and without smoothing: ' +
                             (', '.join(empty) if counts.dim() == 2 else 'no sequences'))
        return (scale * torch.log((counts + smoothing) / sums)).to(torch.float32)
    return weights(pairs, 'rows'), weights(first, 'first phonemes'), weights(last, 'last phonemes')


def chain(phonemes):
    """The left-to-right topology over a sequence s of N distinct phonemes: (transitions, initial, final) with
    transitions[s[n], s[n]] = transitions[s[n], s[n + 1]] = 0, initial[s[0]] = final[s[N - 1]] = 0 and -inf everywhere
    else.  `recognize` under it is `forced(ppg, s)` bit for bit: this is how the two relate (and the test of it).  A
    phoneme cannot come twice, for a state is a phoneme here.  Host only."""
    sequence = _sequence(phonemes)
    if not sequence:
        raise ValueError('a chain takes at least one phoneme')
    if len(set(sequence)) != len(sequence):
        raise ValueError('a chain takes distinct phonemes: a state of the recogniser is a phoneme, not a position')
    count = len(PHONEMES)
    transitions = torch.full((count, count), -math.inf, dtype=torch.float32)
    initial, final = torch.full((count,), -math.inf), torch.full((count,), -math.inf)
    for n, p in enumerate(sequence):
        transitions[p, p] = 0.
        if n + 1 < len(sequence):
            transitions[p, sequence[n + 1]] = 0.
    initial[sequence[0]] = 0.
    final[sequence[-1]] = 0.
    return transitions, initial, final


def _weights(tensor, shape, name):
    """A table of weights of `recognize`: fp32, every entry finite or -inf."""
    if not torch.is_tensor(tensor) or tuple(tensor.shape) != shape or tensor.is_complex() or tensor.dtype == torch.bool:
        raise ValueError(f'{name} must be a {shape} tensor of weights, got {tuple(getattr(tensor, "shape", ()))} '
                         f'{getattr(tensor, "dtype", type(tensor).__name__)}')
    tensor = tensor.detach().to(torch.float32)
    if bool((torch.isnan(tensor) | (tensor == math.inf)).any()):
        raise ValueError(f'{name} holds NaN or +inf: a weight is finite or -inf')
    return tensor


def recognize(ppg, lengths=None, transitions=None, initial=None, final=None, penalty=None, gop=True):
    """What was said, under a transition model: Recognition(phonemes, starts, total, score, gop), the runs of the best
    path through the 40 phonemes (see the module's text), where `decode` gives the runs of the per-frame argmax.

    `ppg` is (40, T) or a batch (B, 40, T) padded to the longest item with `lengths` per item (the padding is never
    read), up to 262144 frames.  `transitions` is a (40, 40) tensor on the CPU or the device: transitions[p, q] is the
    weight of going from p to q, the diagonal that of staying; `initial` and `final` (40,) weigh the first and the last
    frame's phoneme (None: zeros).  Every entry is finite or -inf.  `penalty=c` is shorthand for
    `transitions=switch_penalty(c)`; one of the two must be given, and only one.  One model serves the whole batch.
    One utterance returns device tensors: phonemes (R,) int32, starts (R + 1,) int32, total 0-d, score and gop (R,)
    fp32; a batch returns lists of B such tensors and total (B,), as `forced` does, and equals its single calls bit for
    bit.  gop=False skips that sum and returns None for it.  An utterance that no path fits (the model forbids every
    way through it) has no phonemes, starts = [0] and total = -inf.  `segments`, `frame_labels` and `word_segments`
    take the result as they take an Alignment."""
    batched, batch, frames = _ppg(ppg, RECOGNIZE_MAX_FRAMES, 'recognize')
    if not batched and lengths is not None:
        raise ValueError('lengths go with a batch: slice a single PPG instead')
    lengths = _lengths(lengths, batch, frames)
    if (transitions is None) == (penalty is None):
        raise ValueError('recognize takes either transitions or penalty: one of them, not both')
    if transitions is None:
        transitions = switch_penalty(penalty)
    count = len(PHONEMES)
    transitions = _weights(transitions, (count, count), 'transitions')
    initial = None if initial is None else _weights(initial, (count,), 'initial')
    final = None if final is None else _weights(final, (count,), 'final')
    device = core.device_for(None, ppg)
    x = ppg.to(device)
    phonemes, starts, runs, total, score, below = engine.recognize_items(
        x if batched else x[None], lengths, transitions.to(device), None if initial is None else initial.to(device),
        None if final is None else final.to(device), gop)
    runs = runs.tolist()
    if not batched:
        r = runs[0]
        return Recognition(phonemes[0, :r], starts[0, :r + 1], total[0], score[0, :r], below[0, :r] if gop else None)
    return Recognition(
        [phonemes[b, :r] for b, r in enumerate(runs)], [starts[b, :r + 1] for b, r in enumerate(runs)], total,
        [score[b, :r] for b, r in enumerate(runs)], [below[b, :r] for b, r in enumerate(runs)] if gop else None)


def _weight(value, what):
    """One weight of a graph as a float: finite or -inf."""
    if isinstance(value, bool) or not isinstance(value, (int, float)):
        raise ValueError(f'{what}: a weight must be a number, got {value!r}')
    value = float(value)
    if math.isnan(value) or value == math.inf:
        raise ValueError(f'{what}: a weight is finite or -inf, got {value}')
    return value


def _state_weights(values, count, default, name):
    """A weight per state from None (the default for all), one number (for all), or a list or tensor of `count`."""
    if values is None:
        return [default] * count
    if isinstance(values, (int, float)) and not isinstance(values, bool):
        return [_weight(values, name)] * count
    if torch.is_tensor(values):
        if values.dim() != 1 or values.is_complex() or values.dtype == torch.bool:
            raise ValueError(f'{name} must be a one-dimensional tensor of weights, got {tuple(values.shape)} '
                             f'{values.dtype}')
        values = values.detach().cpu().to(torch.float64).tolist()
    if not isinstance(values, (list, tuple)) or len(values) != count:
        raise ValueError(f'{name} must be a number or hold one weight per state ({count})')
    return [_weight(value, f'{name} of state {n}') for n, value in enumerate(values)]


def _assemble(symbols, stay, arcs_into, initial, final):
    """A Graph from checked host lists: arcs_into[n] is the ordered list of (source, weight) into state n."""
    count = len(symbols)
    if not 1 <= count <= VITERBI_MAX_STATES:
        raise ValueError(f'a graph has 1 to {VITERBI_MAX_STATES} states, got {count}')
    offsets = [0]
    for n, into in enumerate(arcs_into):
        if len(into) > VITERBI_MAX_DEGREE:
            raise ValueError(f'state {n} has {len(into)} arcs coming in, at most {VITERBI_MAX_DEGREE}: a back-pointer '
                             f'is one byte')
        offsets.append(offsets[-1] + len(into))
    if offsets[-1] > VITERBI_MAX_ARCS:
        raise ValueError(f'a graph has at most {VITERBI_MAX_ARCS} arcs, got {offsets[-1]}')
    return Graph(
        torch.tensor(symbols, dtype=torch.int32), torch.tensor(stay, dtype=torch.float32),
        torch.tensor(offsets, dtype=torch.int32),
        torch.tensor([source for into in arcs_into for source, _ in into], dtype=torch.int32),
        torch.tensor([weight for into in arcs_into for _, weight in into], dtype=torch.float32),
        torch.tensor(initial, dtype=torch.float32), torch.tensor(final, dtype=torch.float32))


def graph(phonemes, arcs, stay=0., initial=None, final=None):
    """A Graph for `viterbi` from its states and arcs.  State n carries phonemes[n] (names or indices, 1 to 1024 of
    them); `arcs` is a list of (source, target, weight): the path may go from `source` at one frame to `target` at the
    next for `weight`.  The arcs into a state keep their listed order, which decides ties (the module's text); at most
    255 may enter one state and a graph has at most 32768.  An arc n -> n is legal and opens a new run of n; parallel
    arcs are legal.  `stay`, `initial` and `final` are a number for every state or one weight per state (a list or a
    tensor); initial and final None weigh nothing: the path may begin and end in any state.  Every weight is finite or
    -inf.  Raises ValueError, naming the state, on everything the device would refuse.  Host only."""
    symbols = _sequence(phonemes)
    count = len(symbols)
    if not 1 <= count <= VITERBI_MAX_STATES:
        raise ValueError(f'a graph has 1 to {VITERBI_MAX_STATES} states, got {count}')
    if isinstance(arcs, (str, bytes)) or not isinstance(arcs, (list, tuple)):
        raise ValueError(f'arcs must be a list of (source, target, weight), got {type(arcs).__name__}')
    into = [[] for _ in range(count)]
    for index, arc in enumerate(arcs):
        if not isinstance(arc, (list, tuple)) or len(arc) != 3:
            raise ValueError(f'arc {index} must be (source, target, weight), got {arc!r}')
        source, target, weight = arc
        for name, state in (('source', source), ('target', target)):
            if isinstance(state, bool) or not isinstance(state, int) or not 0 <= state < count:
                raise ValueError(f'arc {index}: the {name} {state!r} is not a state in [0, {count - 1}]')
        into[target].append((source, _weight(weight, f'arc {index} into state {target}')))
    return _assemble(symbols, _state_weights(stay, count, 0., 'stay'), into,
                     _state_weights(initial, count, 0., 'initial'), _state_weights(final, count, 0., 'final'))


def chain_graph(phonemes, optional=None):
    """The left-to-right chain over a phoneme sequence s as a Graph, repeated phonemes allowed (a state is a position,
    not a phoneme): state n carries s[n], staying and advancing weigh 0, the path begins in state 0 and ends in state
    N - 1.  `viterbi` under it is `forced(ppg, s)` bit for bit.  With `optional` (flags as `forced` takes them for one
    sequence) it is the topology of `forced(ppg, s, optional=)`: state n takes the arcs advance (from n - 1), then skip
    (from n - 2 if flags[n - 1]); the path may also begin in state 1 if flags[0] and end in state N - 2 if
    flags[N - 1].  The states a path does not visit are the phonemes left out.  Host only."""
    symbols = _sequence(phonemes)
    count = len(symbols)
    if not 1 <= count <= VITERBI_MAX_STATES:
        raise ValueError(f'a chain takes 1 to {VITERBI_MAX_STATES} phonemes, got {count}')
    flags = [False] * count if optional is None else _flags(optional, [symbols], False, [count])[0]
    into = [[] for _ in range(count)]
    for n in range(1, count):
        into[n].append((n - 1, 0.))
        if n >= 2 and flags[n - 1]:
            into[n].append((n - 2, 0.))
    initial, final = [-math.inf] * count, [-math.inf] * count
    initial[0] = final[count - 1] = 0.
    if flags[0]:
        initial[1] = 0.                                        # (some phoneme is mandatory, so there is a state 1)
    if flags[count - 1]:
        final[count - 2] = 0.
    return _assemble(symbols, [0.] * count, into, initial, final)


def model_graph(transitions, initial=None, final=None):
    """The model of `recognize` as a Graph of 40 states: state q carries phoneme q, stay[q] = transitions[q, q], and
    its arcs come from every p != q in ascending p with transitions[p, q].  `viterbi` under it is `recognize` bit for
    bit.  Host only."""
    count = len(PHONEMES)
    matrix = _weights(transitions, (count, count), 'transitions').cpu().tolist()
    first = [0.] * count if initial is None else _weights(initial, (count,), 'initial').cpu().tolist()
    last = [0.] * count if final is None else _weights(final, (count,), 'final').cpu().tolist()
    into = [[(p, matrix[p][q]) for p in range(count) if p != q] for q in range(count)]
    return _assemble(list(range(count)), [matrix[q][q] for q in range(count)], into, first, last)


def _variants(word, what):
    """The pronunciations of one word: a non-empty list of non-empty index lists."""
    if isinstance(word, (str, bytes)) or not isinstance(word, (list, tuple)) or len(word) < 1:
        raise ValueError(f'{what} takes a non-empty list of pronunciations, each a list of phonemes')
    out = []
    for variant in word:
        if not torch.is_tensor(variant) and not isinstance(variant, (list, tuple)):
            raise ValueError(f'{what}: a pronunciation is a list of phonemes, got {variant!r}')
        sequence = _sequence(variant)
        if not sequence:
            raise ValueError(f'{what} has a pronunciation without phonemes')
        out.append(sequence)
    return out


def pronunciations(words, silence=True):
    """A transcript whose words have alternative pronunciations, for `viterbi`: (graph, word_of, variant_of).

    `words` is a list of words, each a list of alternative phoneme sequences ("either": [['iy', 'dh', 'er'], ['ay',
    'dh', 'er']]).  The variants of a word stand in parallel, every variant of a word joined to every variant of the
    next; with `silence` an optional '<silent>' state stands before the first word, between words and after the last,
    as `transcript` places it.  A word's first states take the arc from the silence before them first, then those from
    the last states of the word before, in the order of its variants.  All weights are 0: the total is the largest
    total `forced(..., optional=)` gives over all combinations of variants.  word_of[n] and variant_of[n] are the word
    and its variant state n belongs to, -1 for the silences: read the words' times and the variants chosen off
    `Path.states`.  Host only."""
    return _word_graph(words, silence, silence, 'pronunciations')


def phrase_graph(words, pauses=True):
    """A phrase whose words have alternative pronunciations, for `search_graph`: (graph, word_of, variant_of).  It is
    `pronunciations` without the silence before the first word and after the last, which a hit would otherwise
    swallow: with `pauses` an optional '<silent>' state stands between words only, and `pauses=False` equals
    `pronunciations(words, silence=False)` field for field.  The path begins in a first state of the first word and
    ends in a last state of the last.  `search_graph` takes at most 256 states and 4096 arcs.  Host only."""
    return _word_graph(words, bool(pauses), False, 'phrase_graph')


def _word_graph(words, between, around, what):
    """The graph of `pronunciations` and `phrase_graph`: an optional silence between words and around the transcript."""
    if isinstance(words, (str, bytes)) or not isinstance(words, (list, tuple)) or len(words) < 1:
        raise ValueError(f'{what} takes a non-empty list of words, each a list of alternative phoneme sequences')
    quiet = PHONEME_TO_INDEX_MAPPING['<silent>']
    symbols, into, word_of, variant_of = [], [], [], []

    def state(symbol, word, variant, sources):
        symbols.append(symbol)
        into.append([(source, 0.) for source in sources])
        word_of.append(word)
        variant_of.append(variant)
        return len(symbols) - 1
    begins, ends = [], []                                      # where the path may begin; the last states so far
    for index, word in enumerate(words):
        before = list(ends)
        if around if index == 0 else between:
            before = [state(quiet, -1, -1, ends)] + before     # the pause first: advance before skip
        if index == 0:
            begins = list(before)
        ends = []
        for number, sequence in enumerate(_variants(word, f'word {index}')):
            sources = before
            for symbol in sequence:
                at = state(symbol, index, number, sources)
                if sources is before and index == 0:
                    begins.append(at)
                sources = [at]
            ends.append(at)
    if around:
        ends = ends + [state(quiet, -1, -1, ends)]
    count = len(symbols)
    initial, final = [-math.inf] * count, [-math.inf] * count
    for n in begins:
        initial[n] = 0.
    for n in ends:
        final[n] = 0.
    return _assemble(symbols, [0.] * count, into, initial, final), word_of, variant_of


def word_loop(lexicon, penalty=0., silence=True):
    """A loop over the words of a lexicon, for `viterbi`: (graph, word_of).  `lexicon` is a dict, or a list of pairs,
    of word -> pronunciations (a list of alternative phoneme sequences).  Any word may follow any word; entering a
    word, also the first, costs `penalty` (>= 0, finite); with `silence` one '<silent>' state may be passed between
    words, before the first and after the last.  Every pronunciation is a chain of its own; its first state takes the
    arc from the silence first, then one from the last state of every pronunciation, in lexicon order.  word_of[n] is
    the index of state n's word in the lexicon's order, -1 for the silence: a word is said wherever `Path.states`
    enters a first state.  The last states of all pronunciations (the word ends) enter every first state, so their
    number is bounded by the degree limit, and their square by the limit on arcs; a lexicon beyond either is refused.
    The limit on arcs comes first, at about 180 word ends (E ends enter E words: E * (E + 1) arcs of 32768), so no word
    loop has a state of the largest degree, 255: only `graph` builds one.  Host only."""
    if isinstance(penalty, bool) or not isinstance(penalty, (int, float)) or not 0 <= penalty < math.inf:
        raise ValueError(f'a word penalty must be a finite number >= 0, got {penalty!r}')
    pairs = list(lexicon.items()) if isinstance(lexicon, dict) else lexicon
    if isinstance(pairs, (str, bytes)) or not isinstance(pairs, (list, tuple)) or len(pairs) < 1:
        raise ValueError('a word loop takes a non-empty lexicon: a dict or a list of (word, pronunciations)')
    chains = []
    for index, pair in enumerate(pairs):
        if not isinstance(pair, (list, tuple)) or len(pair) != 2:
            raise ValueError(f'lexicon entry {index} must be (word, pronunciations), got {pair!r}')
        chains.extend((index, sequence) for sequence in _variants(pair[1], f'word {pair[0]!r}'))
    allowed = VITERBI_MAX_DEGREE - (1 if silence else 0)
    if len(chains) > allowed:
        raise ValueError(f'the lexicon has {len(chains)} word ends (pronunciations), at most {allowed} are allowed: '
                         f'each enters every word, and a state takes {VITERBI_MAX_DEGREE} arcs')
    cost = -float(penalty)
    quiet = PHONEME_TO_INDEX_MAPPING['<silent>']
    base = 1 if silence else 0
    firsts, lasts, at = [], [], base
    for _, sequence in chains:
        firsts.append(at)
        at += len(sequence)
        lasts.append(at - 1)
    if at > VITERBI_MAX_STATES:
        raise ValueError(f'the lexicon takes {at} states, at most {VITERBI_MAX_STATES}')
    entering = ([(0, cost)] if silence else []) + [(last, cost) for last in lasts]
    arcs = len(entering) * len(chains) + (len(lasts) if silence else 0) + at - base - len(chains)
    if arcs > VITERBI_MAX_ARCS:
        raise ValueError(f'the lexicon takes {arcs} arcs, at most {VITERBI_MAX_ARCS}: {len(chains)} word ends enter '
                         f'{len(chains)} words each')
    symbols, into, word_of = [], [], []
    initial, final = [], []
    if silence:
        symbols.append(quiet); into.append([(last, 0.) for last in lasts]); word_of.append(-1)
        initial.append(0.); final.append(0.)
    for index, sequence in chains:
        for position, symbol in enumerate(sequence):
            symbols.append(symbol)
            into.append(list(entering) if position == 0 else [(len(symbols) - 2, 0.)])
            word_of.append(index)
            initial.append(cost if position == 0 else -math.inf)
            final.append(0. if position == len(sequence) - 1 else -math.inf)
    return _assemble(symbols, [0.] * len(symbols), into, initial, final), word_of


def _checked_graph(value):
    """A Graph as `viterbi` takes it: the builders' own, or one made by hand, which is checked here as the device
    would check it (vectorised: no loop over states)."""
    if not isinstance(value, Graph):
        raise ValueError(f'viterbi takes a Graph (graph, chain_graph, model_graph, pronunciations, word_loop), got '
                         f'{type(value).__name__}')
    for name, tensor in zip(Graph._fields, value):
        if not torch.is_tensor(tensor) or tensor.dim() != 1 or tensor.is_cuda:
            raise ValueError(f'Graph.{name} must be a one-dimensional CPU tensor')
    count, arcs = value.phonemes.shape[0], value.sources.shape[0]
    if not 1 <= count <= VITERBI_MAX_STATES:
        raise ValueError(f'a graph has 1 to {VITERBI_MAX_STATES} states, got {count}')
    if arcs > VITERBI_MAX_ARCS:
        raise ValueError(f'a graph has at most {VITERBI_MAX_ARCS} arcs, got {arcs}')
    for name, size in (('stay', count), ('initial', count), ('final', count), ('offsets', count + 1), ('weights', arcs)):
        if getattr(value, name).shape[0] != size:
            raise ValueError(f'Graph.{name} has {getattr(value, name).shape[0]} entries, {size} expected')
    for name in ('phonemes', 'offsets', 'sources'):
        tensor = getattr(value, name)
        if tensor.is_floating_point() or tensor.is_complex() or tensor.dtype == torch.bool:
            raise ValueError(f'Graph.{name} must be an integer tensor, got {tensor.dtype}')
    offsets = value.offsets.to(torch.int64)
    degrees = offsets[1:] - offsets[:-1]
    if int(offsets[0]) != 0 or int(offsets[-1]) != arcs or bool((degrees < 0).any()):
        raise ValueError('Graph.offsets must rise from 0 to the number of arcs')
    if bool((degrees > VITERBI_MAX_DEGREE).any()):
        raise ValueError(f'state {int(degrees.argmax())} has {int(degrees.max())} arcs coming in, at most '
                         f'{VITERBI_MAX_DEGREE}')
    if bool(((value.phonemes < 0) | (value.phonemes >= len(PHONEMES))).any()):
        raise ValueError(f'a phoneme index of the graph is outside [0, {len(PHONEMES) - 1}]')
    if bool(((value.sources < 0) | (value.sources >= count)).any()):
        raise ValueError(f'a source of the graph is not a state in [0, {count - 1}]')
    for name in ('stay', 'weights', 'initial', 'final'):
        tensor = getattr(value, name)
        if not tensor.is_floating_point() or bool((torch.isnan(tensor) | (tensor == math.inf)).any()):
            raise ValueError(f'Graph.{name} must hold weights, each finite or -inf')
    return value


def _graph_list(graph, batch, where, members):
    """The distinct graphs of a call, checked, and the graph of every member (None: the one graph for all): `graph` is
    one Graph, or with `batch` members a list of as many, in which one object may stand for several and travels once."""
    if isinstance(graph, (list, tuple)) and not isinstance(graph, Graph):
        if batch is None or len(graph) != batch:
            raise ValueError(f'a list of graphs goes with {where} of as many {members}, got {len(graph)} for {batch}')
        packed, places, which = [], {}, []
        for value in graph:
            if id(value) not in places:
                places[id(value)] = len(packed)
                packed.append(_checked_graph(value))
            which.append(places[id(value)])
        return packed, which
    return [_checked_graph(graph)], None


def _joined_graphs(packed):
    """Checked graphs as the library takes them packed: (states per graph, state_begin, arc_begin, joined), where
    joined(name) is that field of all graphs behind one another."""
    counts = [value.phonemes.shape[0] for value in packed]
    state_begin = torch.tensor([0] + counts, dtype=torch.int64).cumsum(0)
    arc_base = torch.tensor([0] + [value.sources.shape[0] for value in packed], dtype=torch.int64).cumsum(0)
    arc_begin = torch.cat([value.offsets[:-1].to(torch.int64) + arc_base[g] for g, value in enumerate(packed)] +
                          [arc_base[-1:]])

    def joined(name):
        return torch.cat([getattr(value, name) for value in packed])
    return counts, state_begin, arc_begin, joined


def viterbi(ppg, graph, lengths=None, gop=True):
    """The best path of `ppg` through a graph of phoneme states (see the module's text): Path(states, phonemes,
    starts, total, score, gop), one entry per run of the path.

    `ppg` is (40, T) or a batch (B, 40, T) padded to the longest item with `lengths` per item (the padding is never
    read), up to 262144 frames.  `graph` is a Graph (`graph`, `chain_graph`, `model_graph`, `pronunciations`,
    `word_loop`) for every item, or for a batch a list of B of them (the same object may stand for several items and
    travels once).  One utterance returns device tensors: states and phonemes (R,) int32, starts (R + 1,) int32, total
    0-d, score and gop (R,) fp32; a batch returns lists of B such tensors and total (B,), as `recognize` does, and
    equals its single calls bit for bit.  A run is a stretch of frames in one state; a path that leaves a state through
    an arc back into it opens a new run of that state.  gop=False skips that sum and returns None for it.  An utterance
    that no path fits has no runs, starts = [0] and total = -inf.  `segments` and `frame_labels` take the result as
    they take an Alignment."""
    batched, batch, frames = _ppg(ppg, VITERBI_MAX_FRAMES, 'viterbi')
    if not batched and lengths is not None:
        raise ValueError('lengths go with a batch: slice a single PPG instead')
    lengths = _lengths(lengths, batch, frames)
    packed, which = _graph_list(graph, batch if batched else None, 'a batch', 'items')
    counts, state_begin, arc_begin, joined = _joined_graphs(packed)
    device = core.device_for(None, ppg)
    x = ppg.to(device)
    states, phonemes, starts, runs, total, score, below = engine.viterbi_items(
        x if batched else x[None], lengths, state_begin, joined('phonemes'), joined('stay'), joined('initial'),
        joined('final'), arc_begin, joined('sources'), joined('weights'), which, max(counts), gop)
    runs = runs.tolist()
    if not batched:
        r = runs[0]
        return Path(states[0, :r], phonemes[0, :r], starts[0, :r + 1], total[0], score[0, :r],
                    below[0, :r] if gop else None)
    return Path(
        [states[b, :r] for b, r in enumerate(runs)], [phonemes[b, :r] for b, r in enumerate(runs)],
        [starts[b, :r + 1] for b, r in enumerate(runs)], total, [score[b, :r] for b, r in enumerate(runs)],
        [below[b, :r] for b, r in enumerate(runs)] if gop else None)


_TRANSPOSED = collections.OrderedDict()        # id(graph) -> (graph, its out-arc lists): the graph is held, so the id is its own
_TRANSPOSED_MOST = 64


def _transposed(graph):
    """The out-arc lists of a checked Graph: (offsets (S + 1,) int64, targets (A,) int64, weights (A,)), the in-arcs
    sorted by source with their order kept (a stable sort), so that the arcs out of state n are offsets[n] ..
    offsets[n + 1] - 1.  Kept per graph object: a graph is transposed once."""
    kept = _TRANSPOSED.get(id(graph))
    if kept is not None and kept[0] is graph:
        _TRANSPOSED.move_to_end(id(graph))
        return kept[1]
    count = graph.phonemes.shape[0]
    offsets, sources = graph.offsets.to(torch.int64), graph.sources.to(torch.int64)
    into = torch.repeat_interleave(torch.arange(count, dtype=torch.int64), offsets[1:] - offsets[:-1])
    order = torch.sort(sources, stable=True).indices
    out_offsets = torch.cat([torch.zeros(1, dtype=torch.int64), torch.bincount(sources, minlength=count).cumsum(0)])
    lists = (out_offsets, into[order], graph.weights[order])
    _TRANSPOSED[id(graph)] = (graph, lists)
    while len(_TRANSPOSED) > _TRANSPOSED_MOST:
        _TRANSPOSED.popitem(last=False)
    return lists


def posterior(ppg, graph, lengths=None, states=False):
    """The sum over all paths of `ppg` through a graph of phoneme states (see the module's text): Posterior(total,
    phonemes, states).

    `ppg` and `lengths` as `viterbi` takes them, up to 65536 frames; `graph` is anything `viterbi` accepts: a Graph
    (`graph`, `chain_graph`, `model_graph`, `pronunciations`, `word_loop`) for every item, or for a batch a list of B of
    them.  total is float64, the log-likelihood of the graph given the recording: 0-d for one utterance, (B,) for a
    batch.  phonemes is the phoneme posterior given the graph, (40, T) or (B, 40, T) fp32 on the device, a PPG that
    `distance`, `dtw`, `sparsify` and `edit` take; every frame sums to 1.  states is None, or with states=True the
    occupancy of every state, (T, S) or (B, T, the largest S of the batch).  An utterance that no path fits has total
    -inf; its outputs, the frames past an item's length and the states past its graph's are zero.  A batch equals its
    single calls bit for bit, and the same call gives the same bits."""
    batched, batch, frames = _ppg(ppg, POSTERIOR_MAX_FRAMES, 'posterior')
    if not batched and lengths is not None:
        raise ValueError('lengths go with a batch: slice a single PPG instead')
    lengths = _lengths(lengths, batch, frames)
    packed, which = _graph_list(graph, batch if batched else None, 'a batch', 'items')
    counts, state_begin, arc_begin, joined = _joined_graphs(packed)
    lists = [_transposed(value) for value in packed]
    arc_base = arc_begin[state_begin[:-1]]
    out_begin = torch.cat([out[0][:-1] + arc_base[g] for g, out in enumerate(lists)] + [arc_begin[-1:]])
    device = core.device_for(None, ppg)
    x = ppg.to(device)
    total, phonemes, occupancy = engine.posterior_items(
        x if batched else x[None], lengths, state_begin, joined('phonemes'), joined('stay'), joined('initial'),
        joined('final'), arc_begin, joined('sources'), joined('weights'), out_begin,
        torch.cat([out[1] for out in lists]), torch.cat([out[2] for out in lists]), which, max(counts), states)
    if not batched:
        return Posterior(total[0], phonemes[0], occupancy[0] if states else None)
    return Posterior(total, phonemes, occupancy)


def run_confidence(path, posterior):
    """How sure each run of a `viterbi` Path is, from a Posterior of the same PPG and graph made with states=True: the
    mean occupancy of the run's state over the run's frames, one number in [0, 1] per run ("how sure is this phoneme
    here").  One utterance gives (R,) fp32; a batch gives a list of B such tensors."""
    if posterior.states is None:
        raise ValueError('run_confidence takes a Posterior made with states=True')

    def one(run_states, starts, occupancy):
        runs = run_states.shape[0]
        if runs == 0:
            return occupancy.new_zeros((0,))
        starts = starts.to(torch.int64)
        frames = int(starts[-1])
        spans = starts[1:] - starts[:-1]
        state = torch.repeat_interleave(run_states.to(torch.int64), spans)
        taken = occupancy[torch.arange(frames, device=occupancy.device), state]
        run = torch.repeat_interleave(torch.arange(runs, device=occupancy.device), spans)
        return occupancy.new_zeros((runs,)).index_add_(0, run, taken) / spans.to(occupancy.dtype)
    if isinstance(path.states, (list, tuple)):
        if posterior.states.dim() != 3 or posterior.states.shape[0] != len(path.states):
            raise ValueError('the Path and the Posterior are not of one batch')
        return [one(path.states[b], path.starts[b], posterior.states[b]) for b in range(len(path.states))]
    if posterior.states.dim() != 2:
        raise ValueError('the Path is of one utterance and the Posterior of a batch')
    return one(path.states, path.starts, posterior.states)


def _queries(phonemes):
    """The queries of a search, one sequence or a list of them: (several, list of checked index lists)."""
    several = isinstance(phonemes, (list, tuple)) and len(phonemes) > 0 and all(
        torch.is_tensor(item) or isinstance(item, (list, tuple)) for item in phonemes)
    sequences = [_sequence(item) for item in phonemes] if several else [_sequence(phonemes)]
    for sequence in sequences:
        if len(sequence) < 1:
            raise ValueError('an empty phoneme sequence cannot be searched for')
        if len(sequence) > SEARCH_MAX_PHONEMES:
            raise ValueError(f'search takes at most {SEARCH_MAX_PHONEMES} phonemes per query, got {len(sequence)}')
    return several, sequences


def search(ppg, phonemes, lengths=None, top=1, threshold=None, curve=False):
    """Find where `phonemes` is said in `ppg`: Hits(phonemes, begin, end, total, mean, count, curve).

    `ppg` is (40, T), or a batch (B, 40, T) padded to the longest recording with `lengths` per recording (the padding
    is never read).  `phonemes` is one sequence of names from `ppgs_amd.PHONEMES` or of indices (a list or an integer
    tensor), or a list of Q such sequences; every sequence is searched in every recording.  begin, end (int32), total
    and mean (fp32) are device tensors (B, Q, top), count is (B, Q) int32: the B axis is dropped for a single recording
    and the Q axis for a single sequence.  Hit h of a pair covers frames begin[h] .. end[h] - 1; hits are disjoint and
    listed best first; entries at or past count are -1, -1, NaN, NaN.  `threshold` ends the list at the first mean
    below it (None: `top` hits wherever the recording has room for them).  A sequence longer than its recording has
    count 0.  With `curve` the last field is (curve_total, curve_begin), each (B, Q, T) with the same drops (-inf and
    -1 before a match can end and past a recording's own length), else None.  Hits.phonemes holds the queries as int32
    device tensors.  Nothing here waits for the device."""
    batched, batch, frames = _ppg(ppg, SEARCH_MAX_FRAMES, 'search')
    if not batched and lengths is not None:
        raise ValueError('lengths go with a batch: slice a single PPG instead')
    lengths = _lengths(lengths, batch, frames)
    several, sequences = _queries(phonemes)
    if isinstance(top, bool) or not isinstance(top, int) or not 1 <= top <= SEARCH_MAX_HITS:
        raise ValueError(f'top must be an integer from 1 to {SEARCH_MAX_HITS}, got {top!r}')
    threshold = -math.inf if threshold is None else float(threshold)
    if math.isnan(threshold):
        raise ValueError('the threshold is NaN')
    counts = [len(sequence) for sequence in sequences]
    most = max(counts)
    device = core.device_for(None, ppg)
    table = torch.tensor([sequence + [-1] * (most - len(sequence)) for sequence in sequences], dtype=torch.int32)
    table = table.to(device)
    x = ppg.to(device)
    begin, end, total, mean, count, curves = engine.search_items(x if batched else x[None], lengths, table, counts, top,
                                                                 threshold, bool(curve))

    def drop(tensor):
        tensor = tensor if several else tensor[:, 0]
        return tensor if batched else tensor[0]
    names = [table[q, :n] for q, n in enumerate(counts)]
    return Hits(names if several else names[0], drop(begin), drop(end), drop(total), drop(mean), drop(count),
                None if curves is None else (drop(curves[0]), drop(curves[1])))


def _search_graphs(graphs):
    """The graphs of a search, one Graph or a list of them: (several, the checked graphs)."""
    several = isinstance(graphs, (list, tuple)) and not isinstance(graphs, Graph)
    values = list(graphs) if several else [graphs]
    if not 1 <= len(values) <= SEARCH_GRAPH_MAX_GRAPHS:
        raise ValueError(f'search_graph takes 1 to {SEARCH_GRAPH_MAX_GRAPHS} graphs, got {len(values)}')
    packed = [_checked_graph(value) for value in values]
    for index, value in enumerate(packed):
        count, arcs = value.phonemes.shape[0], value.sources.shape[0]
        if count > SEARCH_GRAPH_MAX_STATES or arcs > SEARCH_GRAPH_MAX_ARCS:
            raise ValueError(f'search_graph takes graphs of at most {SEARCH_GRAPH_MAX_STATES} states and '
                             f'{SEARCH_GRAPH_MAX_ARCS} arcs, graph {index} has {count} and {arcs}')
    return several, packed


def shortest_match(graph):
    """The fewest frames a match of `graph` can span: the fewest states on any path from a state with a finite
    `initial` to a state with a finite `final` (a breadth-first search over the arcs; staying adds nothing), at least
    1; 1 for a graph that has no such path, which never matches anything.  Host only."""
    count = graph.phonemes.shape[0]
    offsets, sources = graph.offsets.tolist(), graph.sources.tolist()
    open_arc = (graph.weights > -math.inf).tolist()
    out = [[] for _ in range(count)]
    for n in range(count):
        for j in range(offsets[n], offsets[n + 1]):
            if open_arc[j]:
                out[sources[j]].append(n)
    final = (graph.final > -math.inf).tolist()
    reached = [bool(value) for value in (graph.initial > -math.inf).tolist()]
    front, states = [n for n in range(count) if reached[n]], 1
    while front:
        if any(final[n] for n in front):
            return states
        following = []
        for p in front:
            for n in out[p]:
                if not reached[n]:
                    reached[n] = True
                    following.append(n)
        front, states = following, states + 1
    return 1


def search_graph(ppg, graphs, lengths=None, top=1, threshold=None, curve=False):
    """Find where a path through a Graph is said in `ppg`: GraphHits(begin, end, total, mean, count, curve).

    `search` with a graph as the query (the module's text): `graphs` is one Graph (`phrase_graph`, `chain_graph`,
    `graph`, `pronunciations`) of at most 256 states and 4096 arcs, or a list of Q of them; every graph is searched in
    every recording.  `ppg`, `lengths`, `top`, `threshold`, `curve`, the shapes and the dropped axes are `search`'s: the
    B axis is dropped for a single recording and the Q axis for a single graph.  A graph that no span fits has count 0.
    `hit_segments` takes the result; the states inside hit h are `viterbi(ppg[:, begin[h]:end[h]], graph).states`.
    Nothing here waits for the device."""
    batched, batch, frames = _ppg(ppg, SEARCH_MAX_FRAMES, 'search_graph')
    if not batched and lengths is not None:
        raise ValueError('lengths go with a batch: slice a single PPG instead')
    lengths = _lengths(lengths, batch, frames)
    several, packed = _search_graphs(graphs)
    if isinstance(top, bool) or not isinstance(top, int) or not 1 <= top <= SEARCH_MAX_HITS:
        raise ValueError(f'top must be an integer from 1 to {SEARCH_MAX_HITS}, got {top!r}')
    threshold = -math.inf if threshold is None else float(threshold)
    if math.isnan(threshold):
        raise ValueError('the threshold is NaN')
    counts, state_begin, arc_begin, joined = _joined_graphs(packed)
    device = core.device_for(None, ppg)
    x = ppg.to(device)
    begin, end, total, mean, count, curves = engine.search_graph_items(
        x if batched else x[None], lengths, state_begin, joined('phonemes'), joined('stay'), joined('initial'),
        joined('final'), arc_begin, joined('sources'), joined('weights'), top, threshold, bool(curve), max(counts))

    def drop(tensor):
        tensor = tensor if several else tensor[:, 0]
        return tensor if batched else tensor[0]
    return GraphHits(drop(begin), drop(end), drop(total), drop(mean), drop(count),
                     None if curves is None else (drop(curves[0]), drop(curves[1])))


class SearchStream:
    """`search` on a live stream: the frames come a few at a time (`Engine.stream`, `Engine.audio_stream`, ...), the
    search is carried across the pushes on the device, and hits come out as soon as they are final.

        spotter = ppgs_amd.alignment.SearchStream(['hh', 'ah', 'l', 'ow'], threshold=-1.)
        for piece in pieces:                                     # each (40, k), k >= 0
            hits = spotter.push(piece)
            for start, end, total, mean in ppgs_amd.alignment.hit_segments(hits): ...
        last = spotter.flush()

    `phonemes` is one sequence or a list of Q sequences, as in `search`.  The curve is `search`'s: whatever the sizes
    of the pushes, the pushed frames' curve values are those of `search(whole recording, ..., curve=True)` at the same
    frames, bit for bit; frame indices count from the last reset.  Hits are decided online.  Per query the detector
    keeps `taken`, the end of the last hit it gave out (0 at first), and at most one pending hit.  At every frame t, in
    order: (1) a pending hit whose last frame lies more than `patience` frames back is given out; (2) if the match
    ending at t begins at or after `taken` and its mean = curve_total[t] / (t - curve_begin[t] + 1) >= `threshold`, it
    is a candidate: it becomes pending if nothing is; if it overlaps the pending hit it replaces it when its mean is
    at least as large (ties go to the later end); if it is disjoint, the pending hit is given out and the candidate
    becomes pending.  So hits are disjoint, come in stream order, and do not depend on how the frames were split.
    `threshold` has no default: no value is sensible for every model.  `patience` = 25 frames is a quarter of a second.

    `batch=None` is one stream: push((40, F)).  `batch=B` is B streams side by side: push((B, 40, Fmax), lengths),
    lengths[b] in [0, Fmax] (None: Fmax each); a stream with 0 sits out the step and the padding is never read.
    push returns `Hits` whose begin, end (int32), total and mean (fp32) are device tensors (B, Q, cap) with
    cap = F // (the shortest query) + 2, more than a push can give out; count (B, Q) is the number given out in this
    push; entries at or past it are -1, -1, NaN, NaN; with `curve` the last field is the pushed frames'
    (curve_total, curve_begin), each (B, Q, F), else None.  The B axis is dropped for one stream and the Q axis for
    one sequence, as in `search`, so `hit_segments` takes the result as it is.  A push of no frames (F = 0) returns
    empty tensors and calls nothing.  flush(item=None) gives out the pending hits (cap = 1) of every stream or of
    stream `item`; reset(item=None) starts every stream, or that one, again at frame 0.  `position` is the host list
    of the frames each stream has received.  Nothing here waits for the device; the state and a workspace that only
    grows belong to the object and live on `device` (None: the device of the first push's tensor, else the current
    one)."""

    def __init__(self, phonemes, threshold, patience=25, batch=None, curve=False, device=None):
        self._several, sequences = _queries(phonemes)
        self._detector(threshold, patience, batch, curve, device)
        self._counts = [len(sequence) for sequence in sequences]
        self._most = max(self._counts)
        self._pairs, self._shortest = len(self._counts), min(self._counts)
        self._host_table = torch.tensor([sequence + [-1] * (self._most - len(sequence)) for sequence in sequences],
                                        dtype=torch.int32)
        self._table = self._device_counts = self._names = None

    def _detector(self, threshold, patience, batch, curve, device):
        """What a live search has whatever its queries are: the detector's two numbers, the streams and their host
        side."""
        threshold = float(threshold)
        if math.isnan(threshold):
            raise ValueError('the threshold is NaN')
        if isinstance(patience, bool) or not isinstance(patience, int) or not 0 <= patience <= 2 ** 31 - 1:
            raise ValueError(f'patience must be a number of frames from 0 to {2 ** 31 - 1}, got {patience!r}')
        if batch is not None and (isinstance(batch, bool) or not isinstance(batch, int) or
                                  not 1 <= batch <= engine.SEARCH_MAX_ITEMS):
            raise ValueError(f'batch must be None or 1 to {engine.SEARCH_MAX_ITEMS} streams, got {batch!r}')
        self.threshold, self.patience, self.batch, self.curve = threshold, patience, batch, bool(curve)
        self._streams = 1 if batch is None else batch
        self._gpu = device
        self._position = [0] * self._streams
        self._state = self._workspace = None
        self._uniform, self._flags = {}, {}

    @property
    def position(self):
        return list(self._position)

    def _ensure(self, tensor=None):
        """The device side, made at the first call that needs it."""
        if self._state is None:
            device = core.device_for(self._gpu, tensor)
            self._table = self._host_table.to(device)
            self._device_counts = torch.tensor(self._counts, dtype=torch.int32).to(device)
            self._names = [self._table[q, :n] for q, n in enumerate(self._counts)]
            with torch.cuda.device(device):
                self._state = engine.search_stream_state(device, self._streams, len(self._counts), self._most)
        return self._state.device

    def _drop(self, tensor):
        tensor = tensor if self._several else tensor[:, 0]
        return tensor if self.batch is not None else tensor[0]

    def _hits(self, begin, end, total, mean, count, curves=None):
        return Hits(self._names if self._several else self._names[0], self._drop(begin), self._drop(end),
                    self._drop(total), self._drop(mean), self._drop(count),
                    None if curves is None else (self._drop(curves[0]), self._drop(curves[1])))

    def _which(self, item):
        """The flags of `item` for flush and reset: None for every stream."""
        if item is None:
            return None
        if isinstance(item, bool) or not isinstance(item, int) or not 0 <= item < self._streams:
            raise ValueError(f'item must be None or a stream index below {self._streams}, got {item!r}')
        device = self._ensure()
        if item not in self._flags:
            self._flags[item] = torch.tensor([int(b == item) for b in range(self._streams)], dtype=torch.int32).to(device)
        return self._flags[item]

    def push(self, ppg, lengths=None):
        if not torch.is_tensor(ppg) or ppg.dim() != (2 if self.batch is None else 3):
            raise ValueError(f'a push takes {"(40, frames)" if self.batch is None else f"({self.batch}, 40, frames)"}, '
                             f'got {tuple(getattr(ppg, "shape", ()))}')
        if ppg.shape[-2] != config.OUTPUT_CHANNELS:
            raise ValueError(f'PPG must have {config.OUTPUT_CHANNELS} channels, got {tuple(ppg.shape)}')
        if self.batch is not None and ppg.shape[0] != self.batch:
            raise ValueError(f'a push takes {self.batch} streams, got {ppg.shape[0]}')
        frames = ppg.shape[-1]
        if frames > SEARCH_MAX_FRAMES:
            raise ValueError(f'a push takes at most {SEARCH_MAX_FRAMES} frames, got {frames}')
        if lengths is None:
            own = [frames] * self._streams
        else:
            if self.batch is None:
                raise ValueError('lengths go with a batch of streams: slice a single PPG instead')
            if torch.is_tensor(lengths):
                lengths = lengths.detach().cpu().reshape(-1).tolist()
            own = [int(value) for value in (lengths if isinstance(lengths, (list, tuple)) else [lengths])]
            if len(own) != self._streams:
                raise ValueError(f'lengths has {len(own)} entries for {self._streams} streams')
            for value in own:
                if not 0 <= value <= frames:
                    raise ValueError(f'lengths: {value} is outside [0, {frames}]')
        for position, value in zip(self._position, own):
            if position + value > 2 ** 31 - 1:
                raise ValueError(f'a stream takes at most {2 ** 31 - 1} frames between resets, got {position} + {value}')
        device = self._ensure(ppg)
        queries = self._pairs
        if frames == 0:
            shape = (self._streams, queries, 0)
            return self._hits(
                torch.empty(shape, dtype=torch.int32, device=device), torch.empty(shape, dtype=torch.int32, device=device),
                torch.empty(shape, dtype=torch.float32, device=device),
                torch.empty(shape, dtype=torch.float32, device=device),
                torch.zeros(shape[:2], dtype=torch.int32, device=device),
                (torch.empty(shape, dtype=torch.float32, device=device),
                 torch.empty(shape, dtype=torch.int32, device=device)) if self.curve else None)
        x = ppg.to(device=device, dtype=torch.float32).contiguous()
        x = x if self.batch is not None else x[None]
        if lengths is None:
            if frames not in self._uniform:
                if len(self._uniform) >= 64:                             # (a stream pushes a few sizes over and over)
                    self._uniform.clear()
                self._uniform[frames] = torch.full((self._streams,), frames, dtype=torch.int32, device=device)
            on_device = self._uniform[frames]
        else:                                                            # through pinned memory: the copy does not wait
            on_device = torch.tensor(own, dtype=torch.int32).pin_memory().to(device, non_blocking=True)
        need = self._workspace_bytes(frames)
        if self._workspace is None or self._workspace.numel() < need:
            self._workspace = torch.empty((need,), dtype=torch.uint8, device=device)
        cap = frames // self._shortest + 2
        begin, end, total, mean, count, curves = self._push_piece(x, on_device, cap)
        self._position = [position + value for position, value in zip(self._position, own)]
        return self._hits(begin, end, total, mean, count, curves)

    def flush(self, item=None):
        which = self._which(item)
        self._ensure()
        return self._hits(*self._flush_all(which))

    def reset(self, item=None):
        which = self._which(item)
        self._ensure()
        self._reset_all(which)
        self._position = [0 if item is None or b == item else position for b, position in enumerate(self._position)]

    # what SearchGraphStream replaces: the library's calls
    def _workspace_bytes(self, frames):
        return engine.library().ppg_search_stream_workspace_bytes(self._streams, frames, self._pairs)

    def _push_piece(self, x, lengths, cap):
        return engine.search_stream_push(self._state, x, lengths, self._table, self._device_counts, self.threshold,
                                         self.patience, cap, self._workspace, self.curve)

    def _flush_all(self, which):
        return engine.search_stream_flush(self._state, self._streams, self._pairs, self._most, which)

    def _reset_all(self, which):
        engine.search_stream_reset(self._state, self._streams, self._pairs, self._most, which)


class SearchGraphStream(SearchStream):
    """`search_graph` on a live stream: SearchStream with graphs as the queries, so that a spotter on a live stream has
    pronunciation variants, optional pauses between words and droppable consonants in one query.

        graph = ppgs_amd.alignment.phrase_graph([[['iy', 'dh', 'er'], ['ay', 'dh', 'er']], [['w', 'ey']]])[0]
        spotter = ppgs_amd.alignment.SearchGraphStream(graph, threshold=-1.)
        for piece in pieces:                                     # each (40, k), k >= 0
            for start, end, total, mean in ppgs_amd.alignment.hit_segments(spotter.push(piece)): ...
        last = spotter.flush()

    `graphs` is one Graph or a list of Q of them, validated as `search_graph` validates them (at most 256 states and
    4096 arcs each); every graph runs on every stream.  The curve is `search_graph`'s: whatever the sizes of the pushes,
    the pushed frames' curve values are those of `search_graph(whole recording, ..., curve=True)` at the same frames, bit
    for bit, with begins that count from the last reset.  `threshold`, `patience`, `batch`, `curve`, `device`, the
    online rule, push, flush, reset and `position` are SearchStream's; push and flush return `GraphHits` with the
    dropped axes of `search_graph`, which `hit_segments` takes as it is.  cap = F // Lmin + 2, Lmin the fewest states
    on a path from a state that may start a match to one that may end it (`shortest_match`), the least over the graphs:
    hits are disjoint, each spans at least Lmin frames, and at most one was pending before the push.  On
    `chain_graph(s)` every output equals `SearchStream(s)`'s bit for bit.  Nothing here waits for the device."""

    def __init__(self, graphs, threshold, patience=25, batch=None, curve=False, device=None):
        self._several, packed = _search_graphs(graphs)
        self._detector(threshold, patience, batch, curve, device)
        counts, state_begin, arc_begin, joined = _joined_graphs(packed)
        self._graphs = engine.PackedGraphs(
            len(packed), sum(counts), int(arc_begin[-1]), max(counts), state_begin.to(torch.int32),
            joined('phonemes').to(torch.int32), joined('stay').to(torch.float32), joined('initial').to(torch.float32),
            joined('final').to(torch.float32), arc_begin.to(torch.int32), joined('sources').to(torch.int32),
            joined('weights').to(torch.float32))
        self._pairs, self._shortest = len(packed), min(shortest_match(value) for value in packed)
        self._weights = None

    def _ensure(self, tensor=None):
        if self._state is None:
            device = core.device_for(self._gpu, tensor)
            self._weights = engine.PackedGraphs(*[value.to(device).contiguous() if torch.is_tensor(value) else value
                                                  for value in self._graphs])
            with torch.cuda.device(device):
                self._state = engine.search_graph_stream_state(device, self._streams, self._weights)
        return self._state.device

    def _hits(self, begin, end, total, mean, count, curves=None):
        return GraphHits(self._drop(begin), self._drop(end), self._drop(total), self._drop(mean), self._drop(count),
                         None if curves is None else (self._drop(curves[0]), self._drop(curves[1])))

    def _workspace_bytes(self, frames):
        return engine.library().ppg_search_graph_stream_workspace_bytes(self._streams, frames, self._pairs)

    def _push_piece(self, x, lengths, cap):
        return engine.search_graph_stream_push(self._state, x, lengths, self._weights, self.threshold, self.patience,
                                               cap, self._workspace, self.curve)

    def _flush_all(self, which):
        return engine.search_graph_stream_flush(self._state, self._streams, self._pairs, self._weights.max_states, which)

    def _reset_all(self, which):
        engine.search_graph_stream_reset(self._state, self._streams, self._pairs, self._weights.max_states, which)


class RecognizeStream:
    """`recognize` on a live stream: the frames come a few at a time, the Viterbi decode is carried across the pushes on
    the device, and runs of phonemes come out as soon as they are final (see the module's text for the definition).

        said = ppgs_amd.alignment.RecognizeStream(penalty=4.)
        for piece in pieces:                                     # each (40, k), k >= 0
            for name, start, end, score, gop in ppgs_amd.alignment.run_segments(said.push(piece)): ...
        last = said.flush()

    Exactly one of `transitions` (40, 40) and `penalty` is given, `initial` and `final` (40,) are optional, all checked
    as `recognize` checks them.  `window` is the ring of every stream in frames, a multiple of 64 from 64 to 65536;
    `max_lag` (None: window // 2) in [0, window) is the number of frames a label may stay open before it is given out
    by force.  As long as nothing is forced (`forced` == 0 at the flush) the runs of all pushes and of the flush are
    `recognize` of the whole recording bit for bit.

    `batch=None` is one stream: push((40, F)).  `batch=B` is B streams side by side: push((B, 40, Fmax), lengths),
    lengths[b] in [0, Fmax] (None: Fmax each); the padding is never read.  push returns `Runs(phonemes, begin, end,
    score, gop, count, total, forced)`: phonemes, begin, end (int32), score and gop (fp32; gop None with gop=False) are
    padded device tensors (cap,) or (B, cap) with cap = max_lag + F, never less than the runs a push can close; count,
    0-d or (B,), is the number closed in this push; slots at or past it are -1 / NaN; total and forced are None.  A
    stream that could not take its frames has count = -1.  A push longer than window - max_lag is fed in pieces of
    that size whose runs are packed behind one another on the device.  A push of no frames (F = 0) returns empty
    tensors and calls nothing.  flush(item=None) commits the rest along the best path under `final`, closes the open
    run and resets every stream, or stream `item`: Runs with cap = max_lag + 1 and total (fp32) and forced (int32),
    0-d or (B,); streams it leaves out have count = 0, total = NaN and forced = -1.  reset(item=None) starts every
    stream, or that one, again at frame 0.  `position` is the host list of the frames each stream has received.
    Nothing here waits for the device; the state, the weights and a workspace that only grows belong to the object and
    live on `device` (None: the device of the first push's tensor, else the current one)."""

    def __init__(self, transitions=None, penalty=None, initial=None, final=None, max_lag=None, window=1024, batch=None,
                 gop=True, device=None):
        if (transitions is None) == (penalty is None):
            raise ValueError('RecognizeStream takes either transitions or penalty: one of them, not both')
        if transitions is None:
            transitions = switch_penalty(penalty)
        count = len(PHONEMES)
        self._host = (_weights(transitions, (count, count), 'transitions').cpu().contiguous(),
                      None if initial is None else _weights(initial, (count,), 'initial').cpu().contiguous(),
                      None if final is None else _weights(final, (count,), 'final').cpu().contiguous())
        self._geometry(max_lag, window, batch, gop, device)

    def _geometry(self, max_lag, window, batch, gop, device):
        """The ring, the lag and the streams, checked; nothing of the device yet."""
        if (isinstance(window, bool) or not isinstance(window, int) or window % 64 or
                not engine.RECOGNIZE_STREAM_MIN_WINDOW <= window <= engine.RECOGNIZE_STREAM_MAX_WINDOW):
            raise ValueError(f'window must be a multiple of 64 from {engine.RECOGNIZE_STREAM_MIN_WINDOW} to '
                             f'{engine.RECOGNIZE_STREAM_MAX_WINDOW} frames, got {window!r}')
        max_lag = window // 2 if max_lag is None else max_lag
        if isinstance(max_lag, bool) or not isinstance(max_lag, int) or not 0 <= max_lag < window:
            raise ValueError(f'max_lag must be a number of frames from 0 to window - 1 = {window - 1}, got {max_lag!r}')
        if batch is not None and (isinstance(batch, bool) or not isinstance(batch, int) or
                                  not 1 <= batch <= engine.RECOGNIZE_STREAM_MAX_STREAMS):
            raise ValueError(f'batch must be None or 1 to {engine.RECOGNIZE_STREAM_MAX_STREAMS} streams, got {batch!r}')
        self.window, self.max_lag, self.batch, self.gop = window, max_lag, batch, bool(gop)
        self._streams = 1 if batch is None else batch
        self._gpu = device
        self._position = [0] * self._streams
        self._state = self._workspace = self._weights = None
        self._uniform, self._flags = {}, {}

    @property
    def position(self):
        return list(self._position)

    def _ensure(self, tensor=None):
        """The device side, made at the first call that needs it."""
        if self._state is None:
            device = core.device_for(self._gpu, tensor)
            with torch.cuda.device(device):
                self._state = self._open(device)
        return self._state.device

    # the device calls: what ViterbiStream replaces
    def _open(self, device):
        self._weights = tuple(None if value is None else value.to(device) for value in self._host)
        return engine.recognize_stream_state(device, self._streams, self.window)

    def _push_piece(self, x, lengths, cap):
        return engine.recognize_stream_push(self._state, self.window, x, lengths, self._weights[0], self._weights[1],
                                            self.max_lag, cap, self._workspace, self.gop)

    def _flush_all(self, which):
        return engine.recognize_stream_flush(self._state, self._streams, self.window, self._weights[2],
                                             self.max_lag + 1, which, self.gop)

    def _reset_all(self, which):
        engine.recognize_stream_reset(self._state, self._streams, self.window, which)

    @staticmethod
    def _workspace_bytes(streams, frames):
        return engine.library().ppg_recognize_stream_workspace_bytes(streams, frames)

    _tuple = Runs                                                        # what push and flush return

    def _runs(self, *outputs):
        """The outputs of a push (without total and forced) or of a flush as the stream's tuple."""
        def drop(tensor):
            return tensor if tensor is None or self.batch is not None else tensor[0]
        outputs = outputs + (None,) * (len(self._tuple._fields) - len(outputs))
        return self._tuple(*[drop(tensor) for tensor in outputs])

    def _which(self, item):
        """The flags of `item` for flush and reset: None for every stream."""
        if item is None:
            return None
        if isinstance(item, bool) or not isinstance(item, int) or not 0 <= item < self._streams:
            raise ValueError(f'item must be None or a stream index below {self._streams}, got {item!r}')
        device = self._ensure()
        if item not in self._flags:
            self._flags[item] = torch.tensor([int(b == item) for b in range(self._streams)], dtype=torch.int32).to(device)
        return self._flags[item]

    def push(self, ppg, lengths=None):
        if not torch.is_tensor(ppg) or ppg.dim() != (2 if self.batch is None else 3):
            raise ValueError(f'a push takes {"(40, frames)" if self.batch is None else f"({self.batch}, 40, frames)"}, '
                             f'got {tuple(getattr(ppg, "shape", ()))}')
        if ppg.shape[-2] != config.OUTPUT_CHANNELS:
            raise ValueError(f'PPG must have {config.OUTPUT_CHANNELS} channels, got {tuple(ppg.shape)}')
        if self.batch is not None and ppg.shape[0] != self.batch:
            raise ValueError(f'a push takes {self.batch} streams, got {ppg.shape[0]}')
        frames = ppg.shape[-1]
        if lengths is None:
            own = [frames] * self._streams
        else:
            if self.batch is None:
                raise ValueError('lengths go with a batch of streams: slice a single PPG instead')
            if torch.is_tensor(lengths):
                lengths = lengths.detach().cpu().reshape(-1).tolist()
            own = [int(value) for value in (lengths if isinstance(lengths, (list, tuple)) else [lengths])]
            if len(own) != self._streams:
                raise ValueError(f'lengths has {len(own)} entries for {self._streams} streams')
            for value in own:
                if not 0 <= value <= frames:
                    raise ValueError(f'lengths: {value} is outside [0, {frames}]')
        for position, value in zip(self._position, own):
            if position + value > 2 ** 31 - 1:
                raise ValueError(f'a stream takes at most {2 ** 31 - 1} frames between resets, got {position} + {value}')
        device = self._ensure(ppg)
        cap = self.max_lag + frames
        if frames == 0:
            def empty(dtype):
                return torch.empty((self._streams, 0), dtype=dtype, device=device)
            integers = [empty(torch.int32) for _ in range(len(self._tuple._fields) - 5)]    # all but score .. forced
            return self._runs(*integers, empty(torch.float32), empty(torch.float32) if self.gop else None,
                              torch.zeros((self._streams,), dtype=torch.int32, device=device))
        x = ppg.to(device=device, dtype=torch.float32)
        x = x if self.batch is not None else x[None]
        piece = self.window - self.max_lag                               # what a stream at its full lag can still take
        whole = None
        if lengths is not None:                                          # through pinned memory: the copy does not wait
            whole = torch.tensor(own, dtype=torch.int32).pin_memory().to(device, non_blocking=True)
        need = self._workspace_bytes(self._streams, min(frames, piece))
        if self._workspace is None or self._workspace.numel() < need:
            self._workspace = torch.empty((need,), dtype=torch.uint8, device=device)
        packed = None
        for at in range(0, frames, piece):
            size = min(piece, frames - at)
            if whole is None:
                if size not in self._uniform:
                    if len(self._uniform) >= 64:                         # (a stream pushes a few sizes over and over)
                        self._uniform.clear()
                    self._uniform[size] = torch.full((self._streams,), size, dtype=torch.int32, device=device)
                on_device = self._uniform[size]
            else:
                on_device = (whole - at).clamp_(0, size)
            part = self._push_piece(x[:, :, at:at + size].contiguous(), on_device,
                                    cap if frames <= piece else self.max_lag + size)
            if frames <= piece:
                packed = part
                break
            packed = self._pack(packed, part, cap)
        if frames > piece:                                               # without the slot that took what was past count
            packed = tuple(None if tensor is None else tensor[:, :cap] for tensor in packed[:-1]) + (packed[-1],)
        self._position = [position + value for position, value in zip(self._position, own)]
        return self._runs(*packed)

    def _pack(self, packed, part, cap):
        """The runs of a piece behind those of the pieces before it, on the device: the counts add up (-1 stays)."""
        count = part[-1]
        if packed is None:
            device = count.device
            packed = tuple(
                None if tensor is None else torch.full(
                    (self._streams, cap + 1), math.nan if tensor.is_floating_point() else -1, dtype=tensor.dtype,
                    device=device) for tensor in part[:-1]) + (torch.zeros_like(count),)
        slots = torch.arange(part[0].shape[1], device=count.device)[None, :]
        fits = (slots < count[:, None]) & (packed[-1][:, None] >= 0)
        where = torch.where(fits, (packed[-1][:, None] + slots).clamp_(max=cap), cap).to(torch.int64)
        for into, tensor in zip(packed[:-1], part[:-1]):
            if tensor is not None:
                into.scatter_(1, where, tensor)
                into[:, cap] = math.nan if tensor.is_floating_point() else -1
        total = torch.where((packed[-1] < 0) | (count < 0), torch.full_like(count, -1), packed[-1] + count)
        return packed[:-1] + (total,)

    def flush(self, item=None):
        which = self._which(item)
        self._ensure()
        out = self._flush_all(which)
        self._position = [0 if item is None or b == item else position for b, position in enumerate(self._position)]
        return self._runs(*out)

    def reset(self, item=None):
        which = self._which(item)
        self._ensure()
        self._reset_all(which)
        self._position = [0 if item is None or b == item else position for b, position in enumerate(self._position)]


class ViterbiStream(RecognizeStream):
    """`viterbi` on a live stream: the frames come a few at a time, the decode through the graph is carried across the
    pushes on the device, and runs of states come out as soon as they are final.

        heard = ppgs_amd.alignment.ViterbiStream(ppgs_amd.alignment.word_loop(lexicon)[0])
        for piece in pieces:                                     # each (40, k), k >= 0
            for name, start, end, score, gop in ppgs_amd.alignment.run_segments(heard.push(piece)): ...
        last = heard.flush()

    `graph` is a Graph (`graph`, `chain_graph`, `model_graph`, `pronunciations`, `word_loop`) for every stream, or with
    `batch=B` a list of B of them (the same object may stand for several streams and travels once), validated as
    `viterbi` validates it.  `window`, `max_lag` (None: window // 2), `batch`, `gop`, `device`, push, flush, reset and
    `position` are RecognizeStream's, and so are the rules of the stream with a state of the graph in the place of a
    phoneme; push and flush return `StateRuns(states, phonemes, begin, end, score, gop, count, total, forced)`, which
    `run_segments` takes as it takes Runs.  A run is a stretch of frames in one state; a path that leaves a state through
    an arc back into it opens a new run of that state.  As long as nothing is forced (`forced` == 0 at the flush) the
    runs of all pushes and of the flush are `viterbi` of the whole recording bit for bit; under `model_graph` every
    output equals RecognizeStream's.  In a left-to-right chain (`chain_graph`) the first state stays alive for ever, so
    nothing commits naturally: there `max_lag` = L makes the stream a forced alignment with a latency of L frames, and
    the states whose history disagrees with what was given out are cut off at each forced step."""

    _tuple = StateRuns

    def __init__(self, graph, max_lag=None, window=1024, batch=None, gop=True, device=None):
        self._geometry(max_lag, window, batch, gop, device)
        packed, which = _graph_list(graph, batch, 'batch=', 'streams')
        counts, state_begin, arc_begin, joined = _joined_graphs(packed)
        self._graphs = engine.PackedGraphs(
            len(packed), sum(counts), int(arc_begin[-1]), max(counts), state_begin.to(torch.int32),
            joined('phonemes').to(torch.int32), joined('stay').to(torch.float32), joined('initial').to(torch.float32),
            joined('final').to(torch.float32), arc_begin.to(torch.int32), joined('sources').to(torch.int32),
            joined('weights').to(torch.float32))
        self._which_graph = None if which is None else torch.tensor(which, dtype=torch.int32)

    def _open(self, device):
        self._weights = engine.PackedGraphs(*[value.to(device).contiguous() if torch.is_tensor(value) else value
                                              for value in self._graphs])
        which = None if self._which_graph is None else self._which_graph.to(device)
        return engine.viterbi_stream_state(device, self._streams, self.window, self._weights, which)

    def _push_piece(self, x, lengths, cap):
        return engine.viterbi_stream_push(self._state, self.window, x, lengths, self._weights, self.max_lag, cap,
                                          self._workspace, self.gop)

    def _flush_all(self, which):
        return engine.viterbi_stream_flush(self._state, self._streams, self.window, self._weights, self.max_lag + 1,
                                           which, self.gop)

    def _reset_all(self, which):
        engine.viterbi_stream_reset(self._state, self._streams, self.window, self._weights.max_states, which)

    @staticmethod
    def _workspace_bytes(streams, frames):
        return engine.library().ppg_viterbi_stream_workspace_bytes(streams, frames)


class PosteriorStream:
    """`posterior` on a live stream: the frames come a few at a time, the forward pass is carried across the pushes on
    the device, and every block of `block` frames is given out as soon as `lag` more frames have been received.

        sure = ppgs_amd.alignment.PosteriorStream(graph, block=16, lag=16, states=True)
        pieces = [sure.push(piece) for piece in arriving]        # each (40, k), k >= 0
        pieces.append(sure.flush())
        cleaned = ppgs_amd.alignment.joined_frames(pieces)       # (40, T): `posterior`'s PPG with a bounded look-ahead

    `graph` is a Graph for every stream, or with `batch=B` a list of B of them (the same object may stand for several
    streams and travels once), validated as `viterbi` validates it.  Block k = frames [kH, (k+1)H) is given out by the
    first push after which the stream has received (k+1)H + L frames, from a backward pass that starts at frame
    (k+1)H + L - 1 with an open end (the graph's `final` is not read): it is columns [kH, (k+1)H) of `posterior(ppg[:,
    :(k+1)H + L], the graph with final = 0)`, bit for bit, for every split into pushes.  block = 1, lag = 0 is the
    filtered posterior.  `window`, a multiple of 64 from 64 to 65536 with block + lag <= window, is the ring of every
    stream in frames.

    `batch=None` is one stream: push((40, F)).  `batch=B` is B streams side by side: push((B, 40, Fmax), lengths),
    lengths[b] in [0, Fmax] (None: Fmax each); the padding is never read.  push returns `PosteriorFrames(phonemes,
    states, begin, count, evidence, total)`: phonemes (40, cap) or (B, 40, cap) fp32 with cap = F + block - 1; states
    None, or with states=True the occupancy (cap, Smax) or (B, cap, Smax); column j is absolute frame begin + j, count,
    0-d or (B,), the number of columns given out, the columns at or past it zero; evidence, float64, the
    log-likelihood of the frames so far (`posterior(ppg[:, :p], the graph with final = 0).total`, bit for bit); total
    None.  A stream that could not take its frames has count = -1.  A frame that leaves no state alive makes the stream
    dead: evidence = -inf and count = 0 from then on.  A push longer than window - (block + lag - 1) is fed in pieces
    of that size whose columns are packed behind one another on the device.  A push of no frames calls nothing (its
    evidence is NaN: nothing was computed).
    flush(item=None) gives out the rest, [c, p), under the graph's own `final`, with total (float64) and evidence None:
    the last columns and the total of `posterior` of the whole recording, bit for bit (within its 65536 frames); it
    restarts every stream, or stream `item`; the streams it leaves out have count = 0 and total = NaN.  reset(item=None)
    starts every stream, or that one, again at frame 0.  `position` and `emitted` are host lists, kept without reading
    the device: the frames each stream has been PUSHED since its last flush or reset, and the emission point that goes
    with that many.  They are the device's p and c as long as every push was taken; a stream that is dead or answered
    count = -1 took nothing on the device, so there the lists run ahead until the next flush or reset puts both back to
    0.  Nothing here waits for the device."""

    def __init__(self, graph, block=16, lag=16, window=1024, batch=None, states=False, device=None):
        if (isinstance(window, bool) or not isinstance(window, int) or window % 64 or
                not engine.VITERBI_STREAM_MIN_WINDOW <= window <= engine.VITERBI_STREAM_MAX_WINDOW):
            raise ValueError(f'window must be a multiple of 64 from {engine.VITERBI_STREAM_MIN_WINDOW} to '
                             f'{engine.VITERBI_STREAM_MAX_WINDOW} frames, got {window!r}')
        if isinstance(block, bool) or not isinstance(block, int) or block < 1:
            raise ValueError(f'block must be a number of frames, at least 1, got {block!r}')
        if isinstance(lag, bool) or not isinstance(lag, int) or lag < 0:
            raise ValueError(f'lag must be a number of frames, at least 0, got {lag!r}')
        if block + lag > window:
            raise ValueError(f'block + lag must fit the window of {window} frames, got {block} + {lag}')
        if batch is not None and (isinstance(batch, bool) or not isinstance(batch, int) or
                                  not 1 <= batch <= engine.VITERBI_STREAM_MAX_STREAMS):
            raise ValueError(f'batch must be None or 1 to {engine.VITERBI_STREAM_MAX_STREAMS} streams, got {batch!r}')
        self.block, self.lag, self.window, self.batch, self.states = block, lag, window, batch, bool(states)
        self._streams = 1 if batch is None else batch
        self._gpu = device
        self._position = [0] * self._streams
        self._state = self._workspace = self._graphs = None
        self._uniform, self._flags = {}, {}
        packed, which = _graph_list(graph, batch, 'batch=', 'streams')
        counts, state_begin, arc_begin, joined = _joined_graphs(packed)
        lists = [_transposed(value) for value in packed]
        arc_base = arc_begin[state_begin[:-1]]
        out_begin = torch.cat([out[0][:-1] + arc_base[g] for g, out in enumerate(lists)] + [arc_begin[-1:]])
        self._host = engine.PackedOutGraphs(
            len(packed), sum(counts), int(arc_begin[-1]), max(counts), state_begin.to(torch.int32),
            joined('phonemes').to(torch.int32), joined('stay').to(torch.float32), joined('initial').to(torch.float32),
            joined('final').to(torch.float32), arc_begin.to(torch.int32), joined('sources').to(torch.int32),
            joined('weights').to(torch.float32), out_begin.to(torch.int32),
            torch.cat([out[1] for out in lists]).to(torch.int32), torch.cat([out[2] for out in lists]).to(torch.float32))
        self._which_graph = None if which is None else torch.tensor(which, dtype=torch.int32)

    @property
    def position(self):
        return list(self._position)

    @property
    def emitted(self):
        return [int(engine.library().ppg_posterior_stream_emitted(position, self.block, self.lag))
                for position in self._position]

    def _ensure(self, tensor=None):
        """The device side, made at the first call that needs it."""
        if self._state is None:
            device = core.device_for(self._gpu, tensor)
            with torch.cuda.device(device):
                self._graphs = engine.PackedOutGraphs(*[value.to(device).contiguous() if torch.is_tensor(value) else value
                                                        for value in self._host])
                which = None if self._which_graph is None else self._which_graph.to(device)
                self._state = engine.posterior_stream_state(device, self._streams, self.window, self._graphs,
                                                            self.block, self.lag, which)
        return self._state.device

    _which = RecognizeStream._which

    def _frames(self, post, states, begin, count, evidence=None, total=None):
        def drop(tensor):
            return tensor if tensor is None or self.batch is not None else tensor[0]
        return PosteriorFrames(*[drop(tensor) for tensor in (post, states, begin, count, evidence, total)])

    def push(self, ppg, lengths=None):
        if not torch.is_tensor(ppg) or ppg.dim() != (2 if self.batch is None else 3):
            raise ValueError(f'a push takes {"(40, frames)" if self.batch is None else f"({self.batch}, 40, frames)"}, '
                             f'got {tuple(getattr(ppg, "shape", ()))}')
        if ppg.shape[-2] != config.OUTPUT_CHANNELS:
            raise ValueError(f'PPG must have {config.OUTPUT_CHANNELS} channels, got {tuple(ppg.shape)}')
        if self.batch is not None and ppg.shape[0] != self.batch:
            raise ValueError(f'a push takes {self.batch} streams, got {ppg.shape[0]}')
        frames = ppg.shape[-1]
        if lengths is None:
            own = [frames] * self._streams
        else:
            if self.batch is None:
                raise ValueError('lengths go with a batch of streams: slice a single PPG instead')
            if torch.is_tensor(lengths):
                lengths = lengths.detach().cpu().reshape(-1).tolist()
            own = [int(value) for value in (lengths if isinstance(lengths, (list, tuple)) else [lengths])]
            if len(own) != self._streams:
                raise ValueError(f'lengths has {len(own)} entries for {self._streams} streams')
            for value in own:
                if not 0 <= value <= frames:
                    raise ValueError(f'lengths: {value} is outside [0, {frames}]')
        for position, value in zip(self._position, own):
            if position + value > 2 ** 31 - 1:
                raise ValueError(f'a stream takes at most {2 ** 31 - 1} frames between resets, got {position} + {value}')
        device = self._ensure(ppg)
        most = self._graphs.max_states
        cap = max(1, frames + self.block - 1)
        if frames == 0:
            return self._frames(
                torch.zeros((self._streams, 40, 0), dtype=torch.float32, device=device),
                torch.zeros((self._streams, 0, most), dtype=torch.float32, device=device) if self.states else None,
                torch.tensor(self.emitted, dtype=torch.int32).to(device),
                torch.zeros((self._streams,), dtype=torch.int32, device=device),
                torch.full((self._streams,), math.nan, dtype=torch.float64, device=device))
        x = ppg.to(device=device, dtype=torch.float32)
        x = x if self.batch is not None else x[None]
        piece = self.window - (self.block + self.lag - 1)                # what a stream can always still take
        piece = max(1, min(piece, engine.POSTERIOR_STREAM_MAX_PUSH // self._streams))
        whole = None
        if lengths is not None:                                          # through pinned memory: the copy does not wait
            whole = torch.tensor(own, dtype=torch.int32).pin_memory().to(device, non_blocking=True)
        need = engine.library().ppg_posterior_stream_workspace_bytes(self._streams, min(frames, piece))
        if self._workspace is None or self._workspace.numel() < need:
            self._workspace = torch.empty((need,), dtype=torch.uint8, device=device)
        packed = None
        for at in range(0, frames, piece):
            size = min(piece, frames - at)
            if whole is None:
                if size not in self._uniform:
                    if len(self._uniform) >= 64:                         # (a stream pushes a few sizes over and over)
                        self._uniform.clear()
                    self._uniform[size] = torch.full((self._streams,), size, dtype=torch.int32, device=device)
                on_device = self._uniform[size]
            else:
                on_device = (whole - at).clamp_(0, size)
            part = engine.posterior_stream_push(
                self._state, self.window, x[:, :, at:at + size].contiguous(), on_device, self._graphs,
                cap if frames <= piece else size + self.block - 1, self._workspace, self.states)
            if frames <= piece:
                packed = part
                break
            packed = self._pack(packed, part, cap)
        if frames > piece:                                               # without the slot that took what was past count
            post, states, begin, count, evidence = packed
            packed = (post[:, :, :cap], None if states is None else states[:, :cap], begin, count, evidence)
        self._position = [position + value for position, value in zip(self._position, own)]
        return self._frames(*packed)

    def _pack(self, packed, part, cap):
        """The columns of a piece behind those of the pieces before it, on the device: the counts add up (-1 stays), the
        first piece's begin and the last piece's evidence stand."""
        post, states, begin, count, evidence = part
        if packed is None:
            packed = (post.new_zeros((self._streams, 40, cap + 1)),
                      None if states is None else states.new_zeros((self._streams, cap + 1, states.shape[2])), begin,
                      torch.zeros_like(count), evidence)
        slots = torch.arange(post.shape[2], device=count.device)[None, :]
        fits = (slots < count[:, None]) & (packed[3][:, None] >= 0)
        where = torch.where(fits, (packed[3][:, None] + slots).clamp_(max=cap), cap).to(torch.int64)
        packed[0].scatter_(2, where[:, None, :].expand(-1, 40, -1), post)
        packed[0][:, :, cap] = 0.
        if states is not None:
            packed[1].scatter_(1, where[:, :, None].expand(-1, -1, states.shape[2]), states)
            packed[1][:, cap] = 0.
        total = torch.where((packed[3] < 0) | (count < 0), torch.full_like(count, -1), packed[3] + count)
        return packed[0], packed[1], packed[2], total, evidence

    def flush(self, item=None):
        which = self._which(item)
        self._ensure()
        post, states, begin, count, total = engine.posterior_stream_flush(
            self._state, self._streams, self.window, self._graphs, max(1, self.block + self.lag - 1), which,
            self.states)
        self._position = [0 if item is None or b == item else position for b, position in enumerate(self._position)]
        return self._frames(post, states, begin, count, None, total)

    def reset(self, item=None):
        which = self._which(item)
        self._ensure()
        engine.posterior_stream_reset(self._state, self._streams, self.window, self._graphs.max_states, which)
        self._position = [0 if item is None or b == item else position for b, position in enumerate(self._position)]


def joined_frames(pieces):
    """The outputs of the pushes and the flush of a PosteriorStream, in order, as one PPG: the first `count` columns of
    every piece behind one another, (40, T) for one stream, a list of B such tensors for a batch.  A piece with count < 0
    (frames the stream could not take) adds nothing.  Host only: this is where the counts are read."""
    pieces = list(pieces)
    if not pieces:
        raise ValueError('joined_frames takes at least one PosteriorFrames')
    batched = pieces[0].phonemes.dim() == 3
    counts = [piece.count.reshape(-1).tolist() for piece in pieces]
    streams = len(counts[0])
    joined = []
    for b in range(streams):
        columns = [(piece.phonemes[b] if batched else piece.phonemes)[:, :max(0, count[b])]
                   for piece, count in zip(pieces, counts)]
        joined.append(torch.cat(columns, dim=1))
    return joined if batched else joined[0]


def run_segments(runs, sample_rate=config.SAMPLE_RATE, hopsize=config.HOPSIZE):
    """The runs of a push or a flush (Runs or StateRuns) as a host list of (phoneme name, start seconds, end seconds, score, gop), the first
    `count` of them, in stream order (gop None if the stream keeps none); a batch of streams gives a list of such
    lists.  Host only: this is where the results are read."""
    phonemes, begin, end = runs.phonemes.tolist(), runs.begin.tolist(), runs.end.tolist()
    score, count = runs.score.tolist(), runs.count.tolist()
    gop = None if runs.gop is None else runs.gop.tolist()

    def walk(phonemes, begin, end, score, gop, count):
        return [(PHONEMES[phonemes[r]], begin[r] * hopsize / sample_rate, end[r] * hopsize / sample_rate, score[r],
                 None if gop is None else gop[r]) for r in range(min(max(count, 0), len(phonemes)))]
    if isinstance(count, list):
        return [walk(phonemes[b], begin[b], end[b], score[b], None if gop is None else gop[b], count[b])
                for b in range(len(count))]
    return walk(phonemes, begin, end, score, gop, count)


def hit_segments(hits, sample_rate=config.SAMPLE_RATE, hopsize=config.HOPSIZE):
    """The hits of a search as a host list of (start seconds, end seconds, total, mean), the first `count` of them, best
    first; nested per sequence and per recording as the search was (a list per recording of lists per sequence).  Host
    only: this is where the results are read."""
    begin, end, count = hits.begin.tolist(), hits.end.tolist(), hits.count.tolist()
    total, mean = hits.total.tolist(), hits.mean.tolist()

    def walk(begin, end, total, mean, count):
        if isinstance(count, list):
            return [walk(*row) for row in zip(begin, end, total, mean, count)]
        return [(begin[h] * hopsize / sample_rate, end[h] * hopsize / sample_rate, total[h], mean[h])
                for h in range(max(count, 0))]
    return walk(begin, end, total, mean, count)


def segments(alignment, sample_rate=config.SAMPLE_RATE, hopsize=config.HOPSIZE):
    """An alignment (or a decoding) of one utterance as a host list of (phoneme name, start seconds, end seconds,
    score, gop), one per phoneme; a batch gives a list of such lists.  Fields the input lacks are None."""
    phonemes, starts = alignment.phonemes, alignment.starts
    score, gop = getattr(alignment, 'score', None), getattr(alignment, 'gop', None)
    if isinstance(phonemes, (list, tuple)):
        return [segments(Alignment(phonemes[b], starts[b], None, None if score is None else score[b],
                                   None if gop is None else gop[b]), sample_rate, hopsize)
                for b in range(len(phonemes))]
    names = [PHONEMES[index] for index in phonemes.tolist()]
    edges = [frame * hopsize / sample_rate for frame in starts.tolist()]
    if len(edges) != len(names) + 1:
        raise ValueError(f'{len(names)} phonemes take {len(names) + 1} starts, got {len(edges)}')
    score = [None] * len(names) if score is None else score.tolist()
    gop = [None] * len(names) if gop is None else gop.tolist()
    return [(name, edges[n], edges[n + 1], score[n], gop[n]) for n, name in enumerate(names)]


def frame_labels(starts, phonemes, frames):
    """An alignment expanded to one label per frame: (frames,) with phonemes[n] at starts[n] <= t < starts[n + 1].
    Plain tensor arithmetic: works on CPU and device tensors alike."""
    if starts.dim() != 1 or phonemes.dim() != 1 or starts.shape[0] != phonemes.shape[0] + 1 or phonemes.shape[0] < 1:
        raise ValueError(f'N >= 1 phonemes take N + 1 starts, got {tuple(phonemes.shape)} and {tuple(starts.shape)}')
    if frames < 1:
        raise ValueError(f'frames must be positive, got {frames}')
    inner = starts[1:-1].to(torch.int64).contiguous()           # the N - 1 boundaries inside the utterance
    time = torch.arange(frames, dtype=torch.int64, device=starts.device)
    return phonemes.to(starts.device)[torch.bucketize(time, inner, right=True)]


def edit_costs(sub=None, delete=None, insert=None):
    """The costs of `edit_distance` as checked CPU tensors (sub (40, 40), delete (40,), insert (40,)), fp32, finite
    and >= 0; one left out is its unit default (1 - I, ones).  None if all three are left out.  Host only."""
    if sub is None and delete is None and insert is None:
        return None
    count = len(PHONEMES)
    defaults = (1. - torch.eye(count), torch.ones(count), torch.ones(count))
    out = []
    for value, default, name in zip((sub, delete, insert), defaults, ('sub', 'delete', 'insert')):
        if value is None:
            value = default
        if not torch.is_tensor(value) or tuple(value.shape) != tuple(default.shape) or not value.is_floating_point():
            raise ValueError(f'{name} must be a floating-point tensor of shape {tuple(default.shape)}')
        value = value.detach().to(device='cpu', dtype=torch.float32).contiguous()
        if not bool(torch.isfinite(value).all()) or bool((value < 0).any()):
            raise ValueError(f'{name} must be finite and >= 0')
        out.append(value)
    return tuple(out)


def _ignored(ignore):
    """`ignore` as a sorted list of phoneme indices."""
    if ignore is None:
        return []
    if isinstance(ignore, (str, int)) and not isinstance(ignore, bool):
        ignore = [ignore]
    return sorted(set(_sequence(list(ignore))))


def _edit_rows(sequences, what, ignore):
    """The host checks of one side of an edit-distance call: every sequence as a list of checked indices with the
    ignored ones dropped, or, for a device tensor, as it is (shape and type checked here, its values by the kernel)."""
    rows = []
    for sequence in sequences:
        if torch.is_tensor(sequence) and sequence.is_cuda:
            if sequence.dim() != 1 or sequence.is_floating_point() or sequence.is_complex() or \
                    sequence.dtype == torch.bool:
                raise ValueError(f'a phoneme sequence must be a one-dimensional integer tensor, got '
                                 f'{tuple(sequence.shape)} {sequence.dtype}')
            rows.append(sequence)
        else:
            rows.append([value for value in _sequence(sequence) if value not in ignore])
        if len(rows[-1]) > EDIT_MAX_TOKENS:
            raise ValueError(f'{what}: edit distance takes at most {EDIT_MAX_TOKENS} phonemes per sequence, got '
                             f'{len(rows[-1])}')
    return rows


def _edit_table(rows, ignore, device):
    """The rows of _edit_rows as (a padded int32 table on the device, its lengths as an int32 device tensor).
    Nothing here waits for the device."""
    width = max(1, max(len(row) for row in rows))
    host = torch.zeros((len(rows), width), dtype=torch.int32)
    for index, row in enumerate(rows):
        if isinstance(row, list) and row:
            host[index, :len(row)] = torch.tensor(row, dtype=torch.int32)
    table = host.to(device)
    lengths = torch.tensor([len(row) for row in rows], dtype=torch.int32).to(device)
    on_device = [index for index, row in enumerate(rows) if not isinstance(row, list)]
    for index in on_device:
        row = rows[index].to(device=device, dtype=torch.int64)
        # an index that would not survive the narrowing to int32 stays invalid for the kernel to find
        row = torch.where((row < 0) | (row >= len(PHONEMES)), torch.full_like(row, -1), row)
        table[index, :len(row)] = row.to(torch.int32)
    if ignore and on_device:
        # drop the ignored phonemes of the device rows in order, without learning how many there were
        keep = torch.arange(width, device=device)[None] < lengths[:, None]
        for index in ignore:
            keep &= table != index
        target = torch.where(keep, torch.cumsum(keep, 1) - 1, torch.full((1, 1), width, device=device))
        packed = torch.zeros((len(rows), width + 1), dtype=torch.int32, device=device)
        packed.scatter_(1, target, table)
        table, lengths = packed[:, :width].contiguous(), keep.sum(1).to(torch.int32)
    return table, lengths


def _edit_sides(reference, hypothesis):
    """(batched, references, hypotheses).  A pair is two sequences; a batch is two lists (or tuples) of as many
    sequences.  A side counts as a batch if it is a non-empty list holding at least one list, tuple or tensor of one
    or more dimensions; the call is a batch if either side is one, and then both must be.  An empty list is therefore
    always an empty sequence: two empty lists are one pair of empty sequences, never a batch of none."""
    def is_batch(value):
        return isinstance(value, (list, tuple)) and any(
            isinstance(v, (list, tuple)) or (torch.is_tensor(v) and v.dim() > 0) for v in value)
    if not (is_batch(reference) or is_batch(hypothesis)):
        return False, [reference], [hypothesis]
    if not (is_batch(reference) and is_batch(hypothesis)) or len(reference) != len(hypothesis):
        raise ValueError('a batch is two lists of as many sequences')
    return True, list(reference), list(hypothesis)


def edit_distance(reference, hypothesis, sub=None, delete=None, insert=None, ignore=None, ops=False):
    """The weighted edit distance of phoneme sequences and the alignment behind it -- what a phoneme error rate and a
    list of mispronunciations are made of (ppg_edit_distance).

    One pair: two sequences of phoneme names or indices, or one-dimensional integer tensors on the CPU or the device
    (`Decoding.phonemes`, `Recognition.phonemes`, a transcript); either may be empty.  A batch: two lists of as many
    such sequences.  A list that holds a list, a tuple or a tensor of one or more dimensions is a batch; an empty
    list is an empty sequence, so two empty lists are one pair of empty sequences and a batch has at least one pair.  `sub` (40, 40), `delete` (40,) and `insert` (40,) are finite costs >= 0 indexed by reference and
    hypothesis phoneme; the defaults are the unit costs 1 - I and ones.  `ignore` names phonemes (e.g. '<silent>')
    that are dropped from both sides first.

    Over the fp32 table D[0, 0] = 0 a cell prefers the diagonal D[i-1, j-1] + sub, then the deletion D[i-1, j] +
    delete, then the insertion D[i, j-1] + insert, a later one winning only if strictly smaller; the path is read back
    from the last cell.  Returns EditDistance(total, hits, substitutions, deletions, insertions, ops): device tensors,
    0-d for a pair and (B,) for a batch (total fp32, the counts int32); a diagonal step is a hit if the two phonemes
    are equal and a substitution otherwise.  With `ops`, a (K, 3) int32 device tensor per pair of (kind, i, j) in
    forward order: 0 hit, 1 substitution, 2 deletion of reference[i] (j = -1), 3 insertion of hypothesis[j] (i = -1);
    indices count the phonemes left after `ignore`.  A device sequence with an index outside [0, 40) gives total NaN
    and zero counts.  Batch results equal the single calls bit for bit."""
    batched, references, hypotheses = _edit_sides(reference, hypothesis)
    costs = edit_costs(sub, delete, insert)
    ignore = _ignored(ignore)
    rows = [_edit_rows(references, 'reference', ignore), _edit_rows(hypotheses, 'hypothesis', ignore)]
    device = core.device_for(None, next((row for row in rows[0] + rows[1] if torch.is_tensor(row)), None))
    ref, lengths_ref = _edit_table(rows[0], ignore, device)
    hyp, lengths_hyp = _edit_table(rows[1], ignore, device)
    if costs is not None:
        costs = [c.to(device) for c in costs]
    total, counts, table, count = engine.edit_pairs(ref, hyp, lengths_ref, lengths_hyp, costs, want_ops=ops)
    out_ops = None
    if ops:
        out_ops = [table[b, :k] for b, k in enumerate(count.tolist())]
    if not batched:
        return EditDistance(total[0], counts[0, 0], counts[0, 1], counts[0, 2], counts[0, 3],
                            out_ops[0] if ops else None)
    return EditDistance(total, counts[:, 0], counts[:, 1], counts[:, 2], counts[:, 3], out_ops)
