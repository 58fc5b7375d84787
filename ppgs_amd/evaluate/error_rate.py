"""Phoneme error rate of a recogniser against transcripts without times (ppg_edit_distance)."""
import torch

from .. import alignment, core, engine
from ..phonemes import PHONEMES


def format_error_rate(statistics):
    """The result dict of ErrorRate from its statistics as EDIT_STATISTICS host integers.  Zero counts give NaN."""
    count = len(PHONEMES)
    words = [int(v) for v in statistics]
    if len(words) != engine.EDIT_STATISTICS:
        raise ValueError(f'statistics have {engine.EDIT_STATISTICS} words, got {len(words)}')
    pairs, invalid = words[-2:]
    if invalid:
        raise ValueError(f'{invalid} pairs have a negative length or a phoneme index outside [0, {count})')
    table = [words[row * (count + 1):(row + 1) * (count + 1)] for row in range(count + 1)]

    def ratio(numerator, denominator):
        return float(numerator) / float(denominator) if denominator else float('nan')
    hits = sum(table[p][p] for p in range(count))
    substitutions = sum(sum(table[p][:count]) for p in range(count)) - hits
    deletions = sum(table[p][count] for p in range(count))
    insertions = sum(table[count][:count])
    reference = hits + substitutions + deletions
    results = {
        'PER': ratio(substitutions + deletions + insertions, reference),
        'Hits': hits, 'Substitutions': substitutions, 'Deletions': deletions, 'Insertions': insertions,
        'Reference phonemes': reference, 'Pairs': pairs}
    for p, phoneme in enumerate(PHONEMES):
        results[f'PER/{phoneme}'] = ratio(sum(table[p]) - table[p][p], sum(table[p]))
        results[f'Insertions/{phoneme}'] = table[count][p]
    return results


class ErrorRate:
    """Phoneme error rate over a corpus: update(references, hypotheses) per batch of sequences as
    `alignment.edit_distance` takes them, __call__() for the result dict.

    update() is one library call per workspace-sized group of pairs and waits for nothing; the statistics -- which
    reference phoneme met which hypothesis phoneme, was deleted, or was inserted -- stay on the device as 64-bit
    integer counts.  Integer sums do not depend on their order, so the results are the same bit for bit however the
    pairs are ordered, grouped into updates or split over calls.

    __call__() returns 'PER' = (S + D + I) / N (NaN for N = 0), 'Hits', 'Substitutions', 'Deletions', 'Insertions',
    'Reference phonemes', 'Pairs', and per phoneme 'PER/{phoneme}' = (S_p + D_p) / N_p over the reference phoneme p
    and 'Insertions/{phoneme}'.  It raises if a pair was invalid (a device sequence with an index outside [0, 40))."""

    def __init__(self, sub=None, delete=None, insert=None, ignore=None, gpu=None):
        costs = alignment.edit_costs(sub, delete, insert)
        self.ignore = alignment._ignored(ignore)
        self.device = core.device_for(gpu)
        self.costs = None if costs is None else [c.to(self.device) for c in costs]
        self.statistics = torch.zeros((engine.EDIT_STATISTICS,), dtype=torch.int64, device=self.device)

    def update(self, references, hypotheses):
        if not isinstance(references, (list, tuple)) or not isinstance(hypotheses, (list, tuple)) or \
                len(references) != len(hypotheses):
            raise ValueError('update takes two lists of as many sequences')
        if not references:
            return
        rows = [alignment._edit_rows(references, 'reference', self.ignore),
                alignment._edit_rows(hypotheses, 'hypothesis', self.ignore)]
        ref, lengths_ref = alignment._edit_table(rows[0], self.ignore, self.device)
        hyp, lengths_hyp = alignment._edit_table(rows[1], self.ignore, self.device)
        engine.edit_pairs(ref, hyp, lengths_ref, lengths_hyp, self.costs, statistics=self.statistics)

    def reset(self):
        self.statistics.zero_()

    def confusion(self):
        """The (41, 41) int64 table on the device: [p, q] reference p met hypothesis q, [p, 40] deletions of p,
        [40, q] insertions of q."""
        return self.statistics[:-2].reshape(len(PHONEMES) + 1, len(PHONEMES) + 1).clone()

    def __call__(self):
        return format_error_rate(self.statistics.cpu().tolist())
