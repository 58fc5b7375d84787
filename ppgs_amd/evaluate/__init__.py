"""Evaluation (reference ``python -m ppgs.evaluate``): frame metrics of a checkpoint against labels,
accumulated on the GPU by one kernel launch per batch (``ppg_metrics_update``) and read once at the end; and the
phoneme error rate of a recogniser against transcripts without times (``ErrorRate``, ``ppg_edit_distance``)."""
from .metrics import Metrics, format_results, phoneme_weights   # noqa: F401
from .core import across_precisions, from_dataloader, save      # noqa: F401
from .error_rate import ErrorRate, format_error_rate             # noqa: F401
