"""Moved to neurec_amd/model/_common.py; the names this module had stay importable from here."""
from .._common import PAIRWISE_STRUCTURE, POINTWISE_STRUCTURE, predict_scores, train_history_model  # noqa: F401
