"""Evaluation of trained models (reference `eval/evaluate_model.py`) on the MI355X modules: predictions,
probabilities, confusion matrix and classification report from device kernels (fervit.metrics), the
token similarities of its attention-like plot from fervit.explain. No plotting."""
