"""Reference `sefa/factorize.py` under its own name: see fervit.sefa."""
from fervit.sefa import factorize_stylegan_weights, factorize_weight  # noqa: F401
