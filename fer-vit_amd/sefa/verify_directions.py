"""Reference `sefa/verify_directions.py` under its own name: see fervit.sefa."""
from fervit.sefa import select_directions, verify_non_expression_directions  # noqa: F401
