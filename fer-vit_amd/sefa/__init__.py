"""SeFa non-expression directions (reference `sefa/`): factorisation on the host, verification on the device."""
from fervit.sefa import (factorize_stylegan_weights, factorize_weight, select_directions,  # noqa: F401
                         verify_non_expression_directions)
