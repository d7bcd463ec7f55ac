"""Numerical inversion of elementwise monotone maps (reference ``bijections/numerical_inversion.py``).

``bisection_no_gradient`` is the ATen composite inverse of the sigmoidal transformers
(``transformers/combination/sigmoid.py``): host tensors, fp64 and calls under autograd.  fp32 tensors on a HIP
device run the whole search inside one kernel instead (csrc/tfk_dsf.hip).
"""
from __future__ import annotations

from typing import Callable, Tuple, Union

import torch


def _bound(value: Union[torch.Tensor, float, None], like: torch.Tensor, default: float) -> torch.Tensor:
    if value is None:
        return torch.full_like(like, default)
    if isinstance(value, float):
        return torch.full_like(like, value)
    return value


def bisection_no_gradient(f: Callable, y: torch.Tensor, a: Union[torch.Tensor, float] = None,
                          b: Union[torch.Tensor, float] = None, n_iterations: int = 500,
                          atol: float = 1e-9) -> Tuple[torch.Tensor, torch.Tensor]:
    """Solve ``f(x)[0] == y`` elementwise on ``[a, b]`` (default ``[-100, 100]``) for an increasing ``f`` that returns
    ``(value, log_det)``.  Returns ``(x, -log_det)``.

    Kept as the reference has it: the bracket moves on ``f(c) < y``; the loop stops once the new midpoints are
    ``allclose`` to the previous ones over the WHOLE batch (``atol``, rtol 1e-5); ``x`` is the last midpoint while the
    log-det is the one ``f`` returned at the midpoint before it.  No gradient flows through the search.
    """
    lo, hi = _bound(a, y, -100.0), _bound(b, y, 100.0)
    mid = (lo + hi) / 2
    log_det = None
    for _ in range(n_iterations):
        value, log_det = f(mid)
        below = value < y
        lo = torch.where(below, mid, lo)
        hi = torch.where(below, hi, mid)
        previous, mid = mid, (lo + hi) / 2
        if torch.allclose(previous, mid, atol=atol):
            break
    return mid, -log_det
