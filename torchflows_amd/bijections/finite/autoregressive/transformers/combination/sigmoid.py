"""Deep sigmoidal transformers (Huang et al. 2018, neural autoregressive flows) -- ATen composite path.

Numerics follow the reference's ``transformers/combination/sigmoid.py``.  Per element a ``Sigmoid`` takes ``3 K``
parameters ``[da (K) | db (K) | dw (K)]`` with ``K = hidden_dim``:

    a = softplus(log(e - 1 - 1e-3) + da / 1000) + 1e-3,   b = db / 1000,   w = softmax(dw / 1000)
    d = clip(sum_i w_i sigmoid(a_i x + b_i), 1e-6, 1 - 1e-6),   z = log d - log1p(-d)

The log-det is what the reference returns -- the SUM over the K hidden units of
``(log d - log(1 - d)) + log w_i + log sigmoid(c_i) + log sigmoid(-c_i) + log a_i`` -- not the logarithm of dz/dx
(kept reference behaviour).  The inverse is a bisection on [-10, 10] without gradient
(``numerical_inversion.bisection_no_gradient``).  ``DeepSigmoid`` chains ``n_hidden_layers`` of them.  The HIP kernels
are csrc/tfk_dsf.hip; this module serves host tensors, fp64, autograd through the inverse and unsupported sizes.
"""
from __future__ import annotations

import math
from typing import Sequence, Tuple

import torch
import torch.nn.functional as F

from torchflows_amd.bijections.finite.autoregressive.transformers.base import ScalarTransformer
from torchflows_amd.bijections.finite.autoregressive.transformers.combination.base import Combination
from torchflows_amd.bijections.finite.autoregressive.transformers.combination.sigmoid_util import (
    log_sigmoid, log_softmax)
from torchflows_amd.bijections.numerical_inversion import bisection_no_gradient
from torchflows_amd.utils import event_size, sum_except_batch


def inverse_sigmoid(p: torch.Tensor) -> torch.Tensor:
    return torch.log(p) - torch.log1p(-p)


class Sigmoid(ScalarTransformer):
    """``z = inverse_sigmoid(w . sigmoid(a x + b))`` with ``a > 0``, ``w > 0``, ``sum(w) = 1``."""
    native_kind = "dsf"
    n_components = 1

    def __init__(self, event_shape: Sequence[int], hidden_dim: int = None, min_scale: float = 1e-3):
        super().__init__(event_shape)
        if hidden_dim is None:
            hidden_dim = max(4, 5 * int(math.log10(event_size(self.event_shape))))
        self.hidden_dim = hidden_dim
        self.min_scale = min_scale
        self.const = 1000
        self.default_u_a = math.log(math.e - 1 - self.min_scale)

    @property
    def parameter_shape_per_element(self) -> Tuple[int, ...]:
        return (3 * self.hidden_dim,)

    @property
    def default_parameters(self) -> torch.Tensor:
        return torch.zeros(self.parameter_shape)

    def extract_parameters(self, h: torch.Tensor):
        """h (n, 3 K) -> a, b, w, log w, each (n, K)."""
        K = self.hidden_dim
        da, db, dw = h[:, :K], h[:, K:2 * K], h[:, 2 * K:3 * K]
        a = F.softplus(self.default_u_a + da / self.const) + self.min_scale
        b = db / self.const
        w_pre = 0.0 + dw / self.const
        return a, b, torch.softmax(w_pre, dim=-1), log_softmax(w_pre, dim=-1)

    def forward_1d(self, x: torch.Tensor, h: torch.Tensor, eps: float = 1e-6):
        """x (n,), h (n, 3 K) -> z (n,), log_det (n,)."""
        a, b, w, log_w = self.extract_parameters(h)
        c = a * x[:, None] + b
        d = torch.clip(torch.einsum("...i,...i->...", w, torch.sigmoid(c)), eps, 1 - eps)
        z = inverse_sigmoid(d)
        log_t1 = (torch.log(d) - torch.log(1 - d))[:, None]
        log_t3 = log_sigmoid(c) + log_sigmoid(-c)
        log_det = torch.sum(log_t1 + log_w + log_t3 + torch.log(a), dim=1)
        return z, log_det

    def inverse_1d(self, z: torch.Tensor, h: torch.Tensor):
        return bisection_no_gradient(lambda inputs: self.forward_1d(inputs, h), z, a=-10.0, b=10.0)

    def _apply_flat(self, fn, v: torch.Tensor, h: torch.Tensor):
        out, log_det = fn(v.reshape(-1), h.reshape(-1, h.shape[-1]))
        return out.view_as(v), sum_except_batch(log_det.view_as(v), self.event_shape)

    def forward(self, x: torch.Tensor, h: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
        return self._apply_flat(self.forward_1d, x, h)

    def inverse(self, z: torch.Tensor, h: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
        return self._apply_flat(self.inverse_1d, z, h)


class DeepSigmoid(Combination):
    """``n_hidden_layers`` ``Sigmoid`` transformers in sequence; keyword arguments go to each of them."""
    native_kind = "dsf"

    def __init__(self, event_shape: Sequence[int], n_hidden_layers: int = 2, **kwargs):
        super().__init__(event_shape, [Sigmoid(event_shape, **kwargs) for _ in range(n_hidden_layers)])

    @property
    def hidden_dim(self) -> int:
        return self.components[0].hidden_dim
