"""Dense sigmoidal transformers (Huang et al. 2018, neural autoregressive flows) -- ATen composite path.

Numerics follow the dense half of the reference's ``transformers/combination/sigmoid.py``.  ``DenseSigmoid`` is
``n_dense_layers + 2`` inner transforms 1 -> H -> ... -> H -> 1 per element, each
``v' = inverse_sigmoid(w @ sigmoid(a * (u @ v) + b))`` with row-softmax matrices ``w (o, o)`` and ``u (o, i)``; per inner
transform an element takes ``[da (o) | db (o) | dw (o o) | du (o i)]``.  Its log-det is, as in the reference, the SUM over
all entries of ``log_dot`` of the o x o log-Jacobian factors with ``log u`` -- not a log-determinant.  ``DeepDenseSigmoid``
chains ``n_hidden_layers`` of them.  The HIP kernel is csrc/tfk_dense_dsf.hip (``native_kind = "dense"``).

The classes live here and not beside ``Sigmoid`` / ``DeepSigmoid`` in ``sigmoid.py``, where the reference keeps them:
tests/test_host_dsf.py pins that module's contents.
"""
from __future__ import annotations

import math
from typing import List, Sequence, Tuple

import torch
import torch.nn as nn
import torch.nn.functional as F

from torchflows_amd.bijections.finite.autoregressive.transformers.base import ScalarTransformer
from torchflows_amd.bijections.finite.autoregressive.transformers.combination.base import Combination
from torchflows_amd.bijections.finite.autoregressive.transformers.combination.sigmoid import inverse_sigmoid
from torchflows_amd.bijections.finite.autoregressive.transformers.combination.sigmoid_util import (
    log_dot, log_sigmoid, log_softmax)
from torchflows_amd.bijections.numerical_inversion import bisection_no_gradient


class DenseSigmoidInnerTransform(nn.Module):
    """``v (n, e, i) -> inverse_sigmoid(w @ sigmoid(a * (u @ v) + b)) (n, e, o)``; h is ``(n, e, o o + 2 o + o i)``."""

    def __init__(self, input_size: int, output_size: int, event_size: int, min_scale: float = 1e-3):
        super().__init__()
        self.input_size = input_size
        self.output_size = output_size
        self.event_size = event_size
        self.min_scale = min_scale
        self.const = 1000
        self.default_u_a = math.log(math.e - 1 - self.min_scale)

    @property
    def n_parameters(self) -> int:
        o, i = self.output_size, self.input_size
        return o * o + 2 * o + o * i

    def extract_parameters(self, h: torch.Tensor):
        """h (n, e, P) -> a, b (n, e, o), w, log w (n, e, o, o), u, log u (n, e, o, i)."""
        o, i = self.output_size, self.input_size
        da, db, dw, du = torch.split(h, [o, o, o * o, o * i], dim=-1)
        u_pre = 0.0 + du.reshape(*h.shape[:2], o, i) / self.const
        w_pre = 0.0 + dw.reshape(*h.shape[:2], o, o) / self.const
        a = F.softplus(self.default_u_a + da / self.const) + self.min_scale
        b = db / self.const
        return (a, b, torch.softmax(w_pre, dim=-1), log_softmax(w_pre, dim=-1),
                torch.softmax(u_pre, dim=-1), log_softmax(u_pre, dim=-1))

    def forward_1d(self, x: torch.Tensor, h: torch.Tensor, eps: float = 1e-6):
        """x (n, e, i), h (n, e, P) -> z (n, e, o), log_det (n, e)."""
        a, b, w, log_w, u, log_u = self.extract_parameters(h)
        c = a * torch.einsum("beoi,bei->beo", u, x) + b
        d = torch.clip(torch.einsum("beij,bej->bei", w, torch.sigmoid(c)), eps, 1 - eps)
        z = inverse_sigmoid(d)
        d_, c_, a_ = d.flatten(0, 1), c.flatten(0, 1), a.flatten(0, 1)
        log_t1 = (torch.log(d_) - torch.log(1 - d_))[:, :, None]
        log_t3 = (log_sigmoid(c_) + log_sigmoid(-c_))[:, None, :]
        m1 = (log_t1 + log_w.flatten(0, 1) + log_t3 + torch.log(a_)[:, None, :])[:, :, :, None]
        m2 = log_u.flatten(0, 1)[:, None, :, :]
        log_det = torch.sum(log_dot(m1, m2), dim=(1, 2, 3))
        return z, log_det.view(*z.shape[:2])


class DenseSigmoid(ScalarTransformer):
    """Inner transforms 1 -> H, ``n_dense_layers`` x (H -> H), H -> 1 applied to every element."""
    native_kind = "dense"
    n_components = 1

    def __init__(self, event_shape: Sequence[int], n_dense_layers: int = 1, hidden_size: int = 8):
        super().__init__(event_shape)
        self.n_dense_layers = n_dense_layers
        self.hidden_size = hidden_size
        self.layers = nn.ModuleList(
            [DenseSigmoidInnerTransform(1, hidden_size, self.n_dim)]
            + [DenseSigmoidInnerTransform(hidden_size, hidden_size, self.n_dim) for _ in range(n_dense_layers)]
            + [DenseSigmoidInnerTransform(hidden_size, 1, self.n_dim)])

    @property
    def parameter_shape_per_element(self) -> Tuple[int, ...]:
        return (sum(layer.n_parameters for layer in self.layers),)

    @property
    def default_parameters(self) -> torch.Tensor:
        return torch.zeros(size=tuple(self.parameter_shape))

    def split_parameters(self, h: torch.Tensor):
        return torch.split(h, [layer.n_parameters for layer in self.layers], dim=-1)

    def forward_1d(self, x_flat: torch.Tensor, h_split_flat: List[torch.Tensor]):
        """x (n, e), per-layer h (n, e, P_l) -> z (n, e), log_det (n,) summed over the event."""
        v = x_flat[..., None]
        log_det = None
        for layer, h in zip(self.layers, h_split_flat):
            v, increment = layer.forward_1d(v, h)
            log_det = increment if log_det is None else log_det + increment
        return v[..., 0], log_det.sum(dim=1)

    def inverse_1d(self, z: torch.Tensor, h: List[torch.Tensor]):
        return bisection_no_gradient(lambda inputs: self.forward_1d(inputs, h), z, a=-10.0, b=10.0)

    def _apply_rows(self, fn, v: torch.Tensor, h: torch.Tensor):
        batch = v.shape[:v.dim() - len(self.event_shape)]
        n = int(math.prod(batch))
        h_split = [part.reshape(n, self.n_dim, -1) for part in self.split_parameters(h)]
        out, log_det = fn(v.reshape(n, self.n_dim), h_split)
        return out.view(*batch, *self.event_shape), log_det.view(*batch)

    def forward(self, x: torch.Tensor, h: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
        return self._apply_rows(self.forward_1d, x, h)

    def inverse(self, z: torch.Tensor, h: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
        return self._apply_rows(self.inverse_1d, z, h)


class DeepDenseSigmoid(Combination):
    """``n_hidden_layers`` ``DenseSigmoid`` transformers in sequence; keyword arguments go to each of them."""
    native_kind = "dense"

    def __init__(self, event_shape: Sequence[int], n_hidden_layers: int = 2, **kwargs):
        super().__init__(event_shape, [DenseSigmoid(event_shape, **kwargs) for _ in range(n_hidden_layers)])

    @property
    def n_dense_layers(self) -> int:
        return self.components[0].n_dense_layers

    @property
    def hidden_size(self) -> int:
        return self.components[0].hidden_size
