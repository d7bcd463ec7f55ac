"""A scalar transformer made of scalar transformers applied one after the other (reference
``transformers/combination/base.py``).  The parameter vector of an element is the concatenation of the components'
vectors in component order; ``inverse`` walks the components last to first.  ``components`` is a plain list, as in the
reference: the components own no parameters or buffers, so nothing is missing from the state dict."""
from __future__ import annotations

from typing import List, Sequence, Tuple

import torch

from torchflows_amd.bijections.finite.autoregressive.transformers.base import ScalarTransformer
from torchflows_amd.utils import get_batch_shape


class Combination(ScalarTransformer):
    def __init__(self, event_shape: Sequence[int], components: List[ScalarTransformer]):
        super().__init__(event_shape)
        self.components = components
        self.n_components = len(components)

    @property
    def parameter_shape_per_element(self) -> Tuple[int, ...]:
        return (sum(c.n_parameters_per_element for c in self.components),)

    @property
    def default_parameters(self) -> torch.Tensor:
        return torch.cat([c.default_parameters.ravel() for c in self.components], dim=0)

    def _slices(self):
        start = 0
        for component in self.components:
            yield component, slice(start, start + component.n_parameters_per_element)
            start += component.n_parameters_per_element

    def forward(self, x: torch.Tensor, h: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
        log_det = torch.zeros(get_batch_shape(x, self.event_shape)).to(x)
        for component, sl in self._slices():
            x, increment = component.forward(x, h[..., sl])
            log_det = log_det + increment
        return x, log_det

    def inverse(self, z: torch.Tensor, h: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
        log_det = torch.zeros(get_batch_shape(z, self.event_shape)).to(z)
        for component, sl in reversed(list(self._slices())):
            z, increment = component.inverse(z, h[..., sl])
            log_det = log_det + increment
        return z, log_det
