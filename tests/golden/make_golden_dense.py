"""Generate the fixtures of the dense sigmoidal family (DenseSigmoid / DeepDenseSigmoid transformers, CouplingDenseSF,
CouplingDeepDenseSF and their MADE twins) by RUNNING the real reference, in the key layout of
``make_golden.flow_fixture``.

Run where the reference is importable (it cannot travel to the GPU box), from the repository root:

    PYTHONDONTWRITEBYTECODE=1 PYTHONPATH=<reference checkout> python tests/golden/make_golden_dense.py

Every array written is data (inputs, parameters, outputs of the reference); no reference source is stored.
"""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from make_golden import flow_fixture  # noqa: E402  (imports the reference; defines functions only)

from torchflows.bijections.finite.autoregressive.architectures import (  # noqa: E402
    CouplingDeepDenseSF, CouplingDenseSF, InverseAutoregressiveDeepDenseSF, MaskedAutoregressiveDenseSF)

H_SCALE = 300.0         # parameters enter divided by 1000: at the initial scale every transformer sits at its default


SEED = 0


def scaled(ctor):
    """``ctor`` with the last Linear and the global parameters of every dense sigmoidal layer scaled by H_SCALE.  The
    global-parameter mask is drawn at construction and is no part of the state dict: every construction (the fp64 twin
    of ``flow_fixture`` included) starts from ``SEED``, which is also what a test has to seed before it builds the flow."""
    def make(event_shape, **kwargs):
        torch.manual_seed(SEED)
        bij = ctor(event_shape, **kwargs)
        for layer in bij.layers:
            if "DenseSigmoid" not in type(getattr(layer, "transformer", None)).__name__:
                continue
            ct = layer.conditioner_transform
            last = [m for m in ct.modules() if isinstance(m, torch.nn.Linear)][-1]
            with torch.no_grad():
                last.weight.mul_(H_SCALE)
                last.bias.mul_(H_SCALE)
                ct.global_theta_flat.mul_(H_SCALE)
        return bij
    return make


if __name__ == "__main__":
    flow_fixture("flow_cdensesf16.npz", scaled(CouplingDenseSF), 16, 32, dict(n_layers=2))
    flow_fixture("flow_cdeepdensesf6.npz", scaled(CouplingDeepDenseSF), 6, 32, dict(n_layers=2))
    flow_fixture("flow_madensesf6.npz", scaled(MaskedAutoregressiveDenseSF), 6, 32, dict(n_layers=2))
    flow_fixture("flow_iadeepdensesf6.npz", scaled(InverseAutoregressiveDeepDenseSF), 6, 32, dict(n_layers=2))
