"""Generate the fixtures of the deep sigmoidal family (Sigmoid / DeepSigmoid transformers, CouplingDeepSF and its
MADE twins) by RUNNING the real reference, the flow fixtures in the key layout of ``make_golden.flow_fixture``.

Run where the reference is importable (it cannot travel to the GPU box), from the repository root:

    PYTHONDONTWRITEBYTECODE=1 PYTHONPATH=<reference checkout> python tests/golden/make_golden_dsf.py

Every array written is data (inputs, parameters, outputs of the reference); no reference source is stored.
"""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from make_golden import _flow_grads, flow_fixture, np32, save  # noqa: E402  (imports the reference; defines functions only)

from torchflows.bijections.finite.autoregressive.architectures import (  # noqa: E402
    CouplingDeepSF, InverseAutoregressiveDeepSF, MaskedAutoregressiveDeepSF)
from torchflows.bijections.finite.autoregressive.transformers.combination.sigmoid import (  # noqa: E402
    DeepSigmoid, Sigmoid)

N, D, T, N_INV = 64, 21, 11, 48
CASES = ((2, 4), (2, 5), (2, 10), (1, 15))          # (components, hidden units)
EPS = 1e-6                                          # the clip of Sigmoid.forward_1d


def clip_mask(tr, x, h):
    """Elements whose weighted sigmoid sum leaves [eps, 1 - eps] in any component (fp64 walk): the map is flat there."""
    comps = getattr(tr, "components", [tr])
    hit = torch.zeros_like(x, dtype=torch.bool)
    start = 0
    for c in comps:
        P = c.n_parameters_per_element
        hc = h[..., start:start + P].reshape(-1, P)
        start += P
        a, b, w, _ = c.extract_parameters(hc)
        d = (w * torch.sigmoid(a * x.reshape(-1)[:, None] + b)).sum(-1)
        hit |= ((d <= EPS) | (d >= 1 - EPS)).view_as(x)
        x, _ = c.forward(x, h[..., start - P:start])
    return hit


def gen_layers():
    out, cases = {}, []
    torch.manual_seed(0)
    tgt = torch.arange(0, D, 2)                      # 11 targets, not the tail
    assert tgt.numel() == T
    out["tgt"] = tgt.numpy().astype(np.int32)
    for n_comp, K in CASES:
        tr = Sigmoid((T,), hidden_dim=K) if n_comp == 1 else DeepSigmoid((T,), n_hidden_layers=n_comp, hidden_dim=K)
        P = 3 * K * n_comp
        assert tuple(tr.parameter_shape) == (T, P)
        x = 2.0 * torch.randn(N, D)
        x[N_INV:] = (torch.rand(N - N_INV, D) * 2 - 1) * 9.0          # stress rows, |x| up to 9
        h = 700.0 * torch.randn(N, T, P)
        assert float(h.std()) >= 500.0                                # (parameters enter divided by 1000)
        xt = x[:, tgt].contiguous()
        with torch.no_grad():
            z, ld = tr.forward(xt, h)
            z64, ld64 = tr.forward(xt.double(), h.double())
            z_in = z64[:N_INV].float().contiguous()
            xi, ldi = tr.inverse(z_in, h[:N_INV])
            xi64, ldi64 = tr.inverse(z_in.double(), h[:N_INV].double())
            clip = clip_mask(tr, xt[:N_INV].double(), h[:N_INV].double())
        share = float(clip.float().mean())
        assert share <= 0.02, f"clip mask covers {share:.3%} of the inverse elements of {(n_comp, K)}"
        tag = f"C{n_comp}_K{K}"
        print(f"{tag}: std(h) {float(h.std()):.0f}, clip mask {share:.3%}, round trip max |x - x_inv| "
              f"{float((xi - xt[:N_INV])[~clip].abs().max()):.2e}")
        out.update({f"{tag}_x": np32(x), f"{tag}_h": np32(h), f"{tag}_z": np32(z), f"{tag}_ld": np32(ld),
                    f"{tag}_z64": np32(z64), f"{tag}_ld64": np32(ld64), f"{tag}_z_in": np32(z_in),
                    f"{tag}_xinv": np32(xi), f"{tag}_ldinv": np32(ldi), f"{tag}_xinv64": np32(xi64),
                    f"{tag}_ldinv64": np32(ldi64), f"{tag}_clip": np32(clip)})
        cases.append(tag)
    out["cases"] = np.array(cases)
    save("dsf.npz", **out)


H_SCALE = 1000.0
_h_std = []


def scaled(ctor):
    """``ctor`` with the final Linear of every conditioner scaled by H_SCALE, so that the transformers leave their
    default; every conditioner output is recorded for the std(h) assertion."""
    def make(event_shape, **kwargs):
        bij = ctor(event_shape, **kwargs)
        for layer in bij.layers:
            tr = getattr(layer, "transformer", None)
            if not isinstance(tr, DeepSigmoid):
                continue
            last = [m for m in layer.conditioner_transform.modules() if isinstance(m, torch.nn.Linear)][-1]
            with torch.no_grad():
                last.weight.mul_(H_SCALE)
                last.bias.mul_(H_SCALE)
            layer.conditioner_transform.register_forward_hook(lambda m, a, o: _h_std.append(float(o.std())))
        return bij
    return make


def checked_fixture(name, ctor, *args, **kwargs):
    _h_std.clear()
    flow_fixture(name, scaled(ctor), *args, **kwargs)
    assert _h_std and min(_h_std) >= 300.0, f"{name}: std(h) {min(_h_std):.0f} < 300"
    print(f"   std(h) over {len(_h_std)} conditioner calls: min {min(_h_std):.0f}, max {max(_h_std):.0f}")


def gen_flows():
    checked_fixture("flow_cdeepsf16.npz", CouplingDeepSF, 16, 64, dict(n_layers=2))                 # K = 4
    checked_fixture("flow_cdeepsf21.npz", CouplingDeepSF, 21, 64, dict(n_layers=2))                 # odd D, T = 11, K = 5
    checked_fixture("flow_madeepsf6.npz", MaskedAutoregressiveDeepSF, 6, 32, dict(n_layers=2))
    checked_fixture("flow_iadeepsf6.npz", InverseAutoregressiveDeepSF, 6, 32, dict(n_layers=2))
    checked_fixture("flow_cdeepsf16_ctx3.npz", CouplingDeepSF, 16, 64, dict(n_layers=2), context_shape=(3,))
    _flow_grads("flow_cdeepsf16.npz", CouplingDeepSF, 16, dict(n_layers=2))


if __name__ == "__main__":
    gen_layers()
    gen_flows()
