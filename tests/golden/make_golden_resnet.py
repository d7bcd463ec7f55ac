"""Fixture of an image flow whose outer block has the ResNet conditioner, by RUNNING the real reference (run as
make_golden.py is).  ``MultiscaleBijection((1, 8, 8), Affine, n_blocks=2, n_checkerboard_layers=1,
n_channel_wise_layers=1, use_resnet=True)``: two ResNet couplings (about 0.6 MB of fp32 parameters) in front of the inner
block's ConvNet ones.  A few training-mode batches come first, so that ActNorm is initialised and every BatchNorm has
running statistics of its own.  Data only; no reference source is stored."""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from make_golden import Flow, np32, save  # noqa: E402
from torchflows.bijections.finite.autoregressive.transformers.linear.affine import Affine  # noqa: E402
from torchflows.bijections.finite.multiscale.base import MultiscaleBijection  # noqa: E402

KWARGS = dict(n_blocks=2, n_checkerboard_layers=1, n_channel_wise_layers=1, use_resnet=True)

if __name__ == "__main__":
    torch.manual_seed(0)
    flow = Flow(MultiscaleBijection((1, 8, 8), Affine, **KWARGS))
    g = torch.Generator().manual_seed(1000)
    flow.train()
    with torch.no_grad():
        for _ in range(4):
            flow.log_prob(1.5 * torch.randn(256, 1, 8, 8, generator=g) + 0.3)
    flow.eval()
    x = torch.randn(24, 1, 8, 8, generator=g)
    x[:6] *= 3.0
    z_in = torch.randn(24, 1, 8, 8, generator=g)
    sd = flow.state_dict()
    out = {f"sd/{k}": np32(v) for k, v in sd.items()}
    out.update(x=np32(x), z_in=np32(z_in))
    f64 = Flow(MultiscaleBijection((1, 8, 8), Affine, **KWARGS)).double()
    f64.load_state_dict({k: v.double() for k, v in sd.items()})
    f64.eval()
    with torch.no_grad():
        for tag, f, cast in (("", flow, torch.float32), ("64", f64, torch.float64)):
            z, ld = f.bijection.forward(x.to(cast))
            xi, ldi = f.bijection.inverse(z_in.to(cast))
            out.update({"z" + tag: z.numpy(), "log_det" + tag: ld.numpy(), "log_prob" + tag: f.log_prob(x.to(cast)).numpy(),
                        "x_inv" + tag: xi.numpy(), "log_det_inv" + tag: ldi.numpy()})
    save("flow_resnet_1x8x8.npz", **out)
