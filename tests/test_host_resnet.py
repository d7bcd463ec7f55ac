"""The ResNet conditioner of the image couplings on the host: the reference's state dict and results
(tests/golden/flow_resnet_1x8x8.npz), where ``use_resnet=True`` reaches, and what image_program packs for the kernel."""
import os

import numpy as np
import pytest
import torch

from test_host_dsf import bar, normwise, rel

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "flow_resnet_1x8x8.npz")
KWARGS = dict(n_blocks=2, n_checkerboard_layers=1, n_channel_wise_layers=1, use_resnet=True)


@pytest.fixture(scope="module")
def golden():
    import torchflows_amd as tfa
    from torchflows_amd.bijections.finite.autoregressive.transformers.linear.affine import Affine
    from torchflows_amd.bijections.finite.multiscale.base import MultiscaleBijection
    fx = np.load(GOLDEN)
    flow = tfa.Flow(MultiscaleBijection((1, 8, 8), Affine, **KWARGS))
    sd = {k[3:]: torch.from_numpy(fx[k]) for k in fx.files if k.startswith("sd/")}
    flow.load_state_dict(sd, strict=True)
    return flow.eval(), fx


def test_reference_state_dict_and_results(golden):
    flow, fx = golden
    assert "bijection.checkerboard_layers.0.layers.1.conditioner_transform.network.stage1.blocks.0.bn1.running_mean" in flow.state_dict()
    x, z_in = torch.from_numpy(fx["x"]), torch.from_numpy(fx["z_in"])
    with torch.no_grad():
        z, ld = flow.bijection.forward(x)
        xi, ldi = flow.bijection.inverse(z_in)
        got = dict(z=z, log_det=ld, log_prob=flow.log_prob(x), x_inv=xi, log_det_inv=ldi)
    for key, dist in (("z", normwise), ("log_det", rel), ("log_prob", rel), ("x_inv", normwise), ("log_det_inv", rel)):
        floor = dist(fx[key], fx[key + "64"])
        assert dist(got[key].numpy(), fx[key]) < bar(floor), key


def test_use_resnet_reaches_the_outer_block_only(golden):
    from torchflows_amd.bijections.finite.multiscale.architectures import AffineGlow
    from torchflows_amd.bijections.finite.multiscale.base import Invertible1x1ConvolutionalCoupling
    from torchflows_amd.bijections.finite.multiscale.conditioning.classic import ConvNetConditioner
    from torchflows_amd.bijections.finite.multiscale.conditioning.resnet import ResNetConditioner
    import torchflows.bijections.finite.multiscale.conditioning.resnet as spelled
    assert spelled.ResNetConditioner is ResNetConditioner
    conds = lambda m: [c for c in m.modules() if isinstance(c, (ConvNetConditioner, ResNetConditioner))]
    outer = golden[0].bijection
    inner = conds(outer.small_bijection)
    assert inner and all(isinstance(c, ConvNetConditioner) for c in inner)
    assert sum(isinstance(c, ResNetConditioner) for c in conds(outer)) == 2
    glow = AffineGlow((3, 8, 8), use_resnet=True)
    ones = [m for m in glow.modules() if isinstance(m, Invertible1x1ConvolutionalCoupling)]
    assert ones and all(isinstance(m.conditioner_transform, ConvNetConditioner) for m in ones)
    assert any(isinstance(c, ResNetConditioner) for c in conds(glow))


def test_packed_block_reproduces_relu_bn_conv(golden):
    """The folded, [ci][ky][kx][co]-packed conv1 of stage 2 against relu(bn1(conv1(x))) in float64, and the program's kinds."""
    from torchflows_amd import image_program
    flow = golden[0]
    prog = image_program.compile_program(flow.bijection, 0, torch.device("cpu"))
    assert prog is not None and prog.levels is None
    kinds = [s.info["kind"] for s in prog.steps]
    assert kinds[:2] == ["affine_resnet", "affine_resnet"] and set(kinds[2:]) == {"affine"}
    assert [s.layer.kind for s in prog.steps[:2]] == [4, 4] and prog.steps[0].info["slots"] == 3
    layer = flow.bijection.checkerboard_layers[0].layers[1]
    cond = layer.conditioner_transform.double()
    pk = image_program._pack_resnet_conditioner(cond, *(int(v) for v in layer.coupling.constant_shape))
    blk = cond.network.stage2.blocks[0]
    off = 4 * 1 + 4 + (18 * 16 + 291 * 4 + 16)                      # modifier, stage 1 (include/tfk.h)
    W = pk["weights"][off:off + 8 * 9 * 16].double().view(8, 3, 3, 16).permute(3, 0, 1, 2)
    b = pk["weights"][off + 1152:off + 1168].double()
    x = torch.randn(3, 8, 16, 16, dtype=torch.float64, generator=torch.Generator().manual_seed(3))
    with torch.no_grad():
        want = torch.relu(blk.bn1(blk.conv1(x)))
        got = torch.relu(torch.nn.functional.conv2d(x, W, b, padding=1))
    assert normwise(got.numpy(), want.numpy()) < 1e-6               # (the pack is fp32: 6e-8 per weight)
    cond.float()
