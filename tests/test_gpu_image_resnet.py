"""Image flows with ``use_resnet=True`` on the one-launch-per-coupling route (csrc/tfk_glow_resnet.hip, kinds 4 and 6 of
tfk_glow_coupling) against this package's own ATen composite path in float64 with the same weights.  Bars:
tests/test_host_dsf.py's ``bar(floor)`` with the floor = the ATen fp32-vs-fp64 distance of the same model on the same
inputs; log_prob / log-dets elementwise relative (``rel``), z and x norm-wise.  Every launch keeps 3 samples resident,
which does not divide the tile of 16: the last round of a full tile holds one."""
import copy
import warnings

import pytest
import torch

from test_host_dsf import bar, normwise, rel

pytestmark = pytest.mark.gpu

CASES = {
    # conditioner images (1, 4, 8) and (2, 4, 4): the 1x1 modifier on both axes, T = 32
    "realnvp_1x8x8": ("MultiscaleRealNVP", (1, 8, 8), {}),
    # (1, 14, 28) and (2, 14, 14): the 2-wide modifier, shift, T = 392 (24.5 groups of 16)
    "nice_1x28x28": ("MultiscaleNICE", (1, 28, 28), {}),
    # ResNet and ConvNet couplings and 1x1 convolutions in one program; pending ActNorm maps in front of a ResNet step
    "glow_3x8x8": ("AffineGlow", (3, 8, 8), {}),
    # one coupling at full frame height; the widest linear2 of any preset (T = 1 536)
    "single_3x32x32": ("MultiscaleRealNVP", (3, 32, 32), dict(n_layers=1, n_checkerboard_layers=0)),
}
_cache = {}


def reference(name):
    """(flow on the host, x, z_in, float64 and fp32 ATen results), computed once per case."""
    if name not in _cache:
        import torchflows_amd as tfa
        from torchflows_amd.bijections.finite.multiscale import architectures
        arch, shape, kwargs = CASES[name]
        torch.manual_seed(11)
        flow = tfa.Flow(getattr(architectures, arch)(shape, use_resnet=True, **kwargs))
        flow.train()
        with torch.no_grad():
            flow.log_prob(torch.randn(64, *shape))              # ActNorm init, BatchNorm statistics
        flow.eval()
        x = torch.randn(37, *shape)
        out = {}
        with torch.no_grad():
            f64 = copy.deepcopy(flow).double()
            z_in = f64.bijection.forward(x.double())[0].float()
            for tag, f, cast in (("64", f64, torch.double), ("32", flow, torch.float)):
                z, ld = f.bijection.forward(x.to(cast))
                xi, ldi = f.bijection.inverse(z_in.to(cast))
                out[tag] = dict(z=z.numpy(), ld=ld.numpy(), lp=f.log_prob(x.to(cast)).numpy(), x_inv=xi.numpy(),
                                ld_inv=ldi.numpy())
        _cache[name] = (flow, x, z_in, out)
    return _cache[name]


def check(got, ref, n, label):
    for key, dist in (("z", normwise), ("ld", rel), ("lp", rel), ("x_inv", normwise), ("ld_inv", rel)):
        if key not in got:
            continue
        a, b, c = got[key].cpu().numpy(), ref["64"][key][:n], ref["32"][key][:n]
        err, floor = dist(a, b), dist(c, b)
        print(f"{label} n={n} {key}: error {err:.2e}, floor {floor:.2e}, bar {bar(floor):.2e}")
        assert torch.isfinite(got[key]).all() and err < bar(floor), key


@pytest.mark.parametrize("n", [1, 16, 37])
@pytest.mark.parametrize("name", list(CASES))
def test_resnet_image_program_vs_float64(name, n):
    from torchflows_amd import image_program, native
    from torchflows_amd.fused import NativeRouteWarning
    host, x, z_in, ref = reference(name)
    flow = copy.deepcopy(host).cuda()
    xg, zg = x[:n].cuda(), z_in[:n].cuda()
    x0, z0 = xg.clone(), zg.clone()
    with warnings.catch_warnings(record=True) as caught, torch.no_grad():
        warnings.simplefilter("always")
        progs = [image_program.get_program(flow.bijection, d, xg.device) for d in (0, 1)]
        assert all(p is not None and any(s.info["kind"].endswith("_resnet") for s in p.steps) for p in progs)
        assert all(s.info["slots"] == 3 for p in progs for s in p.steps if s.layer.kind & 4)
        before = native.calls
        z, ld = flow.bijection.forward(xg)
        assert native.calls - before == len(progs[0].steps) + (progs[0].flush is not None)
        before = native.calls
        lp = flow.log_prob(xg)
        assert native.calls - before == len(progs[0].steps) + 1
        before = native.calls
        xi, ldi = flow.bijection.inverse(zg)
        assert native.calls - before == len(progs[1].steps) + (progs[1].flush is not None)
        torch.cuda.synchronize()
    assert not [w for w in caught if issubclass(w.category, NativeRouteWarning)]
    assert torch.equal(xg, x0) and torch.equal(zg, z0)
    check(dict(z=z, ld=ld, lp=lp, x_inv=xi, ld_inv=ldi), ref, n, name)


def test_routes_agree(monkeypatch):
    """The same model layer by layer (TORCHFLOWS_AMD_IMAGE_PROGRAM=0: the conditioner on ATen) and as a program: each
    within the bar of float64 and the two within the bar of each other."""
    from torchflows_amd import native
    host, x, z_in, ref = reference("glow_3x8x8")
    xg, zg = x.cuda(), z_in.cuda()
    got = {}
    with torch.no_grad():
        for route, env in (("layers", "0"), ("program", "1")):
            monkeypatch.setenv("TORCHFLOWS_AMD_IMAGE_PROGRAM", env)
            flow = copy.deepcopy(host).cuda()
            before = native.calls
            z, ld = flow.bijection.forward(xg)
            xi, ldi = flow.bijection.inverse(zg)
            got[route] = dict(z=z, ld=ld, x_inv=xi, ld_inv=ldi)
            got[route + "_calls"] = native.calls - before
            check(got[route], ref, 37, route)
    assert got["layers_calls"] > got["program_calls"]
    for key, dist in (("z", normwise), ("ld", rel), ("x_inv", normwise), ("ld_inv", rel)):
        floor = dist(ref["32"][key], ref["64"][key])
        assert dist(got["program"][key].cpu().numpy(), got["layers"][key].cpu().numpy()) < bar(floor), key
