"""Deep sigmoidal image flows on the one-launch-per-coupling route (csrc/tfk_glow_dsf.hip) against this package's own
ATen composite path in float64 with the same weights.  Bars: tests/test_host_dsf.py's ``bar(floor)`` with the floor = the
ATen fp32-vs-fp64 distance of the same model on the same inputs; log_prob / log-dets elementwise relative (``rel``), z
and x norm-wise.  Inverse inputs are the float64 forward images of standard-normal data, so that no element sits where
the map is flat (the bracket's edge |x| >= 10, which lies inside the clip of d): the excluded share is asserted <= 2 %
(measured on the host: 0 for every case).  The kernel is the subject, so the batch-size route decision of
``image_program.fills_device`` is taken away (``glow_dsf=program``); ``test_routes_agree`` covers the decision."""
import copy
import warnings

import numpy as np
import pytest
import torch

from test_host_dsf import bar, normwise, rel

pytestmark = pytest.mark.gpu

CASES = {
    "dsglow_3x8x8": ("DeepSigmoidGlow", (3, 8, 8), {}),                    # T = 96, 48, 24: K = 5; 1x1 convolutions between
    "msdsf_1x28x28": ("MultiscaleDeepSigmoid", (1, 28, 28), {}),           # T = 392: K = 10, 24.5 groups, 2-wide modifier
    "msdsf_3x16x16": ("MultiscaleDeepSigmoid", (3, 16, 16), dict(n_layers=2)),            # T = 384
    # ONE coupling of a (3, 32, 32) image: T = 1 536, K = 15, the register-critical instantiation
    "single_3x32x32": ("MultiscaleDeepSigmoid", (3, 32, 32), dict(n_layers=1, n_checkerboard_layers=0)),
}
_cache = {}


def reference(name):
    """(flow on the host, x, float64 and fp32 ATen results), computed once per case."""
    if name not in _cache:
        import torchflows_amd as tfa
        arch, shape, kwargs = CASES[name]
        torch.manual_seed(11)
        flow = tfa.Flow(getattr(tfa, arch)(shape, **kwargs))
        flow.train()
        with torch.no_grad():
            flow.log_prob(torch.randn(64, *shape))              # ActNorm init, BatchNorm statistics
        flow.eval()
        x = torch.randn(37, *shape)
        out = {}
        with torch.no_grad():
            f64 = copy.deepcopy(flow).double()
            z64, ld64 = f64.bijection.forward(x.double())
            z_in = z64.float()
            for tag, f, cast in (("64", f64, torch.double), ("32", flow, torch.float)):
                z, ld = f.bijection.forward(x.to(cast))
                xi, ldi = f.bijection.inverse(z_in.to(cast))
                out[tag] = dict(z=z.numpy(), ld=ld.numpy(), lp=f.log_prob(x.to(cast)).numpy(), x_inv=xi.numpy(),
                                ld_inv=ldi.numpy())
        _cache[name] = (flow, x, z_in, out)
    return _cache[name]


@pytest.mark.parametrize("n", [1, 16, 37])
@pytest.mark.parametrize("name", list(CASES))
def test_dsf_image_program_vs_float64(name, n, monkeypatch):
    from torchflows_amd import image_program, native
    monkeypatch.setenv("TORCHFLOWS_AMD_DEBUG", "glow_dsf=program")
    from torchflows_amd.fused import NativeRouteWarning
    host, x, z_in, ref = reference(name)
    flow = copy.deepcopy(host).cuda()
    xg, zg = x[:n].cuda(), z_in[:n].cuda()
    x0, z0 = xg.clone(), zg.clone()
    with warnings.catch_warnings(record=True) as caught, torch.no_grad():
        warnings.simplefilter("always")
        progs = [image_program.get_program(flow.bijection, d, xg.device) for d in (0, 1)]
        assert all(p is not None and any(s.info["kind"] == "dsf" for s in p.steps) for p in progs)
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
    r64, r32 = ({k: v[:n] for k, v in ref[t].items()} for t in ("64", "32"))
    keep = np.abs(r64["x_inv"]) < 9.99
    assert 1.0 - keep.mean() <= 0.02
    got = dict(z=z, ld=ld, lp=lp, x_inv=xi, ld_inv=ldi)
    for key, dist in (("z", normwise), ("ld", rel), ("lp", rel), ("x_inv", normwise), ("ld_inv", rel)):
        a, b, c = got[key].cpu().numpy(), r64[key], r32[key]
        if key == "x_inv":
            a, b, c = a[keep], b[keep], c[keep]
        err, floor = dist(a, b), dist(c, b)
        print(f"{name} n={n} {key}: error {err:.2e}, floor {floor:.2e}, bar {bar(floor):.2e}")
        assert err < bar(floor), key


def test_routes_agree(monkeypatch):
    """The same model layer by layer (TORCHFLOWS_AMD_IMAGE_PROGRAM=0) and as a program, forward and inverse: each within the
    bar of float64 and the two within the bar of each other; and a batch too small for the wide couplings of the (1, 28, 28)
    model is sent layer by layer unless the decision is taken away."""
    from torchflows_amd import image_program, native
    host, x, z_in, ref = reference("msdsf_1x28x28")
    xg, zg = x.cuda(), z_in.cuda()
    got = {}
    with torch.no_grad():
        for route, env, dbg in (("layers", "0", ""), ("auto", "1", ""), ("program", "1", "glow_dsf=program")):
            monkeypatch.setenv("TORCHFLOWS_AMD_IMAGE_PROGRAM", env)
            monkeypatch.setenv("TORCHFLOWS_AMD_DEBUG", dbg)
            flow = copy.deepcopy(host).cuda()
            before = native.calls
            z, ld = flow.bijection.forward(xg)
            xi, ldi = flow.bijection.inverse(zg)
            got[route] = dict(z=z.cpu().numpy(), ld=ld.cpu().numpy(), x_inv=xi.cpu().numpy(), ld_inv=ldi.cpu().numpy(),
                              calls=native.calls - before)
        progs = [image_program.get_program(flow.bijection, d, xg.device) for d in (0, 1)]
    assert got["program"]["calls"] == sum(len(p.steps) + (p.flush is not None) for p in progs)
    assert got["auto"]["calls"] == got["layers"]["calls"] > got["program"]["calls"]      # 37 rows: below 8 per CU
    for key, dist in (("z", normwise), ("ld", rel), ("x_inv", normwise), ("ld_inv", rel)):
        r64, floor = ref["64"][key], dist(ref["32"][key], ref["64"][key])
        for route in ("layers", "program"):
            assert dist(got[route][key], r64) < bar(floor), (key, route)
        assert dist(got["program"][key], got["layers"][key]) < bar(floor), key
