"""The wide-row route on the GPU (csrc/tfk_flow_wide.h, torchflows_amd/fused_wide.py): chains of affine / shift couplings
on even event sizes in (256, 2048] as ONE libtfk launch -- against the reference's golden outputs, the CPU oracle on seeded
inputs, and the routes of the releases before it (TORCHFLOWS_AMD_DEBUG=wide=0)."""
import warnings

import numpy as np
import pytest
import torch

from conftest import load_golden, state_dict_of, set_debug

pytestmark = pytest.mark.gpu


# (helpers of tests/test_gpu_flows.py)
def rel(a, b):
    a = np.asarray(a, np.float64)
    b = np.asarray(b, np.float64)
    return float(np.nanmax(np.abs(a - b) / np.maximum(1.0, np.abs(b)))) if a.size else 0.0


def pass_rate(a, b, tol=1e-5):
    """share of entries with |a - b| <= tol * max(1, |b|)"""
    a = np.asarray(a, np.float64)
    b = np.asarray(b, np.float64)
    return float(np.mean(np.abs(a - b) <= tol * np.maximum(1.0, np.abs(b)))) if a.size else 1.0


def normwise(a, b):
    a = np.asarray(a, np.float64).ravel()
    b = np.asarray(b, np.float64).ravel()
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-30))


@pytest.fixture(scope="module")
def pkg():
    assert torch.cuda.is_available()
    import torchflows_amd as tfa
    from torchflows_amd import native
    native.lib()
    return tfa


def data_init(flow, D, rows=512, scale=1.0):
    flow.train()
    with torch.no_grad():
        flow.log_prob(torch.randn(rows, *flow.bijection.event_shape) * scale)   # ActNorm's data-dependent init (host)
    return flow.eval()


def drop_programs(flow):
    """Route switches are read when a program is compiled: forget the cached ones."""
    flow.bijection.__dict__.pop("_tfk_compiled", None)
    flow.bijection.__dict__.pop("_tfk_declined_warned", None)


_FLOWS = {}


def seeded_flow(pkg, arch, D, n_layers):
    """One data-initialised flow per (arch, D, n_layers), on the device, shared by the tests that only read it."""
    key = (arch, D, n_layers)
    if key not in _FLOWS:
        torch.manual_seed(7 + D + n_layers)
        flow = data_init(pkg.Flow(getattr(pkg, arch)(D, n_layers=n_layers)), D)
        sd = {k: v.numpy().copy() for k, v in flow.state_dict().items()}
        _FLOWS[key] = (flow.cuda(), sd)
    return _FLOWS[key]


WIDE_FLOWS = [("flow_realnvp_1x28x28.npz", "RealNVP", 3), ("flow_nice258.npz", "NICE", 2)]


@pytest.mark.parametrize("variant", ["fresh", "init"])
@pytest.mark.parametrize("name,arch,n_layers", WIDE_FLOWS)
def test_wide_flow_golden_on_hip(pkg, name, arch, n_layers, variant):
    """The assertions and bars of test_gpu_flows.py::test_flow_golden_on_hip (non-spline branch) on the two fixtures of
    this route, which must be the wide launch (no NativeRouteWarning)."""
    from torchflows_amd import fused, native
    fx = load_golden(name)
    es = tuple(int(v) for v in fx["event_shape"])
    flow = pkg.Flow(getattr(pkg, arch)(es, n_layers=n_layers))
    flow.load_state_dict({k: torch.from_numpy(v) for k, v in state_dict_of(fx, variant).items()})
    flow = flow.cuda().eval()
    x = torch.from_numpy(fx["x"]).cuda()
    z_in = torch.from_numpy(fx["z_in"]).cuda()
    g = lambda k: fx[f"{variant}/{k}"]
    before = native.calls
    with warnings.catch_warnings():
        warnings.simplefilter("error", fused.NativeRouteWarning)
        with torch.no_grad():
            z, lp = flow.forward_with_log_prob(x)
            xr, ldr = flow.bijection.inverse(z_in)
    assert 2 <= native.calls - before <= 4, "one launch per call (+ a row reorder)"
    assert lp.shape == x.shape[:1] and z.shape == x.shape and xr.shape == x.shape

    tol = 1e-5
    floor_lp = rel(g("log_prob"), g("log_prob64"))
    floor_x = normwise(g("x_inv"), g("x_inv64"))
    floor_ld = rel(g("log_det_inv"), g("log_det_inv64"))
    e_lp = rel(lp.cpu().numpy(), g("log_prob"))
    e_z = normwise(z.cpu().numpy(), g("z"))
    e_x = normwise(xr.cpu().numpy(), g("x_inv"))
    e_ld = rel(ldr.cpu().numpy(), g("log_det_inv"))
    e_lp64 = rel(lp.cpu().numpy(), g("log_prob64"))
    print(f"{name} {variant}: log_prob {e_lp:.2e} (floor {floor_lp:.2e}, vs fp64 {e_lp64:.2e}), z nw {e_z:.2e}, "
          f"x_inv nw {e_x:.2e} (floor {floor_x:.2e}), log_det_inv {e_ld:.2e} (floor {floor_ld:.2e})")
    pr_z, pr_z_ref = pass_rate(z.cpu().numpy(), g("z64")), pass_rate(g("z"), g("z64"))
    pr_x, pr_x_ref = pass_rate(xr.cpu().numpy(), g("x_inv64")), pass_rate(g("x_inv"), g("x_inv64"))
    print(f"    elementwise 1e-5 pass rate vs the reference in fp64: z {pr_z:.4f} (reference's fp32 {pr_z_ref:.4f}), "
          f"x_inv {pr_x:.4f} (reference's fp32 {pr_x_ref:.4f})")
    slack = 0.05 + 1.5 / np.sqrt(z.numel())
    assert pr_z >= pr_z_ref - slack and pr_x >= pr_x_ref - slack, (pr_z, pr_z_ref, pr_x, pr_x_ref)
    assert e_lp < 1e-5 or e_lp64 < max(1e-5, 2 * floor_lp), (e_lp, e_lp64, floor_lp)
    assert e_lp < 1e-5 + 3 * floor_lp
    assert e_z < max(tol, 3 * normwise(g("z"), g("z64")))
    assert e_x < max(tol, 3 * floor_x)
    D = int(np.prod(es))
    assert e_ld < max(tol * max(1.0, D / 64), 3 * floor_ld)
    # the caller's tensors are untouched
    assert torch.equal(x.cpu(), torch.from_numpy(fx["x"]))
    assert torch.equal(z_in.cpu(), torch.from_numpy(fx["z_in"]))


def test_wide_route_is_one_launch(pkg):
    """RealNVP((1, 28, 28)), the first model of the reference's image notebook: no NativeRouteWarning, log_prob is ONE
    libtfk entry-point call, the other maps at most two (the chain + a row reorder where it leaves the rows permuted)."""
    from torchflows_amd import fused, native
    torch.manual_seed(0)
    flow = pkg.Flow(pkg.RealNVP((1, 28, 28))).cuda().eval()
    x = torch.randn(33, 1, 28, 28, device="cuda")
    with warnings.catch_warnings():
        warnings.simplefilter("error", fused.NativeRouteWarning)
        with torch.no_grad():
            before = native.calls
            lp = flow.log_prob(x)
            assert native.calls - before == 1
            before = native.calls
            z, lp2 = flow.forward_with_log_prob(x)
            assert native.calls - before <= 2
            before = native.calls
            xr, ld = flow.bijection.inverse(x)
            assert native.calls - before <= 2
            before = native.calls
            xs, lps = flow.sample((33,), return_log_prob=True)
            assert native.calls - before <= 2
    assert lp.shape == (33,) and z.shape == x.shape and xr.shape == x.shape and xs.shape == x.shape and lps.shape == (33,)
    assert torch.isfinite(lp).all() and torch.equal(lp, lp2) and torch.isfinite(lps).all()
    for d in (0, 1):
        chain = fused.get_compiled(flow.bijection, d, x.device)
        assert chain is not None and len(chain.segments) == 1 and chain.segments[0].wide


# every D, every N (one row / one tile plus one row / many tiles with a ragged end) and odd and even layer counts appear
SEEDED = [("RealNVP", 258, 1, 17), ("NICE", 258, 2, 1031), ("RealNVP", 300, 2, 1), ("NICE", 300, 5, 17),
          ("RealNVP", 784, 5, 1031), ("NICE", 784, 1, 1), ("RealNVP", 1024, 2, 17), ("NICE", 1024, 5, 1031),
          ("RealNVP", 2048, 1, 1031), ("NICE", 2048, 2, 17), ("RealNVP", 2048, 5, 1)]


@pytest.mark.parametrize("arch,D,n_layers,N", SEEDED)
def test_wide_flow_vs_oracle_seeded(pkg, oracle, arch, D, n_layers, N):
    """Bars of test_gpu_flows.py::test_flow_vs_oracle_seeded: log_prob rel < 1e-5; z / x normwise and log-det rel < 1e-5."""
    from torchflows_amd import fused
    flow, sd = seeded_flow(pkg, arch, D, n_layers)
    ref = oracle.preset_from_state_dict(arch, D, n_layers, sd)
    torch.manual_seed(11 + N)
    x = torch.randn(N, D)
    x[: N // 8] *= 4.0
    xd = x.cuda()
    with warnings.catch_warnings():
        warnings.simplefilter("error", fused.NativeRouteWarning)
        with torch.no_grad():
            z, lp = flow.forward_with_log_prob(xd)
            xr, ld = flow.bijection.inverse(xd)
    z_ref, lp_ref = ref.log_prob(x.numpy(), return_z=True)
    xr_ref, ld_ref = ref.inverse(x.numpy())
    e = dict(lp=rel(lp.cpu().numpy(), lp_ref), z=normwise(z.cpu().numpy(), z_ref),
             x=normwise(xr.cpu().numpy(), xr_ref), ld=rel(ld.cpu().numpy(), ld_ref))
    print(arch, D, n_layers, N, {k: f"{v:.2e}" for k, v in e.items()})
    assert torch.equal(xd.cpu(), x)
    assert e["lp"] < 1e-5, e
    assert max(e.values()) < 1e-5, e


@pytest.mark.parametrize("arch,D,n_layers", [("RealNVP", 784, 3), ("NICE", 258, 2), ("RealNVP", 1024, 2)])
def test_wide_against_the_previous_routes(pkg, monkeypatch, arch, D, n_layers):
    """wide=1 against wide=0 (layer by layer; the vector-ALU interpreter at 1024) on the same flow and rows: 2e-5 relative
    on z / x / log_prob, the bar test_gpu_fused.py holds fused against layerwise."""
    from torchflows_amd import native
    flow, _ = seeded_flow(pkg, arch, D, n_layers)
    torch.manual_seed(5)
    x = torch.randn(333, D, device="cuda")
    got = {}
    for mode in ("1", "0"):
        set_debug(monkeypatch, wide=mode)
        drop_programs(flow)
        before = native.calls
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            with torch.no_grad():
                z, lp = flow.forward_with_log_prob(x)
                xr, ld = flow.bijection.inverse(x)
        got[mode] = dict(z=z.cpu().numpy(), lp=lp.cpu().numpy(), xr=xr.cpu().numpy(), ld=ld.cpu().numpy(),
                         launches=native.calls - before)
    set_debug(monkeypatch, wide=None)
    drop_programs(flow)
    assert got["1"]["launches"] <= 4 and got["1"]["launches"] < got["0"]["launches"], (got["1"]["launches"], got["0"]["launches"])
    e = {k: rel(got["1"][k], got["0"][k]) for k in ("z", "lp", "xr", "ld")}
    print(arch, D, n_layers, {k: f"{v:.2e}" for k, v in e.items()})
    assert max(e.values()) < 2e-5, e


def test_wide_sample_log_prob(pkg, monkeypatch):
    """Flow.sample((N,), return_log_prob=True) at D = 784: the base density of the incoming rows rides in the launch (flag
    bit 2).  The returned values are held against an independent evaluation on the returned samples -- the FORWARD chain,
    ``log_prob(xs)`` and ``bijection.forward(xs)`` -- at the bar the existing sample test holds against an independent
    evaluation, 1e-5 relative (its 2e-6 is between two runs of the SAME inverse), and samples / values against wide=0 on the
    same seed (2e-5, the A/B bar).
    What ``sample`` returns is the reference's ``base_log_prob(z) + log_det`` with the log-det of the INVERSE map
    (flows.py:699-707), i.e. ``log_prob(xs) - 2 log_det_forward(xs)``, not ``log_prob(xs)`` itself: the plain difference
    to ``log_prob(xs)`` is 1.44e-1 relative here on wide=1 and on wide=0 alike (printed below) -- the semantics every
    route of this package shares with the reference, left as they are -- so the identity asserted carries that term."""
    from torchflows_amd import native
    flow, _ = seeded_flow(pkg, "RealNVP", 784, 3)
    got = {}
    for mode in ("1", "0"):
        set_debug(monkeypatch, wide=mode)
        drop_programs(flow)
        torch.manual_seed(3)
        before = native.calls
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            with torch.no_grad():
                xs, lps = flow.sample((257,), return_log_prob=True)
        got[mode] = (xs, lps, native.calls - before)
    set_debug(monkeypatch, wide=None)
    drop_programs(flow)
    xs, lps, launches = got["1"]
    assert launches <= 2 and xs.shape == (257, 784) and lps.shape == (257,)
    with torch.no_grad():
        lp_back = flow.log_prob(xs)
        _, ld_fwd = flow.bijection.forward(xs)
    want = (lp_back.double() - 2.0 * ld_fwd.double()).cpu().numpy()
    e_self = rel(lps.cpu().numpy(), want)
    e_plain = rel(lps.cpu().numpy(), lp_back.cpu().numpy())
    e_plain0 = rel(got["0"][1].cpu().numpy(), lp_back.cpu().numpy())
    e_x = rel(xs.cpu().numpy(), got["0"][0].cpu().numpy())
    e_lp = rel(lps.cpu().numpy(), got["0"][1].cpu().numpy())
    print(f"sample: vs log_prob(xs) - 2 log_det_forward(xs) {e_self:.2e}; plain difference to log_prob(xs): wide=1 "
          f"{e_plain:.2e}, wide=0 {e_plain0:.2e}; vs wide=0: x {e_x:.2e}, value {e_lp:.2e}")
    assert e_self < 1e-5
    assert e_x < 2e-5 and e_lp < 2e-5


def test_wide_housekeeping(pkg):
    """The caller's tensors are untouched, a non-contiguous (N, D) view works as input, and an in-place parameter edit
    that moves the version counter yields new outputs on the next call."""
    torch.manual_seed(2)
    D = 300
    flow = data_init(pkg.Flow(pkg.RealNVP(D, n_layers=2)), D).cuda()
    base = torch.randn(40, 2 * D, device="cuda")
    keep = base.clone()
    view = base[:, ::2]                                       # strided
    assert not view.is_contiguous()
    with torch.no_grad():
        lp_v = flow.log_prob(view)
        z_v, ld_v = flow.bijection.forward(view)
        lp_c = flow.log_prob(view.contiguous())
        z_c, ld_c = flow.bijection.forward(view.contiguous())
    assert torch.equal(base, keep)
    assert torch.equal(lp_v, lp_c) and torch.equal(z_v, z_c) and torch.equal(ld_v, ld_c)
    inner = base[3:, 1:D + 1]                                 # a window into the middle of a larger buffer
    with torch.no_grad():
        lp_i = flow.log_prob(inner)
        lp_ic = flow.log_prob(inner.clone())
    assert torch.equal(lp_i, lp_ic) and torch.equal(base, keep)
    lin = next(m for m in flow.bijection.modules() if isinstance(m, torch.nn.Linear))
    with torch.no_grad():
        lin.weight.mul_(1.5)                                  # moves the version counter
        lp_new = flow.log_prob(view)
        lp_host = flow.cpu().log_prob(view.cpu())
    assert not torch.equal(lp_new, lp_c)
    assert rel(lp_new.cpu().numpy(), lp_host.numpy()) < 1e-5


def test_wide_leaves_training_alone(pkg, monkeypatch):
    """With gradients enabled the autograd route is untouched: a backward pass through log_prob at D = 784 gives gradients
    bit-identical between wide=0 and wide=1."""
    torch.manual_seed(4)
    flow = data_init(pkg.Flow(pkg.RealNVP((1, 28, 28), n_layers=2)), 784).cuda()
    x = torch.randn(48, 1, 28, 28, device="cuda")
    grads = {}
    for mode in ("1", "0"):
        set_debug(monkeypatch, wide=mode)
        drop_programs(flow)
        flow.zero_grad(set_to_none=True)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            loss = -flow.log_prob(x).mean()
            loss.backward()
        grads[mode] = [None if p.grad is None else p.grad.detach().clone() for p in flow.parameters()]
    set_debug(monkeypatch, wide=None)
    assert any(g is not None and bool(g.abs().sum() > 0) for g in grads["1"])
    for a, b in zip(grads["1"], grads["0"]):
        assert (a is None) == (b is None)
        if a is not None:
            assert torch.equal(a, b)
