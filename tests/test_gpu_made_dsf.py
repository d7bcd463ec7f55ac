"""The sequential map of the MADE-based deep sigmoidal layers in one launch (csrc/tfk_made_dsf.hip) against this package's
ATen composite path in float64 (``layer._sequential`` / ``layer._parallel`` on a ``.double()`` copy).  Bars, as in
tests/test_host_dsf.py: error < max(1e-5, 3 x floor), the floor being the float32 ATen path's distance from the float64
one; x norm-wise, the log-det relative to max(1, |ref|).  Layer built after ``manual_seed(0)``, its last MaskedLinear
times 500 (h std ~ 150), z = randn of a generator seeded 1.  A row is left out only when the float64 reference ends within
0.01 of the bracket's ends or its float64 round trip misses z by more than 1e-6; at most 2 % of the rows.  The reference
ends its bisection on a batch-wide ``allclose``: it is computed once per case on the largest batch used, smaller batches
are its first rows.  No MADE can be built at D = 1 (hidden degrees ``j mod (D - 1)``): that shape goes through the wrapper."""
import copy
import ctypes
import functools

import numpy as np
import pytest
import torch

from conftest import load_golden, set_debug, state_dict_of
from torchflows_amd import native
from test_host_dsf import bar, build_flow, normwise, rel

pytestmark = pytest.mark.gpu

# (D, MADE n_hidden, n_hidden_layers C, hidden_dim K)
CASES = [(2, None, 1, 1), (7, None, 2, 5), (7, 9, 2, 16), (7, None, 4, 8), (33, None, 3, 3), (130, None, 2, 10)]
SMALL = CASES[1]
TWINS = ["DeepSigmoidalForwardMaskedAutoregressive", "DeepSigmoidalInverseMaskedAutoregressive"]
ROWS = 65


def _layer(twin, D, n_hidden, C, K):
    from torchflows_amd.bijections.finite.autoregressive import layers
    torch.manual_seed(0)
    layer = getattr(layers, twin)((D,), transformer_kwargs=dict(n_hidden_layers=C, hidden_dim=K),
                                  conditioner_kwargs=dict(n_hidden=n_hidden)).eval()
    with torch.no_grad():
        layer.conditioner_transform.sequential[-1].weight.mul_(500.0)
        layer.conditioner_transform.sequential[-1].bias.mul_(500.0)
    return layer


def _ref(z, inverse, forward):
    """(z, x64, ld64, x32, ld32, keep) from the two maps, each called on (tensor, dtype)."""
    with torch.no_grad():
        (x64, ld64), (x32, ld32) = inverse(z.double(), torch.float64), inverse(z, torch.float32)
        back = forward(x64, torch.float64)[0]
    keep = (x64.abs().amax(1) < 9.99) & ((back - z.double()).abs().amax(1) <= 1e-6)
    return z, x64.numpy(), ld64.numpy(), x32.numpy(), ld32.numpy(), keep.numpy()


@functools.lru_cache(maxsize=None)
def _reference(case, rows=ROWS):
    """Both twins share it: the same weights, the same map."""
    by = {torch.float32: _layer(TWINS[0], *case)}
    by[torch.float64] = copy.deepcopy(by[torch.float32]).double()
    z = torch.randn(rows, case[0], generator=torch.Generator().manual_seed(1))
    return _ref(z, lambda t, dt: by[dt]._sequential(t, None), lambda t, dt: by[dt]._parallel(t, None))


def _check(ref, n, x, ld, label):
    z, x64, ld64, x32, ld32, keep = (t[:n] for t in ref)
    assert keep.mean() >= 0.98, f"{label}: {int((~keep).sum())} of {n} rows left out"
    x, ld = x.cpu().numpy(), ld.cpu().numpy()
    assert np.isfinite(x).all() and np.isfinite(ld).all()
    e_x, f_x = normwise(x[keep], x64[keep]), normwise(x32[keep], x64[keep])
    e_l, f_l = rel(ld[keep], ld64[keep]), rel(ld32[keep], ld64[keep])
    print(f"{label}: x {e_x:.2e} (floor {f_x:.2e}), log-det {e_l:.2e} (floor {f_l:.2e}), {int((~keep).sum())} rows left out")
    assert e_x < bar(f_x) and e_l < bar(f_l)


def _run(twin, case, n, rows=ROWS):
    layer, ref = _layer(twin, *case).cuda(), _reference(case, rows)
    z = ref[0][:n].cuda()
    before = native.calls
    with torch.no_grad():
        x, ld = layer.inverse(z) if twin == TWINS[0] else layer.forward(z)
    torch.cuda.synchronize()
    assert native.calls - before == 1, "the sequential map must be ONE launch (the host loop makes more than D)"
    assert x.shape == z.shape and ld.shape == (n,)
    _check(ref, n, x, ld, f"{twin} {case} N={n}")


@pytest.mark.parametrize("case,twin,n,rows", [(c, t, ROWS, ROWS) for c in CASES for t in TWINS]
                         + [(SMALL, TWINS[0], 1, 257), (SMALL, TWINS[0], 257, 257)], ids=str)
def test_layer_vs_float64(case, twin, n, rows):
    _run(twin, case, n, rows)


def test_wrapper_canaries_accumulate_alias():
    (D, _, C, K), n, ref = SMALL, ROWS, _reference(SMALL)
    packed = _layer(TWINS[0], *SMALL).cuda()._made_pack()
    z = ref[0].cuda()
    guard, ld_guard = torch.full((n + 2, D), 7.0).cuda(), torch.full((n + 2,), 7.0).cuda()
    out, ld = guard[1:-1], ld_guard[1:-1]
    native.made_dsf_sequential(z, out, ld, *packed, C, K)
    torch.cuda.synchronize()
    assert float(guard[0].min()) == 7.0 == float(guard[-1].max()) and ld_guard[0] == 7.0 == ld_guard[-1]
    _check(ref, n, out, ld, "wrapper")
    prior = torch.randn(n, generator=torch.Generator().manual_seed(3)).cuda()
    acc, x2 = prior.clone(), z.clone()
    native.made_dsf_sequential(x2, x2, acc, *packed, C, K, accumulate=True)            # out aliases z
    assert torch.equal(x2, out) and torch.equal(acc, prior + ld)


def test_single_element_rows():
    """D = 1, C = 2, K = 4: the element's record is b2 + W2 tanh(b1), its log-det the inverse's at z."""
    from torchflows_amd.bijections.finite.autoregressive.transformers.combination.sigmoid import DeepSigmoid
    C, K, n, g = 2, 4, ROWS, torch.Generator().manual_seed(0)
    W1t, b1 = torch.randn(1, 8, generator=g), torch.randn(8, generator=g)
    W2, b2 = 50.0 * torch.randn(1, 3 * K * C, 8, generator=g), 50.0 * torch.randn(1, 3 * K * C, generator=g)
    tr = DeepSigmoid((1,), n_hidden_layers=C, hidden_dim=K)
    h = lambda dt: (b2.to(dt) + W2.to(dt) @ torch.tanh(b1.to(dt))).expand(n, 1, 3 * K * C)
    ref = _ref(torch.randn(n, 1, generator=torch.Generator().manual_seed(1)),
               lambda t, dt: tr.inverse(t, h(dt)), lambda t, dt: tr.forward(t, h(dt)))
    x, ld = torch.empty(n, 1).cuda(), torch.empty(n).cuda()
    native.made_dsf_sequential(ref[0].cuda(), x, ld, W1t.cuda(), b1.cuda(), W2.cuda(), b2.cuda(), C, K)
    _check(ref, n, x, ld, "D = 1")


def test_errors():
    z, out, ld = torch.randn(4, 3).cuda(), torch.empty(4, 3).cuda(), torch.empty(4).cuda()
    f = lambda *s: torch.zeros(*s).cuda()
    for C, K in ((2, 17), (5, 4), (3, 9)):
        with pytest.raises(native.NativeError, match="hidden_dim"):
            native.made_dsf_sequential(z, out, ld, f(3, 8), f(8), f(3, 3 * K * C, 8), f(3, 3 * K * C), C, K)
    w = (f(3, 8), f(8), f(3, 24, 8), f(3, 24))
    with pytest.raises(native.NativeError, match="boundary"):
        native._launch("tfk_made_rqs_sequential", z, z.data_ptr(), out.data_ptr(), ld.data_ptr(), 4, 3,
                       *(t.data_ptr() for t in w), 8, native.made_dsf_code(2, 4), ctypes.c_float(5.0), 0)


@pytest.mark.parametrize("name,arch", [("flow_madeepsf6.npz", "MaskedAutoregressiveDeepSF"),
                                       ("flow_iadeepsf6.npz", "InverseAutoregressiveDeepSF")])
def test_flow_fixtures_with_default_settings(monkeypatch, name, arch):
    """The bars of tests/test_gpu_dsf.py::test_flow_golden_on_hip, on the default route."""
    fx = load_golden(name)
    flow = build_flow(arch, fx, None)
    flow.load_state_dict({k: torch.from_numpy(v) for k, v in state_dict_of(fx, "init").items()}, strict=True)
    flow = flow.cuda().eval()
    x, z_in = torch.from_numpy(fx["x"]).cuda(), torch.from_numpy(fx["z_in"]).cuda()
    before = native.calls
    with torch.no_grad():
        (z, lp), (xr, ldr) = flow.forward_with_log_prob(x), flow.bijection.inverse(z_in)
        n_default = native.calls - before
        set_debug(monkeypatch, made_fused=0)
        flow.forward_with_log_prob(x), flow.bijection.inverse(z_in)
    assert native.calls - before - n_default == n_default + 2 * (x.shape[1] - 1), "one launch per layer in place of D"
    for got, key, measure in ((lp, "log_prob", rel), (z, "z", normwise), (xr, "x_inv", normwise), (ldr, "log_det_inv", rel)):
        e, floor = measure(got.cpu().numpy(), fx[f"init/{key}"]), measure(fx[f"init/{key}"], fx[f"init/{key}64"])
        print(f"{name} {key}: {e:.2e} (floor {floor:.2e})")
        assert e < bar(floor), key
