"""Host-side tests of the deep sigmoidal family (Sigmoid / DeepSigmoid, CouplingDeepSF and its MADE twins): imports,
state dicts, and this package's ATen composite path against the fixtures the reference produced
(tests/golden/make_golden_dsf.py).  No GPU needed.

Bars: every error against max(1e-5, 3 x the fixture's own fp32-vs-fp64 distance), in the measures of
tests/test_gpu_flows.py::test_flow_golden_on_hip (log_prob and log-dets elementwise relative to max(1, |ref|), z and x
norm-wise)."""
import numpy as np
import pytest
import torch

from conftest import load_golden, state_dict_of

FLOWS = [
    ("flow_cdeepsf16.npz", "CouplingDeepSF", None),
    ("flow_cdeepsf21.npz", "CouplingDeepSF", None),
    ("flow_madeepsf6.npz", "MaskedAutoregressiveDeepSF", None),
    ("flow_iadeepsf6.npz", "InverseAutoregressiveDeepSF", None),
    ("flow_cdeepsf16_ctx3.npz", "CouplingDeepSF", (3,)),
]
PRESETS = ("CouplingDeepSF", "MaskedAutoregressiveDeepSF", "InverseAutoregressiveDeepSF")
LAYERS = ("DeepSigmoidalCoupling", "DeepSigmoidalForwardMaskedAutoregressive", "DeepSigmoidalInverseMaskedAutoregressive")


def rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.nanmax(np.abs(a - b) / np.maximum(1.0, np.abs(b)))) if a.size else 0.0


def normwise(a, b):
    a, b = np.asarray(a, np.float64).ravel(), np.asarray(b, np.float64).ravel()
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-30))


def bar(floor):
    return max(1e-5, 3 * floor)


def build_flow(arch, fx, ctx_shape, dtype=torch.float32):
    import torchflows_amd as tfa
    es = tuple(int(v) for v in fx["event_shape"])
    kw = dict(n_layers=2)
    if ctx_shape is not None:
        kw["context_shape"] = ctx_shape
    return tfa.Flow(getattr(tfa, arch)(es, **kw)).to(dtype)


def dsf_transformer(tag, T):
    from torchflows_amd.bijections.finite.autoregressive.transformers.combination.sigmoid import DeepSigmoid, Sigmoid
    C, K = int(tag[1]), int(tag.split("_K")[1])
    return (Sigmoid((T,), hidden_dim=K) if C == 1 else DeepSigmoid((T,), n_hidden_layers=C, hidden_dim=K)), C, K


def test_imports_resolve_by_both_spellings():
    import torchflows
    import torchflows_amd as tfa
    import torchflows.architectures as A1
    import torchflows.bijections.finite.autoregressive as A2
    import torchflows.bijections.finite.autoregressive.architectures as A3
    import torchflows.bijections.finite.autoregressive.layers as L1
    import torchflows_amd.bijections.finite.autoregressive.layers as L2
    import torchflows.bijections.finite.autoregressive.transformers.combination.sigmoid as S1
    import torchflows_amd.bijections.finite.autoregressive.transformers.combination.sigmoid as S2
    import torchflows.bijections.finite.autoregressive.transformers.combination.base as B1
    import torchflows_amd.bijections.finite.autoregressive.transformers.combination.base as B2
    import torchflows.bijections.numerical_inversion as N1
    import torchflows_amd.bijections.numerical_inversion as N2
    for name in PRESETS:
        cls = getattr(tfa, name)
        assert all(getattr(m, name) is cls for m in (torchflows, A1, A2, A3)), name
    for name in LAYERS:
        assert getattr(L1, name) is getattr(L2, name)
    assert S1.Sigmoid is S2.Sigmoid and S1.DeepSigmoid is S2.DeepSigmoid and B1.Combination is B2.Combination
    assert N1.bisection_no_gradient is N2.bisection_no_gradient
    assert S2.Sigmoid.native_kind == "dsf" and S2.DeepSigmoid.native_kind == "dsf"
    # the rest of the family stays out
    for missing in ("DenseSigmoid", "DeepDenseSigmoid"):
        assert not hasattr(S2, missing)
    with pytest.raises(ImportError):
        from torchflows.bijections.finite.autoregressive import CouplingDenseSF  # noqa: F401


def test_transformer_shape_rules():
    from torchflows_amd.bijections.finite.autoregressive.transformers.combination.sigmoid import DeepSigmoid, Sigmoid
    for n, K in ((1, 4), (8, 4), (11, 5), (99, 5), (100, 10), (999, 10), (1000, 15)):
        tr = DeepSigmoid((n,))
        assert tr.hidden_dim == K and tr.n_components == 2 and tuple(tr.parameter_shape) == (n, 6 * K)
        assert Sigmoid((n,)).hidden_dim == K
    tr = DeepSigmoid((3,), n_hidden_layers=3, hidden_dim=7)
    assert tuple(tr.parameter_shape_per_element) == (63,) and isinstance(tr.components, list)
    assert len(list(tr.parameters())) == 0 and len(list(tr.buffers())) == 0 and len(tr.state_dict()) == 0


@pytest.mark.parametrize("name,arch,ctx_shape", FLOWS)
def test_state_dict_loads_strict(name, arch, ctx_shape):
    fx = load_golden(name)
    flow = build_flow(arch, fx, ctx_shape)
    for variant in ("fresh", "init"):
        sd = {k: torch.from_numpy(v) for k, v in state_dict_of(fx, variant).items()}
        assert list(flow.state_dict().keys()) == list(sd.keys())
        flow.load_state_dict(sd, strict=True)


@pytest.mark.parametrize("variant", ["fresh", "init"])
@pytest.mark.parametrize("name,arch,ctx_shape", FLOWS)
def test_aten_path_reproduces_flow_fixture(name, arch, ctx_shape, variant):
    fx = load_golden(name)
    flow = build_flow(arch, fx, ctx_shape)
    flow.load_state_dict({k: torch.from_numpy(v) for k, v in state_dict_of(fx, variant).items()}, strict=True)
    flow.eval()
    ctx = torch.from_numpy(fx["context"]) if ctx_shape else None
    x, z_in = torch.from_numpy(fx["x"]), torch.from_numpy(fx["z_in"])
    g = lambda k: fx[f"{variant}/{k}"]
    with torch.no_grad():
        z, lp = flow.forward_with_log_prob(x, context=ctx)
        xr, ldr = flow.bijection.inverse(z_in, context=ctx)
        lp2 = flow.log_prob(x, context=ctx)
    e_lp, e_z = rel(lp.numpy(), g("log_prob")), normwise(z.numpy(), g("z"))
    e_x, e_ld = normwise(xr.numpy(), g("x_inv")), rel(ldr.numpy(), g("log_det_inv"))
    floors = (rel(g("log_prob"), g("log_prob64")), normwise(g("z"), g("z64")), normwise(g("x_inv"), g("x_inv64")),
              rel(g("log_det_inv"), g("log_det_inv64")))
    print(f"{name} {variant}: log_prob {e_lp:.2e}, z {e_z:.2e}, x_inv {e_x:.2e}, log_det_inv {e_ld:.2e}; floors "
          + ", ".join(f"{f:.2e}" for f in floors))
    assert e_lp < bar(floors[0]) and rel(lp2.numpy(), g("log_prob")) < bar(floors[0])
    assert e_z < bar(floors[1])
    assert e_x < bar(floors[2])
    assert e_ld < bar(floors[3])


def test_aten_path_reproduces_layer_fixture():
    fx = load_golden("dsf.npz")
    tgt = torch.from_numpy(fx["tgt"]).long()
    for tag in fx["cases"]:
        tr, C, K = dsf_transformer(str(tag), tgt.numel())
        g = lambda k: fx[f"{tag}_{k}"]
        x, h, z_in = torch.from_numpy(g("x"))[:, tgt], torch.from_numpy(g("h")), torch.from_numpy(g("z_in"))
        assert h.shape[-1] == 3 * K * C and float(h.std()) >= 500.0
        keep = ~g("clip")
        assert keep.mean() >= 0.98
        with torch.no_grad():
            z, ld = tr.forward(x, h)
            xi, ldi = tr.inverse(z_in, h[:z_in.shape[0]])
        assert normwise(z.numpy(), g("z")) < bar(normwise(g("z"), g("z64")))
        assert rel(ld.numpy(), g("ld")) < bar(rel(g("ld"), g("ld64")))
        assert normwise(xi.numpy()[keep], g("xinv")[keep]) < bar(normwise(g("xinv")[keep], g("xinv64")[keep]))
        assert rel(ldi.numpy(), g("ldinv")) < bar(rel(g("ldinv"), g("ldinv64")))


def test_aten_composite_grads_golden_dsf():
    """The fixture the device route is held to (the reference's own autograd on the weights of flow_cdeepsf16.npz) is
    pinned on the host too, in the form of tests/test_host_wide_train.py::test_aten_composite_grads_golden_wide."""
    from test_grads_cpu import _mirror_flow, normwise as nw
    fx, gr = load_golden("flow_cdeepsf16.npz"), load_golden("grads_flow_cdeepsf16.npz")
    flow = _mirror_flow("CouplingDeepSF", (16,), 2, state_dict_of(fx, "init"))
    x = torch.tensor(fx["x"], requires_grad=True)
    loss = (flow.log_prob(x) * torch.tensor(gr["w"])).sum()
    named = [(n, p) for n, p in flow.named_parameters() if p.requires_grad]
    assert [n for n, _ in named] == list(gr["trainable"])
    grads = torch.autograd.grad(loss, [x] + [p for _, p in named], allow_unused=True)
    assert nw(grads[0].numpy(), gr["gx64"]) < max(1e-5, 3 * nw(gr["gx"], gr["gx64"]))
    for (name, _), g in zip(named, grads[1:]):
        if g is None:
            continue
        r32, r64 = gr["g/" + name], gr["g64/" + name]
        assert nw(g.numpy(), r64) < max(1e-5, 3 * nw(r32, r64)), name


def test_inverse_carries_no_gradient_through_x():
    """The bisection is not differentiated: the gradient of the inverse reaches h through the log-det only."""
    from torchflows_amd.bijections.finite.autoregressive.transformers.combination.sigmoid import DeepSigmoid
    torch.manual_seed(0)
    tr = DeepSigmoid((3,))
    h = (300 * torch.randn(5, 3, 24)).requires_grad_(True)
    z = torch.randn(5, 3, requires_grad=True)
    x, ld = tr.inverse(z, h)
    assert not x.requires_grad and ld.requires_grad
    (gh,) = torch.autograd.grad(ld.sum(), h)
    assert torch.isfinite(gh).all() and float(gh.abs().max()) > 0


def test_supported_matches_the_header():
    from torchflows_amd import native
    L = native.lib()
    for K in range(1, 17):
        for C in (1, 2):
            assert L.tfk_dsf_supported(C, K) == 1, (C, K)
        for C in (3, 4):
            assert L.tfk_dsf_supported(C, K) == (1 if K <= 8 else 0), (C, K)
    for C, K in ((0, 4), (2, 0), (2, 17), (5, 4), (5, 8), (-1, 4), (2, -3)):
        assert L.tfk_dsf_supported(C, K) == 0, (C, K)
    assert native.ABI_VERSION == 29 and L.tfk_abi_version() == 29
    for name in ("tfk_dsf_supported", "tfk_dsf_coupling_fwd", "tfk_dsf_coupling_inv", "tfk_dsf_coupling_bwd"):
        assert name in native.SYMBOLS and hasattr(L, name)


def test_compile_chain_declines_and_says_why():
    import torchflows_amd as tfa
    from torchflows_amd import fused
    torch.manual_seed(0)
    for arch, D in (("CouplingDeepSF", 16), ("MaskedAutoregressiveDeepSF", 6), ("InverseAutoregressiveDeepSF", 6)):
        flow = tfa.Flow(getattr(tfa, arch)(D, n_layers=2)).eval()
        for direction in (0, 1):
            assert fused.compile_chain(flow.bijection, direction, torch.device("cpu")) is None, arch
        why = fused._why_declined(flow.bijection, 0)
        assert "dsf" in why or "DeepSigmoid" in why, why


def test_training_plan_takes_the_density_direction_only():
    """Forward (density) steps have reverse-mode kernels; the inverse of a coupling is a bisection without gradient."""
    import torchflows_amd as tfa
    from torchflows_amd import autograd as ag
    torch.manual_seed(0)
    flow = tfa.Flow(tfa.CouplingDeepSF(16, n_layers=2))
    assert ag.training_plan(flow.bijection, ag.FORWARD) is not None
    assert ag.training_plan(flow.bijection, ag.INVERSE) is None
    maf = tfa.Flow(tfa.MaskedAutoregressiveDeepSF(6, n_layers=2))
    assert ag.training_plan(maf.bijection, ag.FORWARD) is not None
    assert ag.training_plan(maf.bijection, ag.INVERSE) is None
    odd = tfa.Flow(tfa.CouplingDeepSF(16, n_layers=2, transformer_kwargs=dict(hidden_dim=17)))
    assert ag.training_plan(odd.bijection, ag.FORWARD) is None
