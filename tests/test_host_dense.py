"""Host-side tests of the dense sigmoidal family (DenseSigmoid / DeepDenseSigmoid, CouplingDenseSF, CouplingDeepDenseSF and
their MADE twins): imports, parameter counts, state dicts, and the ATen composite path against the fixtures the reference
produced (tests/golden/make_golden_dense.py).  No GPU needed.

The global-parameter mask of a coupling conditioner is drawn at construction and is no part of the state dict: the flows
are built after ``torch.manual_seed(0)``, as the generator builds them.  Bars: test_host_dsf.bar."""
import pytest
import torch

from conftest import load_golden, state_dict_of
from test_host_dsf import bar, normwise, rel

FLOWS = [
    ("flow_cdensesf16.npz", "CouplingDenseSF"),
    ("flow_cdeepdensesf6.npz", "CouplingDeepDenseSF"),
    ("flow_madensesf6.npz", "MaskedAutoregressiveDenseSF"),
    ("flow_iadeepdensesf6.npz", "InverseAutoregressiveDeepDenseSF"),
]
PRESETS = ("CouplingDenseSF", "InverseAutoregressiveDenseSF", "MaskedAutoregressiveDenseSF", "CouplingDeepDenseSF",
           "InverseAutoregressiveDeepDenseSF", "MaskedAutoregressiveDeepDenseSF")


def build_flow(arch, fx, variant="init", **kwargs):
    import torchflows_amd as tfa
    torch.manual_seed(0)
    flow = tfa.Flow(getattr(tfa, arch)(tuple(int(v) for v in fx["event_shape"]), n_layers=2, **kwargs))
    flow.load_state_dict({k: torch.from_numpy(v) for k, v in state_dict_of(fx, variant).items()}, strict=True)
    return flow.eval()


def test_presets_resolve_by_both_spellings():
    import torchflows
    import torchflows_amd as tfa
    import torchflows.architectures as A1
    import torchflows.bijections.finite.autoregressive.architectures as A3
    for name in PRESETS:
        assert all(getattr(m, name) is getattr(tfa, name) for m in (torchflows, A1, A3)), name


def test_parameter_counts():
    import torchflows_amd as tfa
    from torchflows_amd.bijections.finite.autoregressive.transformers.combination.dense_sigmoid import (
        DeepDenseSigmoid, DenseSigmoid)
    assert DenseSigmoid((3,)).n_parameters_per_element == 243 and DeepDenseSigmoid((3,)).n_parameters_per_element == 486
    assert not DenseSigmoid((3,)).state_dict() and float(DeepDenseSigmoid((3,)).default_parameters.abs().sum()) == 0.0
    ct = tfa.CouplingDenseSF(6).layers[2].conditioner_transform
    assert tuple(ct.parameter_shape) == (3, 243) and (ct.n_global_parameters, ct.n_predicted_parameters) == (583, 146)
    for arch in ("MaskedAutoregressiveDenseSF", "InverseAutoregressiveDenseSF"):
        ct = getattr(tfa, arch)(6).layers[2].conditioner_transform
        assert (ct.n_global_parameters, ct.n_predicted_parameters) == (0, 1458)


@pytest.mark.parametrize("variant", ["fresh", "init"])
@pytest.mark.parametrize("name,arch", FLOWS)
def test_aten_path_reproduces_flow_fixture(name, arch, variant):
    fx = load_golden(name)
    flow = build_flow(arch, fx, variant)
    g = lambda k: fx[f"{variant}/{k}"]
    with torch.no_grad():
        z, ld = flow.bijection.forward(torch.from_numpy(fx["x"]))
        xr, ldr = flow.bijection.inverse(torch.from_numpy(fx["z_in"]))
    assert normwise(z.numpy(), g("z")) < bar(normwise(g("z"), g("z64")))
    assert rel(ld.numpy(), g("log_det")) < bar(rel(g("log_det"), g("log_det64")))
    assert normwise(xr.numpy(), g("x_inv")) < bar(normwise(g("x_inv"), g("x_inv64")))
    assert rel(ldr.numpy(), g("log_det_inv")) < bar(rel(g("log_det_inv"), g("log_det_inv64")))


def test_programs_decline_and_the_kernel_is_probed():
    from torchflows_amd import fused, native
    flow = build_flow("CouplingDenseSF", load_golden("flow_cdensesf16.npz"))
    for direction in (0, 1):
        assert fused.compile_chain(flow.bijection, direction, torch.device("cpu")) is None
    assert "dense" in fused._why_declined(flow.bijection, 0)
    L = native.lib()
    ok = {(H, Ld, C): L.tfk_dsf_supported(native.dense_code(C, Ld), H) for H in (0, 1, 8, 9) for Ld in (0, 1, 2, 3)
          for C in (0, 1, 2, 3)}
    assert {k for k, v in ok.items() if v} == {(H, Ld, C) for H in (1, 8) for Ld in (0, 1, 2) for C in (1, 2)} - {(8, 2, 2)}
