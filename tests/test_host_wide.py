"""Host-side tests of the wide-row route (event sizes above 256): packer + fp64 emulator against the composition, and
what ``compile_chain`` takes / declines.  No GPU needed."""
import warnings

import pytest
import torch

from conftest import set_debug

CPU = torch.device("cpu")


def _flow(arch, D, n_layers, **kw):
    import torchflows_amd as tfa
    torch.manual_seed(3)
    flow = tfa.Flow(getattr(tfa, arch)(D, n_layers=n_layers, **kw))
    flow.train()
    with torch.no_grad():
        flow.log_prob(torch.randn(64, D) * 1.5 + 0.3)          # ActNorm's data-dependent initialisation
    return flow.eval()


@pytest.mark.parametrize("direction", [0, 1])
@pytest.mark.parametrize("n_layers", [1, 3])
@pytest.mark.parametrize("D", [258, 784])
@pytest.mark.parametrize("arch", ["RealNVP", "NICE"])
def test_wide_packer_against_fp64_emulator(arch, D, n_layers, direction):
    """fused_wide.compile_wide (elementwise layers deferred and folded into W1 / b1, pre-affines, pre-scaled logits,
    reversals folded into the column order, planes padded to a multiple of 64, lane-major operands per wave): an fp64
    emulator that decodes the packed blocks exactly as csrc/tfk_flow_wide.h reads them must reproduce the composition's
    forward / inverse.  17 rows: one tile and a ragged second one."""
    from wide_emulator import run_wide
    from torchflows_amd import flow_compile, fused, fused_wide
    flow = _flow(arch, D, n_layers)
    comp = flow.bijection.double()
    order = comp.layers if direction == 0 else list(comp.layers)[::-1]
    plan = flow_compile._flatten(order, "forward" if direction == 0 else "inverse")
    chain = fused_wide.compile_wide(comp, plan, CPU, D, direction)
    assert chain is not None and fused_wide.is_wide(chain)
    hp = fused_wide.plane_width(D)
    assert chain.D == 2 * hp and chain.D_log == D and hp % 64 == 0 and hp >= D // 2
    seg = chain.segments[0]
    n_c = len(seg.ops) - 1
    assert seg.ops[-1][0] == fused.OP_EW_FMA and n_c >= 1
    assert seg.params.numel() == n_c * fused_wide.block_floats(hp, arch == "RealNVP") + 4 * hp + 4
    x = torch.randn(17, D, dtype=torch.float64)
    with torch.no_grad():
        want, ld_want = (comp.forward if direction == 0 else comp.inverse)(x)
    rev = fused_wide._reversed_out(chain)
    z, ld = run_wide(seg.ops, seg.params, x, D, reverse_out=rev)
    if chain.identity_out or rev:
        got = z
    else:
        half = D // 2
        got = z[:, torch.where(chain.pos < hp, chain.pos, chain.pos - hp + half)]
    # the blocks are stored in fp32: agreement at fp32 resolution of the weights (the lean emulator tests' bar)
    assert float((got - want).abs().max() / want.abs().max()) < 2e-5
    assert float((ld - ld_want).abs().max() / max(1.0, float(ld_want.abs().max()))) < 2e-5


@pytest.mark.parametrize("D", [258, 300, 784, 1024, 2048])
def test_compile_chain_takes_even_sizes_above_256(D, monkeypatch):
    """One wide segment per direction -- and with wide=0 what the releases before this route returned: nothing, except
    the vector-ALU interpreter's program at its powers of two."""
    from torchflows_amd import fused
    monkeypatch.delenv("TORCHFLOWS_AMD_MFMA", raising=False)
    flow = _flow("RealNVP", D, 2)
    for direction in (0, 1):
        chain = fused.compile_chain(flow.bijection, direction, CPU)
        assert chain is not None and len(chain.segments) == 1 and chain.segments[0].wide and chain.segments[0].mfma
        assert chain.D_log == D and fused.sample_ready(chain) and not fused.sum_ready(chain)
    set_debug(monkeypatch, wide=0)
    for direction in (0, 1):
        chain = fused.compile_chain(flow.bijection, direction, CPU)
        if D in (1024, 2048):                                 # (tfk_flow_supported: powers of two)
            assert chain is None or not any(seg.wide for seg in chain.segments)
        else:
            assert chain is None


def test_compile_chain_512_keeps_the_interpreter_without_mfma(monkeypatch):
    from torchflows_amd import fused
    flow = _flow("RealNVP", 512, 2)
    chain = fused.compile_chain(flow.bijection, 0, CPU)
    assert chain is not None and chain.segments[0].wide
    monkeypatch.setenv("TORCHFLOWS_AMD_MFMA", "0")
    chain = fused.compile_chain(flow.bijection, 0, CPU)
    assert chain is not None and not any(seg.wide or seg.mfma for seg in chain.segments)


def test_compile_chain_still_declines(monkeypatch):
    """Odd sizes, hidden width 17, a context, spline / MADE layers above 256: no program, and the warning's reason says
    which of these it was."""
    import torchflows_amd as tfa
    from torchflows_amd import fused
    monkeypatch.delenv("TORCHFLOWS_AMD_MFMA", raising=False)
    cases = {
        "odd": (_flow("RealNVP", 785, 2), False, "odd"),
        "hidden": (_flow("RealNVP", 784, 2, conditioner_kwargs=dict(n_hidden=17)), False, "hidden width 17"),
        "3072": (_flow("RealNVP", 3072, 1), False, "3072"),
        "spline": (_flow("CouplingRQNSF", 300, 1), False, "rqs"),
        "made": (_flow("MAF", 300, 1), False, "MADE"),
    }
    for name, (flow, ctx, word) in cases.items():
        for direction in (0, 1):
            assert fused.compile_chain(flow.bijection, direction, CPU, context=ctx) is None, name
        assert word in fused._why_declined(flow.bijection, 0), (name, fused._why_declined(flow.bijection, 0))
    torch.manual_seed(0)
    cflow = tfa.Flow(tfa.RealNVP(784, context_shape=(3,), n_layers=2)).eval()
    assert fused.compile_chain(cflow.bijection, 0, CPU, context=True) is None
    assert "context" in fused._why_declined(cflow.bijection, 0)
    # the warning itself
    flow = cases["odd"][0]
    flow.bijection.__dict__.pop("_tfk_declined_warned", None)
    with warnings.catch_warnings(record=True) as seen:
        warnings.simplefilter("always")
        fused.warn_declined(flow.bijection, 0)
    assert any(issubclass(w.category, fused.NativeRouteWarning) and "odd" in str(w.message) for w in seen)


def test_wide_supported_matches_the_header():
    from torchflows_amd import native
    L = native.lib()
    for D, H, want in ((258, 16, 1), (2048, 1, 1), (784, 14, 1), (256, 8, 0), (785, 8, 0), (2050, 8, 0), (784, 17, 0),
                       (784, 0, 0)):
        assert L.tfk_flow_wide_supported(D, H) == want, (D, H)
