"""GEMM 2 of affine / shift chains in the split-f16 operand format (csrc/tfk_flow_chain.h: couple_lean_h, one
v_mfma_f32_16x16x32_f16 per tile; TORCHFLOWS_AMD_DEBUG=lean_f16x2=1) on the GPU, held to the bars of
test_gpu_fused.py::test_affine_chain_bf16x3_operands: log_prob within 1e-5 of the host's fp64 evaluation and within 2e-6 of
the fp32 operand format, one libtfk launch per log_prob, the inverse undoes the forward at atol 2e-4."""
import copy

import numpy as np
import pytest
import torch

from conftest import set_debug

pytestmark = pytest.mark.gpu


def rel(a, b):
    a = np.asarray(a, np.float64)
    b = np.asarray(b, np.float64)
    return float(np.nanmax(np.abs(a - b) / np.maximum(1.0, np.abs(b)))) if a.size else 0.0


def normwise(a, b):
    a = np.asarray(a, np.float64).ravel()
    b = np.asarray(b, np.float64).ravel()
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-30))


def make_flow(arch, D, n_layers, seed=2, **kw):
    import torchflows_amd as tfa
    torch.manual_seed(seed)
    flow = tfa.Flow(getattr(tfa, arch)(D, n_layers=n_layers, **kw))
    flow.train()
    with torch.no_grad():
        flow.log_prob(torch.randn(1024, D))
    flow.eval()
    return flow


def conditioners(flow):
    """(first Linear, second Linear) of every coupling's conditioner."""
    out = []
    for m in flow.bijection.modules():
        ct = getattr(m, "conditioner_transform", None)
        if ct is not None and hasattr(ct, "sequential"):
            out.append((ct.sequential[0], ct.sequential[2]))
    return out


def is_f16(flow):
    from torchflows_amd import fused
    chain = fused.get_compiled(flow.bijection, 0, torch.device("cuda", 0))
    return chain is not None and all(len(op) > 4 and int(op[4]) == 512
                                     for seg in chain.segments for op in seg.ops if 12 <= op[0] <= 15)


def check(flow, x, monkeypatch, label, row_counts=(2000,)):
    """The two log_prob bars, the launch count and the round trip, at every row count (prefixes of x)."""
    from torchflows_amd import native
    with torch.no_grad():
        lp_h = copy.deepcopy(flow).double().log_prob(x.double())          # the reference, once
        flow = flow.cuda()
        xd = x.cuda()
        set_debug(monkeypatch, lean_f16x2="0")
        flow.invalidate_native_caches()
        assert not is_f16(flow)
        lp0 = {n: flow.log_prob(xd[:n]) for n in row_counts}
        set_debug(monkeypatch, lean_f16x2="1")
        flow.invalidate_native_caches()
        assert is_f16(flow), "operand format"
        for n in row_counts:
            before = native.calls
            lp1 = flow.log_prob(xd[:n])
            assert native.calls - before == 1
            z1, ld1 = flow.bijection.forward(xd[:n])
            xr, ldr = flow.bijection.inverse(z1)
            e_h, e_0 = rel(lp1.cpu().numpy(), lp_h[:n].numpy()), rel(lp1.cpu().numpy(), lp0[n].cpu().numpy())
            print(f"{label}, {n} rows, split-f16 operands: log_prob vs fp64 host {e_h:.2e}, vs the fp32 operand format {e_0:.2e}")
            assert e_h < 1e-5 and e_0 < 2e-6
            assert torch.allclose(xr.cpu(), x[:n], atol=2e-4) and torch.allclose(ld1, -ldr, atol=1e-3)
    return flow


@pytest.mark.parametrize("arch,D,n_layers,kw", [
    ("RealNVP", 64, 4, {}), ("NICE", 64, 3, {}), ("RealNVP", 32, 2, {}), ("RealNVP", 128, 2, {}),
    ("RealNVP", 64, 2, dict(conditioner_kwargs=dict(n_hidden=10)))])
def test_split_f16_operands(monkeypatch, arch, D, n_layers, kw):
    """1 row (a partial wave), 17 (not a multiple of 16) and 2000 (several workgroups); 100 rows are scaled x 4."""
    flow = make_flow(arch, D, n_layers, **kw)
    x = torch.randn(2000, D)
    x[:100] *= 4.0
    check(flow, x, monkeypatch, f"{arch}({D}, {n_layers}{', n_hidden=10' if kw else ''})", row_counts=(1, 17, 2000))


def test_split_f16_sample_round_trip(monkeypatch):
    """Flow.sample runs the inverse program (KIND 1: 1 / alpha = exp2(-o)): the same samples and log-probabilities as the
    fp32 operand format from the same noise."""
    flow = make_flow("RealNVP", 64, 4).cuda()
    with torch.no_grad():
        set_debug(monkeypatch, lean_f16x2="1")
        flow.invalidate_native_caches()
        torch.manual_seed(11)
        xs, lps = flow.sample((500,), return_log_prob=True)
        assert is_f16(flow)
        set_debug(monkeypatch, lean_f16x2="0")
        flow.invalidate_native_caches()
        torch.manual_seed(11)
        xs32, lps32 = flow.sample((500,), return_log_prob=True)
    e_x, e_lp = normwise(xs.cpu().numpy(), xs32.cpu().numpy()), rel(lps.cpu().numpy(), lps32.cpu().numpy())
    print(f"sample, split-f16 vs fp32 operands: x {e_x:.2e}, log_prob {e_lp:.2e}")
    assert e_x < 2e-6 and e_lp < 2e-6


def test_split_f16_log_shortcut_rerun(monkeypatch):
    """Scale logits below -8 make the kernel run the chain again with the logarithms: three elements of the LAST coupling get
    their scale logit u shifted by -12.5 (the kernel's (u / 2 + c0) log2 e is then ~ -9, alpha ~ 2e-3).  The last coupling,
    because the inverse divides by alpha: there it sees the stored z itself (error ~ ulp(z) / alpha ~ 3e-5 |z|), while behind
    further couplings it would amplify their round-trip error 500-fold, past the 2e-4 bar in any operand format."""
    flow = make_flow("RealNVP", 64, 4)
    lin2 = conditioners(flow)[-1][1]
    with torch.no_grad():
        lin2.bias.view(-1, 2)[:3, 0] -= 12.5
    x = torch.randn(2000, 64)
    x[:100] *= 4.0
    check(flow, x, monkeypatch, "RealNVP(64, 4), scale logits below -8", row_counts=(17, 2000))


@pytest.mark.parametrize("w2_scale", [1.0, 1e-2, 30.0])
def test_split_f16_small_operands(monkeypatch, w2_scale):
    """|h| <~ 1e-3 (W1 and b1 scaled by 1e-3): the lo pieces of the activations are f16 subnormals, and with W2 scaled by
    1e-2 so are those of the weights -- the cases that decide whether v_mfma_f32_16x16x32_f16 keeps subnormal inputs; W2
    scaled by 30 makes the products large again.  The same two bars."""
    flow = make_flow("RealNVP", 64, 4)
    with torch.no_grad():
        for lin1, lin2 in conditioners(flow):
            lin1.weight.mul_(1e-3)
            lin1.bias.mul_(1e-3)
            lin2.weight.mul_(w2_scale)
    x = torch.randn(2000, 64)
    x[:100] *= 4.0
    check(flow, x, monkeypatch, f"RealNVP(64, 4), W1 x 1e-3, W2 x {w2_scale:g}")
