"""Host logic of the split-f16 operand format of lean affine / shift couplings (flow_pack._pack_lean(f16x2=True),
csrc/tfk_flow_chain.h: couple_lean_h), without a GPU: a decoder that reads the block exactly as the kernel does -- the
W1 row order of the format, f16 pieces of weights and activations in their slot pattern, one K = 32 product per tile on
an fp32 accumulator that starts at b2 -- composed with tests/lean_emulator.py for the closing TFK_OP_EW_FMA."""
import pytest
import torch

from conftest import set_debug
from lean_emulator import run_lean

import torchflows_amd as tfa
from torchflows_amd import flow_compile

LN2 = 0.6931471805599453


def decode_f16_coupling(op, params, rows, D):
    """One lean coupling op in the split-f16 format on rows (N, D) fp64 -> (rows, log-det)."""
    kind, plane, _, off = op[:4]
    assert int(op[4]) == 512 and plane in (0, 1)
    lk = kind - 12
    affine = lk < 2
    EPL, HALF = D // 8, D // 2
    T2 = EPL // 2 if affine else EPL // 4
    prm = params.double()
    raw = params.contiguous().view(torch.int16)                     # two f16 per fp32 slot, element 0 in the low half
    o_b1 = off + EPL * 64
    o_a2 = o_b1 + 16
    o_b2 = o_a2 + T2 * 256
    o_pre = o_b2 + T2 * 16
    A1 = prm[off:o_b1].reshape(EPL // 4, 64, 4)
    b1 = prm[o_b1:o_a2]
    A2h = raw[2 * o_a2:2 * o_b2].view(torch.float16).double().reshape(T2, 64, 8)
    b2 = prm[o_b2:o_pre].reshape(T2, 16)                              # [t][4 q + r]
    pre_s, pre_t = prm[o_pre:o_pre + HALF], prm[o_pre + HALF:o_pre + 2 * HALF]
    src = rows[:, plane * HALF:(plane + 1) * HALF]
    tgt = rows[:, (1 - plane) * HALF:(2 - plane) * HALF].clone()
    # GEMM 1 (fp32 MFMAs): A value of (M-row i, k-group q') sits in lane i + 16 q', k-step s = source column EPL q' + s
    Wm = torch.zeros(16, HALF, dtype=torch.float64)
    for s in range(EPL):
        for qk in range(4):
            Wm[:, EPL * qk + s] = A1[s // 4, 16 * qk:16 * qk + 16, s % 4]
    acc = b1[None, :] + src @ Wm.t()                                # (N, 16): column 4 q + r = register r of lane group q
    tgt = pre_s * tgt + pre_t
    h = (1.0 - 2.0 / (torch.exp2(acc) + 1.0)).float()               # the kernel's tanh is an fp32 value
    hi = h.half()
    lo = (h - hi.float()).half()
    hi, lo = hi.double(), lo.double()
    N = rows.shape[0]
    # the lane's B-operand: [hi0 lo0 hi0 hi1 | lo1 hi1 hi2 lo2] of its registers 0..2 (register 3 is never read)
    B = torch.zeros(N, 4, 8, dtype=torch.float64)
    for q in range(4):
        h0, h1, h2 = 4 * q, 4 * q + 1, 4 * q + 2
        B[:, q] = torch.stack([hi[:, h0], lo[:, h0], hi[:, h0], hi[:, h1], lo[:, h1], hi[:, h1], hi[:, h2], lo[:, h2]], dim=1)
    ld2 = torch.zeros(N, dtype=torch.float64)
    for t in range(T2):
        A = A2h[t].reshape(4, 16, 8)                                # [k-group q][row i][slot]
        o = (b2[t][None, :] + torch.einsum("qis,nqs->ni", A, B)).float().double()     # fp32 accumulator
        for q in range(4):
            for r in range(4):
                v = o[:, 4 * q + r]
                if affine:
                    if r & 1:
                        continue
                    c = EPL * q + 2 * t + (r >> 1)
                    al = torch.exp2(v) + 1e-10
                    beta = o[:, 4 * q + r + 1]
                    ld2 = ld2 + torch.log2(al)
                    tgt[:, c] = al * tgt[:, c] + beta if lk == 0 else (tgt[:, c] - beta) / al
                else:
                    c = EPL * q + 4 * t + r
                    tgt[:, c] = tgt[:, c] + v if lk == 2 else tgt[:, c] - v
    out = rows.clone()
    out[:, (1 - plane) * HALF:(2 - plane) * HALF] = tgt
    sign = (1.0 if lk == 0 else -1.0) if affine else 0.0
    return out, sign * LN2 * ld2


def _flow(arch, D, n_layers, seed=3, **kw):
    torch.manual_seed(seed)
    flow = tfa.Flow(getattr(tfa, arch)(D, n_layers=n_layers, **kw))
    flow.train()
    with torch.no_grad():
        flow.log_prob(torch.randn(512, D) * 1.5 + 0.3)
    flow.eval()
    return flow


def _compile(comp, D, Dp, direction):
    order = comp.layers if direction == 0 else list(comp.layers)[::-1]
    plan = flow_compile._flatten(order, "forward" if direction == 0 else "inverse")
    pos = torch.arange(D)
    if Dp != D:
        pos = torch.where(pos < D // 2, pos, pos - D // 2 + Dp // 2)
    return flow_compile._compile_lean(comp, plan, torch.device("cpu"), D, Dp, pos.clone(), pos.clone()), pos, plan


def _formats(chain):
    return {int(op[4]) if len(op) > 4 else 0 for seg in chain.segments for op in seg.ops if 12 <= op[0] <= 15}


@pytest.mark.parametrize("arch,D,n_layers,direction,kw", [
    ("RealNVP", 64, 8, 0, {}), ("RealNVP", 64, 3, 1, {}), ("NICE", 64, 4, 0, {}), ("RealNVP", 32, 2, 0, {}),
    ("RealNVP", 128, 2, 0, {}), ("RealNVP", 64, 2, 0, dict(conditioner_kwargs=dict(n_hidden=10)))])
def test_split_f16_blocks_against_fp64_composition(arch, D, n_layers, direction, kw, monkeypatch):
    """The packed split-f16 blocks, decoded as the kernel reads them, reproduce the composition's fp64 forward / inverse
    at the tolerance test_lean_chain_packer_against_fp64_emulator holds the other operand formats to."""
    set_debug(monkeypatch, lean_f16x2="1")
    flow = _flow(arch, D, n_layers, **kw)
    comp = flow.bijection.double()
    chain, pos, _ = _compile(comp, D, D, direction)
    assert chain is not None and chain.D == D and len(chain.segments) == 1
    assert _formats(chain) == {512}, "every coupling in the split-f16 format"
    x = torch.randn(64, D, dtype=torch.float64)
    with torch.no_grad():
        want, ld_want = (comp.forward if direction == 0 else comp.inverse)(x)
    rows = torch.zeros(64, D, dtype=torch.float64)
    rows[:, pos] = x
    ld = torch.zeros(64, dtype=torch.float64)
    seg = chain.segments[0]
    for op in seg.ops:
        if 12 <= op[0] <= 15:
            rows, l = decode_f16_coupling(op, seg.params, rows, D)
        else:
            assert op[0] == 16                                      # the closing TFK_OP_EW_FMA: lean_emulator's
            rows, l = run_lean([op], seg.params, rows, D)
        ld = ld + l
    got = rows[:, chain.pos]
    e_x = float((got - want).abs().max() / want.abs().max())
    e_ld = float((ld - ld_want).abs().max() / max(1.0, float(ld_want.abs().max())))
    print(f"{arch}({D}, {n_layers}) direction {direction}: x {e_x:.2e}, log-det {e_ld:.2e}")
    assert e_x < 2e-5
    assert e_ld < 2e-5


@pytest.mark.parametrize("case", ["n_hidden=11", "weight=1e5", "odd", "context"])
def test_split_f16_falls_back_to_fp32_operands(case, monkeypatch):
    """What the format cannot hold compiles to the fp32 operand format, decided on the host at pack time."""
    set_debug(monkeypatch, lean_f16x2="1")
    dev = torch.device("cpu")
    if case == "context":
        torch.manual_seed(4)
        flow = tfa.Flow(tfa.RealNVP(64, context_shape=(5,), n_layers=2))
        flow.train()
        with torch.no_grad():
            flow.log_prob(torch.randn(512, 64), context=torch.randn(512, 5))
        flow.eval()
        comp = flow.bijection.double()
        plan = flow_compile._flatten(comp.layers, "forward")
        pos = torch.arange(64)
        chain = flow_compile._compile_lean(comp, plan, dev, 64, 64, pos.clone(), pos.clone(), context=True)
    elif case == "odd":
        D, w = 63, 64
        comp = _flow("RealNVP", D, 2).bijection.double()
        plan = flow_compile._flatten(comp.layers, "forward")
        l_ = torch.arange(D)
        lay = torch.where(l_ < D // 2, l_, torch.where(l_ == D // 2, torch.full_like(l_, w - 1), w // 2 + l_ - D // 2 - 1))
        chain = flow_compile._compile_lean(comp, plan, dev, D, w, lay, lay.clone(), context=False, odd=True)
    else:
        kw = dict(conditioner_kwargs=dict(n_hidden=11)) if case == "n_hidden=11" else {}
        flow = _flow("RealNVP", 64, 2, **kw)
        if case == "weight=1e5":
            assert _formats(_compile(flow.bijection.double(), 64, 64, 0)[0]) == {512}
            lin = [m for m in flow.bijection.modules() if isinstance(m, torch.nn.Linear)][-1]       # a coupling's W2
            with torch.no_grad():
                lin.weight[3, 2] = 1e5
            flow.bijection.invalidate_native_caches()
        chain = _compile(flow.bijection.double(), 64, 64, 0)[0]
    assert chain is not None
    assert _formats(chain) == {0}, "fp32 operands"
