"""Host-side tests of training above 256 columns (torchflows_amd/train_packs.py:_WideTrainPack, csrc/tfk_wide_bwd.h): the
operand block decoded exactly as the two kernels index it, the un-permute of the tfk_rows_outer outputs, the fp64 emulator
of the whole reverse mode against torch.autograd, and which plans take the route.  No GPU needed."""
import pytest
import torch

from conftest import set_debug

CPU = torch.device("cpu")


def _flow(arch, D, n_layers=1, **kw):
    import torchflows_amd as tfa
    from torchflows_amd.bijections.finite.autoregressive import architectures as A
    torch.manual_seed(5)
    flow = tfa.Flow(getattr(A, arch)(D, n_layers=n_layers, **kw))
    flow.train()
    with torch.no_grad():
        flow.log_prob(torch.randn(64, *((D,) if isinstance(D, int) else D)) * 1.5 + 0.3)   # ActNorm's initialisation
    return flow


def _coupling(flow):
    """(layer, direction, D) of the first coupling of the flow's training plan."""
    from torchflows_amd import autograd as ag
    from torchflows_amd.bijections.base import method_direction
    b = flow.bijection
    plan = ag.training_plan(b, method_direction(b.forward))
    return next((layer, d) for layer, d, kind in plan if kind == "coupling") + (b.n_dim,)


def _pack_of(layer, D):
    from torchflows_amd import autograd as ag
    lin1, lin2 = ag._plain_mlp(layer)
    shift = layer.transformer.native_kind == "shift"
    pack = ag._WideTrainPack.get(D, lin1.out_features, CPU, shift)
    return pack, lin1, lin2, shift


@pytest.mark.parametrize("D", [264, 784])
@pytest.mark.parametrize("arch", ["RealNVP", "NICE"])
def test_forward_block_is_the_inference_packers(arch, D):
    """(a): the head of the training block is fused_wide.pack_coupling's block for the same layer with pre_s = 1,
    pre_t = 0 -- built by one gather and one multiply-add instead of the packer's index construction."""
    from torchflows_amd import autograd as ag, flow_compile, fused, fused_wide
    layer, d, _ = _coupling(_flow(arch, D))
    pack, lin1, lin2, shift = _pack_of(layer, D)
    block = pack.pack(lin1, lin2)
    hp = fused_wide.plane_width(D)
    assert pack.hp == hp and block.numel() == pack.n_bwd and pack.n_fwd == fused_wide.block_floats(hp, not shift)
    lk, plane, H, W1t, b1, W2p, b2p = flow_compile._lean_coupling(layer, d, fused_wide.layout(D, CPU), D, 2 * hp)
    want = fused_wide.pack_coupling(lk, H, hp, W1t, b1, W2p, b2p, torch.ones(hp, dtype=torch.float64),
                                    torch.zeros(hp, dtype=torch.float64))
    assert plane == 0 and pack.ops[lk][0][0] == fused.OP_AFFINE_FWD_LEAN + lk
    got = block[:pack.n_fwd]
    # the same float64 products rounded once to fp32 (b2's logit entries: (b / 2 + c0) log2 e against b (log2 e / 2) +
    # c0 log2 e, equal to an fp64 rounding): one fp32 ulp at the most
    assert float((got - want).abs().max()) <= 1.2e-7 * float(want.abs().max())
    assert torch.equal(got[:256 * pack.E + 16], want[:256 * pack.E + 16])              # A1 | b1: the very same product
    assert ag._WideTrainPack.get(D, H, CPU, shift) is pack                             # cached


@pytest.mark.parametrize("D", [264, 784])
@pytest.mark.parametrize("arch", ["RealNVP", "NICE"])
def test_transposed_operands_as_the_header_documents(arch, D):
    """(b): A2T[w][t][l][r] and A1T[w][g][l][r] hold the module's own (unscaled) weights where csrc/tfk_wide_bwd.h says;
    pad columns and unused hidden units are zero."""
    layer, d, _ = _coupling(_flow(arch, D))
    pack, lin1, lin2, shift = _pack_of(layer, D)
    block = pack.pack(lin1, lin2)
    E, half, H = pack.E, D // 2, lin1.out_features
    T2, G1, P = (E // 4 if shift else E // 2), E // 4, (1 if shift else 2)
    A2T = block[pack.n_fwd:pack.n_fwd + 4 * T2 * 256].reshape(4, T2, 64, 4)
    A1T = block[pack.n_fwd + 4 * T2 * 256:].reshape(4, G1, 64, 4)
    W1 = lin1.weight.detach()
    W2 = lin2.weight.detach().reshape(half, P, H)
    seen2 = seen1 = 0
    for w in range(4):
        for l in range(64):
            ql, i = l >> 4, l & 15
            unit = 4 * (i & 3) + (i >> 2)
            for t in range(T2):
                for r in range(4):
                    col = (4 * w + ql) * E + (4 * t + r if shift else 2 * t + (r >> 1))
                    p = 0 if shift else r & 1
                    want = float(W2[col, p, unit]) if (col < half and unit < H) else 0.0
                    assert float(A2T[w, t, l, r]) == want
                    seen2 += want != 0.0
            for g in range(G1):
                for r in range(4):
                    col = (4 * w + (i >> 2)) * E + 4 * g + (i & 3)
                    u = 4 * r + ql
                    want = float(W1[u, col]) if (col < half and u < H) else 0.0
                    assert float(A1T[w, g, l, r]) == want
                    seen1 += want != 0.0
    assert seen2 == W2.numel() and seen1 == W1.numel()                  # every weight exactly once


@pytest.mark.parametrize("D,arch,H", [(264, "RealNVP", None), (264, "NICE", None), (784, "RealNVP", 5)])
def test_rows_outer_outputs_map_back(D, arch, H):
    """(c): synthetic products A[m] * B[k] in tfk_rows_outer's accumulator order land at the right entry of
    (dW1, db1, dW2, db2); pad columns and unused hidden units (NaN here) are never mapped."""
    from wide_train_emulator import rows_outer
    kw = {} if H is None else dict(conditioner_kwargs=dict(n_hidden=H))
    layer, d, _ = _coupling(_flow(arch, D, **kw))
    pack, lin1, lin2, shift = _pack_of(layer, D)
    H, half, hp, P = lin1.out_features, D // 2, pack.hp, (1 if shift else 2)
    nan = float("nan")
    u = torch.arange(H)
    slot = 4 * (u % 4) + u // 4
    used = torch.zeros(16, dtype=torch.bool)
    used[slot] = True
    used[15] = True

    def vec(n, live):                            # distinct values where the entry is real, NaN where it is padding
        v = torch.full((n,), nan, dtype=torch.float64)
        v[live] = 1.0 + torch.arange(int(live.sum()), dtype=torch.float64) / 7.0
        return v
    a1 = vec(pack.GH, torch.arange(pack.GH) < P * half)
    a2 = vec(hp, torch.arange(hp) < half)
    a3 = vec(16, used & (torch.arange(16) != 15))
    b = vec(16, used)
    acc = torch.cat([rows_outer(a1[None], pack.GH, b[None]), rows_outer(a2[None], hp, b[None]), rows_outer(a3[None], 16, b[None])])
    assert acc.numel() == pack.n_acc
    dW1, db1, dW2, db2 = pack.unpack_grads(acc)
    assert dW1.shape == lin1.weight.shape and dW2.shape == lin2.weight.shape
    assert torch.equal(dW2, a1[:P * half, None] * b[slot][None, :])
    assert torch.equal(db2, a1[:P * half] * b[15])
    assert torch.equal(dW1, b[slot][:, None] * a2[None, :half])
    assert torch.equal(db1, a3[slot] * b[15])


CASES = [("RealNVP", 264, False, False), ("RealNVP", 264, True, True), ("NICE", 264, True, False),
         ("InverseRealNVP", 264, False, True), ("RealNVP", 784, True, True)]


@pytest.mark.parametrize("arch,D,scaled,reversed_", CASES)
def test_emulated_reverse_mode_against_autograd(arch, D, scaled, reversed_):
    """The block, decoded by the fp64 emulator of tfk_wide_coupling_train_bwd + tfk_rows_outer and un-permuted, gives the
    gradients torch.autograd derives from the module in float64 (17 rows: one tile and a ragged second one; the fixed
    elementwise scale and the reversal that ride along)."""
    from wide_train_emulator import coupling_backward
    from torchflows_amd import autograd as ag
    layer, d, _ = _coupling(_flow(arch, D))
    pack, lin1, lin2, shift = _pack_of(layer, D)
    inv = (d == ag.INVERSE) if shift else ag._affine_form_is_inverse(layer, d)
    block = pack.pack(lin1, lin2)
    torch.manual_seed(D + scaled)
    N = 17
    x = torch.randn(N, D, dtype=torch.float64)
    G = torch.randn(N, D, dtype=torch.float64)
    gld = torch.randn(N, dtype=torch.float64)
    s = (torch.rand(D, dtype=torch.float64) + 0.5) if scaled else None
    got = coupling_backward(pack, block, x, G, gld, D, shift, inv, gscale=s, g_reversed=reversed_)
    ref = layer.double()
    params = [ref.conditioner_transform.sequential[0].weight, ref.conditioner_transform.sequential[0].bias,
              ref.conditioner_transform.sequential[2].weight, ref.conditioner_transform.sequential[2].bias]
    xr = x.clone().requires_grad_(True)
    out, ld = (ref.forward if d == ag.FORWARD else ref.inverse)(xr)
    out = out.reshape(N, D)
    if scaled:
        out = out * s
    if reversed_:
        out = out.flip(1)
    want = torch.autograd.grad((G * out).sum() + (gld * ld).sum(), [xr] + params)
    layer.float()
    for name, a, b_ in zip(("g", "dW1", "db1", "dW2", "db2"), got, want):
        # the block holds fp32 roundings of the weights (and of their pre-scaled products)
        assert float((a - b_).norm() / b_.norm().clamp_min(1e-30)) < 2e-6, name


def test_aten_composite_grads_golden_wide():
    """The fixture the device route is held to (grads_flow_realnvp_1x28x28.npz, the reference's own autograd on the weights
    of flow_realnvp_1x28x28.npz) is pinned on the host too: this package's ATen composite path differentiates to it."""
    from conftest import load_golden, state_dict_of
    from test_grads_cpu import _mirror_flow, normwise
    fx, gr = load_golden("flow_realnvp_1x28x28.npz"), load_golden("grads_flow_realnvp_1x28x28.npz")
    flow = _mirror_flow("RealNVP", (1, 28, 28), 3, state_dict_of(fx, "init"))
    x = torch.tensor(fx["x"], requires_grad=True)
    loss = (flow.log_prob(x) * torch.tensor(gr["w"])).sum()
    named = [(n, p) for n, p in flow.named_parameters() if p.requires_grad]
    assert [n for n, _ in named] == list(gr["trainable"])
    grads = torch.autograd.grad(loss, [x] + [p for _, p in named], allow_unused=True)
    assert normwise(grads[0].numpy(), gr["gx64"]) < max(1e-5, 3 * normwise(gr["gx"], gr["gx64"]))
    for (name, _), g in zip(named, grads[1:]):
        if g is None:
            continue
        r32, r64 = gr["g/" + name], gr["g64/" + name]
        assert normwise(g.numpy(), r64) < max(1e-5, 3 * normwise(r32, r64)), name


def test_supported_matches_the_header():
    from torchflows_amd import native
    L = native.lib()
    for D in (264, 512, 784, 1024):
        for H in (1, 15):
            assert L.tfk_wide_coupling_train_bwd_supported(D, H) == 1, (D, H)
    for D, H in ((256, 8), (258, 8), (260, 8), (784, 16), (785, 8), (1025, 8), (1032, 8), (784, 0)):
        assert L.tfk_wide_coupling_train_bwd_supported(D, H) == 0, (D, H)
    # A1 | b1 | A2 | b2 | pre_s, pre_t | A2T | A1T at 28 columns per lane, 14 GEMM-2 tiles per wave
    assert L.tfk_wide_coupling_train_bwd_param_floats(784, 0) == (256 * 28 + 16 + 4 * 14 * 256 + 4 * 14 * 16 + 32 * 28
                                                                  + 4 * 14 * 256 + 256 * 28)
    assert L.tfk_wide_coupling_train_bwd_param_floats(258, 0) == 0


def _plan(flow):
    from torchflows_amd import autograd as ag
    from torchflows_amd.bijections.base import method_direction
    return ag.training_plan(flow.bijection, method_direction(flow.bijection.forward))


def test_which_plans_take_the_route(monkeypatch):
    """RealNVP((1, 28, 28)) and NICE(512) are fully fused at their own width; wide_train=0, D = 258, hidden width 16, a
    context and spline layers keep the layer-by-layer route."""
    import torchflows_amd as tfa
    from torchflows_amd import autograd as ag
    img = _flow("RealNVP", (1, 28, 28), 2)
    nice = _flow("NICE", 512, 2)
    for flow, D in ((img, 784), (nice, 512)):
        plan = _plan(flow)
        assert ag.fully_fused(plan, D) and ag.plan_width(plan, D) == D
        packs = ag._PlanPacks(plan, D, CPU, fold=True)
        wide = packs.fused[ag._WIDE]
        assert len(wide) == 2 and wide == packs.records and not packs.fused[ag._AFFINE] and not packs.flat_capable()
        # the ActNorm behind each coupling rides along, and the reversal between the two (none follows the last one)
        assert all(rec.ew_step is not None for rec in wide) and wide[0].rev_step is not None
    set_debug(monkeypatch, wide_train=0)
    for flow, D in ((img, 784), (nice, 512)):
        plan = _plan(flow)
        assert not ag.fully_fused(plan, D) and ag.plan_width(plan, D) == D
        assert not ag._PlanPacks(plan, D, CPU, fold=True).fused[ag._WIDE]
    set_debug(monkeypatch, wide_train=None)
    for flow, D in ((_flow("RealNVP", 258, 2), 258),
                    (_flow("RealNVP", 784, 2, conditioner_kwargs=dict(n_hidden=16)), 784),
                    (_flow("CouplingRQNSF", 264, 1), 264)):
        plan = _plan(flow)
        assert plan is not None and not ag.fully_fused(plan, D)
        assert not ag._PlanPacks(plan, D, CPU, fold=True).fused[ag._WIDE]
    torch.manual_seed(0)
    cflow = tfa.Flow(tfa.RealNVP(512, context_shape=(3,), n_layers=2))
    plan = _plan(cflow)
    assert plan is None or not ag.fully_fused(plan, 512)


def test_folded_actnorm_block_and_scale():
    """The closing TFK_OP_EW_FMA block of the ActNorm that rides along: s | t in the wide kernels' column order with
    identity padding, the constant log-det, and the D column factors of its reverse mode."""
    from torchflows_amd import autograd as ag
    flow = _flow("RealNVP", 264, 1)
    plan = _plan(flow)
    (ew, ew_d), = [(layer, d) for layer, d, kind in plan if kind == "elementwise"][-1:]
    block, gscale = ag._ew_fma_block(ew, ew_d, 264, 192)
    assert block.numel() == 4 * 192 + 4 and gscale.shape == (264,)
    x = torch.randn(3, 264, dtype=torch.float64)
    with torch.no_grad():
        want, ld = (ew.forward if ew_d == ag.FORWARD else ew.inverse)(x.float())
    s = torch.cat([block[:132], block[192:192 + 132]]).double()
    t = torch.cat([block[384:384 + 132], block[576:576 + 132]]).double()
    assert float((x * s + t - want.double()).abs().max()) < 1e-5
    assert abs(float(block[768]) - float(ld[0])) < 1e-4 * max(1.0, abs(float(ld[0])))
    assert torch.equal(block[132:192], torch.ones(60)) and torch.equal(block[384 + 132:576], torch.zeros(60))
    assert torch.equal(gscale.double(), s)
    assert ag._ew_fma_block(ew, ew_d, 264, 192)[0] is block                   # cached until the value changes
