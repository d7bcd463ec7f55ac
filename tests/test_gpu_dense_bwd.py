"""Reverse mode of the dense sigmoidal family on the GPU: ``native.dense_coupling_bwd`` (csrc/tfk_dense_dsf.hip) against
``torch.autograd.grad`` of this package's ATen transformer in float64 on the CPU, then the four fixture flows and ``Flow.fit``
on the training chain (torchflows_amd/autograd.py).

Bars: test_host_dsf.bar of the floor, the distance of the fp32 ATen autograd from the float64 one on the same inputs; vector
gradients norm-wise.  An element whose float64 d lies within fp32 rounding of a clip bound (3e-7 of 1 - 1e-6, 1e-5 relative
of 1e-6) may fall on either side of it in fp32: such elements, at most 2 %, are left out of dx and dpred."""
import copy
import warnings

import pytest
import torch

from conftest import load_golden, set_debug
from test_gpu_dense import transformer
from test_host_dense import FLOWS, build_flow
from test_host_dsf import bar, normwise

pytestmark = pytest.mark.gpu

SIZES = [(1, 0, 1), (2, 0, 2), (4, 1, 2), (4, 2, 2), (8, 0, 1), (8, 2, 1)]            # (hidden size, dense layers, components)
CASES = [(H, L, C, N, T, D, "mixed") for H, L, C in SIZES for N, T, D in ((1, 1, 2), (37, 3, 7))] + [
    (2, 0, 2, 30000, 3, 7, "mixed"),         # 353 tiles of 85 rows on at most 256 workgroups: every slice, several tiles each
    (4, 1, 2, 37, 3, 7, "constant"), (4, 1, 2, 37, 3, 7, "gld0"), (4, 1, 2, 37, 3, 7, "g0")]


def aten_grads(tr, x_t, h, g_t, gld, dtype):
    """dL/dx (N, T) and dL/dh (N, T, P) of L = sum(g z) + sum(gld log-det) by autograd."""
    x_t, h = x_t.to(dtype).requires_grad_(True), h.to(dtype).requires_grad_(True)
    z, ld = tr.forward(x_t, h)
    return torch.autograd.grad((z * g_t.to(dtype)).sum() + (ld * gld.to(dtype)).sum(), [x_t, h])


@pytest.mark.parametrize("H,L,C,N,T,D,variant", CASES)
def test_kernel_against_float64(monkeypatch, H, L, C, N, T, D, variant):
    from torchflows_amd import native
    gen = torch.Generator().manual_seed(1000 * H + 100 * L + 10 * C + T)
    tr = transformer(H, L, C, T)
    P = tr.n_parameters_per_element
    tgt = torch.randperm(D, generator=gen)[:T]                       # scattered target columns
    constant = torch.zeros(T * P, dtype=torch.bool)
    constant[torch.randperm(T * P, generator=gen)[:int(T * P * (1.0 if variant == "constant" else 0.8))]] = True
    h = torch.randn(N, T * P, generator=gen) * 2000.0                # (x 2000: some d reach the clip)
    h[:, constant] = h[0, constant]
    x = torch.rand(N, D, generator=gen) * 8 - 4
    g = torch.randn(N, D, generator=gen) * (0.0 if variant == "g0" else 1.0)
    gld = torch.randn(N, generator=gen) * (0.0 if variant == "gld0" else 1.0)
    clipped, clip = [], torch.clip                                   # what enters the clip of d, in float64
    monkeypatch.setattr(torch, "clip", lambda v, lo, hi: (clipped.append(v.detach()), clip(v, lo, hi))[1])
    dx64, dh64 = aten_grads(tr, x[:, tgt], h.view(N, T, P), g[:, tgt], gld, torch.float64)
    monkeypatch.undo()
    dx32, dh32 = aten_grads(tr, x[:, tgt], h.view(N, T, P), g[:, tgt], gld, torch.float32)
    edge = torch.zeros(N, T, dtype=torch.bool)
    for d in clipped:
        edge |= (((d - (1 - 1e-6)).abs() < 3e-7) | ((d - 1e-6).abs() < 1e-11)).reshape(N, T, -1).any(-1)
    assert edge.float().mean() <= 0.02
    keep = (~edge).double()
    col = torch.where(constant, -1, torch.cumsum(~constant, 0) - 1)
    stride = int((~constant).sum())
    desc = native.dense_descriptor(tgt.cuda(), stride, col.cuda(), torch.where(constant, h[0], 0.0).cuda())
    pred = h[:, ~constant].contiguous().cuda() if stride else None
    inputs = [t.clone() for t in (x.cuda(), desc)] + ([pred.clone()] if stride else [])
    rows, again, before = g.cuda(), g.cuda(), native.calls
    dpred, dbase = native.dense_coupling_bwd(x.cuda(), pred, rows, gld.cuda(), None, desc, T, C, L, H)
    assert native.calls - before == 1
    dbase2 = native.dense_coupling_bwd(x.cuda(), pred, again, gld.cuda(), None, desc, T, C, L, H)[1]
    assert torch.equal(dbase, dbase2) and torch.equal(rows, again), "two calls must give the same bits"
    assert all(torch.equal(a, b) for a, b in zip(inputs, [x.cuda(), desc] + ([pred] if stride else []))), "inputs changed"
    others = [c for c in range(D) if c not in tgt.tolist()]
    assert torch.equal(rows.cpu()[:, others], g[:, others]), "pass-through columns of g"

    keep_p = keep[:, :, None].expand(N, T, P).reshape(N, T * P)
    def parts(dx, dh):      # dx | the batch sum onto (T P), zero where predicted | the predicted columns; clip-bound elements zeroed
        dh = dh.double().reshape(N, T * P)
        return [dx.double() * keep, torch.where(constant, dh.sum(0), 0.0)] + ([(dh * keep_p)[:, ~constant]] if stride else [])
    want = parts(dx64, dh64)
    floor = [normwise(a, b) for a, b in zip(parts(dx32, dh32), want)]
    got = [rows.cpu()[:, tgt].double() * keep, dbase.cpu()] + ([dpred.cpu().double() * keep_p[:, ~constant]] if stride else [])
    assert stride or dpred is None
    errs = [normwise(a, b) for a, b in zip(got, want)]
    print(f"H{H} L{L} C{C} N{N} T{T} {variant}: on a clip bound {float(edge.float().mean()):.3%}; dx, dbase, dpred "
          + ", ".join(f"{e:.2e} (floor {f:.2e}, bar {bar(f):.2e})" for e, f in zip(errs, floor)))
    assert all(e < bar(f) for e, f in zip(errs, floor))


def grads_of(flow, x, loss):         # dL/dx and dL/dparameter by name, of loss(flow, x)
    x = x.clone().requires_grad_(True)
    flow.zero_grad()
    loss(flow, x).backward()
    return {"x": x.grad.cpu(), **{n: p.grad.cpu() for n, p in flow.named_parameters() if p.grad is not None}}


def groups(gr, like):
    """x | the learned constants | the conditioners' weights, each as one vector (absent gradients: zeros)."""
    cat = lambda names: torch.cat([torch.zeros(0).double()]          # (a MADE has no learned constants)
                                  + [gr.get(n, torch.zeros_like(like[n])).reshape(-1).double() for n in names])
    return [gr["x"].double(), cat([n for n in like if n.endswith("global_theta_flat")]),
            cat([n for n in like if n != "x" and not n.endswith("global_theta_flat")])]


@pytest.mark.parametrize("name,arch", FLOWS)
def test_flow_gradients(monkeypatch, name, arch):
    from torchflows_amd import autograd, native
    from torchflows_amd.fused import NativeRouteWarning
    fx = load_golden(name)
    flow, x = build_flow(arch, fx), torch.from_numpy(fx["x"])
    # the direction with the parallel pass: log_prob, but sampling for the inverse-autoregressive twin
    inverse_ar = arch.startswith("InverseAutoregressive")
    loss = lambda f, v: f.log_prob(v).mean()
    if inverse_ar:
        loss = lambda f, v: (lambda out: (out[0].square().sum(-1) + out[1]).mean())(f.bijection.inverse(v))
    want = grads_of(copy.deepcopy(flow).double(), x.double(), loss)
    floor = [normwise(a, b) for a, b in zip(groups(grads_of(flow, x, loss), want), groups(want, want))]
    flow = flow.cuda()
    plans = [autograd.training_plan(flow.bijection, d) is not None for d in (autograd.FORWARD, autograd.INVERSE)]
    assert plans == ([False, True] if inverse_ar else [True, False])    # (the bisection / the sequential map: declined)
    n, real = [0], native.dense_coupling_bwd
    monkeypatch.setattr(native, "dense_coupling_bwd", lambda *a, **k: (n.__setitem__(0, n[0] + 1), real(*a, **k))[1])
    with warnings.catch_warnings():
        warnings.simplefilter("error", NativeRouteWarning)
        before = native.calls
        got = grads_of(flow, x.cuda(), loss)
    assert n[0] == 2 and native.calls - before >= 4, "two dense layers: a forward and a reverse launch each"
    set_debug(monkeypatch, dense_train="0")
    assert autograd.training_plan(flow.bijection, autograd.INVERSE if inverse_ar else autograd.FORWARD) is None
    aten = grads_of(flow, x.cuda(), loss)
    assert n[0] == 2
    for label, gr in (("kernel", got), ("dense_train=0", aten)):
        errs = [normwise(a, b) for a, b in zip(groups(gr, want), groups(want, want))]
        print(f"{name} {label}: x, constants, weights " + ", ".join(f"{e:.2e} (floor {f:.2e}, bar {bar(f):.2e})"
                                                                   for e, f in zip(errs, floor)))
        assert all(e < bar(f) for e, f in zip(errs, floor))


def test_fit_moves_constants_and_weights():
    import torchflows_amd as tfa
    torch.manual_seed(0)
    flow = tfa.Flow(tfa.CouplingDenseSF(6)).cuda()
    x = (torch.randn(256, 6, generator=torch.Generator().manual_seed(1)) * 2.0 + 1.0).cuda()
    start = {n: p.detach().clone() for n, p in flow.named_parameters()}
    with torch.no_grad():
        before = float(-flow.log_prob(x).mean())
    flow.fit(x, n_epochs=3, lr=0.01, batch_size=256, shuffle=False)
    with torch.no_grad():
        after = float(-flow.log_prob(x).mean())
    print(f"negative log-likelihood {before:.4f} -> {after:.4f}")
    assert abs(after) < float("inf") and after < before
    moved = {n for n, p in flow.named_parameters() if not torch.equal(p.detach(), start[n])}
    assert any(n.endswith("global_theta_flat") for n in moved) and any(n.endswith("weight") for n in moved)
