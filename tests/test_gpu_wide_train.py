"""Training above 256 columns on the device (csrc/tfk_wide_bwd.h, torchflows_amd/train_packs.py: _WideTrainPack,
torchflows_amd/autograd.py: the wide route of ChainFunction): the reverse-mode kernel through the C-ABI against float64,
whole-flow gradients against fp64 autograd and the reference's fixture, run-to-run determinism, a captured ``Flow.fit`` in a child process, and the plans
that keep the layer-by-layer route.

Sizes: the smallest at which the kernel can go wrong -- D = 264 (planes of 192, 60 pad columns each, 12 columns per lane),
512 (no padding), 784 (padding inside the last wave, 28 per lane), 1024 (the largest, 32 per lane)."""
import copy
import json
import os
import subprocess
import sys
import warnings

import numpy as np
import pytest
import torch

from conftest import load_golden, state_dict_of, set_debug
from test_grads_cpu import _mirror_flow, normwise

pytestmark = pytest.mark.gpu

AFF_C0 = -1.000000082790371e-10          # float32(log(1 - 1e-10)), affine.py:19-23


@pytest.fixture(scope="module")
def native():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    from torchflows_amd import native as nat
    nat.lib()
    return nat


def nrm(a, b):
    """Norm-wise distance of a tensor from its float64 truth."""
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).norm() / b.norm().clamp_min(1e-30))


def _coupling_truth(lin1, lin2, x, G, gld, shift, inv, s, rev):
    """float64 restatement of one HalfSplit coupling + fixed column scale + reversal, differentiated by torch.autograd."""
    N, D = x.shape
    half = D // 2
    W1, b1, W2, b2 = (t.detach().double().cpu().requires_grad_(True)
                      for t in (lin1.weight, lin1.bias, lin2.weight, lin2.bias))
    xr = x.double().cpu().requires_grad_(True)
    xa, xb = xr[:, :half], xr[:, half:]
    h = torch.tanh(xa @ W1.t() + b1) @ W2.t() + b2
    if shift:
        out_b, ld = (xb - h if inv else xb + h), torch.zeros(N, dtype=torch.float64)
    else:
        u, beta = h.view(N, half, 2).unbind(-1)
        alpha = torch.exp(u / 2 + AFF_C0) + 1e-10
        if inv:
            out_b, ld = (xb - beta) / alpha, -torch.log(alpha).sum(1)
        else:
            out_b, ld = alpha * xb + beta, torch.log(alpha).sum(1)
    out = torch.cat([xa, out_b], dim=1)
    if s is not None:
        out = out * s.double().cpu()
    if rev:
        out = out.flip(1)
    loss = (G.double().cpu() * out).sum() + (gld.double().cpu() * ld).sum()
    return torch.autograd.grad(loss, [xr, W1, b1, W2, b2], allow_unused=True)


def _run_kernel(native, pack, lin1, lin2, x, G, gld, shift, inv, s, rev):
    """The launches ChainFunction.backward issues for one wide coupling -> (g, dW1, db1, dW2, db2)."""
    N = x.shape[0]
    block = pack.pack(lin1, lin2)
    g = G.clone()
    gh, gpre, hid = pack.records(N)
    native.wide_coupling_train_bwd(x, g, gld, block, gh, gpre, hid, shift=shift, inverse_form=inv, gscale=s, g_reversed=rev)
    acc = torch.empty(pack.n_acc, device=x.device)
    lo2, lo3 = pack.GH * 16, (pack.GH + pack.hp) * 16
    native.rows_outer(gh, pack.GH, hid, acc[:lo2])
    native.rows_outer(x, pack.hp, gpre, acc[lo2:lo3])
    native.rows_outer(gpre, 16, hid, acc[lo3:])
    return (g,) + pack.unpack_grads(acc)


def _layer(D, H, shift, seed):
    """Linear-Tanh-Linear weights of realistic scale (pre-activations of order one, logits of order 0.5)."""
    half, P = D // 2, (1 if shift else 2)
    gen = torch.Generator().manual_seed(seed)
    lin1, lin2 = torch.nn.Linear(half, H), torch.nn.Linear(H, P * half)
    with torch.no_grad():
        lin1.weight.copy_(torch.randn(H, half, generator=gen) / half ** 0.5)
        lin1.bias.copy_(0.2 * torch.randn(H, generator=gen))
        lin2.weight.copy_(0.5 * torch.randn(P * half, H, generator=gen) / H ** 0.5)
        lin2.bias.copy_(0.2 * torch.randn(P * half, generator=gen))
    return lin1.cuda(), lin2.cuda()


# fp32 unit roundoff 6e-8 through chains of at most ~130 dependent roundings (GEMM 1 over 128 k-steps per wave, sums over
# <= 53 rows) and 1-ulp exp2 / rcp: the project's fp32 bar of 1e-5 norm-wise leaves a factor ten on the worst chain
KERNEL_BAR = 1e-5


@pytest.mark.parametrize("riders", [False, True], ids=["plain", "gscale+reversed"])
@pytest.mark.parametrize("kind", ["affine", "inverse_affine", "shift", "shift_inverse"])
@pytest.mark.parametrize("D,H", [(264, 15), (512, 5), (784, 14), (1024, 1)])
def test_kernel_against_float64(native, D, H, kind, riders):
    """tfk_wide_coupling_train_bwd + the three tfk_rows_outer products, un-permuted, against float64 autograd of the same
    coupling: N = 1 and 17 (partial tiles), 53 (N % 4 != 0 in the row contraction; four tiles)."""
    from torchflows_amd import autograd as ag
    shift, inv = kind.startswith("shift"), kind.endswith("inverse") or kind == "inverse_affine"
    lin1, lin2 = _layer(D, H, shift, seed=D + H)
    pack = ag._WideTrainPack.get(D, H, torch.device("cuda", torch.cuda.current_device()), shift)
    gen = torch.Generator().manual_seed(7 * D + len(kind))
    for N in (1, 17, 53):
        x = torch.randn(N, D, generator=gen).cuda()
        G = torch.randn(N, D, generator=gen).cuda()
        gld = torch.randn(N, generator=gen).cuda()
        s = (torch.rand(D, generator=gen) + 0.5).cuda() if riders else None
        got = _run_kernel(native, pack, lin1, lin2, x, G, gld, shift, inv, s, riders)
        want = _coupling_truth(lin1, lin2, x, G, gld, shift, inv, s, riders)
        errs = {n: nrm(a, b) for n, a, b in zip(("g", "dW1", "db1", "dW2", "db2"), got, want)}
        print(f"D={D} H={H} {kind} riders={riders} N={N}: " + " ".join(f"{k} {v:.1e}" for k, v in errs.items()))
        assert max(errs.values()) < KERNEL_BAR, (N, errs)


def test_kernel_more_tiles_than_workgroups(native):
    """D = 264 on more tiles than the launch's grid cap (tfk_wide_coupling_train_bwd_grid_cap): the persistent tile loop
    and the alternating LDS buffer sets run more than once per workgroup; the last tile is ragged."""
    from torchflows_amd import autograd as ag
    D, H = 264, 12
    cap = int(native.lib().tfk_wide_coupling_train_bwd_grid_cap(D, 0))
    assert 1 <= cap <= 256 * 8 * 4
    N = 16 * cap + 16 * 3 + 5                           # just above: four workgroups take a second tile, the last one ragged
    lin1, lin2 = _layer(D, H, False, seed=1)
    pack = ag._WideTrainPack.get(D, H, torch.device("cuda", torch.cuda.current_device()), False)
    gen = torch.Generator().manual_seed(2)
    x = torch.randn(N, D, generator=gen).cuda()
    G = torch.randn(N, D, generator=gen).cuda()
    gld = torch.randn(N, generator=gen).cuda()
    s = (torch.rand(D, generator=gen) + 0.5).cuda()
    got = _run_kernel(native, pack, lin1, lin2, x, G, gld, False, True, s, True)
    want = _coupling_truth(lin1, lin2, x, G, gld, False, True, s, True)
    errs = {n: nrm(a, b) for n, a, b in zip(("g", "dW1", "db1", "dW2", "db2"), got, want)}
    print(f"cap {cap} workgroups, N = {N}: " + " ".join(f"{k} {v:.1e}" for k, v in errs.items()))
    # (the weight gradients are fp32 sums over N rows now: tfk_rows_outer's partial blocks keep the chains short -- about
    # N / (4 * 4 * 2 * 256) ~ 8 MFMA steps per wave at cap = 4096, then 512 blocks added as a tree --, so the same bar holds)
    assert max(errs.values()) < KERNEL_BAR, errs


def _seeded(arch, D, n_layers=2, **kw):
    import torchflows_amd as tfa
    from torchflows_amd.bijections.finite.autoregressive import architectures as A
    torch.manual_seed(3)
    flow = tfa.Flow(getattr(A, arch)(D, n_layers=n_layers, **kw))
    flow.train()
    with torch.no_grad():
        flow.log_prob(torch.randn(512, D) * 1.2 + 0.1)      # ActNorm's data-dependent initialisation (host)
    return flow.eval()


def hip_grads(flow, x, w):
    x = x.clone().requires_grad_(True)
    lp = flow.log_prob(x)
    named = [(n, p) for n, p in flow.named_parameters() if p.requires_grad]
    grads = torch.autograd.grad((lp * w).sum(), [x] + [p for _, p in named], allow_unused=True)
    return lp, grads[0], {n: g for (n, _), g in zip(named, grads[1:])}


def graph_nodes(t, depth=6):
    seen, frontier = set(), [t.grad_fn]
    for _ in range(depth):
        nxt = []
        for fn in frontier:
            if fn is None:
                continue
            seen.add(type(fn).__name__)
            nxt.extend(f for f, _ in fn.next_functions)
        frontier = nxt
    return seen


_TRUTH = {}


def _case(arch, D):
    """(flow on the host, x, w, fp64 truth) -- computed once, shared, left unchanged."""
    key = (arch, D)
    if key not in _TRUTH:
        flow = _seeded(arch, D)
        gen = torch.Generator().manual_seed(D)
        x = torch.randn(48, D, generator=gen) * 1.2 + 0.1
        w = torch.rand(48, generator=gen) + 0.5
        lp64, gx64, g64 = hip_grads(copy.deepcopy(flow).double(), x.double(), w.double())
        _TRUTH[key] = (flow, x, w, lp64.detach(), gx64, g64)
    return _TRUTH[key]


# libtfk calls of one log_prob + backward of the two-coupling presets on the wide route, as counted on the device: per
# coupling 1 forward program + 1 reverse-mode launch + 3 products (10); the leading ElementwiseAffine and reversal, the
# closing ElementwiseAffine + ActNorm and the base density, forward and backward (10).  (The issue's ceiling: 2 * 5 + 12.)
CALLS_TWO_COUPLINGS = 20


@pytest.mark.parametrize("arch,D", [("RealNVP", 264), ("RealNVP", 784), ("RealNVP", 1024), ("NICE", 512)])
def test_whole_flow_gradients(native, monkeypatch, arch, D):
    """sum(w log_prob) gradients of a two-coupling preset, N = 48, against fp64 autograd of a host copy.  Bar per tensor,
    norm-wise: max(1e-5, 3 d0) with d0 the distance of the layer-by-layer route (wide_train=0: the route these sizes
    trained on before) from the same truth, run here on the same device."""
    from torchflows_amd import autograd as ag
    from torchflows_amd.bijections.base import method_direction
    host, x, w, lp64, gx64, g64 = _case(arch, D)
    flow = copy.deepcopy(host).cuda()
    set_debug(monkeypatch, wide_train="0")
    plan = ag.training_plan(flow.bijection, method_direction(flow.bijection.forward))
    assert not ag.fully_fused(plan, D)
    _, gx0, g0 = hip_grads(flow, x.cuda(), w.cuda())
    set_debug(monkeypatch, wide_train=None)
    plan = ag.training_plan(flow.bijection, method_direction(flow.bijection.forward))
    assert ag.fully_fused(plan, D) and ag.plan_width(plan, D) == D
    hip_grads(flow, x.cuda(), w.cuda())                      # (packs, record buffers and workspaces exist from here on)
    before = native.calls
    lp, gx, g = hip_grads(flow, x.cuda(), w.cuda())
    calls = native.calls - before
    assert "ChainFunctionBackward" in graph_nodes(lp)
    print(f"{arch}({D}): {calls} libtfk calls")
    assert calls <= CALLS_TWO_COUPLINGS, calls
    e_lp = float((lp.detach().double().cpu() - lp64).abs().max() / max(1.0, float(lp64.abs().max())))
    assert e_lp < 1e-5, e_lp
    e, d0 = normwise(gx.cpu().numpy(), gx64.numpy()), normwise(gx0.cpu().numpy(), gx64.numpy())
    print(f"{arch}({D}): log_prob {e_lp:.1e}, gx {e:.1e} (layer-by-layer {d0:.1e})")
    assert e < max(1e-5, 3 * d0), (e, d0)
    for name, truth in g64.items():
        if truth is None or truth.numel() == 0:
            continue
        e, d0 = normwise(g[name].cpu().numpy(), truth.numpy()), normwise(g0[name].cpu().numpy(), truth.numpy())
        print(f"  {name}: {e:.1e} (layer-by-layer {d0:.1e})")
        assert e < max(1e-5, 3 * d0), (name, e, d0)


def test_gradients_are_reproducible(native):
    """Two backward passes at D = 784 give bit-identical gradients (partials added in a fixed order everywhere)."""
    host, x, w, *_ = _case("RealNVP", 784)
    flow = copy.deepcopy(host).cuda()
    runs = []
    for _ in range(2):
        _, gx, g = hip_grads(flow, x.cuda(), w.cuda())
        runs.append([gx] + [t for t in g.values() if t is not None])
    assert len(runs[0]) > 8
    for a, b in zip(*runs):
        assert torch.equal(a, b)


def test_flow_grads_golden_wide(native):
    """RealNVP((1, 28, 28)), three couplings, on the weights of tests/golden/flow_realnvp_1x28x28.npz: the route against
    the reference's own autograd (grads_flow_realnvp_1x28x28.npz), held to max(1e-5, 3 x the reference's fp32-vs-fp64
    floor) per tensor as test_flow_grads_golden_on_hip holds the narrower flows."""
    fx, gr = load_golden("flow_realnvp_1x28x28.npz"), load_golden("grads_flow_realnvp_1x28x28.npz")
    flow = _mirror_flow("RealNVP", (1, 28, 28), 3, state_dict_of(fx, "init")).cuda()
    before = native.calls
    lp, gx, grads = hip_grads(flow, torch.tensor(fx["x"]).cuda(), torch.tensor(gr["w"]).cuda())
    assert native.calls - before >= 3 * 5 and "ChainFunctionBackward" in graph_nodes(lp)
    e, floor = normwise(gx.cpu().numpy(), gr["gx64"]), normwise(gr["gx"], gr["gx64"])
    print(f"gx {e:.2e} (floor {floor:.2e})")
    assert e < max(1e-5, 3 * floor)
    worst = 0.0
    for name in gr["trainable"]:
        g = grads[str(name)]
        if g is None or g.numel() == 0:
            continue
        r32, r64 = gr["g/" + name], gr["g64/" + name]
        e, floor = normwise(g.cpu().numpy(), r64), normwise(r32, r64)
        worst = max(worst, e)
        assert e < max(1e-5, 3 * floor), (name, e, floor)
    print(f"worst parameter gradient {worst:.2e}")


def _worker(*args):
    worker = os.path.join(os.path.dirname(os.path.abspath(__file__)), "wide_fit_worker.py")
    proc = subprocess.run([sys.executable, worker, *args], capture_output=True, text=True, timeout=600)
    assert proc.returncode == 0, proc.stderr[-2000:]
    return json.loads(proc.stdout.strip().splitlines()[-1])


def test_fit_is_captured_in_a_subprocess(native):
    """Flow.fit of RealNVP((1, 28, 28), 2 layers) on 2 048 synthetic images, batch 256, 3 epochs: with TORCHFLOWS_AMD_GRAPH=1
    the step is captured once and replayed, and ends where the eager fit ends; with wide_train=0 nothing is captured.  In
    child processes: an invalidated capture takes the process down on this stack instead of raising."""
    out = _worker("1")
    print(out)
    assert out["graph_stats"]["graph_captures"] == 1 and out["graph_stats"]["graph_replays"] > 0
    assert {k: out["graph_stats"][k] for k in ("eager_steps", "graph_replays")} == {"eager_steps": 2, "graph_replays": 22}
    assert out["eager_stats"]["graph_replays"] == 0 and out["eager_stats"]["eager_steps"] == 24
    assert out["after_graph"] > out["before"] and out["after_eager"] > out["before"]
    assert abs(out["after_graph"] - out["after_eager"]) < 1e-3 * max(1.0, abs(out["after_eager"]))
    old = _worker("0")
    print(old)
    assert old["graph_stats"]["graph_replays"] == 0 and old["graph_stats"]["graph_captures"] == 0


@pytest.mark.parametrize("case", ["D258", "hidden16", "context"])
def test_declined_plans_train_as_before(native, monkeypatch, case):
    """D % 8 != 0, hidden width 16 and a conditional flow keep the layer-by-layer route: gradients bit-identical between
    wide_train=1 and wide_train=0, the plan not fully fused, no warning."""
    import torchflows_amd as tfa
    from torchflows_amd import autograd as ag
    from torchflows_amd.bijections.base import method_direction
    torch.manual_seed(8)
    ctx = None
    if case == "D258":
        flow, D = _seeded("RealNVP", 258), 258
    elif case == "hidden16":
        flow, D = _seeded("RealNVP", 784, conditioner_kwargs=dict(n_hidden=16)), 784
    else:
        D = 512
        flow = tfa.Flow(tfa.RealNVP(D, context_shape=(3,), n_layers=2)).eval()
        ctx = torch.randn(48, 3).cuda()
    flow = flow.cuda()
    x = torch.randn(48, D).cuda()
    grads, said = {}, {}
    for mode in ("1", "0"):
        set_debug(monkeypatch, wide_train=mode)
        plan = ag.training_plan(flow.bijection, method_direction(flow.bijection.forward))
        assert plan is None or not ag.fully_fused(plan, D)
        flow.zero_grad(set_to_none=True)
        flow.bijection.__dict__.pop("_tfk_declined_warned", None)
        with warnings.catch_warnings(record=True) as seen:
            warnings.simplefilter("always")
            loss = -(flow.log_prob(x) if ctx is None else flow.log_prob(x, context=ctx)).mean()
            loss.backward()
        said[mode] = sorted(str(w_.message) for w_ in seen)
        grads[mode] = [None if p.grad is None else p.grad.detach().clone() for p in flow.parameters()]
    assert said["1"] == said["0"]                         # no new warning
    assert any(g is not None and bool(g.abs().sum() > 0) for g in grads["1"])
    for a, b in zip(grads["1"], grads["0"]):
        assert (a is None) == (b is None)
        if a is not None:
            assert torch.equal(a, b)
