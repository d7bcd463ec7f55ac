"""The deep sigmoidal family on the GPU: csrc/tfk_dsf.hip (forward, in-kernel bisection, reverse mode) against the
fixtures the reference produced (tests/golden/make_golden_dsf.py), then the flows, ``sample``, gradients and ``Flow.fit``.

Bars.  z, x and the log-dets against the reference's fp32 values within max(1e-5, 3 x floor), the floor being the
fixture's own fp32-vs-fp64 distance, in the measures of tests/test_gpu_flows.py::test_flow_golden_on_hip (z and x
norm-wise, log_prob and log-dets elementwise relative to max(1, |ref|)).  The reference ends its bisection on a
batch-wide ``allclose`` while the kernel runs every element to its own fp32 fixed point: both answers sit within the
fp32 noise of f around the root, which is what the floor measures.  Inverse elements whose forward ``d`` hit the clip
are excluded (the map is flat there); the fixture generator caps them at 2 % (the committed fixture has none).
Gradients: per element within 1e-4 max(1, |ref|) + 4 x the reference's own fp32-vs-fp64 distance
(tests/test_gpu_bwd.py::test_lrs_bwd_golden)."""
import copy

import numpy as np
import pytest
import torch

from conftest import load_golden, set_debug, state_dict_of
from dsf_reference import _within
from test_host_dsf import FLOWS, bar, build_flow, dsf_transformer, normwise, rel

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def native():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    from torchflows_amd import native as nat
    nat.lib()
    return nat


@pytest.fixture(scope="module")
def layer_fx():
    fx = load_golden("dsf.npz")
    return {k: fx[k] for k in fx.files}


CASES = ["C2_K4", "C2_K5", "C2_K10", "C1_K15"]


def _rows(fx, tag, tail, inverse, n_rows):
    """(rows (n, D) with the transformer's inputs at the target columns, h, tgt or None, row indices into the fixture)."""
    tgt = fx["tgt"].astype(np.int64)
    x = fx[f"{tag}_x"]
    D, T = x.shape[1], tgt.size
    avail = fx[f"{tag}_z_in"].shape[0] if inverse else x.shape[0]
    pick = np.arange(n_rows) % avail
    rows = x[pick].copy()
    vals = fx[f"{tag}_z_in"][pick] if inverse else x[pick][:, tgt]
    cols = np.arange(D - T, D) if tail else tgt
    rows[:, cols] = vals
    return rows, fx[f"{tag}_h"][pick], cols, pick


@pytest.mark.parametrize("accumulate", [False, True])
@pytest.mark.parametrize("tail", [False, True])
@pytest.mark.parametrize("inverse", [False, True])
@pytest.mark.parametrize("tag", CASES)
def test_layer_kernels_golden(native, layer_fx, tag, inverse, tail, accumulate):
    fx = layer_fx
    C, K = int(tag[1]), int(tag.split("_K")[1])
    n = 48 if inverse else 64
    rows, h, cols, pick = _rows(fx, tag, tail, inverse, n)
    want, want64 = (fx[f"{tag}_xinv"], fx[f"{tag}_xinv64"]) if inverse else (fx[f"{tag}_z"], fx[f"{tag}_z64"])
    ld, ld64 = (fx[f"{tag}_ldinv"], fx[f"{tag}_ldinv64"]) if inverse else (fx[f"{tag}_ld"], fx[f"{tag}_ld64"])
    keep = ~fx[f"{tag}_clip"] if inverse else np.ones_like(want, bool)
    assert keep.mean() >= 0.98
    x_d, h_d = torch.from_numpy(rows).cuda(), torch.from_numpy(h).cuda().contiguous()
    out = torch.full_like(x_d, float("nan"))
    ld0 = torch.randn(n, generator=torch.Generator().manual_seed(3)).cuda() if accumulate else torch.full((n,), float("nan")).cuda()
    got_ld = ld0.clone()
    tgt_d = None if tail else torch.from_numpy(cols.astype(np.int32)).cuda()
    before = native.calls
    native.dsf_coupling(x_d, h_d, out, got_ld, tgt_d, cols.size, C, K, accumulate=accumulate, inverse=inverse)
    torch.cuda.synchronize()
    assert native.calls - before == 1
    out_h = out.cpu().numpy()
    others = np.setdiff1d(np.arange(rows.shape[1]), cols)
    assert np.array_equal(out_h[:, others], rows[:, others]), "pass-through columns must be copied unchanged"
    got = out_h[:, cols]
    got_l = (got_ld - ld0).cpu().numpy() if accumulate else got_ld.cpu().numpy()
    e_v, f_v = normwise(got[keep], want[keep]), normwise(want[keep], want64[keep])
    e_l, f_l = rel(got_l, ld), rel(ld, ld64)
    print(f"{tag} {'inv' if inverse else 'fwd'} tail={tail} acc={accumulate}: value {e_v:.2e} (floor {f_v:.2e}), "
          f"log-det {e_l:.2e} (floor {f_l:.2e})")
    assert np.isfinite(out_h).all() and np.isfinite(got_l).all()
    assert e_v < bar(f_v)
    # (accumulated: the sum init + ld is rounded once more at the magnitude of the log-det: one more 1e-7 relative)
    assert e_l < bar(f_l)
    # in place gives the same bits
    x2, ld2 = x_d.clone(), ld0.clone()
    native.dsf_coupling(x2, h_d, x2, ld2, tgt_d, cols.size, C, K, accumulate=accumulate, inverse=inverse)
    assert torch.equal(x2, out) and torch.equal(ld2, got_ld)


@pytest.mark.parametrize("tag", CASES)
def test_round_trip(native, layer_fx, tag):
    """fwd(inv(z_in)) against z_in: the bar of z."""
    fx = layer_fx
    C, K = int(tag[1]), int(tag.split("_K")[1])
    rows, h, cols, _ = _rows(fx, tag, False, True, 48)
    keep = ~fx[f"{tag}_clip"]
    x_d, h_d = torch.from_numpy(rows).cuda(), torch.from_numpy(h).cuda().contiguous()
    tgt_d = torch.from_numpy(cols.astype(np.int32)).cuda()
    ld_i, ld_f = torch.empty(48).cuda(), torch.empty(48).cuda()
    mid, back = torch.empty_like(x_d), torch.empty_like(x_d)
    native.dsf_coupling(x_d, h_d, mid, ld_i, tgt_d, cols.size, C, K, inverse=True)
    native.dsf_coupling(mid, h_d, back, ld_f, tgt_d, cols.size, C, K, inverse=False)
    z_in = fx[f"{tag}_z_in"]
    e = normwise(back.cpu().numpy()[:, cols][keep], z_in[keep])
    floor = normwise(fx[f"{tag}_z"][:48][keep], fx[f"{tag}_z64"][:48][keep])
    print(f"{tag}: round trip {e:.2e} (floor of z {floor:.2e}); log-dets cancel to {float((ld_i + ld_f).abs().max()):.2e}")
    assert e < bar(floor)
    # the inverse log-det is minus the forward log-det at the returned x: the two launches evaluate the same expression
    assert float((ld_i + ld_f).abs().max()) <= 1e-5 * max(1.0, float(ld_f.abs().max()))


@pytest.mark.parametrize("n_rows", [1, 65])
@pytest.mark.parametrize("inverse", [False, True])
def test_ragged_batches(native, layer_fx, n_rows, inverse):
    fx, tag, C, K = layer_fx, "C2_K5", 2, 5
    rows, h, cols, pick = _rows(fx, tag, False, inverse, n_rows)
    want, want64 = (fx[f"{tag}_xinv"], fx[f"{tag}_xinv64"]) if inverse else (fx[f"{tag}_z"], fx[f"{tag}_z64"])
    ld, ld64 = (fx[f"{tag}_ldinv"], fx[f"{tag}_ldinv64"]) if inverse else (fx[f"{tag}_ld"], fx[f"{tag}_ld64"])
    x_d, h_d = torch.from_numpy(rows).cuda(), torch.from_numpy(h).cuda().contiguous()
    guard = torch.full((n_rows + 2, rows.shape[1]), 7.0).cuda()           # a row of canaries on either side
    out, got_ld = guard[1:-1], torch.full((n_rows + 2,), 7.0).cuda()
    native.dsf_coupling(x_d, h_d, out, got_ld[1:-1], torch.from_numpy(cols.astype(np.int32)).cuda(), cols.size, C, K,
                        inverse=inverse)
    torch.cuda.synchronize()
    assert float(guard[0].min()) == 7.0 and float(guard[-1].max()) == 7.0 and got_ld[0] == 7.0 and got_ld[-1] == 7.0
    assert normwise(out.cpu().numpy()[:, cols], want[pick]) < bar(normwise(want, want64))
    assert rel(got_ld[1:-1].cpu().numpy(), ld[pick]) < bar(rel(ld, ld64))


def test_unsupported_and_inverse_backward_are_errors(native):
    x = torch.randn(4, 6).cuda()
    h = torch.randn(4, 3, 3 * 17 * 2).cuda()
    ld = torch.empty(4).cuda()
    with pytest.raises(native.NativeError, match="hidden_dim"):
        native.dsf_coupling(x, h, torch.empty_like(x), ld, None, 3, 2, 17)
    h = torch.randn(4, 3, 24).cuda()
    with pytest.raises(native.NativeError, match="bisection"):
        native.dsf_coupling_bwd(x, h, torch.ones_like(x), torch.ones(4).cuda(), torch.empty_like(h), None, 3, 2, 4, inverse=True)


def _launches(native, flow, x, z_in, ctx):
    before = native.calls
    with torch.no_grad():
        out = flow.forward_with_log_prob(x, context=ctx), flow.bijection.inverse(z_in, context=ctx)
    return native.calls - before, out


@pytest.mark.parametrize("variant", ["fresh", "init"])
@pytest.mark.parametrize("name,arch,ctx_shape", FLOWS)
def test_flow_golden_on_hip(native, monkeypatch, name, arch, ctx_shape, variant):
    import torchflows_amd as tfa
    monkeypatch.setenv("TORCHFLOWS_AMD_FUSED", "0")
    fx = load_golden(name)
    flow = build_flow(arch, fx, ctx_shape)
    flow.load_state_dict({k: torch.from_numpy(v) for k, v in state_dict_of(fx, variant).items()}, strict=True)
    flow = flow.cuda().eval()
    ctx = torch.from_numpy(fx["context"]).cuda() if ctx_shape else None
    x, z_in = torch.from_numpy(fx["x"]).cuda(), torch.from_numpy(fx["z_in"]).cuda()
    g = lambda k: fx[f"{variant}/{k}"]
    n_launch, ((z, lp), (xr, ldr)) = _launches(native, flow, x, z_in, ctx)
    with torch.no_grad():
        lp2 = flow.log_prob(x, context=ctx)
    D = x.shape[1]
    # one transformer launch per coupling (per pass of a MADE layer's sequential map), bisection included: exactly the
    # launches of the spline / affine preset of the same shape run layer by layer
    twin_arch = {"CouplingDeepSF": "CouplingRQNSF", "MaskedAutoregressiveDeepSF": "MAF",
                 "InverseAutoregressiveDeepSF": "IAF"}[arch]
    set_debug(monkeypatch, made_fused=0)
    twin = tfa.Flow(getattr(tfa, twin_arch)(D, n_layers=2, **({"context_shape": ctx_shape} if ctx_shape else {}))).cuda().eval()
    n_twin, _ = _launches(native, twin, x, z_in, ctx)
    assert n_launch == n_twin, (n_launch, n_twin)
    e_lp, e_z = rel(lp.cpu().numpy(), g("log_prob")), normwise(z.cpu().numpy(), g("z"))
    e_x, e_ld = normwise(xr.cpu().numpy(), g("x_inv")), rel(ldr.cpu().numpy(), g("log_det_inv"))
    floors = (rel(g("log_prob"), g("log_prob64")), normwise(g("z"), g("z64")), normwise(g("x_inv"), g("x_inv64")),
              rel(g("log_det_inv"), g("log_det_inv64")))
    print(f"{name} {variant}: {n_launch} launches; log_prob {e_lp:.2e}, z {e_z:.2e}, x_inv {e_x:.2e}, log_det_inv {e_ld:.2e}; "
          "floors " + ", ".join(f"{f:.2e}" for f in floors))
    assert e_lp < bar(floors[0]) and rel(lp2.cpu().numpy(), g("log_prob")) < bar(floors[0])
    assert e_z < bar(floors[1])
    assert e_x < bar(floors[2])
    assert e_ld < bar(floors[3])
    assert torch.equal(x.cpu(), torch.from_numpy(fx["x"])) and torch.equal(z_in.cpu(), torch.from_numpy(fx["z_in"]))


def test_sample(native):
    """``sample`` returns the reference's ``base_log_prob(z) + log_det`` with the log-det of the INVERSE map, i.e.
    ``log_prob(x) - 2 log_det_forward(x)`` -- the semantics every route of this package shares with the reference
    (tests/test_gpu_wide.py::test_wide_sample_log_prob) -- so the agreement of ``log_prob(x)`` with the returned
    log-density is asserted with that term carried; the plain difference is printed beside it."""
    import torchflows_amd as tfa
    fx = load_golden("flow_cdeepsf16.npz")
    flow = tfa.Flow(tfa.CouplingDeepSF(16))
    flow.load_state_dict({k: torch.from_numpy(v) for k, v in state_dict_of(fx, "init").items()}, strict=True)
    flow = flow.cuda().eval()
    torch.manual_seed(0)
    before = native.calls
    with torch.no_grad():
        x, lp = flow.sample((257,), return_log_prob=True)
        lp_again = flow.log_prob(x)
        _, ld_fwd = flow.bijection.forward(x)
    assert native.calls - before >= 4, "the HIP kernels did not run"
    assert x.shape == (257, 16) and lp.shape == (257,)
    assert torch.isfinite(x).all() and torch.isfinite(lp).all()
    floor = max(rel(fx["init/log_prob"], fx["init/log_prob64"]), rel(fx["init/log_det_inv"], fx["init/log_det_inv64"]))
    e = rel((lp_again.double() - 2.0 * ld_fwd.double()).cpu().numpy(), lp.cpu().numpy())
    print(f"sample: log_prob(x) - 2 log_det_forward(x) vs the returned log-density {e:.2e} (bar {bar(floor):.2e}); "
          f"log_prob(x) alone {rel(lp_again.cpu().numpy(), lp.cpu().numpy()):.2e}")
    assert e < bar(floor)


def _count(monkeypatch, native, name):
    seen = {"n": 0}
    real = getattr(native, name)

    def counted(*a, **kw):
        seen["n"] += 1
        return real(*a, **kw)
    monkeypatch.setattr(native, name, counted)
    return seen


def _grads(flow, x, w):
    x = x.clone().requires_grad_(True)
    lp = flow.log_prob(x)
    named = [(n, p) for n, p in flow.named_parameters() if p.requires_grad]
    grads = torch.autograd.grad((lp * w).sum(), [x] + [p for _, p in named], allow_unused=True)
    return grads[0], {n: gr for (n, _), gr in zip(named, grads[1:])}


def test_flow_grads_golden_on_hip(native, monkeypatch):
    from test_grads_cpu import _mirror_flow
    fx, gr = load_golden("flow_cdeepsf16.npz"), load_golden("grads_flow_cdeepsf16.npz")
    flow = _mirror_flow("CouplingDeepSF", (16,), 2, state_dict_of(fx, "init")).cuda()
    bwd = _count(monkeypatch, native, "dsf_coupling_bwd")
    gx, grads = _grads(flow, torch.tensor(fx["x"]).cuda(), torch.tensor(gr["w"]).cuda())
    assert bwd["n"] == 2, "tfk_dsf_coupling_bwd did not run once per coupling"
    bad, worst = _within(gx.cpu().numpy(), gr["gx"], gr["gx64"])
    print(f"gx: max err {worst:.2e}, beyond bound {bad}")
    assert bad == 0
    for name in gr["trainable"]:
        g = grads[str(name)]
        if g is None or g.numel() == 0:
            continue
        bad, worst = _within(g.cpu().numpy(), gr["g/" + name], gr["g64/" + name])
        print(f"{name}: max err {worst:.2e}, beyond bound {bad} of {g.numel()}")
        assert torch.isfinite(g).all() and bad == 0, name


@pytest.mark.parametrize("arch,D", [("CouplingDeepSF", 16), ("MaskedAutoregressiveDeepSF", 6)])
def test_flow_grads_vs_fp64_hidden_dim_10(native, monkeypatch, arch, D):
    import torchflows_amd as tfa
    torch.manual_seed(2)
    flow = tfa.Flow(getattr(tfa, arch)(D, n_layers=2, transformer_kwargs=dict(hidden_dim=10)))
    with torch.no_grad():                                 # leave the default transformer: h of a few hundred
        for layer in flow.bijection.layers:
            if getattr(getattr(layer, "transformer", None), "native_kind", None) == "dsf":
                last = [m for m in layer.conditioner_transform.modules() if isinstance(m, torch.nn.Linear)][-1]
                last.weight.mul_(500.0)
                last.bias.mul_(500.0)
    flow.train()
    with torch.no_grad():
        flow.log_prob(torch.randn(512, D))
    flow.eval()
    g = torch.Generator().manual_seed(7)
    x, w = torch.randn(300, D, generator=g), torch.rand(300, generator=g) + 0.5
    gx64, g64 = _grads(copy.deepcopy(flow).double(), x.double(), w.double())
    gx32, g32 = _grads(copy.deepcopy(flow), x, w)
    bwd = _count(monkeypatch, native, "dsf_coupling_bwd")
    gx, grads = _grads(flow.cuda(), x.cuda(), w.cuda())
    assert bwd["n"] == 2
    bad, worst = _within(gx.cpu().numpy(), gx32.numpy(), gx64.numpy())
    assert bad == 0, (bad, worst)
    for name, gr in grads.items():
        if gr is None or gr.numel() == 0:
            continue
        bad, worst = _within(gr.cpu().numpy(), g32[name].numpy(), g64[name].numpy())
        print(f"{arch} {name}: max err {worst:.2e}, beyond bound {bad} of {gr.numel()}")
        assert bad == 0, name


@pytest.mark.parametrize("tag", CASES)
def test_layer_bwd_vs_fp64_autograd(native, layer_fx, tag):
    """tfk_dsf_coupling_bwd on the stress parameters of dsf.npz against autograd through the ATen transformer."""
    fx = layer_fx
    rows, h, cols, _ = _rows(fx, tag, False, False, 64)
    tr, C, K = dsf_transformer(tag, cols.size)
    gen = torch.Generator().manual_seed(5)
    gz, gld = torch.randn(64, cols.size, generator=gen), torch.randn(64, generator=gen)
    ref = {}
    for dt in (torch.float32, torch.float64):
        xt = torch.from_numpy(rows[:, cols]).to(dt).requires_grad_(True)
        ht = torch.from_numpy(h).to(dt).requires_grad_(True)
        z, ld = tr.forward(xt, ht)
        ref[dt] = [t.numpy() for t in torch.autograd.grad((z * gz.to(dt)).sum() + (ld * gld.to(dt)).sum(), (xt, ht))]
    g = torch.full(rows.shape, 0.25)
    g[:, cols] = gz
    g_d, gh = g.cuda(), torch.full(h.shape, float("nan")).cuda()
    native.dsf_coupling_bwd(torch.from_numpy(rows).cuda(), torch.from_numpy(h).cuda().contiguous(), g_d, gld.cuda(), gh,
                            torch.from_numpy(cols.astype(np.int32)).cuda(), cols.size, C, K)
    g_h = g_d.cpu().numpy()
    others = np.setdiff1d(np.arange(rows.shape[1]), cols)
    assert np.all(g_h[:, others] == 0.25), "only the target columns are rewritten"
    for mine, key, (r32, r64) in ((g_h[:, cols], "gx", (ref[torch.float32][0], ref[torch.float64][0])),
                                  (gh.cpu().numpy(), "gh", (ref[torch.float32][1], ref[torch.float64][1]))):
        bad, worst = _within(mine, r32, r64)
        print(f"{tag} {key}: max err {worst:.2e}, beyond bound {bad} of {mine.size}")
        assert np.isfinite(mine).all() and bad == 0


def test_fit_lowers_the_validation_loss(native, monkeypatch):
    import torchflows_amd as tfa
    torch.manual_seed(0)
    base = torch.randn(1024 + 256, 4)
    data = torch.cat([base * 0.5 + 1.0, base * 1.5 + 0.3 * torch.randn(1024 + 256, 4)], dim=1)      # correlated halves
    x, x_val = data[:1024], data[1024:]
    flow = tfa.Flow(tfa.CouplingDeepSF(8, n_layers=2)).cuda()
    flow.train()
    with torch.no_grad():
        flow.log_prob(x.cuda())                           # ActNorm data-dependent init
    flow.eval()
    with torch.no_grad():
        before = float(-flow.log_prob(x_val.cuda()).mean())
    bwd = _count(monkeypatch, native, "dsf_coupling_bwd")
    flow.fit(x, n_epochs=30, lr=0.01, x_val=x_val, shuffle=False)
    assert bwd["n"] >= 2 * 30, "the fit did not train on tfk_dsf_coupling_bwd"
    assert not flow.training
    with torch.no_grad():
        after = float(-flow.log_prob(x_val.cuda()).mean())
    print(f"CouplingDeepSF(8) fit: validation loss {before:.4f} -> {after:.4f}")
    assert np.isfinite(after) and after < before
