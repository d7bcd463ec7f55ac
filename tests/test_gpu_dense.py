"""The dense sigmoidal family on the GPU: csrc/tfk_dense_dsf.hip through ``native.dense_coupling`` against this package's
ATen transformer evaluated in float64 on the CPU, then the four fixture flows (tests/golden/make_golden_dense.py).

Bars: max(1e-5, 3 x floor), values norm-wise, log-dets elementwise relative to max(1, |ref|).  For the kernel cases the
floor is the distance of the fp32 ATen path from float64 on the same inputs; for the flows the fixture's own.

The inverse log-det is held against minus the float64 forward log-det at the returned x.  Its floor is the larger of two
distances of the fp32 ATen path from float64: its forward log-det at that same x, and its own inverse log-det against the
float64 forward log-det at ITS returned x.  The second matters with two components: the inverse log-det is summed at each
component's own root, not at the image of the final x, and where the map is nearly flat the two differ by the inner
root's error (on the host the ATen path misses by 1.06 and 4.5e-2 at (H, L, C) = (4, 2, 2), parameters x 2 000)."""
import numpy as np
import pytest
import torch

from conftest import load_golden, set_debug
from test_host_dense import FLOWS, build_flow
from test_host_dsf import bar, normwise, rel

pytestmark = pytest.mark.gpu

SIZES = [(1, 0, 1), (3, 1, 1), (8, 1, 1), (8, 2, 1), (8, 1, 2), (4, 2, 2)]            # (hidden size, dense layers, components)
ROWS = [                                    # (T, N, tail, accumulate, global share, parameter scale)
    (1, 37, True, False, 0.0, 2000.0),
    (5, 37, False, True, 0.8, 2000.0),
    (70, 37, True, False, 0.8, 1.0),
    (70, 1, False, True, 1.0, 2000.0),
    (5, 1, True, False, 1.0, 1.0),
]


@pytest.fixture(scope="module")
def native():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    from torchflows_amd import native as nat
    nat.lib()
    return nat


def transformer(H, L, C, T):
    from torchflows_amd.bijections.finite.autoregressive.transformers.combination.dense_sigmoid import (
        DeepDenseSigmoid, DenseSigmoid)
    kw = dict(n_dense_layers=L, hidden_size=H)
    return DenseSigmoid((T,), **kw) if C == 1 else DeepDenseSigmoid((T,), n_hidden_layers=C, **kw)


@pytest.mark.parametrize("T,N,tail,accumulate,share,scale", ROWS)
@pytest.mark.parametrize("H,L,C", SIZES)
def test_kernel_against_float64(native, H, L, C, T, N, tail, accumulate, share, scale):
    g = torch.Generator().manual_seed(1000 * H + 100 * L + 10 * C + T)
    D = T + 3
    tr = transformer(H, L, C, T)
    P = tr.n_parameters_per_element
    tgt = torch.arange(3, D) if tail else torch.randperm(D, generator=g)[:T]
    constant = torch.zeros(T * P, dtype=torch.bool)
    constant[torch.randperm(T * P, generator=g)[:int(T * P * share)]] = True
    h = torch.randn(N, T * P, generator=g) * scale
    h[:, constant] = h[0, constant]                                  # learned constants: the same for every row
    x = torch.rand(N, D, generator=g) * 8 - 4
    x[0, tgt[0]], x[-1, tgt[-1]] = 9.5, -9.5                          # (one element: -9.5)
    with torch.no_grad():
        z64, ld64 = tr.forward(x[:, tgt].double(), h.view(N, T, P).double())
        z32, ld32 = tr.forward(x[:, tgt], h.view(N, T, P))
        x32, ldi32 = tr.inverse(z64.float(), h.view(N, T, P))
        _, ld_at32 = tr.forward(x32.double(), h.view(N, T, P).double())
    col = torch.where(constant, -1, torch.cumsum(~constant, 0) - 1)
    stride = int((~constant).sum())
    desc = native.dense_descriptor(tgt.cuda(), stride, col.cuda(), torch.where(constant, h[0], 0.0).cuda())
    pred = h[:, ~constant].contiguous().cuda() if stride else None
    ld0 = torch.randn(N, generator=g).cuda() if accumulate else torch.full((N,), float("nan")).cuda()
    others = np.setdiff1d(np.arange(D), tgt.numpy())

    def run(rows, inverse):
        out, ld = torch.full_like(rows, float("nan")), ld0.clone()
        before = native.calls
        native.dense_coupling(rows, pred, out, ld, desc, T, C, L, H, accumulate=accumulate, inverse=inverse)
        assert native.calls - before == 1
        same, ld_same = rows.clone(), ld0.clone()
        native.dense_coupling(same, pred, same, ld_same, desc, T, C, L, H, accumulate=accumulate, inverse=inverse)
        assert torch.equal(same, out) and torch.equal(ld_same, ld), "in place must give the same bits"
        assert np.array_equal(out.cpu().numpy()[:, others], rows.cpu().numpy()[:, others]), "pass-through columns"
        return out.cpu()[:, tgt], ((ld - ld0) if accumulate else ld).cpu()

    z, ld = run(x.cuda(), False)
    e_z, f_z, e_l, f_l = normwise(z, z64), normwise(z32, z64), rel(ld, ld64), rel(ld32, ld64)
    rows = x.clone()
    rows[:, tgt] = z64.float()
    xi, ldi = run(rows.cuda(), True)
    with torch.no_grad():
        _, ld_at = tr.forward(xi.double(), h.view(N, T, P).double())
        _, ld32_at = tr.forward(xi, h.view(N, T, P))
    e_x, f_x = normwise(xi, x[:, tgt]), normwise(x32, x[:, tgt])
    e_li, f_li = rel(-ldi, ld_at), max(rel(ld32_at, ld_at), rel(-ldi32, ld_at32))
    print(f"H{H} L{L} C{C} T{T} N{N}: z {e_z:.2e} (floor {f_z:.2e}), log-det {e_l:.2e} ({f_l:.2e}), x {e_x:.2e} ({f_x:.2e}), "
          f"inverse log-det {e_li:.2e} ({f_li:.2e})")
    assert e_z < bar(f_z) and e_l < bar(f_l)
    assert e_x < bar(f_x) and e_li < bar(f_li)


def counted(monkeypatch, native):
    """Launches of the dense kernel (native.KINDS looks the wrapper up by name at every call)."""
    n, real = [0], native.dense_coupling
    monkeypatch.setattr(native, "dense_coupling", lambda *a, **k: (n.__setitem__(0, n[0] + 1), real(*a, **k))[1])
    return n


@pytest.mark.parametrize("name,arch", FLOWS)
def test_flow_fixtures(native, monkeypatch, name, arch):
    fx = load_golden(name)
    g = lambda k: fx[f"init/{k}"]
    flow = build_flow(arch, fx).cuda()
    D = int(fx["event_shape"][0])
    sequential = {"MaskedAutoregressiveDenseSF": "inverse", "InverseAutoregressiveDeepDenseSF": "forward"}.get(arch)
    n = counted(monkeypatch, native)
    with torch.no_grad():
        lp = flow.log_prob(torch.from_numpy(fx["x"]).cuda())
        assert n[0] == (2 * D if sequential == "forward" else 2), n
        xr, ldr = flow.bijection.inverse(torch.from_numpy(fx["z_in"]).cuda())
        assert n[0] - (2 * D if sequential == "forward" else 2) == (2 * D if sequential == "inverse" else 2), n
        xs, lps = flow.sample((33,), return_log_prob=True)
    assert rel(lp.cpu().numpy(), g("log_prob")) < bar(rel(g("log_prob"), g("log_prob64")))
    assert normwise(xr.cpu().numpy(), g("x_inv")) < bar(normwise(g("x_inv"), g("x_inv64")))
    assert rel(ldr.cpu().numpy(), g("log_det_inv")) < bar(rel(g("log_det_inv"), g("log_det_inv64")))
    assert xs.shape == (33, D) and torch.isfinite(xs).all() and torch.isfinite(lps).all()


def test_unsupported_size_warns_and_runs_on_aten(native, monkeypatch):
    import torchflows_amd as tfa
    from torchflows_amd.fused import NativeRouteWarning
    torch.manual_seed(0)
    flow = tfa.Flow(tfa.CouplingDenseSF(6, n_layers=2, transformer_kwargs=dict(hidden_size=12))).eval()
    x = torch.randn(9, 6)
    with torch.no_grad():
        want = flow.double().log_prob(x.double())
    flow = flow.float().cuda()
    n = counted(monkeypatch, native)
    with torch.no_grad(), pytest.warns(NativeRouteWarning):
        got = flow.log_prob(x.cuda())
    # (the fp32 ATen path: a log-density summed from about 1 500 terms, each rounded to 6e-8 relative -- 1e-4 at the worst)
    assert n[0] == 0 and rel(got.cpu().numpy(), want.numpy()) < 1e-4


def test_debug_key_forces_the_aten_path(native, monkeypatch):
    fx = load_golden("flow_cdensesf16.npz")
    flow = build_flow("CouplingDenseSF", fx).cuda()
    set_debug(monkeypatch, dense="0")
    n = counted(monkeypatch, native)
    with torch.no_grad():
        lp = flow.log_prob(torch.from_numpy(fx["x"]).cuda())
    assert n[0] == 0
    assert rel(lp.cpu().numpy(), fx["init/log_prob"]) < bar(rel(fx["init/log_prob"], fx["init/log_prob64"]))
