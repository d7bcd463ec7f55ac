"""The deep sigmoidal coupling written plainly: what tests/test_gpu_dsf_shapes.py holds csrc/tfk_dsf.hip to, and what
tests/test_host_dsf_shapes.py proves about the cases on the host before anything runs on a GPU.

The reference is this package's own ATen transformer (transformers/combination/sigmoid.py) in float64, which
tests/test_host_dsf.py pins to the reference project's fixtures.  All inputs are drawn here from fixed seeds.  The
inverse truth is the reference's bisection rule (bracket [-10, 10], moved on f(c) < y, result = the last midpoint) run
for a fixed 100 trips in fp64 -- not ``bisection_no_gradient``, whose batch-wide ``allclose`` (rtol 1e-5) stops as soon
as every step is below 1e-5 |mid|.

Bars (the project's rule, tests/test_gpu_dsf.py): values norm-wise and log-dets element-wise relative to max(1, |ref|),
both against fp64 and below ``bar(floor) = max(1e-5, 3 x floor)``, the floor being the distance of the ATen fp32 result
from fp64 on the same inputs and the same elements; gradients per element through ``_within``."""
from types import SimpleNamespace

import numpy as np
import torch

from test_host_dsf import bar, dsf_transformer, normwise, rel  # noqa: F401  (the measures, re-exported)
from torchflows_amd.bijections.finite.autoregressive.transformers.combination.sigmoid import inverse_sigmoid

EPS = 1e-6                  # the clip of Sigmoid.forward_1d
NEAR = 1e-4                 # d outside [NEAR, 1 - NEAR]: the map is flat or ill-conditioned in fp32
NEAR_CAP = 0.10             # at most this share of an inverse case may be excluded
BISECTION_TRIPS = 100       # 20 * 2^-100: far below one ulp of any fp64 midpoint


def _within(mine, r32, r64):
    err = np.abs(np.asarray(mine, np.float64) - r64)
    bound = 1e-4 * np.maximum(1.0, np.abs(r64)) + 4 * np.abs(np.asarray(r32, np.float64) - r64)
    return int((err > bound).sum()), float(err.max()) if err.size else 0.0


def dsf_block(K):
    """Elements per workgroup (csrc/tfk_dsf.hip: dsf_block)."""
    return 256 if K <= 4 else 128


def transformer(C, K, T):
    return dsf_transformer(f"C{C}_K{K}", T)[0]


def target_columns(D, T, masked):
    """Sorted target columns, as the layers produce them: an evenly strided index list when masked, the tail otherwise."""
    if not masked:
        return np.arange(D - T, D)
    step = max(1, (D - 1) // max(T - 1, 1))
    cols = np.arange(0, D, step)[:T]
    assert cols.size == T
    return cols


def make_case(C, K, N, D, T, masked, h_scale, seed, stress_rows=0):
    """x = 2 randn(N, D) (the last ``stress_rows`` rows uniform on [-9, 9]) and h = h_scale randn(N, T, 3 K C)."""
    g = torch.Generator().manual_seed(seed)
    x = 2.0 * torch.randn(N, D, generator=g)
    h = h_scale * torch.randn(N, T, 3 * K * C, generator=g)
    if stress_rows:
        x[N - stress_rows:] = (torch.rand(stress_rows, D, generator=g) * 2 - 1) * 9.0
    cols = target_columns(D, T, masked)
    return SimpleNamespace(C=C, K=K, N=N, D=D, T=T, masked=masked, h_scale=h_scale, seed=seed, x=x, h=h, cols=cols,
                           tr=transformer(C, K, T))


def targets(case):
    return case.x[:, torch.from_numpy(case.cols)].contiguous()


def _forward(case, dtype):
    with torch.no_grad():
        z, ld = case.tr.forward(targets(case).to(dtype), case.h.to(dtype))
    return z.numpy(), ld.numpy()


def forward64(case):
    return _forward(case, torch.float64)


def forward32(case):
    return _forward(case, torch.float32)


def _components(tr):
    comps = getattr(tr, "components", [tr])
    start = 0
    for c in comps:
        P = c.n_parameters_per_element
        yield c, slice(start, start + P)
        start += P


def inverse64(tr, z_in, h, reference_stop=False):
    """(x, log-det of the inverse) in fp64; the log-det is evaluated at the returned x.  ``reference_stop`` ends each
    component's search where the reference ends it (consecutive midpoints ``allclose`` over the whole batch, atol 1e-9,
    rtol 1e-5) instead of after the fixed trips: only to show that the rule is the reference's."""
    v = torch.as_tensor(z_in, dtype=torch.float64)
    h = torch.as_tensor(h, dtype=torch.float64)
    log_det = torch.zeros(v.shape[0], dtype=torch.float64)
    with torch.no_grad():
        for comp, sl in reversed(list(_components(tr))):
            hc = h[..., sl].reshape(-1, sl.stop - sl.start)
            y = v.reshape(-1)
            a, b, w, _ = comp.extract_parameters(hc)                   # forward_1d's value, the parameters extracted once
            value = lambda t: inverse_sigmoid(torch.clip(
                torch.einsum("...i,...i->...", w, torch.sigmoid(a * t[:, None] + b)), EPS, 1 - EPS))
            lo, hi = torch.full_like(y, -10.0), torch.full_like(y, 10.0)
            mid = (lo + hi) / 2
            for _ in range(BISECTION_TRIPS):
                below = value(mid) < y
                lo, hi = torch.where(below, mid, lo), torch.where(below, hi, mid)
                previous, mid = mid, (lo + hi) / 2
                if reference_stop and torch.allclose(previous, mid, atol=1e-9):
                    break
            log_det = log_det - comp.forward_1d(mid, hc)[1].view_as(v).sum(-1)
            v = mid.view_as(v)
    return v.numpy(), log_det.numpy()


def inverse_log_det_at(tr, mids, h, dtype):
    """What an inverse launch returns as its log-det, given where each component's search ended (``mids``, one (N, T)
    array per component, first component first): minus the sum of the components' forward log-dets there."""
    h = torch.as_tensor(h).to(dtype)
    with torch.no_grad():
        return -sum(comp.forward(torch.as_tensor(m).to(dtype), h[..., sl])[1]
                    for (comp, sl), m in zip(_components(tr), mids)).numpy()


def inverse32(tr, z_in, h):
    """The ATen path in fp32 (``bisection_no_gradient``): measures the floor only."""
    with torch.no_grad():
        x, ld = tr.inverse(torch.as_tensor(z_in, dtype=torch.float32), torch.as_tensor(h, dtype=torch.float32))
    return x.numpy(), ld.numpy()


def walk_d64(tr, x, h):
    """The fp64 walk of x (N, T) through the components.  ``clip``: some component has d <= 1e-6 or d >= 1 - 1e-6;
    ``near``: some component has d outside [1e-4, 1 - 1e-4]."""
    x = torch.as_tensor(x, dtype=torch.float64)
    h = torch.as_tensor(h, dtype=torch.float64)
    clip = torch.zeros_like(x, dtype=torch.bool)
    near = torch.zeros_like(x, dtype=torch.bool)
    with torch.no_grad():
        for comp, sl in _components(tr):
            a, b, w, _ = comp.extract_parameters(h[..., sl].reshape(-1, sl.stop - sl.start))
            d = (w * torch.sigmoid(a * x.reshape(-1)[:, None] + b)).sum(-1).view_as(x)
            clip |= (d <= EPS) | (d >= 1 - EPS)
            near |= (d < NEAR) | (d > 1 - NEAR)
            x, _ = comp.forward(x, h[..., sl])
    return clip.numpy(), near.numpy()


def margins64(tr, x, h):
    """min(d, 1 - d) of every element over the components of the fp64 walk: how close it comes to the clip."""
    x = torch.as_tensor(x, dtype=torch.float64)
    h = torch.as_tensor(h, dtype=torch.float64)
    out = torch.ones_like(x)
    with torch.no_grad():
        for comp, sl in _components(tr):
            a, b, w, _ = comp.extract_parameters(h[..., sl].reshape(-1, sl.stop - sl.start))
            d = (w * torch.sigmoid(a * x.reshape(-1)[:, None] + b)).sum(-1).view_as(x)
            out = torch.minimum(out, torch.minimum(d, 1 - d))
            x, _ = comp.forward(x, h[..., sl])
    return out.numpy()


def grads(case, gz, gld, dtype):
    """d / d (x at the targets, h) of sum(z gz) + sum(log-det gld) by autograd through the ATen transformer."""
    xt = targets(case).to(dtype).requires_grad_(True)
    ht = case.h.to(dtype, copy=True).requires_grad_(True)              # (a copy: the case stays as drawn)
    z, ld = case.tr.forward(xt, ht)
    return [t.numpy() for t in torch.autograd.grad((z * gz.to(dtype)).sum() + (ld * gld.to(dtype)).sum(), (xt, ht))]


def da_beyond_20(case):
    """Share of the ``da`` entries of h whose softplus argument default_u_a + da / 1000 exceeds 20 (fp64)."""
    K, h = case.K, case.h.double()
    comp = getattr(case.tr, "components", [case.tr])[0]
    da = torch.cat([h[..., c * 3 * K:c * 3 * K + K] for c in range(case.C)], dim=-1)
    return float((comp.default_u_a + da / 1000.0 > 20.0).double().mean())


def inverse_problem(case):
    """What an inverse case asks and what it is held to: z_in = fp32(forward64(x)), the fp64 inverse of it, the ATen
    fp32 inverse, and the masks of the walk at x."""
    z64, _ = forward64(case)
    z_in = z64.astype(np.float32)
    x64, ld64 = inverse64(case.tr, z_in, case.h)
    x32, ld32 = inverse32(case.tr, z_in, case.h)
    clip, near = walk_d64(case.tr, targets(case), case.h)
    return SimpleNamespace(z_in=z_in, x64=x64, ld64=ld64, x32=x32, ld32=ld32, clip=clip, near=near)


# ---------------------------------------------------------------------------------------------------------------------
# The case tables, shared by the host file (caps and reach conditions) and the GPU file (the kernels).
# ---------------------------------------------------------------------------------------------------------------------
SUPPORTED = [(C, K) for C in (1, 2) for K in range(1, 17)] + [(C, K) for C in (3, 4) for K in range(1, 9)]
H_SCALE = 700.0


def case_a(C, K):
    return make_case(C, K, 96, 15, 7, True, H_SCALE, seed=1000 + 20 * C + K)


GEOMETRY_CK = [(2, 4), (2, 5)]


def geometry_shapes(K):
    """(N, D, T, masked) of group (b); ``masked`` with T = D is the full index list."""
    B = dsf_block(K)
    return [(300, 1, 1, False), (300, 9, 1, True), (131, 8, 8, False), (131, 8, 8, True), (67, 64, 64, False),
            (37, 19, 8, True), (9, 300, 128, True), (7, 2 * B + 3, B, True), (5, 23, 13, True), (1, 21, 11, True)]


N_GEOMETRY = 10


def case_b(C, K, i):
    N, D, T, masked = geometry_shapes(K)[i]
    return make_case(C, K, N, D, T, masked, H_SCALE, seed=2000 + 100 * K + i)


CHUNK_CK = [(2, 4), (2, 5), (1, 16), (4, 8), (1, 4)]     # (1, 4): one component on the 256-lane tile


def chunk_shapes(K):
    """(D, T) of group (c): rows longer than the tile."""
    B = dsf_block(K)
    return [(2 * B + 5, B + 1), (2 * B + 37 + 9, 2 * B + 37), (2 * B, 2 * B)]


N_CHUNK = 3


def case_c(C, K, i, masked):
    D, T = chunk_shapes(K)[i]
    return make_case(C, K, 3, D, T, masked, H_SCALE, seed=3000 + 100 * K + 10 * C + 2 * i + int(masked))


WRAP = [((1, 1), 260, 256), ((2, 5), 21, 11)]          # (C, K), D, T of group (d), masked


def wrap_rows(cu, K, T):
    """Rows for which some workgroup of the forward, inverse and backward launches takes a second tile: the grid is at
    most 8 workgroups per compute unit whatever the LDS size, and a tile holds R = BLOCK / T rows."""
    return 8 * cu * (dsf_block(K) // T) + 5


def case_d(i, cu):
    (C, K), D, T = WRAP[i]
    return make_case(C, K, wrap_rows(cu, K, T), D, T, True, H_SCALE, seed=4000 + i)


RANGE_CK = [(2, 4), (2, 16), (4, 8)]
RANGE_SCALES = [0.0, 3000.0, 30000.0]


# seeds at which a draw reaches what its case is for (tests/test_host_dsf_shapes.py asserts it): with 16 hidden units a
# clipped element at h_scale 3 000 needs every unit of weight saturated, one draw in forty has one
RANGE_SEEDS = {(2, 16, 3000.0): 5010, (4, 8, 3000.0): 5008}


def case_e(C, K, h_scale):
    seed = RANGE_SEEDS.get((C, K, h_scale), 5000 + 20 * C + K + int(h_scale) // 1000)
    return make_case(C, K, 64, 21, 11, True, h_scale, seed=seed, stress_rows=16)


UNREACHABLE_CK = [(2, 4), (2, 5), (1, 4), (1, 5)]


def case_f(C, K):
    return make_case(C, K, 64, 21, 11, True, H_SCALE, seed=6000 + 20 * C + K)


REFUSAL = dict(C=2, K=16, N=2, D=16000, T=8)


def case_g(masked):
    """Group (g): an index list over a row too wide for the workgroup's LDS, or the tail of the same row."""
    g = REFUSAL
    return make_case(g["C"], g["K"], g["N"], g["D"], g["T"], masked, H_SCALE, seed=7000)


def inverse_cases():
    """Every inverse case of the tables, as (id, thunk): the cap on the ``near`` share is proven for all of them on the
    host.  Group (d) is sized by the device; the host proves it at the 256 compute units of an MI355X."""
    out = [(f"a-C{C}-K{K}", lambda C=C, K=K: case_a(C, K)) for C, K in SUPPORTED]
    out += [(f"b-C{C}-K{K}-{i}", lambda C=C, K=K, i=i: case_b(C, K, i)) for C, K in GEOMETRY_CK for i in range(N_GEOMETRY)]
    out += [(f"c-C{C}-K{K}-{i}-{'masked' if m else 'tail'}", lambda C=C, K=K, i=i, m=m: case_c(C, K, i, m))
            for C, K in CHUNK_CK for i in range(N_CHUNK) for m in (True, False)]
    out += [(f"d-{i}", lambda i=i: case_d(i, 256)) for i in range(len(WRAP))]
    out += [(f"e-C{C}-K{K}-default", lambda C=C, K=K: case_e(C, K, 0.0)) for C, K in RANGE_CK]
    return out
