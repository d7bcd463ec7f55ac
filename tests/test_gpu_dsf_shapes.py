"""csrc/tfk_dsf.hip at every size, tiling path and edge, against the operation written plainly in fp64 on the host
(tests/dsf_reference.py: this package's ATen transformer in float64, the inverse as the reference's bisection rule run
for a fixed 100 trips).  Direct calls of ``native.dsf_coupling`` and ``native.dsf_coupling_bwd``; one flow at the end.

Bars (the rule of tests/test_gpu_dsf.py, no new constants).  z and x norm-wise and log-dets element-wise relative to
max(1, |ref|), both against fp64 and below max(1e-5, 3 x floor); the floor is the distance of the ATen fp32 result from
fp64 on the same inputs and the same elements.  Gradients per element within 1e-4 max(1, |ref64|) + 4 |ref32 - ref64|.
The inverse's x is measured where no component has d outside [1e-4, 1 - 1e-4] (``near``: the map is flat or
ill-conditioned in fp32 elsewhere); that excludes at most 10 % of any case (tests/test_host_dsf_shapes.py proves the
cap on the host) and every element, excluded or not, must come back finite and inside the bracket.  The inverse's
log-det is held to the fp64 inverse on the rows without a ``near`` element and, for one component, on every row to
minus the fp64 forward log-det at the x the kernel returned, which is what the kernel evaluates ((1, 4) joins the
sizes of the long rows for that: one component on the 256-lane tile, as (1, 16) is on the 128-lane one).

Every launch is also checked for: pass-through columns bit-equal, one ``native.calls`` increment, the in-place launch
giving the bits of the out-of-place one, a canary row on either side of ``out`` and a canary element on either side of
``logdet``."""
import copy
import functools
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import dsf_reference as R
from dsf_reference import _within, bar, normwise, rel

pytestmark = pytest.mark.gpu

CANARY = 7.0


@pytest.fixture(scope="module")
def native():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    from torchflows_amd import native as nat
    nat.lib()
    return nat


# ---------------------------------------------------------------------------------------------------------------------
# References: computed once per case on the host, shared by the tests that need them, never written to.
# ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _case(group, *key):
    return getattr(R, f"case_{group}")(*key)


@functools.lru_cache(maxsize=None)
def _forward_ref(group, *key):
    case = _case(group, *key)
    z64, ld64 = R.forward64(case)
    z32, ld32 = R.forward32(case)
    return SimpleNamespace(z64=z64, ld64=ld64, z32=z32, ld32=ld32)


@functools.lru_cache(maxsize=None)
def _inverse_ref(group, *key):
    return R.inverse_problem(_case(group, *key))


@functools.lru_cache(maxsize=None)
def _grad_ref(group, *key):
    case = _case(group, *key)
    gen = torch.Generator().manual_seed(5)
    gz, gld = torch.randn(case.N, case.T, generator=gen), torch.randn(case.N, generator=gen)
    (gx32, gh32), (gx64, gh64) = R.grads(case, gz, gld, torch.float32), R.grads(case, gz, gld, torch.float64)
    return SimpleNamespace(gz=gz, gld=gld, gx32=gx32, gh32=gh32, gx64=gx64, gh64=gh64)


# ---------------------------------------------------------------------------------------------------------------------
# Launches, with the checks every test makes
# ---------------------------------------------------------------------------------------------------------------------
def _launch(native, case, values, inverse, accumulate):
    """One ``dsf_coupling`` launch on the case's rows with ``values`` (N, T) at the target columns.  Returns the
    target columns of the output and the log-det the launch produced (fp64; the initial value taken off again when it
    accumulates)."""
    N, D, T, cols = case.N, case.D, case.T, case.cols
    rows = case.x.numpy().copy()
    rows[:, cols] = values
    x_d, h_d = torch.from_numpy(rows).cuda(), case.h.cuda().contiguous()
    guard = torch.full((N + 2, D), CANARY).cuda()                      # a row of canaries on either side of out
    ld_guard = torch.full((N + 2,), CANARY).cuda()                     # an element on either side of logdet
    ld0 = (torch.randn(N, generator=torch.Generator().manual_seed(3)) if accumulate else torch.full((N,), float("nan"))).cuda()
    out, got_ld = guard[1:-1], ld_guard[1:-1]
    got_ld.copy_(ld0)
    tgt_d = torch.from_numpy(cols.astype(np.int32)).cuda() if case.masked else None
    before = native.calls
    native.dsf_coupling(x_d, h_d, out, got_ld, tgt_d, T, case.C, case.K, accumulate=accumulate, inverse=inverse)
    torch.cuda.synchronize()
    assert native.calls - before == 1
    assert float(guard[0].min()) == CANARY and float(guard[0].max()) == CANARY
    assert float(guard[-1].min()) == CANARY and float(guard[-1].max()) == CANARY
    assert float(ld_guard[0]) == CANARY and float(ld_guard[-1]) == CANARY
    assert torch.equal(x_d.cpu(), torch.from_numpy(rows)), "the input rows were written to"
    out_h = out.cpu().numpy()
    others = np.setdiff1d(np.arange(D), cols)
    assert np.array_equal(out_h[:, others], rows[:, others]), "pass-through columns must be copied unchanged"
    x2, ld2 = x_d.clone(), ld0.clone()                                 # in place gives the same bits
    before = native.calls
    native.dsf_coupling(x2, h_d, x2, ld2, tgt_d, T, case.C, case.K, accumulate=accumulate, inverse=inverse)
    torch.cuda.synchronize()
    assert native.calls - before == 1
    assert torch.equal(x2, out) and torch.equal(ld2, got_ld), "in place and out of place differ"
    ld = got_ld.double().cpu().numpy()
    return out_h[:, cols], (ld - ld0.double().cpu().numpy()) if accumulate else ld


def _offenders(tag, mine, r32, r64, margin=None, limit=4):
    """The elements beyond the gradient bound, worst first: what the kernel, ATen fp32 and fp64 say, and how close the
    element's d comes to 0 or 1 in the fp64 walk."""
    mine, r32 = np.asarray(mine, np.float64), np.asarray(r32, np.float64)
    err = np.abs(mine - r64)
    bound = 1e-4 * np.maximum(1.0, np.abs(r64)) + 4 * np.abs(r32 - r64)
    over = np.argwhere(err > bound)
    for idx in sorted(map(tuple, over), key=lambda i: -err[i] / bound[i])[:limit]:
        m = "" if margin is None else f", min(d, 1 - d) {margin[idx[:margin.ndim]]:.2e}"
        print(f"   {tag}{list(idx)}: kernel {mine[idx]:.7e}, ATen fp32 {r32[idx]:.7e}, fp64 {r64[idx]:.7e}{m}")


WORST = {}


def _note(group, what, err, limit):
    """Error / bar of every comparison, the worst per group printed as it grows (the printed lines are the record)."""
    ratio = err / limit
    if ratio > WORST.get(group, (0.0, ""))[0]:
        WORST[group] = (ratio, what)
        print(f"   worst of group ({group}) so far: {ratio:.3f} of the bar ({what})")


def _check_forward(native, group, key, accumulate=False):
    case, ref = _case(group, *key), _forward_ref(group, *key)
    z, ld = _launch(native, case, R.targets(case).numpy(), False, accumulate)
    e_z, f_z, e_l, f_l = normwise(z, ref.z64), normwise(ref.z32, ref.z64), rel(ld, ref.ld64), rel(ref.ld32, ref.ld64)
    print(f"({group}) {key} fwd acc={accumulate}: z {e_z:.2e} (floor {f_z:.2e}), log-det {e_l:.2e} (floor {f_l:.2e})")
    _note(group, f"{key} fwd z", e_z, bar(f_z))
    _note(group, f"{key} fwd log-det", e_l, bar(f_l))
    assert np.isfinite(z).all() and np.isfinite(ld).all()
    assert e_z < bar(f_z)
    assert e_l < bar(f_l)
    return z, ld


def _check_log_det_at(group, key, what, case, x, ld):
    """One component: the inverse's log-det is minus the forward log-det at the x it returned, on every row: fp64 (and
    the ATen fp32 floor) there.  (With more components the later searches end a rounding of the earlier component's
    value away from where the forward walk of x passes, which near the clip is not small: no identity to hold.)"""
    with torch.no_grad():
        want64 = -case.tr.forward(torch.from_numpy(x).double(), case.h.double())[1].numpy()
        want32 = -case.tr.forward(torch.from_numpy(x).float(), case.h)[1].numpy()
    e, f = rel(ld, want64), rel(want32, want64)
    print(f"({group}) {key} {what}: log-det vs minus the fp64 forward log-det at the returned x {e:.2e} (floor {f:.2e})")
    _note(group, f"{key} {what} log-det at x", e, bar(f))
    assert e < bar(f)


def _check_inverse(native, group, key, accumulate=False):
    case, p = _case(group, *key), _inverse_ref(group, *key)
    share = float(p.near.mean())
    assert share <= R.NEAR_CAP, f"the near mask excludes {share:.1%} of the elements: draw another seed"
    x, ld = _launch(native, case, p.z_in, True, accumulate)
    assert np.isfinite(x).all() and np.isfinite(ld).all() and float(np.abs(x).max()) <= 10.0
    keep = ~p.near
    rows = keep.all(axis=1)
    e_x, f_x = normwise(x[keep], p.x64[keep]), normwise(p.x32[keep], p.x64[keep])
    e_l, f_l = rel(ld[rows], p.ld64[rows]), rel(p.ld32[rows], p.ld64[rows])
    print(f"({group}) {key} inv acc={accumulate}: x {e_x:.2e} (floor {f_x:.2e}) on {keep.mean():.1%} of the elements, "
          f"log-det {e_l:.2e} (floor {f_l:.2e}) on {int(rows.sum())} of {rows.size} rows")
    _note(group, f"{key} inv x", e_x, bar(f_x))
    _note(group, f"{key} inv log-det", e_l, bar(f_l))
    if rows.any() and e_l >= bar(f_l):
        r = int(np.argmax(np.where(rows, np.abs(ld - p.ld64) / np.maximum(1.0, np.abs(p.ld64)), -1.0)))
        margin = R.margins64(case.tr, R.targets(case), case.h)[r]
        print(f"   row {r}: log-det kernel {ld[r]:.7e}, ATen fp32 {p.ld32[r]:.7e}, fp64 {p.ld64[r]:.7e}; max |x - x64| kernel "
              f"{np.abs(x[r] - p.x64[r]).max():.2e}, ATen fp32 {np.abs(p.x32[r] - p.x64[r]).max():.2e}; min(d, 1 - d) {margin.min():.2e}")
    assert e_x < bar(f_x)
    assert e_l < bar(f_l)
    if case.C == 1:
        _check_log_det_at(group, key, "inv", case, x, ld)
    return x, ld


def _check_backward(native, group, key):
    case, ref = _case(group, *key), _grad_ref(group, *key)
    N, D, T, cols = case.N, case.D, case.T, case.cols
    g_guard = torch.full((N + 2, D), CANARY)
    g_guard[1:-1] = 0.25
    g_guard[1:-1, torch.from_numpy(cols)] = ref.gz
    g_guard = g_guard.cuda()
    gh_guard = torch.full((N + 2, T, case.h.shape[-1]), CANARY).cuda()
    gh_guard[1:-1] = float("nan")
    x_d, h_d = case.x.cuda(), case.h.cuda().contiguous()
    tgt_d = torch.from_numpy(cols.astype(np.int32)).cuda() if case.masked else None
    before = native.calls
    native.dsf_coupling_bwd(x_d, h_d, g_guard[1:-1], ref.gld.cuda(), gh_guard[1:-1], tgt_d, T, case.C, case.K)
    torch.cuda.synchronize()
    assert native.calls - before == 1
    for t in (g_guard, gh_guard):
        assert float(t[0].min()) == CANARY and float(t[0].max()) == CANARY
        assert float(t[-1].min()) == CANARY and float(t[-1].max()) == CANARY
    assert torch.equal(x_d.cpu(), case.x) and torch.equal(h_d.cpu(), case.h)
    g_h = g_guard[1:-1].cpu().numpy()
    others = np.setdiff1d(np.arange(D), cols)
    assert np.all(g_h[:, others] == 0.25), "only the target columns are rewritten"
    results = []
    for mine, name, r32, r64 in ((g_h[:, cols], "gx", ref.gx32, ref.gx64),
                                 (gh_guard[1:-1].cpu().numpy(), "gh", ref.gh32, ref.gh64)):
        bad, worst = _within(mine, r32, r64)
        print(f"({group}) {key} bwd {name}: max err {worst:.2e}, beyond bound {bad} of {mine.size}")
        if bad:
            _offenders(name, mine, r32, r64, R.margins64(case.tr, R.targets(case), case.h))
        results.append((np.isfinite(mine).all(), bad))
    for finite, bad in results:
        assert finite and bad == 0


# ---------------------------------------------------------------------------------------------------------------------
# (a) every instantiation: the 48 supported (components, hidden units), the 50 KB LDS launches among them
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C,K", R.SUPPORTED)
def test_every_instantiation(native, C, K):
    assert native.dsf_supported(C, K)
    _check_forward(native, "a", (C, K), accumulate=False)
    _check_inverse(native, "a", (C, K), accumulate=True)
    _check_backward(native, "a", (C, K))


# ---------------------------------------------------------------------------------------------------------------------
# (b) geometry: T = 1, D = 1, T = D with and without the index list, one wave per row, the LDS reduction through
# tid >> T_shift (T = 128, 256), T = BLOCK, ragged last row groups, one row
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("accumulate", [False, True])
@pytest.mark.parametrize("i", range(R.N_GEOMETRY))
@pytest.mark.parametrize("C,K", R.GEOMETRY_CK)
def test_geometry(native, C, K, i, accumulate):
    """(The log-det of the inverse at (2, 5), (N, D, T) = (300, 1, 1) is the case that showed what fl(1 - d) costs the
    root of the bisection: 1.23e-5 against a bar of 1e-5 with 1 - d taken from the rounded d, 2.8e-7 with the
    complement sum of csrc/tfk_dsf.hip: dsf_logit.)"""
    case = _case("b", C, K, i)
    print(f"(b) N = {case.N}, D = {case.D}, T = {case.T}, {'index list' if case.masked else 'tail'}")
    _check_forward(native, "b", (C, K, i), accumulate)
    _check_inverse(native, "b", (C, K, i), accumulate)
    if not accumulate:
        _check_backward(native, "b", (C, K, i))


# ---------------------------------------------------------------------------------------------------------------------
# (c) rows longer than the tile: the per-chunk record load, the per-lane accumulation, the tree reduction, the single
# log-det write, one row per pass-through copy
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("accumulate", [False, True])
@pytest.mark.parametrize("masked", [True, False])
@pytest.mark.parametrize("i", range(R.N_CHUNK))
@pytest.mark.parametrize("C,K", R.CHUNK_CK)
def test_rows_longer_than_the_tile(native, C, K, i, masked, accumulate):
    case = _case("c", C, K, i, masked)
    assert case.T > R.dsf_block(K)
    print(f"(c) N = {case.N}, D = {case.D}, T = {case.T}, {'index list' if masked else 'tail'}")
    _check_forward(native, "c", (C, K, i, masked), accumulate)
    _check_inverse(native, "c", (C, K, i, masked), accumulate)
    if not accumulate:
        _check_backward(native, "c", (C, K, i, masked))


# ---------------------------------------------------------------------------------------------------------------------
# (d) the grid-stride loop takes a second trip
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("i", range(len(R.WRAP)))
def test_grid_wrap(native, i):
    # The launch grid is at most 8 workgroups per compute unit whatever the LDS size, and a tile holds R = BLOCK / T
    # rows (BLOCK elements in the backward), so with N = 8 * cu * R + 5 rows there are more tiles than workgroups in
    # all three kernels: some workgroup takes a second tile.  Every row is checked.
    cu = torch.cuda.get_device_properties(0).multi_processor_count
    case = _case("d", i, cu)
    (C, K), D, T = R.WRAP[i]
    assert case.N == 8 * cu * (R.dsf_block(K) // T) + 5
    assert i != 0 or case.N * T > 8 * cu * R.dsf_block(K)             # the backward's tiles are BLOCK elements
    print(f"(d) {cu} compute units: N = {case.N}, D = {D}, T = {T}")
    _check_forward(native, "d", (i, cu))
    _check_inverse(native, "d", (i, cu))
    if i == 0:
        _check_backward(native, "d", (i, cu))


# ---------------------------------------------------------------------------------------------------------------------
# (e) parameter ranges: the default parameters, the linear branch of softplus (forward and backward), the clip
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("h_scale", R.RANGE_SCALES)
@pytest.mark.parametrize("C,K", R.RANGE_CK)
def test_parameter_ranges(native, C, K, h_scale):
    """(At h_scale 30 000 the elements that are not clipped sit beside the clip: the reverse mode needs 1 / (d (1 - d)) and
    s_j - sum(s w) there, which csrc/tfk_dsf.hip takes from the complement sum; with fl(1 - d) and the plain
    difference 8 elements of (2, 16) and (4, 8) were beyond their bounds, one by 1.3e-3 on a value of 1.4e-3.)"""
    case = _case("e", C, K, h_scale)
    clip, _ = R.walk_d64(case.tr, R.targets(case), case.h)
    beyond = R.da_beyond_20(case)
    print(f"(e) C{C}_K{K} h_scale {h_scale:g}: softplus argument > 20 in {beyond:.1%} of da, clipped {clip.mean():.1%}")
    if h_scale == 30000.0:
        assert beyond >= 0.10, "the case does not reach the linear branch of softplus"
    if h_scale >= 3000.0:
        assert clip.any() and not clip.all(), "the case does not reach both sides of the clip"
    _check_forward(native, "e", (C, K, h_scale))
    _check_backward(native, "e", (C, K, h_scale))
    if h_scale == 0.0:
        x, ld_i = _check_inverse(native, "e", (C, K, h_scale))
        back, ld_f = _launch(native, case, x, False, False)
        p, ref = _inverse_ref("e", C, K, h_scale), _forward_ref("e", C, K, h_scale)
        keep = ~p.near
        e, floor = normwise(back[keep], p.z_in[keep]), normwise(ref.z32[keep], ref.z64[keep])
        cancel = rel(-ld_i, ld_f)
        print(f"(e) C{C}_K{K} round trip {e:.2e} (floor of z {floor:.2e}); log-dets cancel to {cancel:.2e} of the forward's")
        _note("e", f"{(C, K)} round trip", e, bar(floor))
        assert e < bar(floor)


# ---------------------------------------------------------------------------------------------------------------------
# (f) targets outside the reachable range +-logit(1e-6)
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sign", [1.0, -1.0])
@pytest.mark.parametrize("C,K", R.UNREACHABLE_CK)
def test_unreachable_targets(native, C, K, sign):
    """z_in = +-20 on every target.  The component inverted first cannot reach it, so its search ends on the bracket's
    end: with one component x = +-10 on every element.  With two, the second search is asked for +-10, which the first
    component does reach for some elements (on the host, in fp64: 117 of 704 at (2, 4), 70 at (2, 5)); there the bracket's
    end is asserted on the elements where the fp64 rule ends on it too, and the rest must be finite and inside it.
    The log-det is minus the forward log-det where the searches ended: at x for the first component and, with two, at
    +-10 for the second (not at the first's value of x, which is not +-10 where x sits on the bracket's end)."""
    case = _case("f", C, K)
    z_in = np.full((case.N, case.T), 20.0 * sign, np.float32)
    x64, _ = R.inverse64(case.tr, z_in, case.h)
    at_end = np.abs(x64 - 10.0 * sign) <= 1e-4
    assert at_end.all() if C == 1 else at_end.mean() >= 0.5
    x, ld = _launch(native, case, z_in, True, False)
    assert np.isfinite(x).all() and np.isfinite(ld).all() and float(np.abs(x).max()) <= 10.0
    worst = float(np.abs(x - 10.0 * sign)[at_end].max())
    print(f"(f) C{C}_K{K} z_in = {20.0 * sign:+g}: |x - ({10.0 * sign:+g})| <= {worst:.2e} on {int(at_end.sum())} of {at_end.size} elements")
    assert worst <= 1e-4
    mids = [x] + [np.full_like(x, 10.0 * sign)] * (C - 1)
    want64 = R.inverse_log_det_at(case.tr, mids, case.h, torch.float64)
    want32 = R.inverse_log_det_at(case.tr, mids, case.h, torch.float32)
    e, f = rel(ld, want64), rel(want32, want64)
    print(f"(f) C{C}_K{K} z_in = {20.0 * sign:+g}: log-det vs minus the fp64 forward log-det where the searches ended {e:.2e} "
          f"(floor {f:.2e})")
    _note("f", f"{(C, K, sign)} log-det", e, bar(f))
    assert e < bar(f)


# ---------------------------------------------------------------------------------------------------------------------
# (g) an index list over a row too wide for the workgroup's LDS is refused; the tail of the same row runs
# ---------------------------------------------------------------------------------------------------------------------
def test_wide_index_list_is_refused(native):
    case = _case("g", True)
    assert native.dsf_supported(case.C, case.K)
    x_d, h_d = case.x.cuda(), case.h.cuda().contiguous()
    out, ld = torch.full_like(x_d, CANARY), torch.full((case.N,), CANARY).cuda()
    with pytest.raises(native.NativeError, match="LDS"):
        native.dsf_coupling(x_d, h_d, out, ld, torch.from_numpy(case.cols.astype(np.int32)).cuda(), case.T, case.C, case.K)
    torch.cuda.synchronize()
    assert float(out.min()) == CANARY and float(out.max()) == CANARY and float(ld.min()) == CANARY, "a refused launch wrote"
    _check_forward(native, "g", (False,))


# ---------------------------------------------------------------------------------------------------------------------
# The route users take: CouplingDeepSF(300) has T = 150 and 10 hidden units, two chunks per row
# ---------------------------------------------------------------------------------------------------------------------
def _dsf_layers(flow):
    return [l for l in flow.bijection.layers if getattr(getattr(l, "transformer", None), "native_kind", None) == "dsf"]


def test_flow_of_event_size_300(native, monkeypatch):
    """(The gradients here are what 1 - d from the rounded d cost most: 7 of 9 600 elements of gx beyond their bounds,
    the worst 6.1e-2 off, against 4.3e-5 with the complement sum.  The ATen composite path on the same device
    (TORCHFLOWS_AMD_DEBUG="dsf=0") has 12 beyond: the bound is not one that fp32 meets by itself at this width.)"""
    import torchflows_amd as tfa
    from test_gpu_dsf import _count, _grads
    torch.manual_seed(2)
    flow = tfa.Flow(tfa.CouplingDeepSF(300, n_layers=2))
    couplings = _dsf_layers(flow)
    assert len(couplings) == 2
    with torch.no_grad():
        for layer in couplings:
            assert layer.coupling.target_event_size == 150 and layer.transformer.hidden_dim == 10
            assert layer.coupling.target_event_size > R.dsf_block(layer.transformer.hidden_dim)
            last = [m for m in layer.conditioner_transform.modules() if isinstance(m, torch.nn.Linear)][-1]
            last.weight.mul_(500.0)
            last.bias.mul_(500.0)
    g = torch.Generator().manual_seed(7)
    flow.train()
    with torch.no_grad():
        flow.log_prob(torch.randn(64, 300, generator=g))               # ActNorm data-dependent init, on the host
    flow.eval()
    N = 32
    x, w = torch.randn(N, 300, generator=g), torch.rand(N, generator=g) + 0.5
    flow64 = copy.deepcopy(flow).double()
    near_rows = torch.zeros(N, dtype=torch.bool)
    with torch.no_grad():
        v, n_near, n_elem = x.double(), 0, 0
        for layer in flow64.bijection.layers:
            if layer in _dsf_layers(flow64):
                _, near = R.walk_d64(layer.transformer, layer.get_transformed_part(v),
                                     layer.partition_and_predict_parameters(v, None))
                near_rows |= torch.from_numpy(near.any(axis=1))
                n_near, n_elem = n_near + int(near.sum()), n_elem + near.size
            v, _ = layer.forward(v)
        z64, lp64 = flow64.forward_with_log_prob(x.double())
        z32, lp32 = flow.forward_with_log_prob(x)
        z_in = z64.float()
        x64, ldi64 = flow64.bijection.inverse(z_in.double())
        x32, ldi32 = flow.bijection.inverse(z_in)
    assert n_near <= R.NEAR_CAP * n_elem
    keep = ~near_rows.numpy()                    # a ``near`` element feeds the next coupling's conditioner: whole rows
    assert keep.mean() >= 0.9
    gx64, g64 = _grads(flow64, x.double(), w.double())
    gx32, g32 = _grads(copy.deepcopy(flow), x, w)
    flow = flow.cuda()
    fwd, bwd = _count(monkeypatch, native, "dsf_coupling"), _count(monkeypatch, native, "dsf_coupling_bwd")
    before = native.calls
    with torch.no_grad():
        lp = flow.log_prob(x.cuda())
    assert fwd["n"] == 2 and bwd["n"] == 0 and native.calls - before >= 2, "tfk_dsf_coupling_fwd did not run once per coupling"
    with torch.no_grad():
        xr, ldr = flow.bijection.inverse(z_in.cuda())
    assert fwd["n"] == 4, "tfk_dsf_coupling_inv did not run once per coupling"
    e_lp, f_lp = rel(lp.cpu().numpy(), lp64.numpy()), rel(lp32.numpy(), lp64.numpy())
    e_x = normwise(xr.cpu().numpy()[keep], x64.numpy()[keep])
    f_x = normwise(x32.numpy()[keep], x64.numpy()[keep])
    e_ld, f_ld = rel(ldr.cpu().numpy()[keep], ldi64.numpy()[keep]), rel(ldi32.numpy()[keep], ldi64.numpy()[keep])
    print(f"CouplingDeepSF(300): log_prob {e_lp:.2e} (floor {f_lp:.2e}), x {e_x:.2e} (floor {f_x:.2e}) and inverse log-det "
          f"{e_ld:.2e} (floor {f_ld:.2e}) on {int(keep.sum())} of {N} rows")
    for what, e, f in (("log_prob", e_lp, f_lp), ("x", e_x, f_x), ("inverse log-det", e_ld, f_ld)):
        _note("flow", what, e, bar(f))
    assert torch.isfinite(xr).all() and torch.isfinite(ldr).all()
    assert e_lp < bar(f_lp)
    assert e_x < bar(f_x)
    assert e_ld < bar(f_ld)
    fwd["n"] = 0
    gx, grads = _grads(flow, x.cuda(), w.cuda())
    assert fwd["n"] == 2 and bwd["n"] == 2, "the training route did not run the dsf kernels once per coupling"
    bad, worst = _within(gx.cpu().numpy(), gx32.numpy(), gx64.numpy())
    print(f"CouplingDeepSF(300) gx: max err {worst:.2e}, beyond bound {bad} of {gx.numel()}")
    failed = ["gx"] if bad else []
    if bad:
        _offenders("gx", gx.cpu().numpy(), gx32.numpy(), gx64.numpy())
    for name, gr in grads.items():
        if gr is None or gr.numel() == 0:
            continue
        bad, worst = _within(gr.cpu().numpy(), g32[name].numpy(), g64[name].numpy())
        print(f"CouplingDeepSF(300) {name}: max err {worst:.2e}, beyond bound {bad} of {gr.numel()}")
        if bad or not torch.isfinite(gr).all():
            _offenders(name, gr.cpu().numpy(), g32[name].numpy(), g64[name].numpy())
            failed.append(name)
    assert not failed, failed
