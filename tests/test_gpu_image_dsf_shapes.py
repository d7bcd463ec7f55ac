"""csrc/tfk_glow_dsf.hip one launch at a time: every K, both passes' bookkeeping, every component count, both workgroup
sizes, partial groups and tiles, against this package's own ATen path in float64 on the host
(tests/image_dsf_reference.py builds the cases; tests/test_host_image_dsf_shapes.py proves on the host that they exclude
at most 2 % of the inverse, that the parameters of the wrong sample or target move z by ten bars and the log-det by ten
or, where the reference module records it, at least 1.5, and that the order of the components is held by the log-det
alone).

The launch under test is the single step of ``image_program.compile_program(module, d, device)``, called directly
(``native.glow_coupling``) on a copy of the rows, then ``native.rows_fma`` where the program has a flush.

Bars (tests/dsf_reference.py, no new constants): z and x norm-wise on the target columns, log-dets element-wise relative
to max(1, |ref|), both against float64 and below max(1e-5, 3 x floor), the floor being the ATen fp32-vs-fp64 distance on
the same inputs and elements.  The inverse's x is measured where |x64| < 9.99.

Every launch is also checked for: a canary row on either side of the rows and a canary element on either side of the
log-det untouched; ``native.calls`` up by one; every column that is not a target bit-equal to the input; the log-det
accumulated onto seeded random values (the difference is what is compared); a second launch giving the same bits."""
import warnings

import numpy as np
import pytest
import torch

import dsf_reference as DR
import image_dsf_reference as R
from image_dsf_reference import bar, normwise, rel

pytestmark = pytest.mark.gpu

CANARY = 7.0
WORST = {}


@pytest.fixture(scope="module")
def native():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    from torchflows_amd import native as nat
    nat.lib()
    return nat


def _note(group, what, err, limit):
    """Error / bar of every comparison, the worst per group printed as it grows (the printed lines are the record)."""
    ratio = err / limit
    if ratio > WORST.get(group, (-1.0, ""))[0]:
        WORST[group] = (ratio, what)
        print(f"   worst of group ({group}) so far: {ratio:.3f} of the bar ({what})")


def _held(group, what, err, floor):
    print(f"({group}) {what}: error {err:.2e}, floor {floor:.2e}, bar {bar(floor):.2e}")
    _note(group, what, err, bar(floor))
    return err < bar(floor)


def _launch(native, case, d, rows_in):
    """The case's coupling in direction d on rows_in (n, D), compiled under the debug switches in force.  Returns the
    rows behind the launch (and the flush) and the log-det the program adds, as float64 arrays."""
    dev = torch.device("cuda")
    prog, step = R.compile_step(case, d, dev)
    n, D = rows_in.shape
    cols = case.cols
    others = np.setdiff1d(np.arange(D), cols)
    ld0 = torch.randn(n, generator=torch.Generator().manual_seed(3))
    results = []
    for _ in range(2):
        guard = torch.full((n + 2, D), CANARY).cuda()
        ld_guard = torch.full((n + 2,), CANARY).cuda()
        rows, logdet = guard[1:-1], ld_guard[1:-1]
        rows.copy_(torch.from_numpy(rows_in))
        logdet.copy_(ld0)
        before = native.calls
        native.glow_coupling(rows, logdet, step.layer, inverse=step.inverse)
        torch.cuda.synchronize()
        assert native.calls - before == 1
        for g in (guard, ld_guard):
            assert float(g[0].min()) == CANARY == float(g[0].max()) and float(g[-1].min()) == CANARY == float(g[-1].max())
        assert np.array_equal(rows.cpu().numpy()[:, others], rows_in[:, others]), "a column that is no target was written"
        if prog.flush is not None:
            native.rows_fma(rows, prog.flush)
            torch.cuda.synchronize()
            assert float(guard[0].min()) == CANARY == float(guard[0].max()) and float(guard[-1].min()) == CANARY == float(guard[-1].max())
        results.append((rows.cpu(), logdet.cpu()))
    assert torch.equal(results[0][0], results[1][0]) and torch.equal(results[0][1], results[1][1]), "two launches differ"
    out, ld = results[0]
    return out.numpy(), (ld.double() - ld0.double()).numpy() + prog.ld_const


def _forward(native, group, case, ref, n, tag=""):
    z, ld = _launch(native, case, 0, case.x.reshape(R.N_ROWS, -1).numpy()[:n])
    c, what = case.cols, f"{case.name} C{case.C}_K{case.K} n={n}{tag} fwd"
    assert np.isfinite(z).all() and np.isfinite(ld).all()
    ok = _held(group, what + " z", normwise(z[:, c], ref.z64[:n][:, c]), normwise(ref.z32[:n][:, c], ref.z64[:n][:, c]))
    ok &= _held(group, what + " log-det", rel(ld, ref.ld64[:n]), rel(ref.ld32[:n], ref.ld64[:n]))
    others = np.setdiff1d(np.arange(case.D), c)          # (behind an ActNorm the flush moves them: held like z)
    if others.size and not np.array_equal(z[:, others], ref.z32[:n][:, others]):
        ok &= _held(group, what + " sources", normwise(z[:, others], ref.z64[:n][:, others]),
                    normwise(ref.z32[:n][:, others], ref.z64[:n][:, others]))
    return ok, z, ld


def _inverse(native, group, case, ref, n, tag=""):
    x, ld = _launch(native, case, 1, ref.z_in[:n].copy())
    c, what = case.cols, f"{case.name} C{case.C}_K{case.K} n={n}{tag} inv"
    keep = R.keep_mask(case, ref, n)
    assert 1.0 - keep.mean() <= R.EXCLUDED_CAP
    assert np.isfinite(x).all() and np.isfinite(ld).all()
    ok = _held(group, what + " x", normwise(x[:, c][keep], ref.x64[:n][:, c][keep]),
               normwise(ref.x32[:n][:, c][keep], ref.x64[:n][:, c][keep]))
    ok &= _held(group, what + " log-det", rel(ld, ref.ldi64[:n]), rel(ref.ldi32[:n], ref.ldi64[:n]))
    return ok, x, ld


def _both(native, group, name, C, K, n=R.N_ROWS, tag=""):
    case, ref = R.make_case(name, C, K), R.reference(name, C, K)
    ok_f, z, ld = _forward(native, group, case, ref, n, tag)
    ok_i, x, ldi = _inverse(native, group, case, ref, n, tag)
    assert ok_f and ok_i, "a comparison above is beyond its bar"
    return z, ld, x, ldi


# ---------------------------------------------------------------------------------------------------------------------
# (a) every instantiation: all 32 kernels, both values of NS, the component loop at C = 1 .. 4
#     T = 18: one full and one partial target group; 37 rows: two full row tiles and one of 5
# ---------------------------------------------------------------------------------------------------------------------
def test_there_are_48_supported_pairs(native):
    assert [(C, K) for C in range(1, 5) for K in range(1, 17) if native.dsf_supported(C, K)] == sorted(R.SUPPORTED)
    assert len(R.SUPPORTED) == 48


@pytest.mark.parametrize("C,K", R.SUPPORTED)
def test_every_instantiation(native, C, K):
    _both(native, "a", R.EVERY, C, K)


# ---------------------------------------------------------------------------------------------------------------------
# (b) geometry: T < 16, T = 16, T % 16 != 0, more groups than waves, contiguous and strided targets, pending maps;
#     one row, one full tile, one row past it, three tiles
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", R.GEOMETRY_N)
@pytest.mark.parametrize("C,K", R.GEOMETRY_CK)
@pytest.mark.parametrize("name", R.GEOMETRY_SHAPES)
def test_geometry(native, name, C, K, n):
    _both(native, "b", name, C, K, n)


# ---------------------------------------------------------------------------------------------------------------------
# (c) launch shapes: workgroups of 128 threads (two waves: the log-det through ldpart[0 .. 1]), one workgroup walking
#     all three row tiles (V and ldpart reused behind the trailing barrier), two workgroups sharing them
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("block", [256, 128], ids=["block256", "block128"])
@pytest.mark.parametrize("C,K", R.GEOMETRY_CK)
@pytest.mark.parametrize("name", R.LAUNCH_SHAPES)
def test_launch_shapes_one_workgroup_walks_three_tiles(native, monkeypatch, name, C, K, block):
    got = {}
    for grid in (0, 1, 2):
        monkeypatch.setenv("TORCHFLOWS_AMD_DEBUG", f"glow_block={block},glow_grid={grid}")
        _, step = R.compile_step(R.make_case(name, C, K), 0, torch.device("cuda"))
        assert step.info["block"] == block and step.layer.grid == grid and step.info["tile_rows"] == 16
        got[grid] = _both(native, "c", name, C, K, tag=f" block={block} grid={grid or 'default'}")
    for grid in (1, 2):
        for a, b in zip(got[grid], got[0]):
            assert np.array_equal(a, b), f"grid {grid} and the default grid differ at block {block}"


# ---------------------------------------------------------------------------------------------------------------------
# (d) inverse targets the map cannot reach
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sign", [1.0, -1.0])
@pytest.mark.parametrize("C,K", R.UNREACHABLE_CK)
def test_unreachable_targets(native, C, K, sign):
    """z_in = +-20 on every target (tests/test_gpu_dsf_shapes.py::test_unreachable_targets).  The component inverted first
    cannot reach it and its search ends on the bracket's end; x sits there wherever the float64 rule ends there, is finite
    and inside the bracket everywhere, and the log-det is minus the float64 forward log-det where the searches ended.
    With two components the second search is asked for +-10, which a component whose slopes a = softplus(.) + 1e-3 are
    just above 1 reaches a little inside the bracket for most elements: in float64 43 to 91 of the 666 elements end on
    the bracket's end, and those are the ones held to it."""
    case = R.make_case(R.EVERY, C, K)
    c, tr = case.cols, R.coupling_of(case.module).transformer
    rows_in = case.x.reshape(R.N_ROWS, -1).numpy().copy()
    rows_in[:, c] = 20.0 * sign
    h64 = R.conditioner_output(case, rows_in, torch.float64).reshape(R.N_ROWS, case.T, -1)
    h32 = R.conditioner_output(case, rows_in, torch.float32).reshape(R.N_ROWS, case.T, -1)
    x64, _ = DR.inverse64(tr, rows_in[:, c], h64)
    at_end = np.abs(x64 - 10.0 * sign) <= 1e-4
    assert at_end.all() if C == 1 else at_end.any()
    out, ld = _launch(native, case, 1, rows_in)
    x = out[:, c]
    assert np.isfinite(x).all() and np.isfinite(ld).all() and float(np.abs(x).max()) <= 10.0
    worst = float(np.abs(x - 10.0 * sign)[at_end].max())
    print(f"(d) C{C}_K{K} z_in = {20.0 * sign:+g}: |x - ({10.0 * sign:+g})| <= {worst:.2e} on {int(at_end.sum())} of {at_end.size} elements")
    assert worst <= 1e-4
    shaped = lambda a: a.reshape(R.N_ROWS, *tr.event_shape, *a.shape[2:])      # (the transformer's own event shape)
    mids = [shaped(x)] + [shaped(np.full_like(x, 10.0 * sign))] * (C - 1)
    want64 = DR.inverse_log_det_at(tr, mids, shaped(h64), torch.float64)
    want32 = DR.inverse_log_det_at(tr, mids, shaped(h32), torch.float32)
    assert _held("d", f"C{C}_K{K} z_in = {20.0 * sign:+g} log-det where the searches ended", rel(ld, want64), rel(want32, want64))


# ---------------------------------------------------------------------------------------------------------------------
# (e) round trip: the forward launch, then the inverse launch on what it wrote
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C,K", R.GEOMETRY_CK)
@pytest.mark.parametrize("name", R.GEOMETRY_SHAPES)
def test_round_trip(native, name, C, K):
    case, ref = R.make_case(name, C, K), R.reference(name, C, K)
    c = case.cols
    x0 = case.x.reshape(R.N_ROWS, -1).numpy()
    z, ld_f = _launch(native, case, 0, x0)
    back, ld_i = _launch(native, case, 1, z.astype(np.float32))
    keep = R.keep_mask(case, ref, R.N_ROWS)
    floor = normwise(ref.z32[:, c], ref.z64[:, c])
    cancel = rel(-ld_i, ld_f)
    ok = _held("e", f"{name} C{C}_K{K} round trip", normwise(back[:, c][keep], x0[:, c][keep]), floor)
    # both log-dets are the same sum at the same points up to the round trip's error: they cancel at the forward's bar
    ok &= _held("e", f"{name} C{C}_K{K} log-dets cancel", cancel, rel(ref.ld32, ref.ld64))
    assert ok


# ---------------------------------------------------------------------------------------------------------------------
# (f) the reference's own recording of a deep sigmoidal image model: T = 8, K = 4, the one-pass kernel
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", ["fresh", "init"])
def test_reference_recording_1x4x4(native, variant, monkeypatch):
    import torchflows_amd as tfa
    from conftest import load_golden, state_dict_of
    from torchflows_amd import image_program
    from torchflows_amd.fused import NativeRouteWarning
    monkeypatch.setenv("TORCHFLOWS_AMD_DEBUG", "glow_dsf=program")
    fx = load_golden("flow_dsglow_1x4x4.npz")
    flow = tfa.Flow(tfa.DeepSigmoidGlow((1, 4, 4), n_layers=1))
    sd = {k: torch.from_numpy(v) for k, v in state_dict_of(fx, variant).items()}
    assert list(flow.state_dict()) == list(sd)
    flow.load_state_dict(sd, strict=True)
    flow = flow.eval().cuda()
    g = lambda k: fx[f"{variant}/{k}"]
    xg, zg = torch.from_numpy(fx["x"]).cuda(), torch.from_numpy(fx["z_in"]).cuda()
    with warnings.catch_warnings(record=True) as caught, torch.no_grad():
        warnings.simplefilter("always")
        progs = [image_program.get_program(flow.bijection, d, xg.device) for d in (0, 1)]
        assert all(p is not None and any(s.info["kind"] == "dsf" for s in p.steps) for p in progs)
        assert all(s.layer.hw == 4 for p in progs for s in p.steps if s.info["kind"] == "dsf")
        before = native.calls
        z, ld = flow.bijection.forward(xg)
        assert native.calls - before == len(progs[0].steps) + (progs[0].flush is not None)
        before = native.calls
        lp = flow.log_prob(xg)
        assert native.calls - before == len(progs[0].steps) + 1
        before = native.calls
        xi, ldi = flow.bijection.inverse(zg)
        assert native.calls - before == len(progs[1].steps) + (progs[1].flush is not None)
        torch.cuda.synchronize()
    assert not [w for w in caught if issubclass(w.category, NativeRouteWarning)]
    keep = np.abs(g("x_inv64")) < 9.99
    assert keep.mean() >= 0.95
    ok = True
    for got, key, dist in ((z, "z", normwise), (ld, "log_det", rel), (lp, "log_prob", rel), (ldi, "log_det_inv", rel)):
        ok &= _held("f", f"{variant} {key}", dist(got.cpu().numpy(), g(key)), dist(g(key), g(key + "64")))
    ok &= _held("f", f"{variant} x_inv", normwise(xi.cpu().numpy()[keep], g("x_inv")[keep]),
                normwise(g("x_inv")[keep], g("x_inv64")[keep]))
    assert ok


# ---------------------------------------------------------------------------------------------------------------------
# (g) refusals: argument errors only, nothing is launched
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("what,change,match", [
    ("block512", dict(block=512), "at most 256"),
    ("K17", dict(hw=17, n_params=18 * 3 * 17 * 2), "tfk_dsf_supported"),
    ("C3_K9", dict(n_ch=3, hw=9, n_params=18 * 3 * 9 * 3), "tfk_dsf_supported"),
])
def test_refusals(native, monkeypatch, what, change, match):
    from torchflows_amd import image_program
    case = R.make_case(R.EVERY, 2, 4)
    dev = torch.device("cuda")
    _, step = R.compile_step(case, 0, dev)
    bad = type(step.layer).from_buffer_copy(step.layer)   # (a copy of the fields, the same device tables)
    assert bad.kind == 3 and bad.T == 18
    for k, v in change.items():
        setattr(bad, k, v)
    with pytest.raises(native.NativeError, match=match):
        native.glow_plan(bad, case.D)
    rows = case.x.reshape(R.N_ROWS, -1).cuda()
    logdet = torch.full((R.N_ROWS,), CANARY).cuda()
    kept = rows.clone()
    with pytest.raises(native.NativeError, match=match) as refused:
        native.glow_coupling(rows, logdet, bad, inverse=False)
    # (native.calls counts entry points invoked, refused ones too; that the refusal came from the argument check of the
    # entry point, which precedes its launch, is what the message says)
    assert "tfk_glow_coupling failed" in str(refused.value)
    torch.cuda.synchronize()
    assert torch.equal(rows, kept) and float(logdet.min()) == CANARY == float(logdet.max()), "a refused launch wrote"
    if what == "block512":                               # the compiler's route to the same refusal: no program
        monkeypatch.setenv("TORCHFLOWS_AMD_DEBUG", "glow_block=512")
        assert image_program.compile_program(case.module, 0, dev) is None
