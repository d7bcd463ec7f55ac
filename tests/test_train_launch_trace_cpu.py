"""The launch sequence of a training step, pinned on the host (no GPU needed).

Every kernel entry point of ``torchflows_amd.native`` that ``torchflows_amd/autograd.py`` calls is replaced by a stub that
launches nothing and appends to a trace: the entry point's name and, per argument of its signature (defaults included),
a tensor's shape, dtype, storage offset and the earlier tensor argument of the same call it aliases (an in-place launch),
or the scalar / flag / op tuple itself.  ``ChainFunction`` runs end to end on CPU tensors with those stubs -- libtfk's
``*_supported`` / ``*_floats`` host functions answer here --, forward and backward, and the trace of every route is
compared with ``tests/golden/train_launch_trace.json``, recorded once (``tests/golden/make_golden_train_launch_trace.py``).
The kernels' outputs are never written, so what the rows hold is arbitrary: only what is launched, with which operands, in
which order, and which gradients come back, is pinned -- not a number."""
import inspect
import json
import os

import pytest
import torch

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "train_launch_trace.json")
N = 5

ENTRY_POINTS = ("permute", "elementwise_affine", "affine_coupling", "shift_coupling", "rqs_coupling", "lrs_coupling",
                "conv1x1_coupling", "flow_run_mfma", "flow_run_wide", "affine_coupling_bwd", "shift_coupling_bwd",
                "rqs_coupling_bwd", "lrs_coupling_bwd", "conv1x1_coupling_bwd", "elementwise_affine_bwd",
                "affine_coupling_train_bwd", "rqs_coupling_train_bwd", "wide_coupling_train_bwd", "rows_outer")


def _describe(v, earlier, name=None):
    if isinstance(v, torch.Tensor):
        d = {"shape": list(v.shape), "dtype": str(v.dtype).replace("torch.", "")}
        if v.storage_offset():
            d["offset"] = int(v.storage_offset())
        if not v.is_contiguous():
            d["stride"] = list(v.stride())
        if v.numel():
            for other, t in earlier:
                if t.data_ptr() == v.data_ptr():
                    d["alias"] = other
                    break
            earlier.append((name, v))
        return d
    if isinstance(v, (list, tuple)):
        return [_describe(e, earlier) for e in v]
    if v is None or isinstance(v, (bool, int, float, str)):
        return v
    return float(v) if hasattr(v, "__float__") else repr(type(v))


def install_stubs(setattr_, trace):
    """Replace the entry points (``setattr_(module, name, stub)``: monkeypatch.setattr in the test)."""
    from torchflows_amd import native

    def stub_of(name, real):
        sig = inspect.signature(real)

        def stub(*args, **kwargs):
            bound = sig.bind(*args, **kwargs)
            bound.apply_defaults()
            earlier, rec = [], {}
            for k, v in bound.arguments.items():
                rec[k] = _describe(v, earlier, k)
            trace.append([name, rec])
            if name == "elementwise_affine_bwd":
                a = bound.arguments
                if a["out"] is not None:
                    return a["out"]
                return torch.zeros_like(a["value"]) if a["want_param"] else None
            return None
        return stub
    for name in ENTRY_POINTS:
        setattr_(native, name, stub_of(name, getattr(native, name)))


# name -> (architecture or "conv1x1", event size, constructor keywords, options)
# options: init (ActNorm initialised beforehand), flat (parameters in one buffer), inverse (the inverse plan), context,
#          l2 (the L2 penalty inside the node), debug (TORCHFLOWS_AMD_DEBUG switches)
CASES = {
    "realnvp64": ("RealNVP", 64, {}, dict(init=True)),
    "realnvp64_first_batch": ("RealNVP", 64, {}, dict(init=False)),
    "realnvp64_flat": ("RealNVP", 64, {}, dict(init=True, flat=True)),
    "realnvp64_flat_l2": ("RealNVP", 64, {}, dict(init=True, flat=True, l2=True)),
    "realnvp128": ("RealNVP", 128, {}, dict(init=True)),
    "realnvp256": ("RealNVP", 256, {}, dict(init=True)),
    "nice10_padded": ("NICE", 10, {}, dict(init=True)),
    "realnvp7_odd": ("RealNVP", 7, {}, dict(init=True)),
    "rqnsf64": ("CouplingRQNSF", 64, {}, dict(init=True)),
    "rqnsf64_flat": ("CouplingRQNSF", 64, {}, dict(init=True, flat=True)),
    "rqnsf64_no_rows_outer": ("CouplingRQNSF", 64, {}, dict(init=True, debug=dict(rows_outer=0))),
    "rqnsf16_padded": ("CouplingRQNSF", 16, {}, dict(init=True)),
    "realnvp264_wide": ("RealNVP", 264, {}, dict(init=True)),
    "realnvp264_wide_inverse": ("RealNVP", 264, {}, dict(init=True, inverse=True)),
    "nice264_wide": ("NICE", 264, {}, dict(init=True)),
    "nice64_layerwise": ("NICE", 64, {}, dict(init=True, debug=dict(train_fused=0))),
    "realnvp200": ("RealNVP", 200, {}, dict(init=True)),
    "lrs16": ("CouplingLRS", 16, {}, dict(init=True)),
    "maf_rqnsf16": ("MaskedAutoregressiveRQNSF", 16, {}, dict(init=True)),
    "iaf16_inverse": ("IAF", 16, {}, dict(init=True, inverse=True)),
    "realnvp6_context": ("RealNVP", 6, dict(context_shape=(3,)), dict(init=True, context=True)),
    "conv1x1": ("conv1x1", (4, 4, 4), {}, dict(init=False)),
}


def _debug_env(switches):
    return ",".join(f"{k}={v}" for k, v in switches.items())


def record(name, setattr_, setenv):
    """The trace of one case: [[entry point, {argument: description}], ..., ["result", {...}]]."""
    import torchflows_amd as tfa
    from torchflows_amd import autograd as ag, native
    from torchflows_amd.bijections.base import BijectiveComposition
    from torchflows_amd.bijections.finite.autoregressive import architectures as A
    from torchflows_amd.utils import make_adamw
    arch, D, kw, opt = CASES[name]
    debug = dict(opt.get("debug", {}))
    if opt.get("flat"):
        debug["flat_adamw"] = 1                 # FlatAdamW on the host as well
    setenv("TORCHFLOWS_AMD_DEBUG", _debug_env(debug))
    event = (D,) if isinstance(D, int) else tuple(D)
    torch.manual_seed(5)
    if arch == "conv1x1":
        from torchflows_amd.bijections.finite.multiscale import Invertible1x1ConvolutionalCoupling
        b = BijectiveComposition([Invertible1x1ConvolutionalCoupling(event)])
        flow = b
    else:
        flow = tfa.Flow(getattr(A, arch)(D, n_layers=2, **kw))
        b = flow.bijection
    flow.train()
    ctx_rows = torch.randn(N, 3) if opt.get("context") else None
    if opt.get("init"):
        with torch.no_grad():                   # ActNorm's data-dependent initialisation, on the ATen composite path
            flow.log_prob(torch.randn(N, *event) * 1.5 + 0.3, context=ctx_rows)
    optim = make_adamw(flow.parameters(), lr=1e-3) if opt.get("flat") else None
    plan = ag.training_plan(b, ag.INVERSE if opt.get("inverse") else ag.FORWARD)
    assert plan is not None, name
    if opt.get("l2"):
        assert b._request_l2()
        plan.l2 = b.__dict__.pop("_tfk_l2_request")
    trace = []
    install_stubs(setattr_, trace)
    x = torch.randn(N, *event).requires_grad_(True)
    z, ld = ag.run(b, plan, x, ctx_rows)
    loss = z.sum() + ld.sum()
    reg = None
    if opt.get("l2"):
        reg = b.__dict__.pop("_tfk_l2_out")
        assert reg is not None                  # ChainFunction returned three outputs
        loss = loss + reg
    n_forward = len(trace)
    params = [p for layer, _, kind in plan for p in ag._layer_params(layer, kind)]
    loss.backward()
    result = {"forward_launches": n_forward, "z": list(z.shape), "logdet": list(ld.shape),
              "l2_output": None if reg is None else list(reg.shape),
              "input_grad": None if x.grad is None else list(x.grad.shape),
              "param_grads": [None if p.grad is None else list(p.grad.shape) for p in params]}
    if optim is not None:
        G = optim.flat.last_grad
        result["last_grad"] = None if G is None else list(G.shape)
        result["grads_are_flat"] = optim.flat.grads_are_flat() is not None
    trace.append(["result", result])
    return json.loads(json.dumps(trace))        # (tuples -> lists, as the fixture holds them)


@pytest.fixture(scope="module")
def golden():
    with open(FIXTURE) as f:
        return json.load(f)


def test_every_case_is_in_the_fixture(golden):
    assert sorted(golden) == sorted(CASES)


@pytest.mark.parametrize("name", sorted(CASES))
def test_launch_trace(name, golden, monkeypatch):
    got = record(name, monkeypatch.setattr, monkeypatch.setenv)
    want = golden[name]
    assert [e[0] for e in got] == [e[0] for e in want]                  # the sequence of entry points first
    for k, (g, w) in enumerate(zip(got, want)):
        assert g == w, f"{name}: call {k} ({g[0]})"


def _calls(trace, entry):
    return [rec for n, rec in trace if n == entry]


def test_cases_take_their_routes(golden):
    """What each case is in the list for, read off the recorded traces."""
    fused64 = _calls(golden["realnvp64"], "flow_run_mfma")
    assert len(fused64) == 2 and all(len(c["ops"]) == 2 for c in fused64)              # the ActNorm rides along
    assert fused64[0]["reverse_out"] and len(_calls(golden["realnvp64"], "permute")) == 2   # the reversal between them too
    first = golden["realnvp64_first_batch"]
    assert all(len(c["ops"]) == 1 for c in _calls(first, "flow_run_mfma"))             # fold=False
    assert len(_calls(first, "elementwise_affine")) > len(_calls(golden["realnvp64"], "elementwise_affine"))
    for case in ("realnvp64_flat", "realnvp64_flat_l2", "rqnsf64_flat"):               # the one-buffer route
        wanted = [c for c in _calls(golden[case], "elementwise_affine_bwd") if c["want_param"]]
        assert wanted and all(isinstance(c["out"], dict) for c in wanted)              # slices of the one gradient buffer
        assert golden[case][-1][1]["grads_are_flat"]
    assert all(c["out"] is None for c in _calls(golden["realnvp64"], "elementwise_affine_bwd"))
    assert golden["realnvp64_flat_l2"][-1][1]["l2_output"] == []
    assert all(c["x"]["shape"] == [N, 64] for c in _calls(golden["nice10_padded"], "flow_run_mfma"))
    assert any(isinstance(c["perm"], dict) for c in _calls(golden["realnvp7_odd"], "permute"))   # rev_index gathers
    assert all(not c["reverse_out"] for c in _calls(golden["realnvp7_odd"], "flow_run_mfma"))
    assert _calls(golden["rqnsf64"], "rqs_coupling_train_bwd") and _calls(golden["rqnsf64"], "rows_outer")
    assert all(c["hid_perm"] is None for c in _calls(golden["rqnsf64_no_rows_outer"], "rqs_coupling_train_bwd"))
    assert not _calls(golden["rqnsf64_no_rows_outer"], "rows_outer")
    assert all(c["x"]["shape"] == [N, 64] for c in _calls(golden["rqnsf16_padded"], "rqs_coupling_train_bwd"))
    for case in ("realnvp264_wide", "realnvp264_wide_inverse", "nice264_wide"):
        assert len(_calls(golden[case], "flow_run_wide")) == 2 == len(_calls(golden[case], "wide_coupling_train_bwd"))
        assert len(_calls(golden[case], "rows_outer")) == 6
    assert _calls(golden["nice64_layerwise"], "shift_coupling_bwd") and not _calls(golden["nice64_layerwise"], "flow_run_mfma")
    assert _calls(golden["realnvp200"], "affine_coupling_bwd")
    assert _calls(golden["lrs16"], "lrs_coupling_bwd")
    assert all(c["inverse"] is False for c in _calls(golden["maf_rqnsf16"], "rqs_coupling_bwd"))
    assert _calls(golden["iaf16_inverse"], "affine_coupling_bwd")
    assert _calls(golden["realnvp6_context"], "affine_coupling_bwd")
    assert _calls(golden["conv1x1"], "conv1x1_coupling") and _calls(golden["conv1x1"], "conv1x1_coupling_bwd")
