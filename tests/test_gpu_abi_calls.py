"""What crosses the C-ABI, call by call: every public launching wrapper of ``torchflows_amd.native`` driven once per
branch at the smallest shapes its checks accept, against ``tests/golden/abi_calls.json``.

For the test's duration ``native._lib`` is a recording stand-in around the real library: an entry point whose prototype
in include/tfk.h ends in ``void *stream`` is recorded and answers 0 WITHOUT being called -- no libtfk kernel is launched --,
every other function (``*_supported``, ``*_bytes``, ``*_floats``, ``tfk_glow_plan``, ``tfk_last_error`` ...) goes through.
The tensors live on the HIP device because ``native._ptr`` rejects host tensors; they are never read or written.

Per launch the fixture holds the symbol, every integer / float argument verbatim, ctypes arrays as lists, structures
field by field, and every pointer as ``null``, ``<argument name>+<byte offset>`` when it falls inside a tensor the case
passed in, or ``fresh#k+<byte offset>`` (k: order of first appearance within the launch, offset from the start of the
allocation) otherwise; whether the stream argument is the current raw stream; and per case the change of
``native.calls``.  Which entry points take a stream and which arguments are pointers is read from the header's text
(tests/tfk_header.py), not from the binding under test.

The fixture is regenerated only when the ABI or a wrapper's contract changes on purpose:
``python tests/test_gpu_abi_calls.py <output.json>`` on a GPU machine."""
import ctypes as C
import json
import os
import sys
import types

import pytest
import torch

import tfk_header

pytestmark = pytest.mark.gpu

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "abi_calls.json")
DEV = "cuda"
N, D, T = 3, 4, 2


def _current_raw_stream() -> int:
    return int(torch._C._cuda_getCurrentRawStream(torch.cuda.current_device()))


def _allocations():
    """(start, size) of every live block of the caching allocator."""
    out = []
    for seg in torch.cuda.memory_snapshot():
        addr = seg["address"]
        for b in seg["blocks"]:
            if b["state"] == "active_allocated":
                out.append((addr, b["size"]))
            addr += b["size"]
    return out


class Recorder:
    """Stands in for the loaded library (``native._lib``).  ``quiet``: the launching entry points only answer 0
    (tools/abi_host_cost.py times the wrappers this way, so that rendering is not in its numbers)."""

    def __init__(self, real, quiet: bool = False):
        self._real = real
        self._protos = tfk_header.prototypes()
        self._quiet = quiet
        self.named = {}
        self.launches = []

    def __getattr__(self, name):
        fn = getattr(self._real, name)
        proto = self._protos.get(name)
        if proto is not None and tfk_header.takes_stream(proto):
            if self._quiet:
                def fn(*args):
                    return 0
            else:
                def fn(*args, _name=name, _params=proto[1]):
                    self.launches.append(self._render(_name, _params, args))
                    return 0
        self.__dict__[name] = fn
        return fn

    # -- rendering -----------------------------------------------------------------------------------------------
    def _pointer(self, p, fresh) -> str:
        p = getattr(p, "value", p)
        if not p:
            return "null"
        for name, t in self.named.items():
            base = t.data_ptr()
            if base <= p < base + max(t.numel() * t.element_size(), 1):
                return f"{name}+{p - base}"
        base = p
        for start, size in fresh["allocations"]:
            if start <= p < start + size:
                base = start
                break
        if base not in fresh["bases"]:
            fresh["bases"].append(base)
        return f"fresh#{fresh['bases'].index(base)}+{p - base}"

    def _field(self, ftype, v, fresh):
        if issubclass(ftype, C.Structure):
            return {n: self._field(t, getattr(v, n), fresh) for n, t in ftype._fields_}
        if issubclass(ftype, C.Array):
            return [self._field(ftype._type_, v[k], fresh) for k in range(len(v))]
        if ftype is C.c_void_p:
            return self._pointer(v, fresh)
        return v

    def _render(self, name, params, args):
        assert len(args) == len(params), f"{name}: {len(args)} arguments for {len(params)} parameters"
        fresh = {"bases": [], "allocations": _allocations()}
        out = []
        for (cls, _), a in zip(params[:-1], args[:-1]):
            if cls.startswith("ptr"):
                if isinstance(a, C.Array):
                    out.append({"array": list(a)})
                elif hasattr(a, "_obj"):                      # ctypes.byref(structure)
                    out.append({"struct": self._field(type(a._obj), a._obj, fresh)})
                else:
                    out.append(self._pointer(a, fresh))
            else:
                v = getattr(a, "value", a)                    # c_float(...) -> its fp32 value; Python numbers as they are
                assert isinstance(v, (bool, int, float)), f"{name}: {type(a).__name__} for a {cls} parameter"
                out.append(v)
        stream = getattr(args[-1], "value", args[-1]) or 0
        return {"symbol": name, "args": out, "stream_is_current": stream == _current_raw_stream()}


def _collect(name, v, named):
    if isinstance(v, torch.Tensor):
        named[name] = v
    elif isinstance(v, (list, tuple)):
        for k, e in enumerate(v):
            _collect(f"{name}[{k}]", e, named)
    elif isinstance(v, torch.nn.Module):
        for k, t in list(v.named_parameters()) + list(v.named_buffers()):
            _collect(f"{name}.{k}", t, named)


def f(*shape):
    return torch.empty(*shape, dtype=torch.float32, device=DEV)


def i32(n):
    return torch.empty(n, dtype=torch.int32, device=DEV)


def u8(*shape):
    return torch.empty(*shape, dtype=torch.uint8, device=DEV)


def _bn(c, **kw):
    return torch.nn.BatchNorm2d(c, **kw).to(DEV)


def _transformer(kind):
    return types.SimpleNamespace(native_kind=kind, n_bins=8, boundary=5.0, n_components=2, hidden_dim=4, n_channels=2)


# parameters per target element (conv1x1: per sample) of the transformer above
_P = {"affine": 2, "inverse_affine": 2, "shift": 1, "rqs": 23, "lrs": 32, "dsf": 24}


def _h_for(kind, targets):
    return f(N, 4) if kind == "conv1x1" else f(N, targets, _P[kind])


def record_all():
    """[{case, calls, launches}] of every driven call, in a fixed order."""
    from torchflows_amd import autograd as ag, native
    from torchflows_amd.bijections.base import FORWARD, INVERSE, RowState
    from torchflows_amd.bijections.finite.autoregressive.layers_base import (CouplingBijection,
                                                                              MaskedAutoregressiveBijection)
    real = native.lib()
    rec = Recorder(real)
    out = []

    def case(label, fn, names=None, **kw):
        rec.named = {}
        for k, v in {**kw, **(names or {})}.items():
            _collect(k, v, rec.named)
        rec.launches = []
        before = native.calls
        fn(**kw)
        out.append({"case": label, "calls": native.calls - before, "launches": rec.launches})

    native._lib = rec
    try:
        x, z, ld, idx = f(N, D), f(N, D), f(N), i32(T)
        # ---- the coupling kernels, forward maps ----
        singles = [("affine_coupling", native.affine_coupling, 2, {}), ("shift_coupling", native.shift_coupling, 1, {})]
        for K in (4, 8):
            singles.append((f"rqs_coupling/K{K}", native.rqs_coupling, 3 * K - 1, dict(n_bins=K, boundary=5.0)))
            singles.append((f"lrs_coupling/K{K}", native.lrs_coupling, 4 * K, dict(n_bins=K, boundary=2.5)))
        for nc, hd in ((1, 1), (2, 4)):
            singles.append((f"dsf_coupling/{nc}x{hd}", native.dsf_coupling, 3 * nc * hd, dict(n_components=nc, hidden_dim=hd)))
        for label, fn, P, extra in singles:
            h = f(N, T, P)
            for inverse in (False, True):
                case(f"{label}/inverse={inverse}/tail", fn, x=x, h=h, out=z, logdet=ld, tgt_idx=None, T=T, inverse=inverse, **extra)
                case(f"{label}/inverse={inverse}/idx+acc", fn, x=x, h=h, out=x, logdet=ld, tgt_idx=idx, T=T, accumulate=True,
                     inverse=inverse, **extra)
        case("shift_coupling/no_logdet", native.shift_coupling, x=x, h=f(N, T, 1), out=z, logdet=None, tgt_idx=None, T=T,
             accumulate=True)
        for inverse in (False, True):
            case(f"conv1x1_coupling/inverse={inverse}/tail", native.conv1x1_coupling, x=x, h=f(N, 4), out=z, logdet=ld,
                 tgt_idx=None, T=T, n_channels=2, inverse=inverse)
            case(f"conv1x1_coupling/inverse={inverse}/idx+acc", native.conv1x1_coupling, x=x, h=f(N, 4), out=z, logdet=ld,
                 tgt_idx=idx, T=T, n_channels=2, accumulate=True, inverse=inverse)
        # ---- elementwise, permutation, base density ----
        value = f(D, 2)
        for inverse_affine in (False, True):
            for inverse in (False, True):
                case(f"elementwise_affine/ia={inverse_affine}/inverse={inverse}", native.elementwise_affine, x=x, value=value,
                     out=z, logdet=ld, inverse_affine=inverse_affine, accumulate=inverse, inverse=inverse)
        case("permute/reversal", native.permute, x=x, perm=None, out=z)
        case("permute/perm", native.permute, x=x, perm=i32(D), out=z)
        loc, log_scale, lp = f(D), f(D), f(N)
        case("diag_gauss_logprob/no_logdet", native.diag_gauss_logprob, z=z, loc=loc, log_scale=log_scale, logdet_in=None, out=lp)
        case("diag_gauss_logprob/logdet", native.diag_gauss_logprob, z=z, loc=loc, log_scale=log_scale, logdet_in=ld, out=lp)
        # ---- reverse mode ----
        g, gld = f(N, D), f(N)
        bwds = [("affine_coupling_bwd", native.affine_coupling_bwd, 2 * T, {}),
                ("conv1x1_coupling_bwd", native.conv1x1_coupling_bwd, 4, dict(n_channels=2))]
        for K in (4, 8):
            bwds.append((f"rqs_coupling_bwd/K{K}", native.rqs_coupling_bwd, T * (3 * K - 1), dict(n_bins=K, boundary=5.0)))
            bwds.append((f"lrs_coupling_bwd/K{K}", native.lrs_coupling_bwd, T * 4 * K, dict(n_bins=K, boundary=2.5)))
        for nc, hd in ((1, 1), (2, 4)):
            bwds.append((f"dsf_coupling_bwd/{nc}x{hd}", native.dsf_coupling_bwd, T * 3 * nc * hd, dict(n_components=nc, hidden_dim=hd)))
        for label, fn, per_row, extra in bwds:
            h, gh = f(N, per_row), f(N, per_row)
            case(f"{label}/tail", fn, x=x, h=h, g=g, gld=gld, gh=gh, tgt_idx=None, T=T, **extra)
            case(f"{label}/idx+inverse", fn, x=x, h=h, g=g, gld=gld, gh=gh, tgt_idx=idx, T=T, inverse=True, **extra)
        case("affine_coupling_bwd/no_gld", native.affine_coupling_bwd, x=x, h=f(N, T, 2), g=g, gld=None, gh=f(N, T, 2), tgt_idx=None, T=T)
        case("shift_coupling_bwd/tail", native.shift_coupling_bwd, g=g, gh=f(N, T), tgt_idx=None, T=T)
        case("shift_coupling_bwd/idx+inverse", native.shift_coupling_bwd, g=g, gh=f(N, T), tgt_idx=idx, T=T, inverse=True)
        case("elementwise_affine_bwd/rows_only", native.elementwise_affine_bwd, x=x, value=value, g=g, gld=gld, want_param=False)
        case("elementwise_affine_bwd/rows_only+inverse", native.elementwise_affine_bwd, x=None, value=value, g=g, gld=None,
             want_param=False, inverse=True)
        case("elementwise_affine_bwd/param", native.elementwise_affine_bwd, x=x, value=value, g=g, gld=gld, want_param=True)
        case("elementwise_affine_bwd/param+out", native.elementwise_affine_bwd, x=x, value=value, g=g, gld=gld, want_param=True,
             inverse=True, out=f(2 * D))
        case("diag_gauss_logprob_bwd", native.diag_gauss_logprob_bwd, z=z, loc=loc, log_scale=log_scale, glp=lp, g=g)
        # ---- fused training launches (D = 64), their weight-gradient contraction, the wide ones (D = 264) ----
        x64, g64, params = f(N, 64), f(N, 64), f(1024)
        acc = f(int(real.tfk_coupling_train_bwd_out_floats(64)))
        ws = f(max(int(real.tfk_coupling_train_bwd_workspace_bytes(64)) // 4, 1))
        case("affine_coupling_train_bwd", native.affine_coupling_train_bwd, x=x64, g=g64, gld=gld, params=params, gemm2_steps=2,
             out=acc, workspace=ws)
        case("affine_coupling_train_bwd/inverse+gscale+reversed", native.affine_coupling_train_bwd, x=x64, g=g64, gld=gld,
             params=params, gemm2_steps=3, out=acc, workspace=ws, inverse_form=True, gscale=f(64), g_reversed=True)
        gh_perm, gpre_perm = f(N, 768), f(N, 16)
        case("rqs_coupling_train_bwd", native.rqs_coupling_train_bwd, x=x64, g=g64, gld=gld, params=params, gemm2_steps=2,
             gh_perm=gh_perm, gpre_perm=gpre_perm, n_bins=8, boundary=5.0)
        case("rqs_coupling_train_bwd/inverse+gscale+reversed", native.rqs_coupling_train_bwd, x=x64, g=g64, gld=gld, params=params,
             gemm2_steps=4, gh_perm=gh_perm, gpre_perm=gpre_perm, n_bins=8, boundary=2.5, inverse=True, gscale=f(64), g_reversed=True)
        case("rqs_coupling_train_bwd/hid", native.rqs_coupling_train_bwd, x=x64, g=g64, gld=gld, params=params, gemm2_steps=2,
             gh_perm=gh_perm, gpre_perm=gpre_perm, n_bins=8, boundary=5.0, hid_perm=f(N, 16))
        case("rows_outer", native.rows_outer, A=f(N, 768), M=768, B=f(N, 16), out=f(768 * 16))
        case("rows_outer/narrow", native.rows_outer, A=f(N, 16), M=8, B=f(N, 16), out=f(8 * 16))
        x264, g264, hp = f(N, 264), f(N, 264), 192
        case("wide_coupling_train_bwd/affine", native.wide_coupling_train_bwd, x=x264, g=g264, gld=gld, params=params,
             gh_rec=f(N, 2 * hp), gpre_rec=f(N, 16), hid_rec=f(N, 16))
        case("wide_coupling_train_bwd/shift+gscale+reversed", native.wide_coupling_train_bwd, x=x264, g=g264, gld=gld, params=params,
             gh_rec=f(N + 2, hp), gpre_rec=f(N, 16), hid_rec=f(N, 16), shift=True, gscale=f(264), g_reversed=True)
        case("wide_coupling_train_bwd/inverse_form", native.wide_coupling_train_bwd, x=x264, g=g264, gld=gld, params=params,
             gh_rec=f(N, 2 * hp), gpre_rec=f(N, 16), hid_rec=f(N, 16), inverse_form=True)
        # ---- MADE sequential maps ----
        HP = 8
        made = dict(z=x, out=z, logdet=ld, W1t=f(D, HP), b1=f(HP))
        case("made_affine_sequential/divide", native.made_affine_sequential, **made, W2=f(D, 2, HP), b2=f(D, 2), divide=True)
        case("made_affine_sequential/multiply+acc", native.made_affine_sequential, **made, W2=f(D, 2, HP), b2=f(D, 2), divide=False,
             accumulate=True)
        case("made_rqs_sequential/rqs", native.made_rqs_sequential, **made, W2=f(D, 23, HP), b2=f(D, 23), n_bins=8, boundary=5.0)
        case("made_rqs_sequential/lrs+acc", native.made_rqs_sequential, **made, W2=f(D, 32, HP), b2=f(D, 32), n_bins=8, boundary=2.5,
             accumulate=True, lrs=True)
        # ---- the ConvNet conditioner: inference pieces, per-layer training launches, whole-network calls ----
        img, w3 = f(N, 4, 4, 4), f(8, 4, 3, 3)
        case("conv3x3_relu_pool_affine", native.conv3x3_relu_pool_affine, x=img, weight=w3, bias=f(8), scale=f(8), shift=f(8))
        case("bounded_sigmoid", native.bounded_sigmoid, h=x, lo=-2.0, hi=2.0)
        case("bounded_sigmoid_bwd", native.bounded_sigmoid_bwd, out=x, g=g, lo=-2.0, hi=2.0)
        case("conv1x1_frame", native.conv1x1_frame, x=f(N, 4, 2, 2), weight=f(4, 4), bias=f(4), h_out=4, w_out=6)
        wide_rows = f(N, 20)
        case("conv1x1_frame/view", native.conv1x1_frame, names=dict(rows=wide_rows), x=wide_rows[:, 4:].unflatten(1, (4, 2, 2)),
             weight=f(1, 4, 1, 1), bias=f(1), h_out=2, w_out=2)
        bn8 = _bn(8)
        case("convnet_train_block_fwd/train", native.convnet_train_block_fwd, x=img, in_affine=None, weight=w3, bias=f(8), bn=bn8,
             training=True, update_running=True)
        bn_plain = _bn(8, momentum=None)
        bn_plain.num_batches_tracked = None
        case("convnet_train_block_fwd/eval+affine", native.convnet_train_block_fwd, x=img, in_affine=f(8), weight=w3, bias=f(8),
             bn=bn_plain, training=False, update_running=False)
        blk = dict(gz=f(N, 8, 2, 2), coef=f(24), y=f(N, 8, 2, 2), amax=u8(N, 8, 2, 2), x=img, weight=w3)
        case("convnet_train_block_bwd/first", native.convnet_train_block_bwd, **blk, in_affine=None, bn_stats=None, bn_training=False)
        case("convnet_train_block_bwd/behind_bn", native.convnet_train_block_bwd, **blk, in_affine=f(8), bn_stats=f(16), bn_training=True)
        wm = f(4, 4, 2, 1)
        case("convnet_train_frame_fwd", native.convnet_train_frame_fwd, x=img, in_affine=None, weight=wm, bias=f(4), h_out=7, w_out=6)
        case("convnet_train_frame_fwd/affine", native.convnet_train_frame_fwd, x=img, in_affine=f(8), weight=wm, bias=f(4), h_out=7, w_out=6)
        case("convnet_train_frame_bwd/first", native.convnet_train_frame_bwd, g_out=f(N, 4, 7, 6), x=img, in_affine=None, weight=wm,
             bn_stats=None, bn_training=False)
        case("convnet_train_frame_bwd/behind_bn", native.convnet_train_frame_bwd, g_out=f(N, 4, 7, 6), x=img, in_affine=f(8), weight=wm,
             bn_stats=f(16), bn_training=True)
        M = 2
        case("convnet_train_linear_prep", native.convnet_train_linear_prep, weight=f(M, 100), bias=f(M), frame_bias=f(1), h_out=10, w_out=10)
        case("convnet_train_linear_fwd", native.convnet_train_linear_fwd, a16=f(N, 16), W16=f(M, 16), b_eff=f(M))
        case("convnet_train_linear_bwd_input", native.convnet_train_linear_bwd_input, g=f(N, M), W16=f(M, 16))
        case("convnet_train_linear_wgrad", native.convnet_train_linear_wgrad, g=f(N, M), a16=f(N, 16), frame_bias=f(1), h_out=10, w_out=10)
        net = [f(4, 1, 2, 1), f(4), f(8, 4, 3, 3), f(8), f(8), f(8), f(8, 8, 3, 3), f(8), f(8), f(8), f(4, 8, 3, 3), f(4), f(4), f(4),
               f(1, 4, 1, 1), f(1), f(M, 100), f(M)]
        bns = [_bn(8), _bn(8), _bn(4)]
        bns[1].num_batches_tracked = None
        plan, ximg = native.ConvNetTrainPlan(), f(N, 1, 7, 8)
        kept = []
        case("convnet_train_forward/train", lambda **kw: kept.append(native.convnet_train_forward(**kw)), plan=plan, params=net,
             bns=bns, x=ximg, training=True, update_running=True)
        case("convnet_train_backward/train", native.convnet_train_backward, names=dict(acts=kept[0][1], amax=kept[0][2]), plan=plan,
             x=ximg, g_theta=f(N, M), training=True)
        case("convnet_train_forward/eval", lambda **kw: kept.append(native.convnet_train_forward(**kw)), plan=plan, params=net,
             bns=bns, x=ximg, training=False, update_running=False)
        case("convnet_train_backward/eval", native.convnet_train_backward, names=dict(acts=kept[1][1], amax=kept[1][2]), plan=plan,
             x=ximg, g_theta=f(N, M), training=False)
        # ---- flow programs ----
        x16, ops = f(N, 16), [(2, 0, 4, 0), (0, 0, 0, 64)]
        prog = dict(gauss_loc=f(16), gauss_log_scale=f(16), ops=ops, params=f(128))
        case("flow_run/all_outputs", native.flow_run, x=x16, z=f(N, 16), logdet=ld, logprob=lp, **prog)
        case("flow_run/logprob_only+acc", native.flow_run, x=x16, z=None, logdet=None, logprob=lp, accumulate=True, **prog)
        rq = [(17, 0, 2, 0, 8 + 256, 5.0, 0.992, 0.5413), (16, 0, 0, 512)]
        prog = dict(gauss_loc=f(64), gauss_log_scale=f(64), params=f(1024))
        case("flow_run_mfma/plain", native.flow_run_mfma, x=x64, z=f(N, 64), logdet=ld, logprob=lp, ops=rq, **prog)
        case("flow_run_mfma/plain/flags", native.flow_run_mfma, x=x64, z=f(N, 64), logdet=ld, logprob=None, ops=rq,
             accumulate=True, reverse_out=True, base_of_input=True, D=64, **prog)
        case("flow_run_mfma/plain/packed_ops", native.flow_run_mfma, x=x64, z=f(N, 64), logdet=None, logprob=None,
             ops=native._pack_ops_uncached(rq), **prog)
        case("flow_run_mfma/in", native.flow_run_mfma, x=f(N, 10), z=f(N, 64), logdet=ld, logprob=lp, ops=rq, reverse_out=True, D=64, **prog)
        case("flow_run_mfma/ctx", native.flow_run_mfma, x=x64, z=f(N, 64), logdet=ld, logprob=lp, ops=rq, accumulate=True,
             context=f(N, 2), **prog)
        case("flow_run_mfma/sum", native.flow_run_mfma, x=f(N, 10), z=None, logdet=None, logprob=lp, ops=rq, D=64,
             sum_out=torch.empty(1, dtype=torch.float64, device=DEV), **prog)
        case("flow_run_mfma/sum/full_width", native.flow_run_mfma, x=x64, z=f(N, 64), logdet=ld, logprob=lp, ops=rq, base_of_input=True,
             sum_out=torch.empty(1, dtype=torch.float64, device=DEV), **prog)
        wide_ops = [(12, 0, 8, 0), (16, 0, 0, 4096)]
        prog = dict(gauss_loc=f(384), gauss_log_scale=f(384), ops=wide_ops, params=f(8192))
        case("flow_run_wide", native.flow_run_wide, x=x264, z=f(N, 264), logdet=ld, logprob=lp, **prog)
        case("flow_run_wide/flags", native.flow_run_wide, x=x264, z=None, logdet=None, logprob=lp, accumulate=True, reverse_out=True,
             base_of_input=True, **prog)
        # ---- image programs ----
        tables = dict(src_idx=i32(4), src_st=f(8), tgt_idx=i32(16), tgt_st=f(32), weights=f(64), bg1=f(8), bg2=f(8), w_eff=f(64), b_eff=f(4))
        layer = native.GlowLayer(kind=0, c_in=1, hi=2, wi=2, oy=15, ox=15, kh=1, kw=1, T=2, n_params=4, n_ch=0, hw=0, slots=1, block=256,
                                 cg1=2, cg2=4, grid=3, **{k: t.data_ptr() for k, t in tables.items()})
        for inverse in (False, True):
            case(f"glow_coupling/inverse={inverse}", native.glow_coupling, names=tables, rows=x, logdet=ld, layer=layer, inverse=inverse)
        blob_host, blob_dev = torch.empty(64, dtype=torch.uint8), u8(64)
        case("glow_level/whole_row", native.glow_level, rows_in=x, rows_out=z, logdet=ld, row_idx=None, blob_host=blob_host, blob_dev=blob_dev)
        case("glow_level/row_idx", native.glow_level, rows_in=x, rows_out=x, logdet=ld, row_idx=i32(2), blob_host=blob_host, blob_dev=blob_dev)
        st = f(D, 2)
        case("rows_fma", native.rows_fma, rows=x, st=st)
        case("rows_fma_gauss_logprob/no_logdet", native.rows_fma_gauss_logprob, rows=x, st=st, loc=loc, log_scale=log_scale, logdet_in=None, out=lp)
        case("rows_fma_gauss_logprob/logdet", native.rows_fma_gauss_logprob, rows=x, st=st, loc=loc, log_scale=log_scale, logdet_in=ld, out=lp)
        case("sum_f32/one_workgroup", native.sum_f32, values=f((1 << 14) - 1))
        case("sum_f32/workspace", native.sum_f32, values=f(1 << 7, 1 << 7))
        # ---- the transformer-kind routes: a coupling layer's native step, the MADE pass, the training chain's two hooks ----
        for kind in ("affine", "inverse_affine", "shift", "rqs", "lrs", "dsf", "conv1x1"):
            tr = _transformer(kind)
            h = _h_for(kind, T)
            for d, dname in ((FORWARD, "forward"), (INVERSE, "inverse")):
                for tail in (True, False):
                    layer_ = types.SimpleNamespace(
                        coupling=types.SimpleNamespace(source_event_size=D - T, target_event_size=T, constant_shape=(D - T,)),
                        _source_is_head=True, _source_index=None, context_shape=None, transformer=tr,
                        conditioner_transform=lambda x_a, context=None, h=h: h, _target_is_tail=tail, _target_index32=idx)
                    state = RowState(x, torch.Size([N]))
                    state.started = not tail
                    case(f"CouplingBijection._native_step/{kind}/{dname}/{'tail' if tail else 'idx+acc'}",
                         lambda: CouplingBijection._native_step(layer_, state, None, d), names=dict(rows=x, h=h, target_index=idx))
                hook = types.SimpleNamespace(transformer=tr)
                case(f"autograd._transform_forward/{kind}/{dname}", ag._transform_forward, layer=hook, d=d, x=x, h=h, out=z, logdet=ld,
                     tgt=idx if d == FORWARD else None, T=T, accumulate=(d == INVERSE))
                gh = torch.empty_like(h)
                case(f"autograd._transform_backward/{kind}/{dname}", ag._transform_backward, layer=hook, d=d, x_in=x, hc=h, g=g, gld=gld,
                     gh=gh, tgt=idx if d == FORWARD else None, T=T)
            if kind in ("shift", "conv1x1"):
                continue
            h = _h_for(kind, D)
            made_layer = types.SimpleNamespace(context_shape=None, event_shape=(D,), transformer=tr,
                                               conditioner_transform=lambda rows, ctx, h=h: h)
            for transformer_inverse in (False, True):
                case(f"MaskedAutoregressiveBijection._native_pass/{kind}/inverse={transformer_inverse}",
                     lambda: MaskedAutoregressiveBijection._native_pass(made_layer, x, z, ld, None, transformer_inverse,
                                                                        not transformer_inverse),
                     names=dict(rows=x, out=z, logdet=ld, h=h))
    finally:
        native._lib = real
    return json.loads(json.dumps(out))


@pytest.fixture(scope="module")
def golden():
    with open(FIXTURE) as fh:
        return json.load(fh)


@pytest.fixture(scope="module")
def recorded():
    return record_all()


def test_same_cases_in_the_same_order(golden, recorded):
    assert [e["case"] for e in recorded] == [e["case"] for e in golden]
    assert len({e["case"] for e in recorded}) == len(recorded)


def test_every_call_crosses_the_boundary_as_recorded(golden, recorded):
    for got, want in zip(recorded, golden):
        assert got == want, got["case"]
    assert len(recorded) == len(golden)


def test_every_launching_entry_point_is_driven(golden):
    """Each function of the header that takes a stream appears in the fixture (a new export needs a case here)."""
    launching = {n for n, p in tfk_header.prototypes().items() if tfk_header.takes_stream(p)}
    seen = {launch["symbol"] for e in golden for launch in e["launches"]}
    assert launching == seen, sorted(launching ^ seen)


if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    with open(sys.argv[1], "w") as fh:
        fh.write("[\n" + ",\n".join(json.dumps(e, sort_keys=True) for e in record_all()) + "\n]\n")
