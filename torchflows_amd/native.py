"""ctypes binding of libtfk.so (C-ABI declared in include/tfk.h).

PyTorch is used here only as plumbing: device memory (``tensor.data_ptr()``), the
current HIP stream and the device guard.  No torch types cross the boundary.

The product path never falls back: if the library is missing or a call fails the
error is raised (``NativeError``).  Nothing in this package imports ``oracle/``.
"""
from __future__ import annotations

import ctypes as C
import os
import struct
import subprocess
from operator import attrgetter
from typing import Callable, NamedTuple, Optional

import torch

_PKG = os.path.dirname(os.path.abspath(__file__))
# TORCHFLOWS_AMD_LIB: load another build of the same ABI (kernel experiments / ablations)
LIB_PATH = os.environ.get("TORCHFLOWS_AMD_LIB") or os.path.join(_PKG, "lib", "libtfk.so")
CSRC = os.path.join(_PKG, "csrc")

ABI_VERSION = 29


class NativeError(RuntimeError):
    """libtfk is missing, mismatched, or a kernel call was rejected."""


_vp = C.c_void_p
_i32 = C.c_int32
_i64 = C.c_int64


class GlowLayer(C.Structure):
    """``tfk_glow_layer`` of include/tfk.h: one convolutional coupling of an image flow, everything that does not
    depend on the sample prepared by the caller (torchflows_amd/image_program.py)."""
    _fields_ = [("kind", _i32), ("c_in", _i32), ("hi", _i32), ("wi", _i32), ("oy", _i32), ("ox", _i32),
                ("kh", _i32), ("kw", _i32), ("T", _i32), ("n_params", _i32), ("n_ch", _i32), ("hw", _i32),
                ("slots", _i32), ("block", _i32), ("cg1", _i32), ("cg2", _i32), ("grid", _i32),
                ("src_idx", _vp), ("src_st", _vp), ("tgt_idx", _vp), ("tgt_st", _vp),
                ("weights", _vp), ("bg1", _vp), ("bg2", _vp), ("w_eff", _vp), ("b_eff", _vp)]


class ConvNetTrainPlan(C.Structure):
    """``tfk_convnet_train_plan`` (include/tfk.h): the ConvNet conditioner's parameters and the activations its two passes
    share, as device pointers."""
    _fields_ = [("mod1_w", C.c_void_p), ("mod1_b", C.c_void_p),
                ("conv_w", C.c_void_p * 3), ("conv_b", C.c_void_p * 3),
                ("bn_w", C.c_void_p * 3), ("bn_b", C.c_void_p * 3),
                ("bn_mean", C.c_void_p * 3), ("bn_var", C.c_void_p * 3), ("bn_count", C.c_void_p * 3),
                ("bn_eps", C.c_float * 3), ("bn_momentum", C.c_float * 3),
                ("mod2_w", C.c_void_p), ("mod2_b", C.c_void_p), ("lin_w", C.c_void_p), ("lin_b", C.c_void_p),
                ("c", C.c_int32), ("h", C.c_int32), ("w", C.c_int32), ("kh", C.c_int32), ("kw", C.c_int32),
                ("M", C.c_int32),
                ("a0", C.c_void_p), ("y", C.c_void_p * 3), ("amax", C.c_void_p * 3), ("stats", C.c_void_p * 3),
                ("a16", C.c_void_p), ("lin_fold", C.c_void_p), ("workspace", C.c_void_p)]


class GlowLevelStep(C.Structure):
    """``tfk_glow_level_step`` of include/tfk.h: a coupling inside a level program (tfk_glow_level)."""
    _fields_ = [("layer", GlowLayer), ("inverse", _i32), ("reserved", _i32), ("src_loc", _vp), ("tgt_loc", _vp),
                ("w4", _vp), ("b4", _vp), ("weights_host", _vp)]


# The C-ABI, once: name -> (restype, argtypes) for every function include/tfk.h declares, in the header's order
# (tests/test_cabi_host.py holds each row to its prototype, parameter by parameter).  A signature the header repeats is
# one list here.
_int, _f, _pi = C.c_int, C.c_float, C.POINTER(_i32)
_coupling_t = [_vp, _vp, _vp, _vp, _i64, _i32, _vp, _i32, _i32, _vp]
_spline_t = [_vp, _vp, _vp, _vp, _i64, _i32, _vp, _i32, _i32, _f, _i32, _vp]
_spline_bwd_t = [_vp, _vp, _vp, _vp, _vp, _i64, _i32, _vp, _i32, _i32, _f, _i32, _vp]
_conv1x1_t = [_vp, _vp, _vp, _vp, _i64, _i32, _vp, _i32, _i32, _i32, _vp]
_dsf_t = [_vp, _vp, _vp, _vp, _i64, _i32, _vp, _i32, _i32, _i32, _i32, _vp]
_ew_t = [_vp, _vp, _vp, _vp, _i64, _i32, _i32, _i32, _vp]
_flow_t = [_vp, _vp, _vp, _vp, _vp, _vp, _i64, _i32, _pi, _i32, _vp, _i64, _i32, _vp]
_made_spline_t = [_vp, _vp, _vp, _i64, _i32, _vp, _vp, _vp, _vp, _i32, _i32, _f, _i32, _vp]
_ABI = {
    "tfk_abi_version": (_int, []),
    "tfk_last_error": (C.c_char_p, []),
    "tfk_device_info": (_int, [C.c_char_p, _i32, _pi]),
    "tfk_affine_coupling_fwd": (_int, _coupling_t),
    "tfk_affine_coupling_inv": (_int, _coupling_t),
    "tfk_shift_coupling_fwd": (_int, _coupling_t),
    "tfk_shift_coupling_inv": (_int, _coupling_t),
    "tfk_rqs_coupling_fwd": (_int, _spline_t),
    "tfk_rqs_coupling_inv": (_int, _spline_t),
    "tfk_conv1x1_coupling_fwd": (_int, _conv1x1_t),
    "tfk_conv1x1_coupling_inv": (_int, _conv1x1_t),
    "tfk_conv1x1_coupling_bwd": (_int, [_vp, _vp, _vp, _vp, _vp, _i64, _i32, _vp, _i32, _i32, _i32, _vp]),
    "tfk_elementwise_affine_fwd": (_int, _ew_t),
    "tfk_elementwise_affine_inv": (_int, _ew_t),
    "tfk_permute": (_int, [_vp, _vp, _vp, _i64, _i32, _vp]),
    "tfk_diag_gauss_logprob": (_int, [_vp, _vp, _vp, _vp, _vp, _i64, _i32, _vp]),
    "tfk_sum_f32": (_int, [_vp, _vp, _i64, _vp]),
    "tfk_sum_workspace_bytes": (_i64, [_i64]),
    "tfk_sum_f32_ws": (_int, [_vp, _vp, _vp, _i64, _vp]),
    "tfk_flow_supported": (_int, [_i32]),
    "tfk_flow_run": (_int, _flow_t),
    "tfk_flow_mfma_supported": (_int, [_i32]),
    "tfk_flow_lean_supported": (_int, [_i32]),
    "tfk_flow_run_mfma": (_int, _flow_t),
    "tfk_flow_sum_workspace_bytes": (_i64, []),
    "tfk_flow_run_mfma_sum": (_int, [_vp, _i32] + _flow_t[1:-1] + [_vp, _vp, _vp]),
    "tfk_flow_run_mfma_ctx": (_int, [_vp, _vp, _i32] + _flow_t[1:]),
    "tfk_flow_run_mfma_in": (_int, [_vp, _i32] + _flow_t[1:]),
    "tfk_flow_wide_supported": (_int, [_i32, _i32]),
    "tfk_flow_run_wide": (_int, _flow_t),
    "tfk_lrs_coupling_fwd": (_int, _spline_t),
    "tfk_lrs_coupling_inv": (_int, _spline_t),
    "tfk_dsf_supported": (_int, [_i32, _i32]),
    "tfk_dsf_coupling_fwd": (_int, _dsf_t),
    "tfk_dsf_coupling_inv": (_int, _dsf_t),
    "tfk_dsf_coupling_bwd": (_int, [_vp, _vp, _vp, _vp, _vp, _i64, _i32, _vp, _i32, _i32, _i32, _i32, _vp]),
    "tfk_made_affine_sequential": (_int, [_vp, _vp, _vp, _i64, _i32, _vp, _vp, _vp, _vp, _i32, _i32, _i32, _vp]),
    "tfk_made_rqs_sequential_lds_bytes": (_i64, [_i32, _i32, _i32]),
    "tfk_made_rqs_sequential": (_int, _made_spline_t),
    "tfk_made_lrs_sequential_lds_bytes": (_i64, [_i32, _i32, _i32]),
    "tfk_made_lrs_sequential": (_int, _made_spline_t),
    "tfk_conv3x3_block_supported": (_int, [_i32, _i32]),
    "tfk_conv3x3_relu_pool_affine": (_int, [_vp, _vp, _vp, _vp, _vp, _vp, _i64, _i32, _i32, _i32, _i32, _vp]),
    "tfk_conv1x1_frame": (_int, [_vp, _i64, _vp, _vp, _vp, _i64, _i32, _i32, _i32, _i32, _i32, _i32, _vp]),
    "tfk_bounded_sigmoid": (_int, [_vp, _vp, _i64, _f, _f, _vp]),
    "tfk_bounded_sigmoid_bwd": (_int, [_vp, _vp, _vp, _i64, _f, _f, _vp]),
    "tfk_convnet_train_workspace_bytes": (_i64, []),
    "tfk_convnet_train_block_supported": (_int, [_i32, _i32, _i32]),
    "tfk_convnet_train_block_fwd": (_int, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _f, _f, _i32, _i32, _vp, _vp,
                                           _i64, _i32, _i32, _i32, _i32, _vp]),
    "tfk_convnet_train_block_bwd": (_int, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i32, _vp, _i64,
                                           _i32, _i32, _i32, _vp]),
    "tfk_convnet_train_frame_fwd": (_int, [_vp, _vp, _vp, _vp, _vp, _i64, _i32, _i32, _i32, _i32, _i32, _i32, _i32, _i32, _vp]),
    "tfk_convnet_train_frame_bwd": (_int, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i32, _vp, _i64, _i32, _i32, _i32,
                                           _i32, _i32, _i32, _i32, _i32, _vp]),
    "tfk_convnet_train_forward": (_int, [C.POINTER(ConvNetTrainPlan), _vp, _vp, _i64, _i32, _i32, _vp]),
    "tfk_convnet_train_sums_floats": (_i64, [_i32, _i32, _i32, _i32]),
    "tfk_convnet_train_backward": (_int, [C.POINTER(ConvNetTrainPlan), _vp, _vp, _vp, _vp, _vp, _vp, _i64, _i32, _vp]),
    "tfk_convnet_train_linear_prep": (_int, [_vp, _vp, _vp, _vp, _vp, _vp, _i32, _i32, _i32, _vp]),
    "tfk_convnet_train_linear_fwd": (_int, [_vp, _vp, _vp, _vp, _i64, _i32, _vp]),
    "tfk_convnet_train_linear_bwd_input": (_int, [_vp, _vp, _vp, _i64, _i32, _vp]),
    "tfk_convnet_train_linear_wgrad": (_int, [_vp, _vp, _vp, _vp, _vp, _i64, _i32, _i32, _i32, _vp]),
    "tfk_glow_weight_floats": (_i64, [_i32]),
    "tfk_glow_plan": (_int, [C.POINTER(GlowLayer), _i32, _pi, _pi, _pi, _pi, _pi, _pi]),
    "tfk_glow_coupling": (_int, [_vp, _vp, _i64, _i32, C.POINTER(GlowLayer), _i32, _vp]),
    "tfk_glow_level_blob_bytes": (_i64, [C.POINTER(GlowLevelStep), _i32, _i32, _i32, _i32, _i32]),
    "tfk_glow_level_pack": (_int, [C.POINTER(GlowLevelStep), _i32, _i32, _i32, _i32, _i32, _vp, _i64]),
    "tfk_glow_level_info": (_int, [_vp, _pi, _pi, _pi, _pi]),
    "tfk_glow_level": (_int, [_vp, _vp, _vp, _i64, _i32, _vp, _vp, _vp, _vp]),
    "tfk_rows_fma": (_int, [_vp, _vp, _i64, _i32, _vp]),
    "tfk_rows_fma_gauss_logprob": (_int, [_vp, _vp, _vp, _vp, _vp, _vp, _i64, _i32, _vp]),
    "tfk_affine_coupling_bwd": (_int, [_vp, _vp, _vp, _vp, _vp, _i64, _i32, _vp, _i32, _i32, _vp]),
    "tfk_shift_coupling_bwd": (_int, [_vp, _vp, _i64, _i32, _vp, _i32, _i32, _vp]),
    "tfk_rqs_coupling_bwd_supported": (_int, [_i32]),
    "tfk_rqs_coupling_bwd": (_int, _spline_bwd_t),
    "tfk_lrs_coupling_bwd": (_int, _spline_bwd_t),
    "tfk_elementwise_affine_bwd_workspace_bytes": (_i64, [_i64, _i32]),
    "tfk_elementwise_affine_bwd": (_int, [_vp, _vp, _vp, _vp, _vp, _vp, _i64, _i32, _i32, _vp]),
    "tfk_diag_gauss_logprob_bwd": (_int, [_vp, _vp, _vp, _vp, _vp, _i64, _i32, _vp]),
    "tfk_coupling_train_bwd_supported": (_int, [_i32]),
    "tfk_coupling_train_bwd_out_floats": (_i64, [_i32]),
    "tfk_coupling_train_bwd_workspace_bytes": (_i64, [_i32]),
    "tfk_affine_coupling_train_bwd": (_int, [_vp, _vp, _vp, _vp, _i64, _i32, _vp, _vp, _i64, _i32, _i32, _vp, _i32, _vp]),
    "tfk_rqs_coupling_train_bwd_supported": (_int, [_i32, _i32]),
    "tfk_rqs_coupling_train_bwd": (_int, [_vp, _vp, _vp, _vp, _i64, _i32, _vp, _vp, _i64, _i32, _i32, _f, _i32, _vp, _i32, _vp]),
    "tfk_rqs_coupling_train_bwd_hid": (_int, [_vp, _vp, _vp, _vp, _i64, _i32, _vp, _vp, _vp, _i64, _i32, _i32, _f, _i32, _vp, _i32,
                                              _vp]),
    "tfk_rows_outer_workspace_bytes": (_i64, [_i32]),
    "tfk_rows_outer": (_int, [_vp, _i32, _i32, _vp, _vp, _vp, _i64, _vp]),
    "tfk_wide_coupling_train_bwd_supported": (_int, [_i32, _i32]),
    "tfk_wide_coupling_train_bwd_param_floats": (_i64, [_i32, _i32]),
    "tfk_wide_coupling_train_bwd_grid_cap": (_i64, [_i32, _i32]),
    "tfk_wide_coupling_train_bwd": (_int, [_vp, _vp, _vp, _vp, _i64, _vp, _vp, _vp, _i64, _i32, _i32, _i32, _vp, _i32, _vp]),
}
SYMBOLS = tuple(_ABI)        # every symbol include/tfk.h declares (tests check the built library exports all of them)

_lib: Optional[C.CDLL] = None
calls = 0   # number of kernel entry points invoked (tests assert the HIP path really ran)


def build(verbose: bool = False) -> str:
    """Compile libtfk.so for gfx950 with hipcc (cross-compiles without a GPU)."""
    out = None if verbose else subprocess.DEVNULL
    subprocess.run(["make", "-C", CSRC, "-B", "-j", str(min(os.cpu_count() or 1, 8))], check=True, stdout=out)
    global _lib
    _lib = None
    return LIB_PATH


def bind(L: C.CDLL, names=None) -> None:
    """Give the functions ``names`` of ``L`` (default: all of them) their prototypes from the table -- libtfk.so here, the
    CPU restatement of the same ABI in tests/test_cabi_host.py."""
    for name in (_ABI if names is None else names):
        fn = getattr(L, name)
        fn.restype, fn.argtypes = _ABI[name]


def lib() -> C.CDLL:
    """The loaded library; raises NativeError (never falls back) if it cannot be used."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise NativeError(
                f"{LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; "
                f"g.build()'` (hipcc --offload-arch=gfx950). There is no fallback path.")
        try:
            L = C.CDLL(LIB_PATH)
        except OSError as e:   # e.g. libamdhip64 not loadable
            raise NativeError(f"cannot load {LIB_PATH}: {e}") from e
        missing = [s for s in SYMBOLS if not hasattr(L, s)]
        if missing:
            raise NativeError(f"{LIB_PATH} lacks symbols {missing}; rebuild it")
        if L.tfk_abi_version() != ABI_VERSION:
            raise NativeError(f"{LIB_PATH} has ABI {L.tfk_abi_version()}, expected {ABI_VERSION}")
        bind(L)
        _lib = L
    return _lib


def available() -> bool:
    try:
        lib()
        return True
    except NativeError:
        return False


def eligible(*tensors: Optional[torch.Tensor]) -> bool:
    """True when the HIP path applies: fp32 tensors on a HIP device, no autograd needed.
    (Training / fp64 / host tensors take the ATen composite path, as SURVEY.md app. B.)"""
    seen = False
    for t in tensors:
        if t is None:
            continue
        seen = True
        if t.device.type != "cuda" or t.dtype != torch.float32:
            return False
        if t.requires_grad and torch.is_grad_enabled():
            return False
    return seen


def _check(rc: int, what: str) -> None:
    if rc != 0:
        raise NativeError(f"{what} failed (code {rc}): {lib().tfk_last_error().decode()}")


def _ptr(t: Optional[torch.Tensor], what: str) -> Optional[int]:
    if t is None:
        return None
    if t.device.type != "cuda":
        raise NativeError(f"{what}: tensor is on {t.device}, the kernels need a HIP device")
    if not t.is_contiguous():
        raise NativeError(f"{what}: tensor must be contiguous")
    return t.data_ptr()


def _f32(t: Optional[torch.Tensor], what: str) -> Optional[int]:
    if t is None:
        return None
    if t.dtype != torch.float32:
        raise NativeError(f"{what}: expected float32, got {t.dtype}")
    if t.device.type != "cuda" or not t.is_contiguous():
        return _ptr(t, what)                # (raises, with the reason)
    return t.data_ptr()


def _idx(t: Optional[torch.Tensor], what: str) -> Optional[int]:
    if t is not None and t.dtype != torch.int32:
        raise NativeError(f"{what}: expected int32 indices, got {t.dtype}")
    return _ptr(t, what)


class _NoGuard:
    def __enter__(self):
        return None

    def __exit__(self, *exc):
        return False


_NO_GUARD = _NoGuard()


def _device_guard(t: torch.Tensor):
    """Make the tensor's device current for the launch -- a no-op (and no context-manager cost on
    the launch path) when it already is."""
    idx = t.device.index
    if idx is None or idx == torch.cuda.current_device():
        return _NO_GUARD
    return torch.cuda.device(idx)


_raw_stream = getattr(torch._C, "_cuda_getCurrentRawStream", None)


def _stream(t: torch.Tensor) -> int:
    """The caller's current HIP stream on the tensor's device, as the integer handle the C-ABI takes."""
    if _raw_stream is not None:             # one C call (torch.cuda.current_stream() builds a Stream object: ~5 us)
        idx = t.device.index
        return _raw_stream(torch.cuda.current_device() if idx is None else idx)
    return torch.cuda.current_stream(t.device).cuda_stream


def _rows(x: torch.Tensor, what: str):
    if x.dim() != 2:
        raise NativeError(f"{what}: expected a (N, D) tensor, got shape {tuple(x.shape)}")
    return x.shape[0], x.shape[1]


def _launch(name, anchor, *args, n=1):
    """Enqueue entry point ``name`` on the current stream of ``anchor``'s device, that device made current; ``n``: how many
    kernel entry points the call stands for in ``calls``."""
    global calls
    fn = getattr(_lib if _lib is not None else lib(), name)
    with _device_guard(anchor):
        rc = fn(*args, _stream(anchor))
    calls += n
    if rc != 0:
        _check(rc, name)


def _coupling(name, x, h, out, logdet, tgt_idx, T, per_row, what, accumulate, extra=()):
    """``per_row``: the parameters h holds per row, spelled ``what`` in the message (as in ``_coupling_bwd``)."""
    N, D = _rows(x, name)
    if out.shape != x.shape:
        raise NativeError(f"{name}: out shape {tuple(out.shape)} != x shape {tuple(x.shape)}")
    if h.numel() != N * per_row:
        raise NativeError(f"{name}: h has {h.numel()} elements, expected {what} = {N * per_row}")
    if logdet is not None and logdet.numel() != N:
        raise NativeError(f"{name}: logdet has {logdet.numel()} elements, expected {N}")
    if tgt_idx is not None and tgt_idx.numel() != T:
        raise NativeError(f"{name}: tgt_idx has {tgt_idx.numel()} entries, expected T = {T}")
    _launch(name, x, _f32(x, name), _f32(h, name), _f32(out, name), _f32(logdet, name), N, D,
            _idx(tgt_idx, name), T, *extra, 1 if accumulate else 0)


def affine_coupling(x, h, out, logdet, tgt_idx, T, accumulate=False, inverse=False):
    """x, out: (N, D); h: (N, T, 2); logdet: (N,).  tgt_idx None = contiguous tail."""
    _coupling("tfk_affine_coupling_inv" if inverse else "tfk_affine_coupling_fwd",
              x, h, out, logdet, tgt_idx, T, T * 2, "N*T*2", accumulate)


def shift_coupling(x, h, out, logdet, tgt_idx, T, accumulate=False, inverse=False):
    _coupling("tfk_shift_coupling_inv" if inverse else "tfk_shift_coupling_fwd",
              x, h, out, logdet, tgt_idx, T, T, "N*T", accumulate)


def rqs_coupling(x, h, out, logdet, tgt_idx, T, n_bins, boundary, accumulate=False,
                 inverse=False):
    """h: (N, T, 3*n_bins - 1)."""
    _coupling("tfk_rqs_coupling_inv" if inverse else "tfk_rqs_coupling_fwd",
              x, h, out, logdet, tgt_idx, T, T * (3 * n_bins - 1), "N*T*P", accumulate,
              extra=(int(n_bins), C.c_float(float(boundary))))


def lrs_coupling(x, h, out, logdet, tgt_idx, T, n_bins, boundary, accumulate=False, inverse=False):
    """Linear rational spline coupling; h: (N, T, 4*n_bins)."""
    _coupling("tfk_lrs_coupling_inv" if inverse else "tfk_lrs_coupling_fwd",
              x, h, out, logdet, tgt_idx, T, T * 4 * n_bins, "N*T*P", accumulate,
              extra=(int(n_bins), C.c_float(float(boundary))))


def dsf_supported(n_components, hidden_dim) -> bool:
    """Is there a kernel for a deep sigmoidal transformer of this size (tfk_dsf_supported)?"""
    return bool(lib().tfk_dsf_supported(int(n_components), int(hidden_dim)))


def dsf_coupling(x, h, out, logdet, tgt_idx, T, n_components, hidden_dim, accumulate=False, inverse=False):
    """Deep sigmoidal coupling; h: (N, T, 3 * hidden_dim * n_components).  ``inverse``: the whole bisection in the launch."""
    _coupling("tfk_dsf_coupling_inv" if inverse else "tfk_dsf_coupling_fwd",
              x, h, out, logdet, tgt_idx, T, T * 3 * int(hidden_dim) * int(n_components), "N*T*P", accumulate,
              extra=(int(n_components), int(hidden_dim)))


def conv1x1_coupling(x, h, out, logdet, tgt_idx, T, n_channels, accumulate=False, inverse=False):
    """Invertible 1x1 convolution on the T target positions (n_channels x T/n_channels pixels,
    channel-major); h: (N, n + n(n-1)) LU parameters per sample."""
    name = "tfk_conv1x1_coupling_inv" if inverse else "tfk_conv1x1_coupling_fwd"
    n = int(n_channels)
    _coupling(name, x, h, out, logdet, tgt_idx, T, n * n, "N * n^2", accumulate, extra=(n,))


def elementwise_affine(x, value, out, logdet, inverse_affine, accumulate=False, inverse=False):
    """value: (D, 2) global parameters; inverse_affine selects the ActNorm transformer."""
    name = "tfk_elementwise_affine_inv" if inverse else "tfk_elementwise_affine_fwd"
    N, D = _rows(x, name)
    if value.numel() != 2 * D:
        raise NativeError(f"{name}: value has {value.numel()} elements, expected 2*D = {2 * D}")
    if out.shape != x.shape or logdet.numel() != N:
        raise NativeError(f"{name}: bad out/logdet shape")
    _launch(name, x, _f32(x, name), _f32(value, name), _f32(out, name), _f32(logdet, name), N, D,
            1 if inverse_affine else 0, 1 if accumulate else 0)


def permute(x, perm, out):
    """out[n, j] = x[n, perm[j]]; perm None = reversal."""
    name = "tfk_permute"
    N, D = _rows(x, name)
    if out.shape != x.shape:
        raise NativeError("tfk_permute: bad out shape")
    if perm is not None and perm.numel() != D:
        raise NativeError(f"tfk_permute: perm has {perm.numel()} entries, expected D = {D}")
    _launch(name, x, _f32(x, name), _idx(perm, name), _f32(out, name), N, D)


def diag_gauss_logprob(z, loc, log_scale, logdet_in, out):
    name = "tfk_diag_gauss_logprob"
    N, D = _rows(z, name)
    if loc.numel() != D or log_scale.numel() != D or out.numel() != N:
        raise NativeError(f"{name}: bad parameter/out shape")
    _launch(name, z, _f32(z, name), _f32(loc, name), _f32(log_scale, name), _f32(logdet_in, name), _f32(out, name), N, D)


# ---- reverse mode (csrc/tfk_bwd.hip) ------------------------------------------------------
def _bwd_common(name, x, g, gld, tgt_idx, T):
    N, D = _rows(g, name)
    if x is not None and x.shape != g.shape:
        raise NativeError(f"{name}: x shape {tuple(x.shape)} != g shape {tuple(g.shape)}")
    if gld is not None and gld.numel() != N:
        raise NativeError(f"{name}: gld has {gld.numel()} elements, expected {N}")
    if tgt_idx is not None and tgt_idx.numel() != T:
        raise NativeError(f"{name}: tgt_idx has {tgt_idx.numel()} entries, expected T = {T}")
    return N, D


def _coupling_bwd(name, x, h, g, gld, gh, tgt_idx, T, per_row, what, extra, inverse):
    """In place on g (N, D): target columns dL/d out -> dL/d x; gh, shaped like h (``per_row`` parameters a row, spelled
    ``what`` in the message), written."""
    N, D = _bwd_common(name, x, g, gld, tgt_idx, T)
    if h.numel() != N * per_row or gh.numel() != N * per_row:
        raise NativeError(f"{name}: h / gh must hold {what} = {N * per_row} elements")
    _launch(name, g, _f32(x, name), _f32(h, name), _f32(g, name), _f32(gld, name), _f32(gh, name), N, D,
            _idx(tgt_idx, name), T, *extra, 1 if inverse else 0)


def affine_coupling_bwd(x, h, g, gld, gh, tgt_idx, T, inverse=False):
    """In place on g (N, D): target columns dL/d out -> dL/d x; gh (N, T, 2) written."""
    _coupling_bwd("tfk_affine_coupling_bwd", x, h, g, gld, gh, tgt_idx, T, T * 2, "N*T*2", (), inverse)


def conv1x1_coupling_bwd(x, h, g, gld, gh, tgt_idx, T, n_channels, inverse=False):
    """Reverse mode of ``conv1x1_coupling``: in place on g (N, D) at the T target positions, gh (N, n + n(n-1)) written."""
    n = int(n_channels)
    _coupling_bwd("tfk_conv1x1_coupling_bwd", x, h, g, gld, gh, tgt_idx, T, n * n, "N * n^2", (n,), inverse)


def shift_coupling_bwd(g, gh, tgt_idx, T, inverse=False):
    name = "tfk_shift_coupling_bwd"
    N, D = _bwd_common(name, None, g, None, tgt_idx, T)
    if gh.numel() != N * T:
        raise NativeError(f"{name}: gh must hold N*T = {N * T} elements")
    _launch(name, g, _f32(g, name), _f32(gh, name), N, D, _idx(tgt_idx, name), T, 1 if inverse else 0)


def rqs_coupling_bwd(x, h, g, gld, gh, tgt_idx, T, n_bins, boundary, inverse=False):
    _coupling_bwd("tfk_rqs_coupling_bwd", x, h, g, gld, gh, tgt_idx, T, T * (3 * int(n_bins) - 1), "N*T*P",
                  (int(n_bins), C.c_float(float(boundary))), inverse)


def lrs_coupling_bwd(x, h, g, gld, gh, tgt_idx, T, n_bins, boundary, inverse=False):
    _coupling_bwd("tfk_lrs_coupling_bwd", x, h, g, gld, gh, tgt_idx, T, T * 4 * int(n_bins), "N*T*P",
                  (int(n_bins), C.c_float(float(boundary))), inverse)


def dsf_coupling_bwd(x, h, g, gld, gh, tgt_idx, T, n_components, hidden_dim, inverse=False):
    """Reverse mode of ``dsf_coupling`` (forward direction only: the bisection carries no gradient)."""
    _coupling_bwd("tfk_dsf_coupling_bwd", x, h, g, gld, gh, tgt_idx, T, T * 3 * int(hidden_dim) * int(n_components), "N*T*P",
                  (int(n_components), int(hidden_dim)), inverse)


# ---- the transformer kinds (``transformer.native_kind``): which wrappers serve each, with which scalar arguments, and when
# there is a kernel -- what the layers (layers_base.py) and the training chain (autograd.py) ask instead of naming kinds.
def _dsf_native(tr) -> bool:
    """A deep sigmoidal transformer of a size csrc/tfk_dsf.hip is instantiated for (tfk_dsf_supported); other sizes --
    and all of them under TORCHFLOWS_AMD_DEBUG="dsf=0" (comparison runs) -- take the ATen composite path."""
    from torchflows_amd.utils import debug_switch
    if debug_switch("dsf", "1") == "0":
        return False
    return dsf_supported(tr.n_components, tr.hidden_dim)


def _always(tr) -> bool:
    return True


def _never(tr) -> bool:
    return False


def _rqs_bins(tr) -> bool:
    return 2 <= tr.n_bins <= 32


def _lrs_bins(tr) -> bool:
    return int(tr.n_bins) in (4, 8)


class TransformerKind(NamedTuple):
    forward: str                # wrapper names, looked up in this module when called: a stubbed wrapper is what runs
    reverse: str
    scalars: Optional[Callable]  # transformer -> the wrappers' scalar arguments behind T (None: there are none)
    flipped: bool               # the transformer's forward is the kernel's inverse form (InverseAffine)
    coupling: Callable          # transformer -> is there a coupling kernel
    made: Callable              # ... a parallel pass for a MADE layer of it
    reverse_mode: Callable      # ... reverse-mode kernels
    reverse_reads_x: bool = True   # the reverse wrapper takes (x, h, g, gld, gh, ...); a shift's only (g, gh, ...)


KINDS = {
    "affine": TransformerKind("affine_coupling", "affine_coupling_bwd", None, False, _always, _always, _always),
    "inverse_affine": TransformerKind("affine_coupling", "affine_coupling_bwd", None, True, _always, _always, _always),
    "shift": TransformerKind("shift_coupling", "shift_coupling_bwd", None, False, _always, _never, _always, False),
    "rqs": TransformerKind("rqs_coupling", "rqs_coupling_bwd", attrgetter("n_bins", "boundary"), False, _rqs_bins, _rqs_bins,
                           lambda tr: bool(lib().tfk_rqs_coupling_bwd_supported(int(tr.n_bins)))),
    "lrs": TransformerKind("lrs_coupling", "lrs_coupling_bwd", attrgetter("n_bins", "boundary"), False, _lrs_bins, _lrs_bins, _lrs_bins),
    "dsf": TransformerKind("dsf_coupling", "dsf_coupling_bwd", attrgetter("n_components", "hidden_dim"), False,
                           _dsf_native, _dsf_native, _dsf_native),
    "conv1x1": TransformerKind("conv1x1_coupling", "conv1x1_coupling_bwd", lambda tr: (tr.n_channels,), False,
                               lambda tr: tr.n_channels <= 16,      # channels are kept in registers
                               _never, lambda tr: int(tr.n_channels) <= 16),
}


def coupling_kernel(tr) -> bool:
    """Is there a coupling kernel for this transformer?"""
    kind = KINDS.get(tr.native_kind)
    return kind is not None and bool(kind.coupling(tr))


def made_kernel(tr) -> bool:
    """... a parallel pass for a MADE layer of it?"""
    kind = KINDS.get(tr.native_kind)
    return kind is not None and bool(kind.made(tr))


def reverse_kernel(tr) -> bool:
    """... reverse-mode kernels?"""
    kind = KINDS.get(tr.native_kind)
    return kind is not None and bool(kind.reverse_mode(tr))


def transform(tr, inverse, x, h, out, logdet, tgt, T, accumulate):
    """The transformer's forward (``inverse``: inverse) map on the T target columns ``tgt`` (None: the tail) of x (N, D) with
    the parameters ``h``."""
    kind = KINDS.get(tr.native_kind)
    if kind is None:
        raise NativeError(f"no kernel for transformer kind {tr.native_kind!r}")
    forward, _, scalars, flipped = kind[:4]
    if scalars is None:
        globals()[forward](x, h, out, logdet, tgt, T, accumulate=accumulate, inverse=inverse != flipped)
    else:
        globals()[forward](x, h, out, logdet, tgt, T, *scalars(tr), accumulate=accumulate, inverse=inverse != flipped)


def transform_bwd(tr, inverse, x, h, g, gld, gh, tgt, T):
    """Reverse mode of ``transform``: in place on ``g`` at the target columns, dL/dh written to ``gh``."""
    kind = KINDS.get(tr.native_kind)
    if kind is None:
        raise NativeError(f"no kernel for transformer kind {tr.native_kind!r}")
    extra = kind.scalars(tr) if kind.scalars is not None else ()
    lead = (x, h, g, gld, gh) if kind.reverse_reads_x else (g, gh)
    globals()[kind.reverse](*lead, tgt, T, *extra, inverse=inverse != kind.flipped)


def elementwise_affine_bwd(x, value, g, gld, want_param, inverse=False, out=None):
    """In place on g (all D columns).  Returns dL/dvalue (D, 2) when ``want_param`` (written into ``out``, 2 D
    contiguous floats, when given)."""
    name = "tfk_elementwise_affine_bwd"
    N, D = _rows(g, name)
    if value.numel() != 2 * D:
        raise NativeError(f"{name}: value has {value.numel()} elements, expected 2*D = {2 * D}")
    gvalue = ws = None
    if want_param:
        if x is None or x.shape != g.shape or gld is None or gld.numel() != N:
            raise NativeError(f"{name}: the parameter gradient needs x (N, D) and gld (N,)")
        if out is not None and (out.numel() != 2 * D or not out.is_contiguous() or out.dtype != torch.float32):
            raise NativeError(f"{name}: out must hold 2*D = {2 * D} contiguous floats")
        gvalue = torch.empty(D, 2, dtype=torch.float32, device=g.device) if out is None else out.view(D, 2)
        nbytes = int(lib().tfk_elementwise_affine_bwd_workspace_bytes(N, D))
        ws = torch.empty(max(nbytes // 4, 1), dtype=torch.float32, device=g.device)
    _launch(name, g, _f32(x if want_param else None, name), _f32(value, name), _f32(g, name),
            _f32(gld if want_param else None, name), _f32(gvalue, name), _f32(ws, name), N, D, 1 if inverse else 0)
    return gvalue


def diag_gauss_logprob_bwd(z, loc, log_scale, glp, g):
    name = "tfk_diag_gauss_logprob_bwd"
    N, D = _rows(z, name)
    if loc.numel() != D or log_scale.numel() != D or glp.numel() != N or g.shape != z.shape:
        raise NativeError(f"{name}: bad parameter / gradient shape")
    _launch(name, z, _f32(z, name), _f32(loc, name), _f32(log_scale, name), _f32(glp, name), _f32(g, name), N, D)


def affine_coupling_train_bwd(x, g, gld, params, gemm2_steps, out, workspace, inverse_form=False,
                              gscale=None, g_reversed=False):
    """Fused conditioner + transform + MLP backward of one HalfSplit affine coupling (in place on
    g, accumulator-layout weight gradients into ``out``)."""
    name = "tfk_affine_coupling_train_bwd"
    N, D = _rows(g, name)
    if x.shape != g.shape or gld.numel() != N:
        raise NativeError(f"{name}: bad x / gld shape")
    if out.numel() != int(lib().tfk_coupling_train_bwd_out_floats(D)):
        raise NativeError(f"{name}: out must hold tfk_coupling_train_bwd_out_floats(D) floats")
    if workspace.numel() * 4 < int(lib().tfk_coupling_train_bwd_workspace_bytes(D)):
        raise NativeError(f"{name}: workspace too small")
    args = (_f32(x, name), _f32(g, name), _f32(gld, name), _f32(params, name), params.numel(),
            int(gemm2_steps), _f32(out, name), _f32(workspace, name), N, D, 1 if inverse_form else 0,
            _f32(gscale, name), 1 if g_reversed else 0)
    if gscale is not None and gscale.numel() != D:
        raise NativeError(f"{name}: gscale must hold D = {D} floats")
    _launch(name, g, *args)


def rqs_coupling_train_bwd(x, g, gld, params, gemm2_steps, gh_perm, gpre_perm, n_bins, boundary,
                           inverse=False, gscale=None, g_reversed=False, hid_perm=None):
    """Conditioner re-evaluation + RQ-spline backward + dL/dhidden + dL/dx_A in one launch (in place on
    g); gh_perm (N, 768) and gpre_perm (N, 16) in accumulator order; ``hid_perm`` (N, 16): also the hidden activations,
    column 15 == 1 (tfk_rqs_coupling_train_bwd_hid)."""
    name = "tfk_rqs_coupling_train_bwd" if hid_perm is None else "tfk_rqs_coupling_train_bwd_hid"
    N, D = _rows(g, name)
    if x.shape != g.shape or gld.numel() != N or gh_perm.shape != (N, 768) or gpre_perm.shape != (N, 16):
        raise NativeError(f"{name}: bad x / gld / gh_perm / gpre_perm shape")
    if hid_perm is not None and hid_perm.shape != (N, 16):
        raise NativeError(f"{name}: hid_perm must be (N, 16)")
    if gscale is not None and gscale.numel() != D:
        raise NativeError(f"{name}: gscale must hold D = {D} floats")
    head = (_f32(x, name), _f32(g, name), _f32(gld, name), _f32(params, name), params.numel(),
            int(gemm2_steps), _f32(gh_perm, name), _f32(gpre_perm, name))
    tail = (N, D, int(n_bins), C.c_float(float(boundary)), 1 if inverse else 0, _f32(gscale, name), 1 if g_reversed else 0)
    hid = () if hid_perm is None else (_f32(hid_perm, name),)
    _launch(name, g, *head, *hid, *tail)


_rows_outer_ws = {}


def _rows_outer_workspace(device, M: int, stream: int):
    """ONE workspace per (device, M) -- about 25 MB at M = 768 -- whatever the stream: every graph-mode ``Flow.fit`` runs
    on a fresh side stream, and a copy per stream pinned up to ~0.8 GB for the life of the process.  The
    buffer is never freed (a captured training step bakes in its address).  A use on ANOTHER stream than the last one
    first waits for that stream's tail, so two streams never hold the partial sums at the same time; only a stream that
    is being captured and finds the buffer last used elsewhere gets a private copy (a capture cannot wait on work outside
    it)."""
    key = (device.index, M)
    entry = _rows_outer_ws.get(key)
    if entry is None:
        entry = _rows_outer_ws[key] = [torch.empty(int(lib().tfk_rows_outer_workspace_bytes(M)) // 4,
                                                   dtype=torch.float32, device=device), stream]
    elif entry[1] != stream:
        if torch.cuda.is_current_stream_capturing():
            pkey = (device.index, M, stream)
            private = _rows_outer_ws.get(pkey)
            if private is None:
                private = _rows_outer_ws[pkey] = [torch.empty_like(entry[0]), stream]
            return private[0]
        prev = torch.cuda.ExternalStream(entry[1], device=device) if entry[1] else torch.cuda.default_stream(device)
        torch.cuda.current_stream(device).wait_stream(prev)
        entry[1] = stream
    return entry[0]


def rows_outer(A, M, B, out):
    """out[M * 16] (accumulator order, include/tfk.h) = sum over the rows of A[n, :M]^T B[n, :16] (tfk_rows_outer):
    the weight-gradient products that contract over the batch rows, deterministic, no GEMM-library call."""
    name = "tfk_rows_outer"
    N, lda = _rows(A, name)
    if B.shape != (N, 16) or out.numel() != M * 16 or not out.is_contiguous():
        raise NativeError(f"{name}: B must be (N, 16) and out hold M * 16 = {M * 16} contiguous floats")
    ws = _rows_outer_workspace(A.device, int(M), _stream(A))
    _launch(name, A, _f32(A, name), int(lda), int(M), _f32(B, name), _f32(out, name), _f32(ws, name), N)


def wide_coupling_train_bwd(x, g, gld, params, gh_rec, gpre_rec, hid_rec, shift=False, inverse_form=False,
                            gscale=None, g_reversed=False):
    """Reverse mode of one affine / shift coupling on an event size in (256, 1024], D % 8 == 0 (tfk_wide_coupling_train_bwd):
    in place on g; gh_rec (N, 2 hp) -- (N, hp) for a shift coupling --, gpre_rec (N, 16) and hid_rec (N, 16) are the records
    tfk_rows_outer contracts over the batch rows (include/tfk.h).  The records may be longer than N rows (buffers kept
    across steps): only the first N are written."""
    name = "tfk_wide_coupling_train_bwd"
    N, D = _rows(g, name)
    hp = (D // 2 + 63) // 64 * 64
    if x.shape != g.shape or gld.numel() != N:
        raise NativeError(f"{name}: bad x / gld shape")
    for t, w in ((gh_rec, hp if shift else 2 * hp), (gpre_rec, 16), (hid_rec, 16)):
        if t.dim() != 2 or t.shape[1] != w or t.shape[0] < N or not t.is_contiguous():
            raise NativeError(f"{name}: record of shape {tuple(t.shape)}, expected (>= {N}, {w}) contiguous")
    if gscale is not None and gscale.numel() != D:
        raise NativeError(f"{name}: gscale must hold D = {D} floats")
    args = (_f32(x, name), _f32(g, name), _f32(gld, name), _f32(params, name), params.numel(), _f32(gh_rec, name),
            _f32(gpre_rec, name), _f32(hid_rec, name), N, D, 1 if shift else 0, 1 if inverse_form else 0,
            _f32(gscale, name), 1 if g_reversed else 0)
    _launch(name, g, *args)


def made_affine_sequential(z, out, logdet, W1t, b1, W2, b2, divide, accumulate=False):
    """The sequential map of a MADE-based affine layer in one launch; W1t (D, HP), b1 (HP,),
    W2 (D, 2, HP), b2 (D, 2) masked and zero-padded to HP hidden units."""
    name = "tfk_made_affine_sequential"
    N, D = _rows(z, name)
    HP = b1.numel()
    if out.shape != z.shape or logdet.numel() != N or W1t.numel() != D * HP or W2.numel() != 2 * D * HP \
            or b2.numel() != 2 * D:
        raise NativeError(f"{name}: bad tensor shapes")
    _launch(name, z, _f32(z, name), _f32(out, name), _f32(logdet, name), N, D, _f32(W1t, name), _f32(b1, name),
            _f32(W2, name), _f32(b2, name), HP, 1 if divide else 0, 1 if accumulate else 0)


def made_rqs_sequential(z, out, logdet, W1t, b1, W2, b2, n_bins, boundary, accumulate=False, lrs=False):
    """The sequential map of a MADE-based RQ-spline (or, ``lrs``, linear-rational-spline) layer in one
    launch; W1t (D, HP), b1 (HP,), W2 (D, P, HP), b2 (D, P) masked and zero-padded to HP hidden units,
    P = 3 n_bins - 1 (RQ) or 4 n_bins (LRS)."""
    name = "tfk_made_lrs_sequential" if lrs else "tfk_made_rqs_sequential"
    N, D = _rows(z, name)
    HP, P = b1.numel(), (4 * int(n_bins) if lrs else 3 * int(n_bins) - 1)
    if out.shape != z.shape or logdet.numel() != N or W1t.numel() != D * HP or W2.numel() != P * D * HP \
            or b2.numel() != P * D:
        raise NativeError(f"{name}: bad tensor shapes")
    _launch(name, z, _f32(z, name), _f32(out, name), _f32(logdet, name), N, D, _f32(W1t, name), _f32(b1, name),
            _f32(W2, name), _f32(b2, name), HP, int(n_bins), C.c_float(float(boundary)), 1 if accumulate else 0)


def conv3x3_relu_pool_affine(x, weight, bias, scale, shift):
    """conv3x3(pad 1) -> ReLU -> MaxPool2d(2) -> per-channel scale / shift in one launch (NCHW)."""
    name = "tfk_conv3x3_relu_pool_affine"
    if x.dim() != 4 or weight.dim() != 4 or tuple(weight.shape[2:]) != (3, 3) or weight.shape[1] != x.shape[1]:
        raise NativeError(f"{name}: x (N, C, H, W) and weight (C_out, C, 3, 3) expected")
    N, c_in, H, W = x.shape
    c_out = weight.shape[0]
    if bias.numel() != c_out or scale.numel() != c_out or shift.numel() != c_out:
        raise NativeError(f"{name}: bias / scale / shift must hold c_out = {c_out} values")
    out = torch.empty(N, c_out, H // 2, W // 2, dtype=torch.float32, device=x.device)
    _launch(name, x, _f32(x, name), _f32(weight, name), _f32(bias, name), _f32(scale, name), _f32(shift, name),
            _f32(out, name), N, c_in, c_out, H, W)
    return out


def bounded_sigmoid(h: torch.Tensor, lo: float, hi: float) -> torch.Tensor:
    """``lo + (hi - lo) * sigmoid(h)`` in one pass (ATen: three kernels, two temporaries)."""
    name = "tfk_bounded_sigmoid"
    out = torch.empty_like(h)
    _launch(name, h, _f32(h, name), _f32(out, name), h.numel(), float(lo), float(hi))
    return out


def bounded_sigmoid_bwd(out: torch.Tensor, g: torch.Tensor, lo: float, hi: float) -> torch.Tensor:
    """d(loss)/dh of ``out = lo + (hi - lo) * sigmoid(h)`` from ``out`` and d(loss)/d(out), one pass."""
    name = "tfk_bounded_sigmoid_bwd"
    g_in = torch.empty_like(out)
    _launch(name, out, _f32(out, name), _f32(g, name), _f32(g_in, name), out.numel(), float(lo), float(hi))
    return g_in


def conv1x1_frame(x, weight, bias, h_out: int, w_out: int):
    """1x1 convolution c_in -> c_out placed in the middle of an (h_out, w_out) frame that holds the bias.
    ``x`` (N, C, H, W) may be a view whose images are contiguous but further apart than C*H*W."""
    name = "tfk_conv1x1_frame"
    if x.dim() != 4 or x.dtype != torch.float32 or x.device.type != "cuda":
        raise NativeError(f"{name}: x must be a float32 (N, C, H, W) tensor on a HIP device")
    N, c_in, H, W = x.shape
    if N > 1 and (x.stride(3) != 1 or x.stride(2) != W or x.stride(1) != H * W):
        raise NativeError(f"{name}: the images of x must be contiguous")
    c_out = weight.shape[0]
    if weight.numel() != c_out * c_in or bias.numel() != c_out:
        raise NativeError(f"{name}: weight (c_out, c_in[, 1, 1]) and bias (c_out,) expected")
    x_stride = x.stride(0) if N > 1 else c_in * H * W
    out = torch.empty(N, c_out, h_out, w_out, dtype=torch.float32, device=x.device)
    _launch(name, x, x.data_ptr(), x_stride, _f32(weight, name), _f32(bias, name), _f32(out, name),
            N, c_in, c_out, H, W, h_out, w_out)
    return out


_convnet_ws = {}      # (device index, stream handle) -> zeroed workspace of the tfk_convnet_train_* launches


def convnet_train_workspace(t: torch.Tensor) -> torch.Tensor:
    """The partial-sum rows + ticket counter the ConvNet training launches share, one per (device, stream): zeroed
    once, every launch leaves the counter at zero and consumes its own partial sums before it ends."""
    key = (t.device.index, _stream(t))
    ws = _convnet_ws.get(key)
    if ws is None:
        ws = _convnet_ws[key] = torch.zeros(int(lib().tfk_convnet_train_workspace_bytes()) // 4, dtype=torch.float32,
                                            device=t.device)
    return ws


# floats per sample the two passes of the whole-network calls keep / use
CONVNET_ACT_FLOATS = 4 * 32 * 32 + 8 * 16 * 16 + 8 * 8 * 8 + 4 * 4 * 4 + 16       # a0, y1, y2, y3, a16
CONVNET_AMAX_BYTES = 8 * 16 * 16 + 8 * 8 * 8 + 4 * 4 * 4
CONVNET_SCRATCH_FLOATS = 16 + 64 + 512 + 2048 + 4096                             # g16, gz3, gz2, gz1, g_a0


def convnet_train_forward(plan: "ConvNetTrainPlan", params, bns, x, training: bool, update_running: bool):
    """The whole ConvNet conditioner in ONE call (tfk_convnet_train_forward): fills ``plan`` from ``params`` (the 18
    tensors in convnet_train._params order), the three BatchNorm modules and fresh activation buffers; returns (theta,
    acts, amax) -- the two buffers are what the backward call needs besides ``plan``."""
    name = "tfk_convnet_train_forward"
    N, c, h, w = x.shape
    (w_m1, b_m1, w1, b1, g1, be1, w2, b2, g2, be2, w3, b3, g3, be3, w_m2, b_m2, w_lin, b_lin) = params
    M = w_lin.shape[0]
    dev = x.device
    acts = torch.empty(N * CONVNET_ACT_FLOATS + 80 + 18 * M, dtype=torch.float32, device=dev)
    amax = torch.empty(N * CONVNET_AMAX_BYTES, dtype=torch.uint8, device=dev)
    theta = torch.empty(N, M, dtype=torch.float32, device=dev)
    p = plan
    p.mod1_w, p.mod1_b, p.mod2_w, p.mod2_b = w_m1.data_ptr(), b_m1.data_ptr(), w_m2.data_ptr(), b_m2.data_ptr()
    p.lin_w, p.lin_b = w_lin.data_ptr(), b_lin.data_ptr()
    for k, (cw, cb, bw, bb, bn) in enumerate(((w1, b1, g1, be1, bns[0]), (w2, b2, g2, be2, bns[1]), (w3, b3, g3, be3, bns[2]))):
        p.conv_w[k], p.conv_b[k], p.bn_w[k], p.bn_b[k] = cw.data_ptr(), cb.data_ptr(), bw.data_ptr(), bb.data_ptr()
        p.bn_mean[k], p.bn_var[k] = bn.running_mean.data_ptr(), bn.running_var.data_ptr()
        p.bn_count[k] = None if bn.num_batches_tracked is None else bn.num_batches_tracked.data_ptr()
        p.bn_eps[k], p.bn_momentum[k] = float(bn.eps), float(bn.momentum)
    p.c, p.h, p.w, p.kh, p.kw, p.M = c, h, w, w_m1.shape[2], w_m1.shape[3], M
    base, fs = acts.data_ptr(), 4
    off = 0
    p.a0 = base
    off += N * 4096
    for k, n_el in enumerate((2048, 512, 64)):
        p.y[k] = base + off * fs
        off += N * n_el
    p.a16 = base + off * fs
    off += N * 16
    for k, n_el in enumerate((32, 32, 16)):
        p.stats[k] = base + off * fs
        off += n_el
    p.lin_fold = base + off * fs
    ab = amax.data_ptr()
    p.amax[0], p.amax[1], p.amax[2] = ab, ab + N * 2048, ab + N * (2048 + 512)
    p.workspace = convnet_train_workspace(x).data_ptr()
    _launch(name, x, C.byref(p), _f32(x, name), theta.data_ptr(), N, 1 if training else 0, 1 if update_running else 0,
            n=7)      # (seven kernel launches behind the one FFI crossing)
    return theta, acts, amax


def convnet_train_backward(plan: "ConvNetTrainPlan", x, g_theta, training: bool):
    """The reverse pass of the whole network in ONE call (tfk_convnet_train_backward; ``plan`` as the forward call left it,
    its buffers alive): (g_x, bn_out (100 floats), sums) -- the layout of ``sums`` is in include/tfk.h."""
    name = "tfk_convnet_train_backward"
    N = x.shape[0]
    p = plan
    n_sums = int(lib().tfk_convnet_train_sums_floats(p.c, p.kh, p.kw, p.M))
    g_x = torch.empty_like(x)
    scratch = torch.empty(N * CONVNET_SCRATCH_FLOATS, dtype=torch.float32, device=x.device)
    out = torch.empty(100 + n_sums, dtype=torch.float32, device=x.device)     # (its slices become the .grad tensors)
    base = out.data_ptr()
    _launch(name, x, C.byref(p), _f32(x, name), _f32(g_theta, name), g_x.data_ptr(), scratch.data_ptr(), base, base + 400, N,
            1 if training else 0, n=7)
    return g_x, out[:100], out[100:]


def convnet_train_block_fwd(x, in_affine, weight, bias, bn, training: bool, update_running: bool):
    """One ConvNetBlock (conv3x3 -> ReLU -> MaxPool2d(2)) ahead of its BatchNorm ``bn``: returns (y before
    normalisation, argmax bytes, stats = scale | shift | mean | 1/std of that BatchNorm); ``in_affine``: the scale | shift
    of the BatchNorm in front of the block (applied on load) or None."""
    name = "tfk_convnet_train_block_fwd"
    N, c_in, H, W = x.shape
    c_out = weight.shape[0]
    y = torch.empty(N, c_out, H // 2, W // 2, dtype=torch.float32, device=x.device)
    amax = torch.empty(N, c_out, H // 2, W // 2, dtype=torch.uint8, device=x.device)
    stats = torch.empty(4 * c_out, dtype=torch.float32, device=x.device)
    nb = bn.num_batches_tracked
    momentum = 0.0 if bn.momentum is None else float(bn.momentum)
    ws = convnet_train_workspace(x)
    _launch(name, x, _f32(x, name), _f32(in_affine, name), _f32(weight, name), _f32(bias, name), _f32(y, name), amax.data_ptr(),
            _f32(bn.weight, name), _f32(bn.bias, name), _f32(bn.running_mean, name), _f32(bn.running_var, name),
            None if nb is None else nb.data_ptr(), float(bn.eps), momentum, 1 if training else 0,
            1 if update_running else 0, _f32(stats, name), ws.data_ptr(), N, c_in, c_out, H, W)
    return y, amax, stats


def convnet_train_block_bwd(gz, coef, y, amax, x, in_affine, weight, bn_stats, bn_training: bool):
    """Reverse mode of the block: returns (g_in, weight gradient, bias gradient, and -- when the input came through a
    BatchNorm with ``bn_stats`` -- (coef, d weight, d bias) of that BatchNorm, else None)."""
    name = "tfk_convnet_train_block_bwd"
    N, c_in, H, _ = x.shape
    c_out = weight.shape[0]
    g_in = torch.empty_like(x)
    sums = torch.empty(c_out * c_in * 9 + c_out, dtype=torch.float32, device=x.device)
    bnout = None
    if bn_stats is not None:
        bnout = torch.empty(5 * c_in, dtype=torch.float32, device=x.device)
    ws = convnet_train_workspace(x)
    _launch(name, x, _f32(gz, name), _f32(coef, name), _f32(y, name), amax.data_ptr(), _f32(x, name), _f32(in_affine, name),
            _f32(weight, name), _f32(g_in, name), _f32(sums, name), _f32(bn_stats, name),
            None if bnout is None else bnout.data_ptr(), None if bnout is None else bnout[3 * c_in:].data_ptr(),
            None if bnout is None else bnout[4 * c_in:].data_ptr(), 1 if bn_training else 0, ws.data_ptr(), N, c_in,
            c_out, H)
    dW, db = sums[:c_out * c_in * 9].view(c_out, c_in, 3, 3), sums[c_out * c_in * 9:]
    prev = None if bnout is None else (bnout[:3 * c_in], bnout[3 * c_in:4 * c_in], bnout[4 * c_in:])
    return g_in, dW, db, prev


def convnet_train_frame_fwd(x, in_affine, weight, bias, h_out: int, w_out: int):
    """ConvModifier (weight (c_out, c_in, kh, kw), kh / kw 1 or 2), the BatchNorm in front applied on load."""
    name = "tfk_convnet_train_frame_fwd"
    N, c_in, H, W = x.shape
    c_out, _, kh, kw = weight.shape
    out = torch.empty(N, c_out, h_out, w_out, dtype=torch.float32, device=x.device)
    _launch(name, x, _f32(x, name), _f32(in_affine, name), _f32(weight, name), _f32(bias, name), _f32(out, name),
            N, c_in, c_out, H, W, h_out, w_out, kh, kw)
    return out


def convnet_train_frame_bwd(g_out, x, in_affine, weight, bn_stats, bn_training: bool):
    """Reverse mode of the ConvModifier: (g_in, weight gradient (c_out, c_in, kh, kw), bias gradient (c_out), BatchNorm
    triple or None as in ``convnet_train_block_bwd``)."""
    name = "tfk_convnet_train_frame_bwd"
    N, c_in, H, W = x.shape
    _, c_out, h_out, w_out = g_out.shape
    kh, kw = weight.shape[2:]
    g_in = torch.empty_like(x)
    K0 = c_out * c_in * kh * kw
    K1 = K0 + 2 * c_in
    sums = torch.empty(K1 + c_out, dtype=torch.float32, device=x.device)
    bnout = None
    if bn_stats is not None:
        bnout = torch.empty(5 * c_in, dtype=torch.float32, device=x.device)
    ws = convnet_train_workspace(x)
    _launch(name, x, _f32(g_out, name), _f32(x, name), _f32(in_affine, name), _f32(weight, name), _f32(g_in, name),
            _f32(sums, name), _f32(bn_stats, name), None if bnout is None else bnout.data_ptr(),
            None if bnout is None else bnout[3 * c_in:].data_ptr(), None if bnout is None else bnout[4 * c_in:].data_ptr(),
            1 if bn_training else 0, ws.data_ptr(), N, c_in, c_out, H, W, h_out, w_out, kh, kw)
    prev = None if bnout is None else (bnout[:3 * c_in], bnout[3 * c_in:4 * c_in], bnout[4 * c_in:])
    return g_in, sums[:K0].view(c_out, c_in, kh, kw), sums[K1:], prev


def convnet_train_linear_prep(weight, bias, frame_bias, h_out: int, w_out: int):
    """The Linear layer behind the second ConvModifier folded to its 16 interior inputs: (W16 (M, 16), b_eff (M), w_frame
    (M)); weight (M, h_out * w_out), ``frame_bias`` the modifier's bias (1 element)."""
    name = "tfk_convnet_train_linear_prep"
    M = weight.shape[0]
    buf = torch.empty(M * 18, dtype=torch.float32, device=weight.device)
    W16, b_eff, w_frame = buf[:M * 16].view(M, 16), buf[M * 16:M * 17], buf[M * 17:]
    _launch(name, weight, _f32(weight, name), _f32(bias, name), _f32(frame_bias, name), W16.data_ptr(), b_eff.data_ptr(),
            w_frame.data_ptr(), M, h_out, w_out)
    return W16, b_eff, w_frame


def convnet_train_linear_fwd(a16, W16, b_eff):
    """b_eff + a16 (N, 16) W16 (M, 16)^T -> (N, M)."""
    name = "tfk_convnet_train_linear_fwd"
    N, M = a16.shape[0], W16.shape[0]
    out = torch.empty(N, M, dtype=torch.float32, device=a16.device)
    _launch(name, a16, _f32(a16, name), W16.data_ptr(), b_eff.data_ptr(), _f32(out, name), N, M)
    return out


def convnet_train_linear_bwd_input(g, W16):
    """g (N, M) W16 (M, 16) -> (N, 16)."""
    name = "tfk_convnet_train_linear_bwd_input"
    N, M = g.shape
    g16 = torch.empty(N, 16, dtype=torch.float32, device=g.device)
    _launch(name, g, _f32(g, name), W16.data_ptr(), _f32(g16, name), N, M)
    return g16


def convnet_train_linear_wgrad(g, a16, frame_bias, h_out: int, w_out: int):
    """(dW (M, h_out * w_out), db (M)) of the Linear layer behind the second ConvModifier, whose input equals
    ``frame_bias`` outside the 4 x 4 interior a16 (N, 16)."""
    name = "tfk_convnet_train_linear_wgrad"
    N, M = g.shape
    dW = torch.empty(M, h_out * w_out, dtype=torch.float32, device=g.device)
    db = torch.empty(M, dtype=torch.float32, device=g.device)
    _launch(name, g, _f32(g, name), _f32(a16, name), _f32(frame_bias, name), _f32(dW, name), _f32(db, name), N, M, h_out, w_out)
    return dW, db


def _pack_ops(ops):
    """Host-side op records: int32[8] each = kind, src_plane, H (or GEMM-2 steps), offset, K and
    the fp32 bit patterns of boundary, scale, c (spline ops only).  An array that is already
    packed (``fused.Segment.packed_ops``) passes through."""
    if isinstance(ops, C.Array):
        return ops
    key = tuple(ops)                      # (the training step packs the same few one- and two-op programs every step)
    hit = _OPS_CACHE.get(key)
    if hit is not None:
        return hit
    arr = _pack_ops_uncached(ops)
    if len(_OPS_CACHE) > 256:
        _OPS_CACHE.clear()
    _OPS_CACHE[key] = arr
    return arr


_OPS_CACHE = {}


def _pack_ops_uncached(ops):
    flat = []
    for op in ops:
        kind, plane, H, off = (int(v) for v in op[:4])
        K = int(op[4]) if len(op) > 4 else 0
        fl = [float(v) for v in op[5:8]] + [0.0] * (3 - len(op[5:8]))
        bits = struct.unpack("<3i", struct.pack("<3f", *fl))
        flat += [kind, plane, H, off, K, *bits]
    return (_i32 * max(len(flat), 1))(*flat)


def _n_ops(ops) -> int:
    return len(ops) // 8 if isinstance(ops, C.Array) else len(ops)


def _flow_sizes(name, N, D, gauss_width, z, logdet, logprob, gauss_loc, gauss_log_scale):
    """The element counts the tfk_flow_run family asks of its optional outputs and of the base-density parameters (spelled
    out: no tuples are built on the launch path)."""
    if z is not None and z.numel() != N * D:
        raise NativeError(f"{name}: tensor with {z.numel()} elements, expected {N * D}")
    if logdet is not None and logdet.numel() != N:
        raise NativeError(f"{name}: tensor with {logdet.numel()} elements, expected {N}")
    if logprob is not None and logprob.numel() != N:
        raise NativeError(f"{name}: tensor with {logprob.numel()} elements, expected {N}")
    if gauss_loc is not None and gauss_loc.numel() != gauss_width:
        raise NativeError(f"{name}: tensor with {gauss_loc.numel()} elements, expected {gauss_width}")
    if gauss_log_scale is not None and gauss_log_scale.numel() != gauss_width:
        raise NativeError(f"{name}: tensor with {gauss_log_scale.numel()} elements, expected {gauss_width}")


def flow_run(x, z, logdet, gauss_loc, gauss_log_scale, logprob, ops, params, accumulate=False):
    """Fused flow program (tfk_flow_run).  ops: list of (kind, src_plane, H, offset[, K,
    boundary, scale, c]) tuples (host side), params: fp32 device block.  z / logdet / logprob
    may be None."""
    name = "tfk_flow_run"
    N, D = _rows(x, name)
    ops_arr = _pack_ops(ops)
    _flow_sizes(name, N, D, D, z, logdet, logprob, gauss_loc, gauss_log_scale)
    _launch(name, x, _f32(x, name), _f32(z, name), _f32(logdet, name), _f32(gauss_loc, name), _f32(gauss_log_scale, name),
            _f32(logprob, name), N, D, ops_arr, _n_ops(ops), _f32(params, name), params.numel(), 1 if accumulate else 0)


def _stream_flag() -> int:
    """Flag bit 3 of tfk_flow_run_mfma: stream the operands of an affine / shift chain (D >= 128) even if they fit the LDS
    (tuning: TORCHFLOWS_AMD_DEBUG=stream_chain=force)."""
    from torchflows_amd.utils import debug_switch
    return 8 if debug_switch("stream_chain", "1") == "force" else 0


_sum_ws = {}      # (device index, stream handle) -> zero-initialised workspace of tfk_flow_run_mfma_sum (resets itself)


def flow_sum_workspace(t: torch.Tensor) -> torch.Tensor:
    key = (t.device.index, _stream(t))
    ws = _sum_ws.get(key)
    if ws is None:
        ws = _sum_ws[key] = torch.zeros(int(lib().tfk_flow_sum_workspace_bytes()) // 8, dtype=torch.float64, device=t.device)
    return ws


def flow_run_mfma(x, z, logdet, gauss_loc, gauss_log_scale, logprob, ops, params, accumulate=False,
                  reverse_out=False, base_of_input=False, D=None, context=None, sum_out=None):
    """Fused flow program with the conditioner GEMMs on the matrix cores (tfk_flow_run_mfma).
    ops: list of (kind, src_plane, gemm2_steps, offset); params packed by flow_pack._pack_mfma.
    ``D``: the kernel's row width when ``x`` is narrower (lean programs, tfk_flow_run_mfma_in): x (N, x_width) is read
    half by half into the heads of the two planes."""
    name = "tfk_flow_run_mfma"
    N, xw = _rows(x, name)
    Dk, lead, trail = xw, (), ()          # the entry point's row width, its arguments behind x and behind the flag word
    if sum_out is not None:               # lean program + the fp64 sum of its log-probabilities (tfk_flow_run_mfma_sum)
        name = "tfk_flow_run_mfma_sum"
        if context is not None or logprob is None or sum_out.dtype != torch.float64 or sum_out.numel() != 1:
            raise NativeError(f"{name}: needs logprob, a 1-element float64 sum_out and no context")
        Dk = xw if D is None else D
        lead, trail = (xw,), (flow_sum_workspace(x).data_ptr(), sum_out.data_ptr())
    elif context is not None:             # context-conditioned program (tfk_flow_run_mfma_ctx); rows at full width
        name = "tfk_flow_run_mfma_ctx"
        if context.dim() != 2 or context.shape[0] != N:
            raise NativeError(f"{name}: context must be (N, C), got {tuple(context.shape)}")
        lead = (_f32(context, name), int(context.shape[1]))
    elif D is not None and D != xw:
        name = "tfk_flow_run_mfma_in"
        Dk, lead = D, (xw,)
    ops_arr = _pack_ops(ops)
    _flow_sizes(name, N, Dk, Dk, z, logdet, logprob, gauss_loc, gauss_log_scale)
    _launch(name, x, _f32(x, name), *lead, _f32(z, name), _f32(logdet, name), _f32(gauss_loc, name),
            _f32(gauss_log_scale, name), _f32(logprob, name), N, Dk, ops_arr, _n_ops(ops), _f32(params, name), params.numel(),
            (1 if accumulate else 0) | (2 if reverse_out else 0) | (4 if base_of_input else 0) | _stream_flag(), *trail)


def flow_run_wide(x, z, logdet, gauss_loc, gauss_log_scale, logprob, ops, params, accumulate=False,
                  reverse_out=False, base_of_input=False):
    """Chain of affine / shift couplings on an even event size in (256, 2048] as one launch (tfk_flow_run_wide).
    x / z (N, D) at the logical width; ops and params packed by fused_wide.compile_wide; gauss_loc / gauss_log_scale in the
    kernel's column order (2 x the padded plane width).  z / logdet / logprob may be None."""
    name = "tfk_flow_run_wide"
    N, D = _rows(x, name)
    hp2 = 2 * ((D // 2 + 63) // 64 * 64)
    ops_arr = _pack_ops(ops)
    _flow_sizes(name, N, D, hp2, z, logdet, logprob, gauss_loc, gauss_log_scale)
    _launch(name, x, _f32(x, name), _f32(z, name), _f32(logdet, name), _f32(gauss_loc, name), _f32(gauss_log_scale, name),
            _f32(logprob, name), N, D, ops_arr, _n_ops(ops), _f32(params, name), params.numel(),
            (1 if accumulate else 0) | (2 if reverse_out else 0) | (4 if base_of_input else 0))


def glow_plan(layer: GlowLayer, D: int) -> dict:
    """The launch shape libtfk picks for this layer (or the overrides, validated)."""
    vals = [_i32(0) for _ in range(6)]
    rc = lib().tfk_glow_plan(C.byref(layer), D, *[C.byref(v) for v in vals])
    _check(rc, "tfk_glow_plan")
    return dict(zip(("slots", "block", "cg1", "cg2", "lds_bytes", "tile_rows"), (int(v.value) for v in vals)))


def glow_coupling(rows: torch.Tensor, logdet: torch.Tensor, layer: GlowLayer, inverse: bool = False) -> None:
    """One convolutional coupling in place on the rows (conditioner, bounded output, transform, log-det added)."""
    name = "tfk_glow_coupling"
    N, D = _rows(rows, name)
    if logdet.numel() != N:
        raise NativeError(f"tfk_glow_coupling: logdet has {logdet.numel()} elements, expected {N}")
    _launch(name, rows, _f32(rows, name), _f32(logdet, name), N, D, C.byref(layer), 1 if inverse else 0)


def glow_level_pack(steps, D: int, D_level: int, samples: int = 0, block: int = 0) -> torch.Tensor:
    """The host copy of a level program's blob (uint8 CPU tensor): launch shape, geometry and background cell lists of
    ``steps`` (a ctypes array of GlowLevelStep whose pointers are DEVICE pointers).  Pure host work, no GPU needed."""
    n = len(steps)
    nbytes = int(lib().tfk_glow_level_blob_bytes(steps, n, int(D), int(D_level), int(samples), int(block)))
    if nbytes <= 0:
        _check(-nbytes if nbytes < 0 else 1, "tfk_glow_level_blob_bytes")
    blob = torch.zeros(nbytes, dtype=torch.uint8)
    rc = lib().tfk_glow_level_pack(steps, n, int(D), int(D_level), int(samples), int(block), blob.data_ptr(), nbytes)
    _check(rc, "tfk_glow_level_pack")
    return blob


def glow_level_info(blob_host: torch.Tensor) -> dict:
    vals = [_i32(0) for _ in range(4)]
    rc = lib().tfk_glow_level_info(blob_host.data_ptr(), *[C.byref(v) for v in vals])
    _check(rc, "tfk_glow_level_info")
    return dict(zip(("samples", "block", "lds_bytes", "wgs_per_cu"), (int(v.value) for v in vals)))


def glow_level(rows_in: torch.Tensor, rows_out: torch.Tensor, logdet: torch.Tensor, row_idx: Optional[torch.Tensor],
               blob_host: torch.Tensor, blob_dev: torch.Tensor) -> None:
    """The couplings of one level back to back on rows held in the LDS (in place unless the level covers the whole row)."""
    name = "tfk_glow_level"
    N, D = _rows(rows_out, name)
    if rows_in.shape != rows_out.shape or logdet.numel() != N:
        raise NativeError(f"{name}: rows_in {tuple(rows_in.shape)}, rows_out {tuple(rows_out.shape)}, logdet {logdet.numel()}")
    if row_idx is not None and (row_idx.dtype != torch.int32 or row_idx.device != rows_out.device):
        raise NativeError(f"{name}: row_idx must be an int32 tensor on the rows' device")
    if blob_host.device.type != "cpu" or blob_dev.device != rows_out.device:
        raise NativeError(f"{name}: the blob's two copies must live on the host and on the rows' device")
    _launch(name, rows_out, _f32(rows_in, name), _f32(rows_out, name), _f32(logdet, name), N, D,
            None if row_idx is None else row_idx.data_ptr(), blob_host.data_ptr(), blob_dev.data_ptr())


def rows_fma(rows: torch.Tensor, st: torch.Tensor) -> None:
    """rows[n, d] = st[d, 0] * rows[n, d] + st[d, 1] in place."""
    name = "tfk_rows_fma"
    N, D = _rows(rows, name)
    if st.numel() != 2 * D:
        raise NativeError(f"tfk_rows_fma: st has {st.numel()} elements, expected 2 * {D}")
    _launch(name, rows, _f32(rows, name), _f32(st, name), N, D)


def rows_fma_gauss_logprob(rows, st, loc, log_scale, logdet_in, out) -> None:
    """out[n] = base log-density of st[d, 0] * rows[n, d] + st[d, 1] (+ logdet_in[n]); the rows are only read."""
    name = "tfk_rows_fma_gauss_logprob"
    N, D = _rows(rows, name)
    if st.numel() != 2 * D or loc.numel() != D or log_scale.numel() != D or out.numel() != N:
        raise NativeError(f"{name}: bad parameter / out shape")
    _launch(name, rows, _f32(rows, name), _f32(st, name), _f32(loc, name), _f32(log_scale, name), _f32(logdet_in, name),
            _f32(out, name), N, D)


def sum_f32(values: torch.Tensor) -> torch.Tensor:
    """fp64 sum of an fp32 vector as a 1-element float64 device tensor (feeds the all-reduce)."""
    v = values.reshape(-1)
    N = v.numel()
    _f32(v, "tfk_sum_f32")
    out = torch.empty(1, dtype=torch.float64, device=v.device)
    if N < (1 << 14):                 # one workgroup, no workspace (SURVEY 8(b)'s four-argument form)
        _launch("tfk_sum_f32", v, v.data_ptr(), out.data_ptr(), N)
    else:
        ws = torch.empty(int(lib().tfk_sum_workspace_bytes(N)), dtype=torch.uint8, device=v.device)
        _launch("tfk_sum_f32_ws", v, v.data_ptr(), out.data_ptr(), ws.data_ptr(), N)
    return out


def device_info():
    name = C.create_string_buffer(256)
    cus = _i32(0)
    rc = lib().tfk_device_info(name, 256, C.byref(cus))
    _check(rc, "tfk_device_info")
    return name.value.decode(), int(cus.value)
