"""The route from a ``BijectiveComposition`` to libtfk *flow programs*: what a compiled chain is (``Segment``,
``CompiledChain``), the cache of compiled chains with its version / epoch / guard machinery (``get_compiled``,
``invalidate``), the warning for compositions the compiler declines, and ``run_chain``, which launches a chain.

The compiler itself is ``flow_compile.compile_chain`` (layers -> ops), the operand layouts are ``flow_pack``'s, the op
codes and the table of lean kinds ``flow_ops``'s; ``fused_wide`` holds the packer and launcher of event sizes above 256.
Programs are cached per (direction, device) and rebuilt when any parameter version changes.
"""
from __future__ import annotations

import os
import warnings
from dataclasses import dataclass
from typing import List, Optional

import torch
import torch.nn as nn

from torchflows_amd.utils import debug_switch

from torchflows_amd import native
from torchflows_amd.flow_ops import COUPLING_FAMILIES, FORWARD, LEAN_BY_OP, OP_EW_FMA
from torchflows_amd.flow_ops import OP_AFFINE_FWD_LEAN, OP_MADE_FWD_LEAN  # noqa: F401  (callers name them through here)


def compile_chain(composition, direction: int, device: torch.device, mfma: Optional[bool] = None,
                  context: bool = False) -> Optional["CompiledChain"]:
    """``flow_compile.compile_chain``: flow programs for ``composition.forward`` (direction 0) or ``.inverse`` (1), or
    None.  (Looked up at call time: the compiler imports this module for ``Segment`` and ``CompiledChain``.)"""
    from torchflows_amd import flow_compile
    return flow_compile.compile_chain(composition, direction, device, mfma=mfma, context=context)


def __getattr__(name: str):
    """Compatibility only: ``_flatten``, ``_compile_lean`` and ``_lean_coupling`` live in ``flow_compile``; code written
    against earlier releases reached them as ``fused._...`` and still finds them (looked up at call time: ``flow_compile``
    imports this module).  New code imports them from ``flow_compile``."""
    if name in ("_flatten", "_compile_lean", "_lean_coupling"):
        from torchflows_amd import flow_compile
        return getattr(flow_compile, name)
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")


def enabled() -> bool:
    return os.environ.get("TORCHFLOWS_AMD_FUSED", "1") != "0"


def mfma_enabled() -> bool:
    return os.environ.get("TORCHFLOWS_AMD_MFMA", "1") != "0"


@dataclass
class Segment:
    ops: List[tuple]                          # (kind, src_plane, H, offset[, K, boundary, scale, c])
    params: torch.Tensor                      # fp32 device block, numel % 4 == 0
    mfma: bool = False                        # packed for tfk_flow_run_mfma (matrix-core conditioner)
    wide: bool = False                        # packed for tfk_flow_run_wide (event sizes above 256, fused_wide.py)

    def packed_ops(self):
        """The op records as the ctypes array the C-ABI takes, built once per segment."""
        arr = self.__dict__.get("_ops_c")
        if arr is None:
            arr = self.__dict__["_ops_c"] = native._pack_ops(self.ops)
        return arr


@dataclass
class CompiledChain:
    D: int                     # width of the rows the kernels see (padded: 64 / 128 / 256)
    segments: List[Segment]
    pos: torch.Tensor          # int64 (D_log,): physical position of logical element l at the end
    identity_out: bool         # rows come out in logical order
    version: int
    D_log: int = 0             # event size; < D when the two halves are padded to a supported width
    pos_in: Optional[torch.Tensor] = None     # padded chains: physical position of logical element l on entry
    ctx_width: Optional[int] = None           # context programs: elements per context row the packed weights expect

    def reversed_out(self) -> bool:
        """The rows come out exactly reversed (an odd number of ReversePermutationMatrix layers behind the last fold) and
        the last launch is a matrix-core one: its store writes column c to D - 1 - c (flag bit 1 of tfk_flow_run_mfma)
        instead of a tfk_permute pass over the rows afterwards."""
        hit = self.__dict__.get("_reversed_out")
        if hit is None:
            hit = (not self.identity_out and self.pos_in is None and bool(self.segments) and self.segments[-1].mfma
                   and self.pos.numel() == self.D
                   and bool(torch.equal(self.pos, torch.arange(self.D - 1, -1, -1, device=self.pos.device))))
            self.__dict__["_reversed_out"] = hit
        return hit


def _tensor_slots(module: nn.Module):
    """[(owner dict, name, tensor)] for every parameter and buffer below ``module``."""
    slots = []
    for m in module.modules():
        for owner in (m._parameters, m._buffers):
            for k, t in owner.items():
                if t is not None:
                    slots.append((owner, k, t))
    return slots


# Bumped whenever ANY module of this package has its tensors moved or converted (``_apply``: .to() / .cuda() /
# .double() ...) and whenever a tensor slot is found replaced: mixed into every version below, so that a cache entry built
# before such an event -- under any key, on the moved module or on an ancestor whose program packs its weights -- can never
# match again.  (A move keeps the tensor objects and their version counters; only the storage changes.)
_EPOCH = [0]


def _params_version(module: nn.Module) -> int:
    """Changes whenever a parameter / buffer below ``module`` is modified in place (version counter) or replaced by
    another tensor (slot identity).  Moves and conversions (``.to()``, ``.cuda()``, ``.double()``: the tensor object
    stays, its storage changes) are caught by ``Bijection._apply`` / ``BaseFlow._apply``, which drop the caches -- so
    the per-call check is ONE pass over a flat list reading ``_version`` (the ``data_ptr()`` walk this replaces cost
    ~35 us of the ~57 us a small-batch ``log_prob`` call spent on the host)."""
    slots = _slots(module)
    for owner, k, t in slots:
        if owner.get(k) is not t:                     # a tensor was replaced: re-walk the tree, retire every older entry
            slots = module.__dict__["_tfk_slots"] = _tensor_slots(module)
            module.__dict__.pop("_tfk_static_ok", None)
            _EPOCH[0] += 1
            break
    v = len(slots) + 1000003 * _EPOCH[0]
    for _, _, t in slots:
        v = v * 1000003 + t._version
    return v & 0xFFFFFFFFFFFFFFF


def _slots(module: nn.Module):
    """The cached slot list of ``module`` (rebuilt when a tensor is replaced; dropped by ``_apply`` when tensors move)."""
    slots = module.__dict__.get("_tfk_slots")
    if slots is None:
        slots = module.__dict__["_tfk_slots"] = _tensor_slots(module)
    return slots


def static_ok(module: nn.Module) -> bool:
    """Every floating-point parameter / buffer below ``module`` is fp32 on one HIP device (cached until a tensor moves:
    ``_apply`` drops the cache)."""
    hit = module.__dict__.get("_tfk_static_ok")
    if hit is not None and hit[0] == _EPOCH[0]:
        return hit[1]
    devices = set()
    ok = True
    for _, _, t in _slots(module):
        if t.is_floating_point():
            devices.add(t.device)
            ok = ok and t.device.type == "cuda" and t.dtype == torch.float32
    ok = ok and len(devices) <= 1
    module.__dict__["_tfk_static_ok"] = (_EPOCH[0], ok)
    return ok


def tensors_moved(module: nn.Module) -> None:
    """Called from ``_apply`` (``.to()`` / ``.cuda()`` / ``.float()`` ...): every cache that depends on where the
    tensors live or on their values is dropped, on this module and -- because a parent's program packs this module's
    weights -- this is also invoked for every ancestor that is itself being moved (Module._apply recurses)."""
    _EPOCH[0] += 1                      # ancestors that are NOT being moved hold programs packed from these tensors too
    for m in module.modules():          # (submodules that are not bijections -- conditioner blocks -- keep caches too)
        d = m.__dict__
        for k in [k for k in d if k.startswith("_tfk_") and k != "_tfk_declined_warned"]:
            del d[k]


def any_requires_grad(module: nn.Module) -> bool:
    return any(t.requires_grad for _, _, t in _slots(module))


def narrow_enabled() -> bool:
    return debug_switch("narrow_in", "1") != "0"


def sample_ready(chain: Optional[CompiledChain]) -> bool:
    """One matrix-core launch: the base density of the incoming rows can ride along (flag bit 2)."""
    return (chain is not None and len(chain.segments) == 1 and chain.segments[0].mfma
            and (chain.pos_in is None or chain.segments[0].wide))


def invalidate(module: nn.Module, compiled_only: bool = False) -> None:
    """Drop EVERY cached packing below ``module``: compiled flow programs (``_tfk_compiled``), MADE weight packs,
    elementwise blocks, BatchNorm scale / shift, image programs, training packs, the flat tensor lists.  The caches are
    keyed on the tensors' autograd version counters, on slot identity (a replaced Parameter) and on a process-wide epoch
    that every ``.to()`` / ``.cuda()`` / dtype conversion of a module of this package bumps -- NOT on data pointers.  An
    in-place edit through ``.data`` (``p.data.mul_(0.5)``, manual weight averaging or clamping), an assignment
    ``p.data = other`` or a replayed hipGraph moves none of these.  After such an
    edit call this (``Bijection.invalidate_native_caches()`` / ``Flow.invalidate_native_caches()``); ``train()`` /
    ``eval()`` and ``load_state_dict`` call it themselves.
    ``compiled_only``: just the compiled flow programs -- what ``Flow.fit`` drops after an epoch of hipGraph replays
    (the captured graph keeps READING the other packs' tensors on every replay, so those must stay allocated)."""
    for m in module.modules():
        d = m.__dict__
        if compiled_only:
            d.pop("_tfk_compiled", None)
            continue
        for k in [k for k in d if k.startswith("_tfk_") and k not in _STRUCTURAL_CACHES]:
            del d[k]


# caches that hold no parameter VALUES -- index maps of the training packs (keyed on layer identity, direction and
# device), the flat tensor-slot list and the dtype / device check -- and therefore never go stale through a value
# edit.  They must survive invalidate(): a captured hipGraph of the training step (Flow.fit, TORCHFLOWS_AMD_GRAPH=1)
# reads the packs' index tensors on every replay, and fit() invalidates after every epoch of replays.
_STRUCTURAL_CACHES = ("_tfk_plan_packs", "_tfk_slots", "_tfk_declined_warned")
# (the (module, name) slot lists of the L2 term and of the autograd node -- "_tfk_l2_slots", "_tfk_param_slots" -- hold no
# tensors and are rebuilt in microseconds: invalidate() drops them like any other cache)


_CACHE_CHECK = int(debug_switch("cache_check", "0") or 0)
_cache_calls = 0

# Edits through ``.data`` (``p.data.mul_(...)``) move no version counter: a compiled program would go on serving the old
# weights in silence -- a hazard the reference does not have (it reads the live tensors on every call).  Default guard,
# WITHOUT a host synchronisation on the hit path: every GUARD_EVERY-th hit of a compiled program on a HIP device enqueues a
# checksum of the live tensors (two multi-tensor kernels), its comparison with the checksum taken when the program was
# packed, and a copy of the verdict into pinned host memory; the verdict is READ on a later hit, once its event has
# completed.  A mismatch drops every packed copy below the composition, warns, and recompiles in the same call.  A stale
# program can therefore serve at most ~2 GUARD_EVERY calls after such an edit (TORCHFLOWS_AMD_DEBUG=guard_every=N; 0 = off);
# ``invalidate_native_caches()`` right after the edit stays the way to serve none.
GUARD_EVERY = int(debug_switch("guard_every", "64") or 0)


class StaleProgramWarning(UserWarning):
    """Parameters changed without their version counters moving (an edit through ``.data``); the packed copies were
    dropped and rebuilt."""


def _device_checksum(module: nn.Module) -> Optional[torch.Tensor]:
    """0-dim fp64 device tensor: a position-weighted checksum of every fp32 parameter / buffer below ``module``."""
    ts = [t.detach() for t in list(module.parameters()) + list(module.buffers())
          if t.is_floating_point() and t.numel() and t.is_cuda]
    if not ts:
        return None
    n1 = torch.stack(torch._foreach_norm(ts, 1)).double()          # sum |x|
    n2 = torch.stack(torch._foreach_norm(ts, 2)).double()          # sqrt(sum x^2)
    w = torch.arange(1, len(ts) + 1, dtype=torch.float64, device=n1.device)
    return (n1 * w).sum() + 3.0 * (n2 * w).sum()


class _Guard:
    __slots__ = ("packed", "hits", "flag", "event")

    def __init__(self, module: nn.Module):
        self.packed = _device_checksum(module)
        self.hits, self.flag, self.event = 0, None, None

    def stale(self, module: nn.Module) -> bool:
        """Called on every cache hit.  True when an EARLIER check has come back with a mismatch."""
        if self.packed is None or GUARD_EVERY <= 0:
            return False
        if self.event is not None and self.event.query():
            bad = bool(self.flag.item())                              # (pinned host memory, the copy has completed)
            self.event = None
            if bad:
                return True
        self.hits += 1
        if self.hits % GUARD_EVERY == 0 and self.event is None and not torch.cuda.is_current_stream_capturing():
            live = _device_checksum(module)
            if live is not None and live.device == self.packed.device:
                if self.flag is None:
                    self.flag = torch.zeros((), dtype=torch.bool).pin_memory()
                self.flag.copy_(live != self.packed, non_blocking=True)
                self.event = torch.cuda.Event()
                self.event.record()
        return False


def _live_checksum(module: nn.Module) -> float:
    """fp64 sum of all floating-point tensors below ``module`` (one host sync: debug only)."""
    acc = 0.0
    for t in list(module.parameters()) + list(module.buffers()):
        if t.is_floating_point() and t.numel():
            acc += float(t.detach().double().sum()) + 3.0 * float(t.detach().double().abs().sum())
    return acc


def _context_width(composition) -> Optional[int]:
    """Elements per context row the packed weights expect.  A hand-built composition takes its ``context_shape`` from
    its FIRST layer (bijections/base.py:203-209), which is None when an ActNorm or a permutation stands in front of the
    context-conditioned couplings: the width comes from the first layer that does define one (None if none does)."""
    from torchflows_amd.utils import event_size
    if composition.context_shape is not None:
        return event_size(composition.context_shape)
    for m in composition.modules():
        cs = getattr(m, "context_shape", None)
        if m is not composition and cs is not None:
            return event_size(cs)
    return None


def get_compiled(composition, direction: int, device: torch.device, context: bool = False) -> Optional[CompiledChain]:
    """Cached ``compile_chain``; recompiles when a parameter / buffer was modified in place."""
    cache = composition.__dict__.setdefault("_tfk_compiled", {})
    key = (direction, str(device), bool(composition.training), bool(context))
    hit = cache.get(key)
    version = _params_version(composition)
    if (hit is not None and hit[0] == version and device.type == "cuda" and len(hit) > 3 and hit[3] is not None
            and hit[3].stale(composition)):
        warnings.warn("torchflows_amd: parameters below this composition changed without their version counters moving "
                      "(an in-place edit through .data?); the packed copies were served stale for up to "
                      f"{2 * GUARD_EVERY} calls and are rebuilt now -- call invalidate_native_caches() right after such "
                      "edits", StaleProgramWarning, stacklevel=3)
        invalidate(composition)
        cache = composition.__dict__.setdefault("_tfk_compiled", {})
        hit = None
    if hit is not None and hit[0] == version:
        if _CACHE_CHECK:
            # opt-in debug check (TORCHFLOWS_AMD_DEBUG=cache_check=N): every N-th hit compares a checksum of the LIVE
            # tensors with the one taken when the program was packed -- catches edits through ``.data``
            global _cache_calls
            _cache_calls += 1
            if _cache_calls % _CACHE_CHECK == 0 and hit[2] is not None and hit[2] != _live_checksum(composition):
                raise RuntimeError(
                    "torchflows_amd: parameters below this composition changed without their version counters "
                    "moving (an in-place edit through .data?): call invalidate_native_caches() after such edits")
        return hit[1]
    chain = compile_chain(composition, direction, device, context=context)
    if chain is not None and context:
        chain.ctx_width = _context_width(composition)
    guard = _Guard(composition) if (device.type == "cuda" and chain is not None and GUARD_EVERY > 0) else None
    cache[key] = (version, chain, _live_checksum(composition) if _CACHE_CHECK else None, guard)
    if chain is None:
        warn_declined(composition, direction)
    return chain


def warn_declined(composition, direction: int) -> None:
    """Never silent: the layer-by-layer route (one libtfk kernel per reference layer + PyTorch-ROCm conditioner
    GEMMs) is ~10x slower than a flow program.  Said once per composition."""
    if not enabled() or composition.__dict__.get("_tfk_declined_warned"):
        return
    composition.__dict__["_tfk_declined_warned"] = True
    if len(tuple(composition.event_shape)) >= 3:
        return          # image blocks (ConvNet conditioners): one kernel per layer IS their route, nothing was lost
    from torchflows_amd.bijections.finite.autoregressive.layers_base import MaskedAutoregressiveBijection
    from torchflows_amd.flow_compile import _flatten
    order = composition.layers if direction == FORWARD else list(composition.layers)[::-1]
    plan = _flatten(order, "forward" if direction == FORWARD else "inverse") or []
    if any(isinstance(layer, MaskedAutoregressiveBijection) and d == layer._sequential_when for layer, d in plan):
        return          # the element-by-element map of a MADE layer runs as ONE launch per layer (tfk_made_*_sequential)
    warnings.warn("torchflows_amd: this composition is not compiled to a flow program and runs layer by layer on "
                  "the HIP kernels (about 10x slower): " + _why_declined(composition, direction),
                  NativeRouteWarning, stacklevel=4)


class NativeRouteWarning(UserWarning):
    """A composition runs on the slower layer-by-layer route (see ``get_compiled``)."""


def _why_declined(composition, direction: int) -> str:
    """First layer of the chain the flow-program compiler has no op for (best effort, for the warning)."""
    from torchflows_amd.bijections.finite.autoregressive.layers_base import (
        CouplingBijection, ElementwiseBijection, MaskedAutoregressiveBijection)
    from torchflows_amd.bijections.finite.matrix.permutation import PermutationMatrix
    from torchflows_amd.flow_compile import _flatten
    D = composition.n_dim
    order = composition.layers if direction == FORWARD else list(composition.layers)[::-1]
    plan = _flatten(order, "forward" if direction == FORWARD else "inverse")
    if plan is None:
        return "a layer's forward / inverse is not one of this package's implementations"
    # what the kernels back: every event size 3 .. 256 (chain kernels / interpreters, padded where needed), above that
    # EVEN sizes up to 2048 for affine / shift coupling chains with hidden width <= 16 and no context (the wide-row chain
    # kernel, tfk_flow_run_wide), and 512 on the vector-ALU interpreter
    if D < 3 or D > 2048:
        return f"event size {D} is outside the supported range (3 .. 256, and even sizes up to 2048 for affine / shift couplings)"
    if D > 256 and D % 2 == 1:
        return f"event size {D} is odd: above 256 only even event sizes have a flow-program kernel"
    wide_only = D > 256 and D != 512
    for layer, _ in plan:
        if isinstance(layer, PermutationMatrix):
            continue
        name = type(layer).__name__
        if isinstance(layer, (CouplingBijection, MaskedAutoregressiveBijection)):
            ct = layer.conditioner_transform
            what = (f"{name} (transformer {layer.transformer.native_kind or type(layer.transformer).__name__}, "
                    f"conditioner {type(ct).__name__}")
            if layer.context_shape is not None:
                if type(ct).__name__ != "FeedForward" or D > 256:
                    return what + f", context_shape {tuple(layer.context_shape)}" + (
                        f": no context-conditioned flow program above event size 256)" if D > 256 else ")")
            seq = getattr(ct, "sequential", None)
            hidden = getattr(seq[0], "out_features", None) if seq is not None and len(seq) else None
            kind = layer.transformer.native_kind
            plain = type(ct).__name__ in ("FeedForward", "MADE") and hidden is not None
            if wide_only:
                if type(ct).__name__ == "FeedForward" and hidden is not None and hidden <= 16 \
                        and kind in ("affine", "inverse_affine", "shift"):
                    continue
                if type(ct).__name__ == "FeedForward" and hidden is not None and kind in ("affine", "inverse_affine", "shift"):
                    return what + f", hidden width {hidden} > 16 at event size {D}: the wide-row chain kernel holds one " \
                                  f"16-unit hidden tile)"
                return what + (f", hidden width {hidden}" if hidden else "") + \
                    f", event size {D}: above 256 only affine / shift couplings with a FeedForward conditioner run fused)"
            if plain and kind in ("affine", "inverse_affine", "shift") and hidden <= 128:
                continue
            if plain and kind == "rqs" and hidden <= 16 and getattr(layer.transformer, "n_bins", 8) == 8 and D <= 128:
                continue
            return what + (f", hidden width {hidden}" if hidden else "") + f", event size {D})"
        if isinstance(layer, ElementwiseBijection):
            if getattr(layer, "first_training_batch_pass", False) and layer.training:
                return f"{name} still has to initialise itself from a batch (train mode)"
            if not layer.use_global_parameters:
                if type(layer.conditioner_transform).__name__ != "Linear":
                    return f"{name} takes its parameters from the context through a {type(layer.conditioner_transform).__name__}"
                continue
            if layer.transformer.native_kind not in ("affine", "inverse_affine"):
                return f"{name} (transformer {type(layer.transformer).__name__})"
            continue
        return f"{name} has no flow-program op"
    return f"event size {D} / layer mix not covered by one kernel"


def sum_ready(chain: Optional[CompiledChain]) -> bool:
    """One LEAN launch: the fp64 sum of the log-probabilities can ride along (tfk_flow_run_mfma_sum).  Opt-in
    (TORCHFLOWS_AMD_DEBUG=sum_in_kernel=1): measured on RealNVP-64, 2^20 rows, it removes the reduction's two launches (~8 us
    of a 261 us step) and adds ~6 us to the kernel (one agent-scope ticket per workgroup, 3 072 of them): 263.7 against
    261.2 us per step over 20 steps, 239.3 against 241.3 us at the median of 100 -- a wash."""
    return (chain is not None and len(chain.segments) == 1 and chain.segments[0].mfma
            and (chain.segments[0].ops[0][0] in LEAN_BY_OP or chain.segments[0].ops[0][0] == OP_EW_FMA)
            and not chain.segments[0].wide
            and debug_switch("sum_in_kernel", "0") == "1")


def run_chain(chain: CompiledChain, rows: torch.Tensor, want_rows: bool, base=None, base_of_input: bool = False,
              context: Optional[torch.Tensor] = None, sum_out: Optional[torch.Tensor] = None):
    """Apply the compiled chain to ``rows`` (N, D).  Returns ``(out_rows or None, logdet or
    None, logprob or None)``; with ``base`` (loc, log_scale in logical order) the final launch
    also evaluates the diagonal-Gaussian log-density and adds the log-det (flows.py:647-648).
    ``base_of_input`` (single-launch matrix-core programs only, see ``sample_ready``): the density is that
    of the rows as they come in -- ``Flow.sample``'s ``base_log_prob(z) + log_det`` in the same launch.
    ``sum_out`` (1-element float64, ``sum_ready`` chains with ``base``): receives the fp64 sum of the log-probabilities
    from the same launch."""
    assert sum_out is None or (sum_ready(chain) and base is not None and not base_of_input and context is None)
    if chain.segments and chain.segments[0].wide:           # event sizes above 256: one tfk_flow_run_wide launch
        from torchflows_amd import fused_wide
        assert context is None
        return fused_wide.run_wide(chain, rows, want_rows, base=base, base_of_input=base_of_input)
    if context is not None and chain.ctx_width is not None and (context.dim() != 2 or context.shape[1] != chain.ctx_width):
        # the kernels only count 4-wide k-steps: a context of another width would be truncated or zero-padded in
        # silence where the reference's Linear layer raises a shape error (conditioning/context.py:46-60)
        raise ValueError(f"context rows have {tuple(context.shape[1:])} elements, the flow was built for "
                         f"context_shape with {chain.ctx_width}")
    if base_of_input:
        assert sample_ready(chain) and base is not None
        N, D = rows.shape
        logprob = torch.empty(N, dtype=torch.float32, device=rows.device)
        out = torch.empty_like(rows)
        seg = chain.segments[0]
        native.flow_run_mfma(rows, out, None, base[0], base[1], logprob, seg.packed_ops(), seg.params,
                             base_of_input=True, reverse_out=chain.reversed_out())
        if not chain.identity_out and not chain.reversed_out():
            cur, out = out, torch.empty_like(out)
            native.permute(cur, chain.pos.to(torch.int32), out)
        return out, None, logprob
    N, D = rows.shape
    dev = rows.device
    n_seg = len(chain.segments)
    padded = chain.pos_in is not None
    # lean programs read narrower rows themselves (tfk_flow_run_mfma_in): no padding pass over the rows
    # (odd event sizes: the lean affine / shift chains read them in place too -- the interpreter's plane-per-element programs
    # start with an op below OP_AFFINE_FWD_LEAN and take the padding pass)
    # -- that is the coupling chains, and at even sizes a chain that is nothing but its closing TFK_OP_EW_FMA
    narrow_in = padded and n_seg > 0 and chain.segments[0].mfma and context is None and narrow_enabled()
    if narrow_in:
        first = chain.segments[0].ops[0][0]
        kind = LEAN_BY_OP.get(first)
        narrow_in = ((kind is not None and kind.family in COUPLING_FAMILIES)
                     or (first == OP_EW_FMA and chain.D_log % 2 == 0))
    if padded and not narrow_in:                 # (N, D_log) -> (N, D): each half at the head of its plane
        wide = rows.new_zeros(N, chain.D)
        if chain.D_log % 2 == 0:                 # each half at the head of its plane: two strided copies
            half, hp = chain.D_log // 2, chain.D // 2
            wide[:, :half] = rows[:, :half]
            wide[:, hp:hp + half] = rows[:, half:]
        else:                                    # odd sizes: logical element l at column pos_in[l]
            wide.index_copy_(1, chain.pos_in, rows)
        rows = wide
    logprob = torch.empty(N, dtype=torch.float32, device=dev) if base is not None else None
    logdet = torch.empty(N, dtype=torch.float32, device=dev) if (base is None or n_seg > 1) else None
    cur = rows
    buf = None
    if n_seg == 0:                               # only permutations: nothing to launch
        out = rows[:, chain.pos] if want_rows else None
        ld = torch.zeros(N, dtype=torch.float32, device=dev)
        lp = None
        if base is not None:
            native.diag_gauss_logprob(rows[:, chain.pos].contiguous(), base[0], base[1], ld, logprob)
            lp = logprob
        return out, ld, lp
    loc_p = ls_p = None
    if base is not None:                          # base parameters in physical order, cached
        key = (base[0].data_ptr(), base[0]._version, base[1].data_ptr(), base[1]._version)
        hit = chain.__dict__.get("_base_cache")
        if hit is None or hit[0] != key:
            # padding elements hold 0 throughout: loc 0 and log_scale = -0.5 log(2 pi) make their density term
            # -(0 + 0.5 log(2 pi) + log_scale) vanish exactly
            loc_p = base[0].new_zeros(chain.D)
            ls_p = base[1].new_full((chain.D,), -0.9189385332046727)
            loc_p[chain.pos] = base[0]
            ls_p[chain.pos] = base[1]
            chain.__dict__["_base_cache"] = hit = (key, loc_p, ls_p)
        loc_p, ls_p = hit[1], hit[2]
    for i, seg in enumerate(chain.segments):
        last = i == n_seg - 1
        need_rows = (not last) or want_rows
        out = None
        if need_rows:
            if buf is None:
                buf = torch.empty(N, chain.D, dtype=rows.dtype, device=dev)
            out = buf                             # in place from the second segment on
        run = native.flow_run_mfma if seg.mfma else native.flow_run
        kw = dict(D=chain.D) if (narrow_in and i == 0) else {}
        if context is not None:
            kw["context"] = context
        if sum_out is not None:
            kw["sum_out"] = sum_out
        if last and need_rows and chain.reversed_out():
            kw["reverse_out"] = True              # (the reversal behind the program, folded into its store)
        run(cur, out, None if (last and base is not None and n_seg == 1) else logdet,
            loc_p if last else None, ls_p if last else None,
            logprob if last else None, seg.packed_ops(), seg.params, accumulate=(i > 0), **kw)
        if need_rows:
            cur = out
    out_rows = None
    if want_rows and padded:
        out_rows = cur.index_select(1, chain.pos)            # logical order, padding dropped
    elif want_rows:
        if chain.identity_out or chain.reversed_out():
            out_rows = cur
        else:                                     # logical l <- physical pos[l]
            out_rows = torch.empty_like(cur)
            native.permute(cur, chain.pos.to(torch.int32), out_rows)
    return out_rows, logdet, logprob
