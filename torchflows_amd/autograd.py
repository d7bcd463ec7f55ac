"""Training on the HIP path: one autograd node per composition.

The reference trains through ``torch.autograd`` over its per-layer ATen graphs
(``Flow.fit`` flows.py:226-455 -> ``log_prob`` :628-658 -> ``BijectiveComposition.forward``
bijections/base.py:203-224).  Here a whole composition is ONE ``torch.autograd.Function``:

* forward: the same libtfk layer kernels as inference, out of place, keeping only the
  (N, D) rows that entered each coupling / trainable elementwise layer.  The conditioner
  output ``h`` (2.9 KB per row per RQ-spline layer) is NOT kept.
* backward: walk the layers in reverse over one gradient row buffer ``g`` (N, D) and the
  per-row log-det gradient; per layer one reverse-mode kernel of csrc/tfk_bwd.hip, which
  recomputes alpha / knots / bins from the saved input rows and a re-evaluated ``h``
  ("recompute, not store").  The conditioner MLP's own backward (two skinny GEMMs) is
  ``torch.autograd.grad`` on PyTorch-ROCm, fed with the kernel's ``dL/dh``.

Affine / shift couplings with the plain Linear-Tanh-Linear conditioner skip even that: at 64 / 128 / 256 columns the whole
layer backward is one launch (``_TrainPack``), above 256 columns (D % 8 == 0 up to 1024) one launch plus three
``tfk_rows_outer`` products (``_WideTrainPack``, csrc/tfk_wide_bwd.h) -- no GEMM-library call, so ``Flow.fit`` can capture
the step.  The pack classes live in train_packs.py.  ``_PlanPacks`` resolves every step of a plan to a route once;
``ChainFunction`` is set-up, one loop over the steps' ``_STEPS[route]`` functions, and the epilogue.

Only what the kernels cover takes this route (affine / inverse-affine / shift / RQ-spline
couplings with 4, 8 or 16 bins, ElementwiseAffine / ActNorm, permutations, no context);
anything else keeps the ATen composite graph.  ``TORCHFLOWS_AMD_TRAIN=0`` forces the latter.
"""
from __future__ import annotations

import contextlib
import copy
import math
import os
import threading
from typing import List, NamedTuple, Optional, Tuple

import torch

from torchflows_amd.utils import debug_switch

from torchflows_amd import native
from torchflows_amd.flow_compile import _flatten
from torchflows_amd.train_packs import (_LAYOUTS, _RqsTrainPack, _TrainPack, _WideTrainPack,  # noqa: F401
                                        reversal_index, training_layout)

FORWARD, INVERSE = 0, 1


def enabled() -> bool:
    return os.environ.get("TORCHFLOWS_AMD_TRAIN", "1") != "0"


_live = threading.local()


@contextlib.contextmanager
def live_route():
    """Inside: an evaluation WITHOUT gradients takes the training route too (the chain's per-layer launches, operands
    gathered from the live parameter tensors) instead of the packed flow programs.  A packed program is a copy of the
    weights, refreshed when a parameter's version counter moves -- which a replayed hipGraph never does; the launches of
    this route read the parameters themselves, so they can sit in a captured validation pass (Flow.fit)."""
    prev = getattr(_live, "on", False)
    _live.on = True
    try:
        yield
    finally:
        _live.on = prev


def live_forced() -> bool:
    return getattr(_live, "on", False)


def _step_kind(layer) -> Optional[str]:
    from torchflows_amd.bijections.finite.autoregressive.layers_base import (
        CouplingBijection, ElementwiseBijection, MaskedAutoregressiveBijection)
    from torchflows_amd.bijections.finite.matrix.permutation import PermutationMatrix
    if isinstance(layer, PermutationMatrix):
        return "perm"
    if isinstance(layer, MaskedAutoregressiveBijection):
        # the parallel pass (MAF density / IAF sampling): MADE on PyTorch-ROCm, the transformer's
        # forward and reverse-mode kernels with every position a target
        tr = layer.transformer
        ok = layer.context_shape is None and native.made_kernel(tr) and native.reverse_kernel(tr)
        return "made" if ok else None
    if isinstance(layer, ElementwiseBijection):
        if layer.transformer.native_kind not in ("affine", "inverse_affine"):
            return None
        # with a context the parameters come from a conditioner on it (layers_base.py:300-318): the affine coupling
        # kernels with every position a target, the conditioner (default: Linear) on PyTorch-ROCm
        return "elementwise" if layer.use_global_parameters else "elementwise_ctx"
    if isinstance(layer, CouplingBijection):
        # (a context only enters the conditioner, by concatenation: conditioning/context.py:38-64)
        if native.reverse_kernel(layer.transformer):
            return "coupling"
    return None


def training_plan(composition, direction: int):
    """[(layer, direction, kind)] if every layer has forward and reverse-mode kernels, else None."""
    # the steps depend on the layer objects and their configuration only: kept on the composition per direction, keyed
    # by the identity of its layers (dropped with every other ``_tfk_`` cache on train() / eval() / load_state_dict /
    # a move); 27 layers x isinstance chains cost 60 us of a 1.5 ms step
    from torchflows_amd import fused
    key = (fused._EPOCH[0], tuple(map(id, composition.layers)))
    cache = composition.__dict__.setdefault("_tfk_train_plan", {})
    hit = cache.get(direction)
    if hit is not None and hit[0] == key:
        return None if hit[1] is None else Plan(hit[1])
    order = composition.layers if direction == FORWARD else list(composition.layers)[::-1]
    flat = _flatten(order, "forward" if direction == FORWARD else "inverse")
    steps = None
    if flat is not None:
        steps = []
        for layer, d in flat:
            kind = _step_kind(layer)
            if kind is None or (kind == "made" and d == layer._sequential_when):
                steps = None    # (the element-by-element map is not differentiated on the HIP path)
                break
            if kind == "coupling" and d == INVERSE and layer.transformer.native_kind == "dsf":
                steps = None    # (a bisection without gradient: the ATen graph, as the reference differentiates it)
                break
            steps.append((layer, d, kind))
    cache[direction] = (key, steps)
    return None if steps is None else Plan(steps)


class Plan(list):
    """[(layer, direction, kind)] + the context rows (N, *context_shape) of this call, or None; ``l2``: the
    {coefficient: [parameters]} of the L2 penalty the caller wants evaluated in the same autograd node
    (``Flow._base_batch_loss``), or None."""
    context = None
    l2 = None


def applicable(composition, x: torch.Tensor, context) -> bool:
    """Autograd is on, something needs a gradient, and everything is fp32 on one HIP device."""
    if not enabled() or not (torch.is_grad_enabled() or live_forced()):
        return False
    if x.device.type != "cuda" or x.dtype != torch.float32:
        return False
    if context is not None and (context.device != x.device or context.dtype != torch.float32 or context.requires_grad):
        return False            # (a gradient with respect to the context: the ATen graph)
    from torchflows_amd import fused
    if not fused.static_ok(composition):
        return False
    first = next(composition.parameters(), None)
    if first is not None and first.device != x.device:
        return False
    return x.requires_grad or fused.any_requires_grad(composition)


def _module_params(module) -> List[torch.Tensor]:
    """``list(module.parameters())`` without the module walk on every call (27 layers x forward + backward = 0.3 ms of a
    3 ms training step): the (submodule, name) slots are walked once and looked up by name afterwards, so a replaced
    Parameter is seen; dropped by fused.invalidate (train() / eval() / load_state_dict / invalidate_native_caches)."""
    slots = module.__dict__.get("_tfk_param_slots")
    if slots is None:
        seen, slots = set(), []
        for m in module.modules():
            for n, p in m._parameters.items():
                if p is not None and id(p) not in seen:
                    seen.add(id(p))
                    slots.append((m, n))
        module.__dict__["_tfk_param_slots"] = slots
    return [m._parameters[n] for m, n in slots]


def _layer_params(layer, kind: str) -> List[torch.Tensor]:
    if kind == "elementwise":
        return [layer.value]
    if kind in ("coupling", "made", "elementwise_ctx"):
        return _module_params(layer.conditioner_transform)
    return []


def _source_rows(layer, rows: torch.Tensor) -> torch.Tensor:
    S = layer.coupling.source_event_size
    return rows[:, :S] if layer._source_is_head else rows.index_select(1, layer._source_index)


def _conditioner(layer, x_a: torch.Tensor, context) -> torch.Tensor:
    """h (N, T*P) from the source columns of the rows that enter the coupling (layers_base.py:117-143)."""
    return layer.conditioner_transform(x_a.reshape(x_a.shape[0], *layer.coupling.constant_shape),
                                       context=_layer_context(layer, context)).reshape(x_a.shape[0], -1)


def _layer_context(layer, context):
    """The call's context rows for a layer that takes one, else None."""
    return context if (context is not None and layer.context_shape is not None) else None


def _keeps_graph(layer) -> bool:
    """Couplings whose conditioner is evaluated once per step with its autograd graph kept for the backward pass,
    instead of being re-evaluated there: the convolutional conditioners of the image flows."""
    from torchflows_amd.bijections.finite.multiscale.conditioning.classic import ConvNetConditioner
    return isinstance(layer.conditioner_transform, ConvNetConditioner)


def _plain_mlp(layer):
    """(Linear, Linear) when the conditioner is the default FeedForward: Linear, Tanh, Linear on
    x_A alone (transforms.py:274-307), no global parameters, unbounded output -- the case whose
    backward is written out below instead of being left to torch.autograd."""
    import torch.nn as nn
    from torchflows_amd.bijections.finite.autoregressive.conditioning.transforms import FeedForward
    ct = layer.conditioner_transform
    if type(ct) is not FeedForward or ct.n_global_parameters != 0 or ct.context_shape is not None:
        return None
    if ct.output_lower_bound != -math.inf or ct.output_upper_bound != math.inf:
        return None
    mods = list(ct.sequential)
    if (len(mods) == 4 and isinstance(mods[0], nn.Linear) and isinstance(mods[1], nn.Tanh)
            and isinstance(mods[2], nn.Linear) and isinstance(mods[3], nn.Unflatten)):
        return mods[0], mods[2]
    return None


_AFFINE_KINDS = ("affine", "inverse_affine", "shift")      # (shift: the affine launches with a scale logit of zero, _TrainPack)


def _half_split_mlp(layer, D: int, kinds, fp32: bool):
    """(lin1, lin2) for the geometry every fused training launch is written for: a transformer of ``kinds``, the first D // 2
    columns the sources, the others the targets at the tail, the plain Linear-Tanh-Linear conditioner (``fp32``: in float32
    throughout).  The ``_fused_*_layer`` predicates add their own conditions."""
    c = layer.coupling
    if layer.transformer.native_kind not in kinds or not (layer._source_is_head and layer._target_is_tail
                                                          and c.source_event_size == D // 2 and c.target_event_size == D - D // 2):
        return None
    mlp = _plain_mlp(layer)
    if mlp is not None and fp32 and any(p.dtype != torch.float32 for lin in mlp for p in (lin.weight, lin.bias)):
        return None
    return mlp


def wide_train_enabled() -> bool:
    """Couplings on event sizes above 256 (D % 8 == 0, D <= 1024, hidden width <= 15) train on the wide launches: one
    tfk_flow_run_wide forward, one tfk_wide_coupling_train_bwd + three tfk_rows_outer backward
    (TORCHFLOWS_AMD_DEBUG=wide_train=0: the layer-by-layer route; independent of ``wide``, the inference switch)."""
    return debug_switch("wide_train", "1") != "0"


def _fused_wide_layer(layer, D: int):
    """(lin1, lin2) when the layer trains on the wide launches: ``_fused_bwd_layer``'s conditions above 256 columns."""
    if not (fused_train_enabled() and wide_train_enabled()) or D <= 256:
        return None
    mlp = _half_split_mlp(layer, D, _AFFINE_KINDS, fp32=True)
    return mlp if (mlp is not None and native.lib().tfk_wide_coupling_train_bwd_supported(D, mlp[0].out_features)) else None


def _ew_fma_block(layer, d: int, D: int, hp: int):
    """(closing TFK_OP_EW_FMA block, gscale) of a fixed ElementwiseAffine / ActNorm that rides along with a wide coupling:
    s[2 hp] | t[2 hp] | constant log-det | pad[3] in the wide kernels' column order (each half at the head of its plane;
    pad columns s = 1, t = 0), z = s x + t -- s = alpha, t = beta, or 1 / alpha, -beta / alpha for the dividing form,
    evaluated in float64 as fused_wide.compile_wide does -- and the D logical column factors of its reverse mode.  Cached on
    the layer until its value changes (ActNorm: once, at its data-dependent initialisation); the log-det constant is summed
    on the device."""
    key = (layer.value._version, layer.value.data_ptr(), d, hp)
    hit = layer.__dict__.get("_tfk_ew_fma_block")
    if hit is not None and hit[0] == key:
        return hit[1], hit[2]
    v = layer.value.detach().reshape(D, 2)
    alpha = layer.transformer.constrain_scale(v[:, 0]).double()            # affine.py:33-34, the fp32 scale
    beta = v[:, 1].double()
    ldc = torch.log(alpha).sum().reshape(1)
    if _affine_form_is_inverse(layer, d):
        s, t, ldc = 1.0 / alpha, (0.0 - beta) / alpha, -ldc
    else:
        s, t = alpha, beta
    half = D // 2
    one, zero = s.new_ones(hp - half), s.new_zeros(hp - half)
    block = torch.cat([s[:half], one, s[half:], one, t[:half], zero, t[half:], zero, ldc, s.new_zeros(3)]).float().contiguous()
    gscale = s.float().contiguous()
    layer.__dict__["_tfk_ew_fma_block"] = (key, block, gscale)
    return block, gscale


def _fused_rqs_layer(layer, D: int):
    """(lin1, lin2) when the layer can use tfk_rqs_coupling_train_bwd (and the _RQS flow-program op)."""
    if not fused_train_enabled() or layer.transformer.native_kind != "rqs":
        return None
    lib, K = native.lib(), int(layer.transformer.n_bins)
    if not (lib.tfk_rqs_coupling_train_bwd_supported(D, K)
            or (padded_train_enabled() and 3 <= D < 64 and lib.tfk_rqs_coupling_train_bwd_supported(64, K))):
        return None                           # (D < 64: on rows padded to 64 -- whether the plan may be is plan_width's call)
    mlp = _half_split_mlp(layer, D, ("rqs",), fp32=False)
    return mlp if (mlp is not None and mlp[0].out_features <= 16) else None


def flat_enabled() -> bool:
    """Operands gathered from / gradients returned as slices of ONE buffer when the parameters live in one
    (torchflows_amd/flat_optim.py; TORCHFLOWS_AMD_DEBUG=flat=0: always the per-tensor route)."""
    return debug_switch("flat", "1") != "0"


def rows_outer_enabled() -> bool:
    """The weight-gradient products of the fused spline training step on tfk_rows_outer (TORCHFLOWS_AMD_DEBUG=rows_outer=0:
    split-K batched GEMMs on the GEMM library, as before round 3)."""
    return debug_switch("rows_outer", "1") != "0"


def fused_train_enabled() -> bool:
    return debug_switch("train_fused", "1") != "0"


def padded_train_enabled() -> bool:
    """Fused training launches for even event sizes below 128 that are not 64 / 128, on rows padded to the next of the
    two (TORCHFLOWS_AMD_DEBUG=train_pad=0: the layer-by-layer reverse mode, as before round 3)."""
    return debug_switch("train_pad", "1") != "0"


def train_width(D: int) -> Optional[int]:
    """Row width the fused training launches run an event size of ``D`` at, or None."""
    if native.lib().tfk_coupling_train_bwd_supported(D):
        return D
    if padded_train_enabled() and 3 <= D < 128:          # (odd sizes: D - D // 2 targets fit a plane of W / 2 as well)
        return 64 if D < 64 else 128
    return None


def _padding_capable(plan) -> bool:
    """Every step keeps the padded training layout (source half at the head of plane A, target half at the tail of
    plane B): reversals -- a logical reversal IS the physical one there --, global elementwise layers, and couplings
    with the fused launches."""
    D = plan[0][0].n_dim if len(plan) else 0
    def fused(layer) -> bool:                 # (the fused spline launches exist at 64 columns only)
        return _fused_bwd_layer(layer, D) is not None or (D < 64 and _fused_rqs_layer(layer, D) is not None)
    return all(kind == "elementwise" or (kind == "perm" and layer._is_reversal) or (kind == "coupling" and fused(layer))
               for layer, _, kind in plan)


def plan_width(plan, D: int) -> int:
    """The width of the rows ChainFunction runs this plan on: ``D``, or the padded width when D itself has no fused
    training launches and every step keeps the padded layout."""
    W = train_width(D)
    if W is None or W == D or not _padding_capable(plan):
        return D
    return W


def _fused_bwd_layer(layer, D: int):
    """(lin1, lin2) when the layer's whole backward can run as tfk_affine_coupling_train_bwd (at the width
    ``train_width(D)``: whether a plan may be padded is ``plan_width``'s call)."""
    if not fused_train_enabled() or train_width(D) is None:
        return None
    mlp = _half_split_mlp(layer, D, _AFFINE_KINDS, fp32=True)
    return mlp if (mlp is not None and mlp[0].out_features <= 15) else None


def _ew_block(layer, d: int, D: int, W: Optional[int] = None) -> torch.Tensor:
    """Parameter block of a fixed ElementwiseAffine / ActNorm op as tfk_flow_run reads it
    (alpha[W] | beta[W] | sum log alpha, pad[3] | 1/alpha[W] for the dividing form), cached on the
    layer until its value changes (ActNorm: once, at its data-dependent initialisation).  ``W`` > D: rows in the padded
    training layout -- the padding columns get alpha = 1, beta = 0."""
    W = W or D
    key = (layer.value._version, layer.value.data_ptr(), d, W)
    hit = layer.__dict__.get("_tfk_ew_block")
    if hit is not None and hit[0] == key:
        return hit[1]
    v = layer.value.detach().reshape(D, 2)
    alpha = layer.transformer.constrain_scale(v[:, 0])                     # affine.py:33-34
    beta = v[:, 1].contiguous()
    ldc = torch.log(alpha).sum().reshape(1)
    if W != D:
        phys = training_layout(D, W, v.device)
        alpha = torch.ones(W, dtype=alpha.dtype, device=v.device).index_copy_(0, phys, alpha)
        beta = torch.zeros(W, dtype=beta.dtype, device=v.device).index_copy_(0, phys, beta)
    inverse_form = _affine_form_is_inverse(layer, d)
    pad = torch.zeros(3, dtype=torch.float32, device=v.device)
    parts = [alpha, beta, -ldc if inverse_form else ldc, pad]
    if inverse_form:
        parts.append(1.0 / alpha)
    block = torch.cat(parts).float().contiguous()
    layer.__dict__["_tfk_ew_block"] = (key, block)
    return block


def _ew_block_floats(layer, d: int, W: int) -> int:
    """Floats of ``_ew_block``: alpha | beta | log-det, pad[3] (| 1 / alpha for the dividing form)."""
    return (3 * W + 4) if _affine_form_is_inverse(layer, d) else (2 * W + 4)


def _ew_ops(plan, rec, offset: int) -> list:
    """[the TFK_OP_EW_* op of the fixed elementwise layer that rides along with ``rec``, its block ``offset`` floats into the
    program's], [] when none does."""
    if rec.ew_step is None:
        return []
    return [(1 if _affine_form_is_inverse(plan[rec.ew_step][0], plan[rec.ew_step][1]) else 0, 0, 0, offset)]


def _fold_after(plan, i: int, fold: bool, fold_rev: bool):
    """(step of the fixed elementwise layer, step of the reversal) that follow coupling ``i`` and ride along with its fused
    launches, None where nothing does.  ``fold_rev`` False: reversals stay steps of their own (padded rows of an odd size)."""
    ew_step = rev_step = None
    j = i + 1
    if fold and j < len(plan) and plan[j][2] == "elementwise" and not plan[j][0].value.requires_grad:
        ew_step = j
        j += 1
    if fold and fold_rev and j < len(plan) and plan[j][2] == "perm" and plan[j][0]._is_reversal:
        rev_step = j
    return ew_step, rev_step


# The route of a step, resolved once per plan (_PlanPacks.routes): its kind in the plan unless it is a coupling (on fused
# launches or layer by layer) or rides along with one; its forward and backward functions: _STEPS[route].
_FOLDED, _PERM, _ELEMENTWISE, _ELEMENTWISE_CTX, _MADE = "folded", "perm", "elementwise", "elementwise_ctx", "made"
_AFFINE, _RQS, _WIDE, _LAYERWISE = "affine", "rqs", "wide", "layerwise"


class _FusedCoupling(NamedTuple):
    """One coupling on fused training launches."""
    step: int                       # index in the plan
    route: str                      # _AFFINE (_TrainPack), _RQS (_RqsTrainPack) or _WIDE (_WideTrainPack)
    k: int                          # index among the plan's couplings of the same route: its packed block
    lin1: torch.nn.Module
    lin2: torch.nn.Module
    pack: object
    ew_step: Optional[int]          # the fixed elementwise layer / the reversal behind it that ride along (_fold_after)
    rev_step: Optional[int]
    lean: Optional[int] = None      # _WIDE: 0 affine, 1 dividing affine, 2 shift forward, 3 shift inverse

    def mlp_params(self):
        return self.lin1.weight, self.lin1.bias, self.lin2.weight, self.lin2.bias


class _PlanPacks:
    """The fused couplings of one plan and the route of every step.

    ``records``: one ``_FusedCoupling`` per coupling on fused launches, in plan order (``fused[route]``: those of one route,
    ``record_at[step]``: the step's, or None); ``routes[step]``: the step's route.  ONE concatenation + ONE gather packs every
    _AFFINE (or _WIDE) layer's weights into MFMA-operand order per step, and ONE gather maps all accumulator-layout
    gradient blocks back -- instead of three small launches per layer.

    With ``fold`` the fixed elementwise layer (ActNorm) and the reversal that FOLLOW a fused coupling ride along: forward =
    one flow program [coupling, elementwise] with a reversed store, backward = the reversed / scaled load of the reverse-mode
    launch; their own steps are _FOLDED."""

    def __init__(self, plan, D: int, device, fold: bool):
        self.D = D
        # the rows' width: D, or -- event sizes without fused launches of their own, every step padding-capable -- the
        # next width that has them, the rows in the padded training layout (training_layout)
        self.W = W = plan_width(plan, D)
        self.phys = training_layout(D, W, device) if W != D else None
        # odd event sizes: a logical reversal is not the physical one -- no folding of reversals into the coupling
        # launches, the permutation steps gather with reversal_index
        self.rev_index = reversal_index(D, W, device) if (W != D and D % 2) else None
        fusable = bool(native.lib().tfk_coupling_train_bwd_supported(W))
        self.plan = list(plan)        # (a plain copy: the call's context must not be kept alive by the cache)
        self.records: List[_FusedCoupling] = []
        self.record_at: List[Optional[_FusedCoupling]] = [None] * len(plan)
        self.routes = [_LAYERWISE if kind == "coupling" else kind for _, _, kind in plan]
        self.fused = by_route = {_AFFINE: [], _RQS: [], _WIDE: []}
        pidx, gidx, off_flat, off_out = [], [], 0, 0                  # AFFINE: operand gather, accumulator gather
        widx, wmul, wadd, off_wide = [], [], [], 0                    # WIDE: operand gather and its float64 pre-scaling
        for i, (layer, d, kind) in enumerate(plan):
            if kind != "coupling":
                continue
            route, mlp = self._fused_route(layer, fusable)
            if route is None:
                continue
            shift, lean = layer.transformer.native_kind == "shift", None
            if route == _AFFINE:
                pack = _TrainPack.get(W, mlp[0].out_features, device, D, shift=shift)
            elif route == _RQS:
                pack = _RqsTrainPack.get(mlp[0].out_features, device, D)
            else:
                pack = _WideTrainPack.get(D, mlp[0].out_features, device, shift)
                lean = (2 + (d == INVERSE)) if shift else int(_affine_form_is_inverse(layer, d))
            # (wide rows are never padded: their reversals always fold)
            ew_step, rev_step = _fold_after(plan, i, fold, route == _WIDE or self.rev_index is None)
            rec = _FusedCoupling(i, route, len(by_route[route]), mlp[0], mlp[1], pack, ew_step, rev_step, lean)
            by_route[route].append(rec)
            self.records.append(rec)
            self.record_at[i], self.routes[i] = rec, route
            for t in (ew_step, rev_step):
                if t is not None:
                    self.routes[t] = _FOLDED
            if route == _AFFINE:              # the elementwise block follows the operand block
                n_ew = 0 if ew_step is None else _ew_block_floats(plan[ew_step][0], plan[ew_step][1], W)
                pidx.append(torch.cat([pack.param_index + off_flat]
                                      + ([torch.arange(n_ew, device=device) + (off_flat + pack.n_flat)] if n_ew else [])))
                gidx.append(pack.grad_index + off_out)
                off_flat += pack.n_flat + n_ew
                off_out += pack.n_out
            elif route == _WIDE:              # the closing TFK_OP_EW_FMA block follows, the identity when nothing rides along
                widx += [pack.param_index + off_wide, torch.arange(pack.n_ew, device=device) + (off_wide + pack.n_flat)]
                wmul += [pack.param_mul, torch.ones(pack.n_ew, dtype=torch.float64, device=device)]
                wadd += [pack.param_add, torch.zeros(pack.n_ew, dtype=torch.float64, device=device)]
                off_wide += pack.n_flat + pack.n_ew
        self.n_out_total = off_out
        if pidx:
            self.block_sizes = [int(t.numel()) for t in pidx]
            self.param_index = torch.cat(pidx)
            self.grad_index = torch.cat(gidx)
            self.zero = by_route[_AFFINE][0].pack.zero
        if widx:
            self.wide_index, self.wide_mul, self.wide_add = torch.cat(widx), torch.cat(wmul), torch.cat(wadd)
            self.wide_sizes = [r.pack.n_bwd + r.pack.n_ew for r in by_route[_WIDE]]

    def _fused_route(self, layer, fusable: bool):
        """(route, (lin1, lin2)) of a coupling that runs on fused launches at this plan's row width, else (None, None): the
        affine launches first, then the wide ones, then the spline's."""
        mlp = _fused_bwd_layer(layer, self.D) if fusable else None
        if mlp is not None:
            return _AFFINE, mlp
        mlp = _fused_wide_layer(layer, self.D) if self.W == self.D else None
        if mlp is not None:
            return _WIDE, mlp
        K = int(getattr(layer.transformer, "n_bins", 0) or 0)
        mlp = _fused_rqs_layer(layer, self.D) if native.lib().tfk_rqs_coupling_train_bwd_supported(self.W, K) else None
        return (_RQS, mlp) if mlp is not None else (None, None)

    # ---- parameters that live in ONE buffer (torchflows_amd/flat_optim.py) --------------------------------------
    def flat_capable(self) -> bool:
        """Every step is a permutation, a global elementwise layer or a coupling with the fused training launches:
        all gradients of the plan then come out of libtfk accumulators and can leave as slices of one buffer."""
        if not self.fused[_AFFINE] and not self.fused[_RQS]:
            return False
        if self.fused[_WIDE]:                 # (wide couplings return their gradients per tensor: no one-buffer maps yet)
            return False
        # ONE layer object (or one parameter tensor) twice in the chain (shared weights): grad_src maps a slot of the parameter buffer to exactly
        # one accumulator position, so the second use would overwrite the first instead of adding to it -- such a plan
        # keeps the per-tensor route, where autograd sums the per-step gradients
        ids = [id(p) for layer, _, kind in self.plan for p in _layer_params(layer, kind)]
        if len(ids) != len(set(ids)):
            return False
        outer = rows_outer_enabled()
        for route, rec in zip(self.routes, self.record_at):
            if route in (_FOLDED, _PERM, _ELEMENTWISE, _AFFINE):
                continue
            if route == _RQS and outer and rec.lin1.out_features <= 15:
                continue                      # (spline couplings: their row-contracting products on tfk_rows_outer)
            return False
        return True

    def flat_maps(self, fb):
        """Index maps between a FlatParams buffer and this plan, built once per buffer:
        ``src_index``: position in torch.cat([fb.P, aux]) of every element of the packed operand blocks (aux = the blocks
        of the folded fixed elementwise layers); ``grad_src``: for every element of fb.P the position of its gradient in
        the backward pass's output buffer [coupling accumulators | trainable elementwise gradients | one zero];
        ``ret``: per plan parameter (in ChainFunction's argument order) the piece of fb.split_sizes and its shape."""
        hit = self.__dict__.get("_flat_maps")
        if hit is not None and hit[0]() is fb:
            return hit[1]
        import weakref
        dev = fb.P.device
        D, W = self.D, self.W
        phys = (self.phys if self.phys is not None else torch.arange(D)).cpu()
        slot_of = fb.slot_of
        aux_layers, aux_off = [], fb.n

        def positions(rec):       # of the coupling's [W1 | b1 | W2 | b2 | 0] in fb.P; None: a frozen weight (the general route)
            slots = [slot_of.get(id(t)) for t in rec.mlp_params()]
            if None in slots:
                return None
            return [torch.arange(fb.numel[k]) + fb.offset[k] for k in slots] + [torch.tensor([fb.zero_slot])]

        def aux_block(rec):       # positions, behind fb.P, of the block of the fixed elementwise layer that rides along
            nonlocal aux_off
            ew_layer, ew_d, _ = self.plan[rec.ew_step]
            pos = torch.arange(_ew_block_floats(ew_layer, ew_d, W)) + aux_off
            aux_layers.append((ew_layer, ew_d))
            aux_off += pos.numel()
            return pos

        def map_grads(rec, sizes, index):     # index: where the gradients of (W1, b1, W2, b2) lie in the backward's buffer
            lo = 0
            for t, n in zip(rec.mlp_params(), sizes):
                k = slot_of[id(t)]
                grad_src[fb.offset[k]:fb.offset[k] + n] = index[lo:lo + n]
                lo += n
        cat_to_src = []
        for rec in self.fused[_AFFINE]:
            pos = positions(rec)
            if pos is None:
                return None
            cat_to_src += pos
            if rec.ew_step is not None:
                cat_to_src.append(aux_block(rec))
        src_index = None
        if cat_to_src:
            cat_to_src = torch.cat(cat_to_src).to(dev)
            src_index = cat_to_src[self.param_index]
        # spline couplings: per layer the full operand block (what the backward kernel takes) and, when a fixed
        # elementwise layer rides along, a second segment [forward operands | that layer's block] for the forward program
        rqs_index, rqs_sizes, rqs_seg = [], [], []
        for rec in self.fused[_RQS]:
            pos = positions(rec)
            if pos is None:
                return None
            full = torch.cat(pos)[rec.pack.param_index.cpu()]
            bwd_seg = len(rqs_sizes)
            rqs_index.append(full)
            rqs_sizes.append(int(full.numel()))
            fwd_seg = None
            if rec.ew_step is not None:
                fwd_seg = len(rqs_sizes)
                rqs_index.append(torch.cat([full[:rec.pack.n_fwd], aux_block(rec)]))
                rqs_sizes.append(int(rqs_index[-1].numel()))
            rqs_seg.append((bwd_seg, fwd_seg))
        # gradients: accumulator layout of all layers | trainable elementwise (D, 2) blocks | zero
        grad_src = torch.full((fb.n,), -1, dtype=torch.long)
        lo = 0
        gi = self.grad_index.cpu() if self.fused[_AFFINE] else None
        for rec in self.fused[_AFFINE]:
            n = sum(rec.pack.sizes)
            map_grads(rec, rec.pack.sizes, gi[lo:lo + n])
            lo += n
        ext = self.n_out_total
        rqs_out = {}
        for rec in self.fused[_RQS]:              # the three tfk_rows_outer products of the layer, accumulator order
            rqs_out[rec.step] = ext
            map_grads(rec, rec.pack.acc_sizes, ext + rec.pack.acc_index.cpu())
            ext += rec.pack.n_acc
        ew_out = {}
        for i, (layer, d, kind) in enumerate(self.plan):
            if self.routes[i] == _ELEMENTWISE and layer.value.requires_grad:
                k = slot_of.get(id(layer.value))
                if k is None:
                    return None
                ew_out[i] = ext              # the kernel writes dL/dvalue as (W, 2): logical row l is physical row phys[l]
                grad_src[fb.offset[k]:fb.offset[k] + 2 * D] = (ext + 2 * phys[:, None] + torch.arange(2)[None, :]).reshape(-1)
                ext += 2 * W
        grad_src[grad_src < 0] = ext                 # padding, parameters outside the plan: the zero
        ret = []
        for layer, _, kind in self.plan:
            for t in _layer_params(layer, kind):
                k = slot_of.get(id(t)) if t.requires_grad else None
                ret.append(None if k is None else (fb.piece_of_slot[k], tuple(t.shape)))
        maps = dict(src_index=src_index, aux_layers=aux_layers, grad_src=grad_src.to(dev), ew_out=ew_out,
                    n_ext=ext + 1, ret=ret, l2={}, rqs_out=rqs_out, rqs_seg=rqs_seg, rqs_sizes=rqs_sizes,
                    rqs_index=torch.cat(rqs_index).to(dev) if rqs_index else None)
        self.__dict__["_flat_maps"] = (weakref.ref(fb), maps)
        return maps

    def pack_flat(self, fb, maps):
        """``pack()`` as ONE gather out of the parameter buffer (+ the cached blocks of the folded fixed layers)."""
        src = fb.P
        if maps["aux_layers"]:
            src = torch.cat([fb.P] + [_ew_block(l, d, self.D, self.W) for l, d in maps["aux_layers"]])
        affine = list(src.index_select(0, maps["src_index"]).split(self.block_sizes)) if self.fused[_AFFINE] else []
        rqs = (list(src.index_select(0, maps["rqs_index"]).split(maps["rqs_sizes"]))
               if maps["rqs_index"] is not None else [])
        return affine, rqs

    @staticmethod
    def l2_vector(fb, maps, l2):
        """coef at the positions of the L2-regularised parameters of ``l2`` = {coef: [parameters]}, 0 elsewhere
        (cached per parameter set); None when one of them is not in the buffer."""
        key = tuple((c, tuple(id(t) for t in ps)) for c, ps in sorted(l2.items()))
        vec = maps["l2"].get(key)
        if vec is None:
            v = torch.zeros(fb.n, dtype=torch.float32)
            for c, ps in l2.items():
                for t in ps:
                    k = fb.slot_of.get(id(t))
                    if k is None or fb.params[k] is not t:
                        return None
                    v[fb.offset[k]:fb.offset[k] + fb.numel[k]] = c
            if len(maps["l2"]) > 4:
                maps["l2"].clear()
            vec = maps["l2"][key] = v.to(fb.P.device)
        return vec

    # ---- rows in the padded training layout (self.W > self.D) -----------------------------------------------------
    def pad_rows(self, rows: torch.Tensor) -> torch.Tensor:
        """(N, D) -> (N, W): first half at the head of plane A, second half at the tail of plane B, zeros between."""
        h = self.D // 2                               # (odd sizes: h sources at the head, D - h targets at the tail)
        wide = rows.new_zeros(rows.shape[0], self.W)
        wide[:, :h] = rows[:, :h]
        wide[:, self.W - (self.D - h):] = rows[:, h:]
        return wide

    def unpad_rows(self, wide: torch.Tensor) -> torch.Tensor:
        h = self.D // 2
        return torch.cat([wide[:, :h], wide[:, self.W - (self.D - h):]], dim=1)

    def ew_value(self, layer) -> torch.Tensor:
        """``layer.value`` as the (W, 2) block the elementwise kernels read (padding rows: zeros = the identity)."""
        v = layer.value.detach().reshape(self.D, 2)
        if self.phys is None:
            return v.contiguous()
        return v.new_zeros(self.W, 2).index_copy_(0, self.phys, v)

    def pack(self):
        """[packed block of layer k: operands (+ the folded elementwise parameters)] for the current weights."""
        pieces = []
        for rec in self.fused[_AFFINE]:
            pieces += [rec.lin1.weight.detach().reshape(-1), rec.lin1.bias.detach(),
                       rec.lin2.weight.detach().reshape(-1), rec.lin2.bias.detach(), self.zero]
            if rec.ew_step is not None:
                pieces.append(_ew_block(self.plan[rec.ew_step][0], self.plan[rec.ew_step][1], self.D, self.W))
        packed = torch.cat(pieces)[self.param_index]
        return list(packed.split(self.block_sizes))

    def pack_wide(self):
        """[block of wide layer k: forward operands | A2T | A1T | closing TFK_OP_EW_FMA block] for the current weights:
        one concatenation, one gather and one multiply-add (the lean pre-scaling, float64) for the whole plan."""
        pieces = []
        for rec in self.fused[_WIDE]:
            pieces += rec.pack.flat_of(rec.lin1, rec.lin2)
            pieces.append(rec.pack.ew_identity if rec.ew_step is None else
                          _ew_fma_block(self.plan[rec.ew_step][0], self.plan[rec.ew_step][1], self.D, rec.pack.hp)[0])
        src = torch.cat(pieces).double()
        packed = torch.addcmul(self.wide_add, src.index_select(0, self.wide_index), self.wide_mul).float()
        return list(packed.split(self.wide_sizes))


def _plan_packs(plan, D: int, device, fold: bool) -> _PlanPacks:
    owner = plan[0][0]
    key = (tuple(id(l) for l, _, _ in plan), tuple(d for _, d, _ in plan), str(device),
           fused_train_enabled(), fold, padded_train_enabled(), rows_outer_enabled(), wide_train_enabled())
    cache = owner.__dict__.setdefault("_tfk_plan_packs", {})
    if key not in cache:
        if len(cache) > 4:
            cache.clear()
        cache[key] = _PlanPacks(plan, D, device, fold)
    return cache[key]


def fully_fused(plan, D: int) -> bool:
    """Every coupling of the plan runs as the fused launches (flow program forward, fused training
    backward): the step then consists of libtfk kernels and elementwise ATen ops only -- no GEMM
    library calls -- which is the configuration verified to survive hipGraph capture."""
    couplings = [layer for layer, _, kind in plan if kind == "coupling"]
    if not couplings or any(kind not in ("coupling", "perm", "elementwise") for _, _, kind in plan):
        return False
    if all(_fused_bwd_layer(layer, D) is not None for layer in couplings):
        # (an event size that would need padding in a plan that cannot keep it has no fused launches after all)
        return bool(native.lib().tfk_coupling_train_bwd_supported(plan_width(plan, D)))
    # above 256 columns: the wide forward program, tfk_wide_coupling_train_bwd and the products on tfk_rows_outer
    if D > 256 and all(_fused_wide_layer(layer, D) is not None for layer in couplings):
        return True
    # RQ-spline couplings: the fused launch + the row-contracting products on tfk_rows_outer (hidden width <= 15)
    def spline_ok(layer):
        mlp = _fused_rqs_layer(layer, D)
        return mlp is not None and rows_outer_enabled() and mlp[0].out_features <= 15
    return plan_width(plan, D) == 64 and all(spline_ok(layer) for layer in couplings)


SPLIT_K_ROWS = 1024


def _outer_sum(a: torch.Tensor, b_aug: torch.Tensor) -> torch.Tensor:
    """``a^T @ b_aug`` for tall operands (N x m, N x k, N >> m, k): the contraction runs over the
    batch rows, so a plain GEMM has one tiny output tile and no parallelism (hipBLASLt: ~450 us at
    N = 2^18).  Split the rows into slabs of 1024, one batched GEMM over the slabs, then add the
    slab results (fixed order: deterministic)."""
    N, m = a.shape
    C = SPLIT_K_ROWS
    S = N // C
    if S >= 2:
        out = torch.bmm(a[:S * C].view(S, C, m).transpose(1, 2), b_aug[:S * C].view(S, C, -1)).sum(dim=0)
        if S * C < N:
            out = out + a[S * C:].t() @ b_aug[S * C:]
        return out
    return a.t() @ b_aug


def _mlp_backward(W1: torch.Tensor, W2: torch.Tensor, x_a: torch.Tensor, a1: torch.Tensor, gh: torch.Tensor):
    """Reverse mode of h = W2 tanh(W1 x_a + b1) + b2 given a1 = tanh(.) and gh = dL/dh.
    Returns (g_xa, dW1, db1, dW2, db2); the bias gradients ride along as a column of ones."""
    N = gh.shape[0]
    ones = torch.ones(N, 1, dtype=gh.dtype, device=gh.device)
    dW2b = _outer_sum(gh, torch.cat([a1, ones], dim=1))             # (TP, H + 1)
    g_pre = (gh @ W2) * (1.0 - a1 * a1)                              # tanh'
    dW1b = _outer_sum(g_pre, torch.cat([x_a, ones], dim=1))          # (H, S + 1)
    g_xa = g_pre @ W1
    return g_xa, dW1b[:, :-1], dW1b[:, -1], dW2b[:, :-1], dW2b[:, -1]


def _made_mlp(layer):
    """(MaskedLinear, MaskedLinear) when the conditioner is the default two-layer _MADE (masked Linear,
    Tanh, masked Linear; transforms.py:184-267) without global parameters or output bounds."""
    import torch.nn as nn
    from torchflows_amd.bijections.finite.autoregressive.conditioning.transforms import MADE
    ct = layer.conditioner_transform
    if not isinstance(ct, MADE) or ct.n_global_parameters != 0 or ct.context_shape is not None:
        return None
    if ct.output_lower_bound != -math.inf or ct.output_upper_bound != math.inf:
        return None
    mods = list(ct.sequential)
    if (len(mods) == 3 and isinstance(mods[0], MADE.MaskedLinear) and isinstance(mods[1], nn.Tanh)
            and isinstance(mods[2], MADE.MaskedLinear) and mods[0].in_features == layer.n_dim):
        return mods[0], mods[2]
    return None


def _affine_form_is_inverse(layer, d: int) -> bool:
    """Does this step evaluate (x - beta) / alpha (True) or alpha x + beta (False)?"""
    return (d == INVERSE) != (layer.transformer.native_kind == "inverse_affine")


def _awaits_statistics(layer, d: int) -> bool:
    """An ActNorm that still has to take its statistics from this batch (it cannot ride along with a coupling)."""
    if not (d == FORWARD and layer.training and getattr(layer, "first_training_batch_pass", False)):
        return False
    from torchflows_amd.bijections.finite.autoregressive.layers import ActNorm
    return isinstance(layer, ActNorm)


def _transform_forward(layer, d: int, x, h, out, logdet, tgt, T: int, accumulate: bool) -> None:
    """The transformer's forward kernel on the T target columns ``tgt`` (None: the tail) with the parameters ``h``.  ``d``: the
    step's direction -- FORWARD for a pass that always applies ``transformer.forward`` (MADE's: layers_base.py:196-199)."""
    native.transform(layer.transformer, d == INVERSE, x, h, out, logdet, tgt, T, accumulate)


def _transform_backward(layer, d: int, x_in, hc, g, gld, gh, tgt, T: int) -> None:
    """Reverse mode of ``_transform_forward``: in place on ``g`` at the target columns, dL/dh written to ``gh``."""
    native.transform_bwd(layer.transformer, d == INVERSE, x_in, hc, g, gld, gh, tgt, T)


def _mlp_param_grads(cparams, lin1, lin2, dW1, db1, dW2, db2) -> List[Optional[torch.Tensor]]:
    """Per conditioner parameter, in ``cparams`` order: its gradient, zeros for a trainable one the MLP does not use
    (global_theta_flat of a plain conditioner is empty: its gradient is an empty tensor), None for a frozen one."""
    by_param = {id(lin1.weight): dW1, id(lin1.bias): db1, id(lin2.weight): dW2, id(lin2.bias): db2}
    return [(by_param[id(p)] if id(p) in by_param else torch.zeros_like(p)) if p.requires_grad else None for p in cparams]


def _graph_grads(h2, inputs, gh, cparams):
    """``torch.autograd.grad`` of the conditioner output ``h2`` (evaluated with a graph) for dL/dh = ``gh``, with respect
    to ``inputs`` and the trainable ones of ``cparams``: (gradients of the inputs, gradients of the trainable parameters)."""
    wanted = [p for p in cparams if p.requires_grad]
    outs = torch.autograd.grad(h2, inputs + wanted, gh, allow_unused=True) if (inputs or wanted) else ()
    return outs[:len(inputs)], outs[len(inputs):]


def _graph_param_grads(outs, cparams, zeros: bool) -> List[Optional[torch.Tensor]]:
    """``_graph_grads``' parameter gradients per parameter of ``cparams``: None for a frozen one; for a trainable one the
    graph does not reach, zeros when ``zeros`` else None."""
    it = iter(outs)
    grads = [next(it) if p.requires_grad else None for p in cparams]
    if zeros:
        grads = [torch.zeros_like(p) if (gp is None and p.requires_grad) else gp for gp, p in zip(grads, cparams)]
    return grads


def _weight_products(x_in, S: int, gh, GH: int, gpre, hid, acc) -> None:
    """The three products of a fused coupling's backward that contract over the batch rows, on tfk_rows_outer (the matrix
    cores, no GEMM-library call: deterministic, capturable), into ``acc`` in accumulator order (include/tfk.h)."""
    lo2, lo3 = GH * 16, (GH + S) * 16
    native.rows_outer(gh, GH, hid, acc[:lo2])                # dW2 | db2 (column 15)
    native.rows_outer(x_in, S, gpre, acc[lo2:lo3])           # dW1 (source columns the layer does not have: not mapped)
    native.rows_outer(gpre, 16, hid, acc[lo3:])              # db1


def _folded_gscale(packs: _PlanPacks, rec: _FusedCoupling, packed: Optional[torch.Tensor] = None):
    """d out / d in per column of the fixed elementwise layer that rides along with a fused coupling (None: none does), read
    from ``packed``, the coupling's block with that layer's ``_ew_block`` behind the operands, else from the layer's own."""
    if rec.ew_step is None:
        return None
    ew_layer, ew_d, _ = packs.plan[rec.ew_step]
    if rec.route == _WIDE:
        return _ew_fma_block(ew_layer, ew_d, packs.D, rec.pack.hp)[1]           # d(s x + t)/dx = s
    W = packs.W
    block, lo = (_ew_block(ew_layer, ew_d, packs.D, W), 0) if packed is None else (packed, rec.pack.param_index.numel())
    if _affine_form_is_inverse(ew_layer, ew_d):      # d(alpha x + beta)/dx = alpha, d((x - beta)/alpha)/dx = 1/alpha
        lo += 2 * W + 4
    return block[lo:lo + W]


class _State:
    """What the step functions of one pass share.  Forward: ``cur`` the rows so far (``cur_is_saved``: somebody still needs
    them -- never write into them), ``started``: the log-det has been written, and per step ``saved`` (input rows), ``kept``
    (conditioner input, output WITH graph; used once), ``rqs_blocks`` (operand block), all for its backward.  That works on a
    copy and adds ``g`` / ``gld`` the gradient rows / log-det's, ``grads_per_step``, ``out_all`` the fused launches' accumulators."""

    def advance(self, out: torch.Tensor, keep: Optional[torch.Tensor], started: bool = True) -> None:
        """``out`` are the rows now; ``keep``: what the step's backward needs (its input rows, or None)."""
        self.saved.append(keep)
        self.cur, self.cur_is_saved = out, False
        self.started = self.started or started

    def transform(self, layer, d: int, h: torch.Tensor, tgt, T: int) -> None:
        """A step whose transformer reads its parameters ``h`` from memory: out of place, the input rows kept."""
        out = torch.empty_like(self.cur)
        _transform_forward(layer, d, self.cur, h, out, self.logdet, tgt, T, self.started)
        self.advance(out, self.cur)

    def program(self, run, rec: _FusedCoupling, ops, prm: torch.Tensor) -> None:
        """A fused coupling's flow program (``run``: native.flow_run_mfma / _wide), its reversal folded into the store."""
        out = torch.empty_like(self.cur)
        run(self.cur, out, self.logdet, None, None, None, ops, prm, accumulate=self.started, reverse_out=rec.rev_step is not None)
        self.advance(out, self.cur)


# ---- one forward and one backward function per route: f(state, step, layer, direction) -------------------------------
def _fwd_folded(st, step, layer, d):
    st.saved.append(None)                    # ran inside the preceding coupling's flow program


def _bwd_folded(st, i, layer, d):            # handled by the load of the coupling's backward kernel
    st.grads_per_step[i] = [None] * len(_layer_params(layer, st.plan[i][2]))


def _permute(packs, layer, rows, inverse: bool) -> torch.Tensor:
    out = torch.empty_like(rows)
    perm = packs.rev_index                   # (padded rows of an odd event size: reversals only, as a gather -- an involution)
    if perm is None and not layer._is_reversal:
        perm = layer._inv_index32 if inverse else layer._fwd_index32
    native.permute(rows, perm, out)
    return out


def _fwd_perm(st, step, layer, d):
    st.advance(_permute(st.packs, layer, st.cur, d == INVERSE), None, started=False)


def _bwd_perm(st, i, layer, d):
    st.g = _permute(st.packs, layer, st.g, d == FORWARD)


def _fwd_elementwise(st, step, layer, d):
    cur = st.cur
    if _awaits_statistics(layer, d):
        layer._data_dependent_init((cur if st.W == st.D else st.packs.unpad_rows(cur)).view(st.N, *layer.event_shape))
    keep_input = layer.value.requires_grad
    out = cur if (not st.cur_is_saved and not keep_input) else torch.empty_like(cur)
    native.elementwise_affine(cur, st.packs.ew_value(layer), out, st.logdet,
                              layer.transformer.native_kind == "inverse_affine",
                              accumulate=st.started, inverse=(d == INVERSE))
    st.advance(out, cur if keep_input else None)


def _bwd_elementwise(st, i, layer, d):
    want = layer.value.requires_grad
    flat = st.maps is not None
    lo = st.maps["ew_out"].get(i) if flat else None
    gv = native.elementwise_affine_bwd(st.saved[i], st.packs.ew_value(layer), st.g, st.gld, want,
                                       inverse=_affine_form_is_inverse(layer, d),
                                       out=None if lo is None else st.out_all[lo:lo + 2 * st.W])
    if want and st.W != st.D and not flat:
        gv = gv.index_select(0, st.packs.phys)              # (W, 2) -> the D logical rows
    st.grads_per_step[i] = [gv.view_as(layer.value) if (want and not flat) else None]


def _fwd_elementwise_ctx(st, step, layer, d):
    h = layer.conditioner_transform(x=None, context=st.plan.context).reshape(st.N, -1).contiguous()
    st.transform(layer, d, h, None, st.D)


def _bwd_elementwise_ctx(st, i, layer, d):
    cparams = _module_params(layer.conditioner_transform)
    with torch.enable_grad():
        h2 = layer.conditioner_transform(x=None, context=st.plan.context).reshape(st.N, -1)
    hc = h2.detach().contiguous()
    gh = torch.empty_like(hc)
    _transform_backward(layer, d, st.saved[i], hc, st.g, st.gld, gh, None, st.D)
    st.grads_per_step[i] = _graph_param_grads(_graph_grads(h2, [], gh, cparams)[1], cparams, zeros=True)


def _fwd_made(st, step, layer, d):
    h = layer.conditioner_transform(st.cur.view(st.N, *layer.event_shape), None).reshape(st.N, -1).contiguous()
    st.transform(layer, FORWARD, h, None, st.D)


def _bwd_made(st, i, layer, d):
    # h depends on every input position (through the masks): re-evaluate MADE with a graph,
    # the transformer's reverse-mode kernel gives dL/dh and the direct dL/dx, autograd the rest
    x_in, g, N = st.saved[i], st.g, st.N
    cparams = _module_params(layer.conditioner_transform)
    mlp = _made_mlp(layer)
    if mlp is not None:             # masked MLP written out (weight-gradient GEMMs split over rows)
        lin1, lin2 = mlp
        W1, W2 = lin1.weight.detach() * lin1.mask, lin2.weight.detach() * lin2.mask
        a1 = torch.tanh(torch.addmm(lin1.bias.detach(), x_in, W1.t()))
        hc = torch.addmm(lin2.bias.detach(), a1, W2.t())
    else:
        x_req = x_in.detach().requires_grad_(True)
        with torch.enable_grad():
            h2 = layer.conditioner_transform(x_req.view(N, *layer.event_shape), None).reshape(N, -1)
        hc = h2.detach().contiguous()
    gh = torch.empty_like(hc)
    _transform_backward(layer, FORWARD, x_in, hc, g, st.gld, gh, None, st.D)
    if mlp is not None:
        g_x, dW1, db1, dW2, db2 = _mlp_backward(W1, W2, x_in, a1, gh)
        g.add_(g_x)
        st.grads_per_step[i] = _mlp_param_grads(cparams, lin1, lin2, dW1 * lin1.mask, db1, dW2 * lin2.mask, db2)
        return
    (g_x,), outs = _graph_grads(h2, [x_req], gh, cparams)
    g.add_(g_x.reshape(N, st.D))
    st.grads_per_step[i] = _graph_param_grads(outs, cparams, zeros=True)


def _fwd_affine(st, step, layer, d):
    # conditioner + transform (+ the fixed elementwise layer and the reversal that follow) in one launch: a flow program
    # on the matrix cores whose operand block is the head of the layer's training pack
    rec = st.packs.record_at[step]
    ops = [(3 if _affine_form_is_inverse(layer, d) else 2, 0, rec.pack.steps2, 0)]   # TFK_OP_AFFINE_*
    ops += _ew_ops(st.plan, rec, rec.pack.param_index.numel())
    st.program(native.flow_run_mfma, rec, ops, st.packed[_AFFINE][rec.k])


def _bwd_affine(st, i, layer, d):            # one launch: conditioner, transform and MLP backward
    rec = st.packs.record_at[i]
    pack, k, block = rec.pack, rec.k, st.packed[_AFFINE][rec.k]
    native.affine_coupling_train_bwd(st.saved[i], st.g, st.gld, block[:pack.param_index.numel()], pack.steps2,
                                     st.out_all[k * pack.n_out:(k + 1) * pack.n_out], pack.workspace,
                                     inverse_form=_affine_form_is_inverse(layer, d),
                                     gscale=_folded_gscale(st.packs, rec, block), g_reversed=rec.rev_step is not None)
    # (the weight gradients leave the accumulators of all layers at once: ChainFunction.backward's epilogues)


def _fwd_wide(st, step, layer, d):
    # above 256 columns: conditioner + transform (+ the fixed elementwise layer and the reversal that follow) as a
    # one-coupling program of the wide-row chain kernel, on the head of the layer's training block
    rec = st.packs.record_at[step]
    st.program(native.flow_run_wide, rec, rec.pack.ops[rec.lean], st.packed[_WIDE][rec.k])


def _bwd_wide(st, i, layer, d):              # one reverse-mode launch + the three row-contracting products
    rec = st.packs.record_at[i]
    pack, x_in = rec.pack, st.saved[i]
    gh_rec, gpre_rec, hid_rec = pack.records(st.N)
    inv = (d == INVERSE) if pack.shift else _affine_form_is_inverse(layer, d)
    native.wide_coupling_train_bwd(x_in, st.g, st.gld, st.packed[_WIDE][rec.k][:pack.n_bwd], gh_rec, gpre_rec, hid_rec,
                                   shift=pack.shift, inverse_form=inv, gscale=_folded_gscale(st.packs, rec),
                                   g_reversed=rec.rev_step is not None)
    _weight_products(x_in, pack.hp, gh_rec, pack.GH, gpre_rec, hid_rec, pack.acc_out)
    st.grads_per_step[i] = _mlp_param_grads(_module_params(layer.conditioner_transform), rec.lin1, rec.lin2,
                                            *pack.unpack_grads(pack.acc_out))


def _fwd_rqs(st, step, layer, d):
    # conditioner + spline (+ the fixed elementwise layer and the reversal that follow) in one launch, a flow program;
    # the operand block is kept for the backward kernel
    rec = st.packs.record_at[step]
    rp = rec.pack
    seg = st.maps["rqs_seg"][rec.k] if st.maps is not None else None   # (the parameters live in one buffer)
    block = st.rqs_packed[seg[0]] if seg is not None else rp.pack(rec.lin1, rec.lin2)
    tr = layer.transformer
    ops = [(7 if d == INVERSE else 6, 0, rp.steps2, 0, 8, float(tr.boundary),
            float(1.0 - tr.min_bin_size * tr.n_bins), float(math.log(math.expm1(1 - tr.min_delta))))]
    ops += _ew_ops(st.plan, rec, rp.n_fwd)
    prm = block[:rp.n_fwd]
    if rec.ew_step is not None:
        ew_layer, ew_d, _ = st.plan[rec.ew_step]
        prm = st.rqs_packed[seg[1]] if seg is not None else torch.cat([prm, _ew_block(ew_layer, ew_d, st.D, st.W)])
    st.rqs_blocks[step] = block
    st.program(native.flow_run_mfma, rec, ops, prm)


def _bwd_rqs(st, i, layer, d):               # conditioner re-evaluated in the kernel, dL/dh written once
    rec = st.packs.record_at[i]
    rp, lin1, lin2 = rec.pack, rec.lin1, rec.lin2
    x_in, g, N = st.saved[i], st.g, st.N
    cparams = _module_params(layer.conditioner_transform)
    gh_perm = torch.empty(N, 768, dtype=torch.float32, device=g.device)
    gpre_perm = torch.empty(N, 16, dtype=torch.float32, device=g.device)
    outer = rows_outer_enabled() and lin1.out_features <= 15
    hid_perm = torch.empty(N, 16, dtype=torch.float32, device=g.device) if outer else None
    native.rqs_coupling_train_bwd(x_in, g, st.gld, st.rqs_blocks[i], rp.steps2, gh_perm, gpre_perm,
                                  layer.transformer.n_bins, layer.transformer.boundary,
                                  inverse=(d == INVERSE), gscale=_folded_gscale(st.packs, rec),
                                  g_reversed=rec.rev_step is not None, hid_perm=hid_perm)
    if outer:
        # un-permuted by ONE gather -- per layer, or, with the parameters in one buffer, by the gather that maps every
        # accumulator of the plan at once
        flat = st.maps is not None
        lo_acc = st.maps["rqs_out"][i] if flat else None
        acc = (st.out_all[lo_acc:lo_acc + rp.n_acc] if flat
               else torch.empty(rp.n_acc, dtype=torch.float32, device=g.device))
        _weight_products(x_in, 32, gh_perm, 768, gpre_perm, hid_perm, acc)
        if flat:
            return
        grads = (t.view(shp) for t, shp in zip(acc.index_select(0, rp.acc_index).split(rp.acc_sizes), rp.acc_shapes))
        st.grads_per_step[i] = _mlp_param_grads(cparams, lin1, lin2, *grads)
        return
    x_a = x_in[:, :layer.coupling.source_event_size]
    a1 = torch.tanh(torch.addmm(lin1.bias, x_a, lin1.weight.t()))
    ones = torch.ones(N, 1, dtype=torch.float32, device=g.device)
    dW2b = _outer_sum(gh_perm, torch.cat([a1, ones], dim=1)).index_select(0, rp.gh_col)
    g_pre = gpre_perm.index_select(1, rp.gpre_col)
    dW1b = _outer_sum(g_pre, torch.cat([x_a, ones], dim=1))
    st.grads_per_step[i] = _mlp_param_grads(cparams, lin1, lin2, dW1b[:, :-1], dW1b[:, -1], dW2b[:, :-1], dW2b[:, -1])


def _fwd_layerwise(st, step, layer, d):
    x_a = _source_rows(layer, st.cur)
    if _keeps_graph(layer) and st.keep_graphs:
        # a convolutional conditioner: evaluated ONCE, with its graph (the activations it saves are what a
        # re-evaluation in the backward pass would produce again -- and a BatchNorm in training mode counts
        # the batch once, as the reference's single forward does)
        x_a = x_a.detach().requires_grad_(True)
        with torch.enable_grad():
            h2 = _conditioner(layer, x_a, st.plan.context)
        st.kept[step] = x_a, h2
        h = h2.detach().contiguous()
    else:
        h = _conditioner(layer, x_a, st.plan.context).contiguous()
    st.transform(layer, d, h, None if layer._target_is_tail else layer._target_index32, layer.coupling.target_event_size)


def _bwd_layerwise(st, i, layer, d):
    x_in, g, N = st.saved[i], st.g, st.N
    S = layer.coupling.source_event_size
    tgt = None if layer._target_is_tail else layer._target_index32
    cparams = _module_params(layer.conditioner_transform)
    x_a = _source_rows(layer, x_in)
    mlp = _plain_mlp(layer)
    if mlp is not None:            # re-evaluate h; keep the hidden activations
        lin1, lin2 = mlp
        a1 = torch.tanh(torch.addmm(lin1.bias, x_a, lin1.weight.t()))
        hc = torch.addmm(lin2.bias, a1, lin2.weight.t())
    elif st.kept.get(i) is not None:      # the forward pass kept the conditioner's graph (used once)
        x_a, h2 = st.kept[i]
        st.kept[i] = None
        hc = h2.detach().contiguous()
    else:                          # any other conditioner: re-evaluate with a graph
        from torchflows_amd import convnet_train
        x_a = x_a.detach().requires_grad_(True)
        with torch.enable_grad(), convnet_train.recomputing():     # (same batch again: BatchNorm's running statistics stay)
            h2 = _conditioner(layer, x_a, st.plan.context)
        hc = h2.detach().contiguous()
    gh = torch.empty_like(hc)
    _transform_backward(layer, d, x_in, hc, g, st.gld, gh, tgt, layer.coupling.target_event_size)
    if mlp is not None:
        g_xa, dW1, db1, dW2, db2 = _mlp_backward(lin1.weight, lin2.weight, x_a, a1, gh)
        st.grads_per_step[i] = _mlp_param_grads(cparams, lin1, lin2, dW1, db1, dW2, db2)
    else:                          # (a trainable parameter the graph does not reach stays None here)
        (g_xa,), outs = _graph_grads(h2, [x_a], gh, cparams)
        g_xa = g_xa.reshape(N, S)
        st.grads_per_step[i] = _graph_param_grads(outs, cparams, zeros=False)
    if layer._source_is_head:
        g[:, :S].add_(g_xa)
    else:
        g.index_add_(1, layer._source_index, g_xa)


# A new training route plugs in here: a predicate next to _fused_bwd_layer, a route in _PlanPacks._fused_route, and its pair.
_STEPS = {_FOLDED: (_fwd_folded, _bwd_folded), _PERM: (_fwd_perm, _bwd_perm),
          _ELEMENTWISE: (_fwd_elementwise, _bwd_elementwise), _ELEMENTWISE_CTX: (_fwd_elementwise_ctx, _bwd_elementwise_ctx),
          _MADE: (_fwd_made, _bwd_made), _AFFINE: (_fwd_affine, _bwd_affine), _RQS: (_fwd_rqs, _bwd_rqs),
          _WIDE: (_fwd_wide, _bwd_wide), _LAYERWISE: (_fwd_layerwise, _bwd_layerwise)}


class ChainFunction(torch.autograd.Function):
    """rows (N, D) -> (rows (N, D), log-det (N,)) through a whole plan: set-up, one ``_STEPS`` function per step by its
    route (``_PlanPacks.routes``), epilogue."""

    @staticmethod
    def forward(ctx, plan, rows: torch.Tensor, *params: torch.Tensor):
        N, D = rows.shape
        st = _State()
        st.logdet = torch.empty(N, dtype=torch.float32, device=rows.device)
        # an ActNorm that still has to take its statistics from this batch cannot ride along
        needs_init = any(kind == "elementwise" and _awaits_statistics(layer, d) for layer, d, kind in plan)
        packs = _plan_packs(plan, D, rows.device, fold=not needs_init)
        # parameters homed in one buffer (FlatAdamW): operands by one gather, gradients as slices of one buffer
        fb = maps = l2vec = None
        if flat_enabled() and packs.flat_capable():
            from torchflows_amd import flat_optim
            fb = flat_optim.lookup(params)
            maps = packs.flat_maps(fb) if fb is not None else None
            if maps is None:
                fb = None
        st.plan, st.packs, st.N, st.D, st.W, st.fb, st.maps, st.device = plan, packs, N, D, packs.W, fb, maps, rows.device
        st.cur, st.cur_is_saved, st.started = rows, True, False         # never write into the caller's tensor
        st.saved, st.kept, st.rqs_blocks, st.rqs_packed = [], {}, {}, None
        if fb is not None:
            packed, st.rqs_packed = packs.pack_flat(fb, maps)
            if plan.l2:
                l2vec = packs.l2_vector(fb, maps, plan.l2)
        else:
            packed = packs.pack() if packs.fused[_AFFINE] else []
        st.packed = {_AFFINE: packed, _WIDE: packs.pack_wide() if packs.fused[_WIDE] else []}
        st.keep_graphs = any(ctx.needs_input_grad)
        if st.W != D:                # padded training layout: every kernel below sees (N, W) rows
            st.cur, st.cur_is_saved = packs.pad_rows(rows), False
        for step, ((layer, d, _), route) in enumerate(zip(plan, packs.routes)):
            _STEPS[route][0](st, step, layer, d)
        cur, logdet = st.cur, st.logdet
        st.cur = st.logdet = None       # (the state goes on to the backward pass: it keeps what that needs, not the outputs)
        if not st.started:
            logdet.zero_()
        if cur is rows:
            cur = rows.clone()
        if st.W != D:
            cur = packs.unpad_rows(cur)
        ctx.state, ctx.n_params, ctx.l2vec = st, len(params), l2vec
        if l2vec is not None:
            # sum_coef coef * sum_p ||p||^2 (layers_base.py:38-48) over the buffer: the gradient joins the flat one
            ctx.flat_version = fb.P._version
            reg = torch.dot(fb.P * l2vec, fb.P)
            return cur, logdet, reg
        return cur, logdet

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_rows: Optional[torch.Tensor], g_logdet: Optional[torch.Tensor],
                 g_reg: Optional[torch.Tensor] = None):
        st = copy.copy(ctx.state)      # (what this pass adds -- the gradient rows, the accumulators -- dies with it)
        plan, packs, fb, maps = st.plan, st.packs, st.fb, st.maps
        N, D, W, device = st.N, st.D, st.W, st.device     # (rows in the padded training layout when W > D)
        if g_rows is None:
            st.g = torch.zeros(N, W, dtype=torch.float32, device=device)
        else:
            st.g = packs.pad_rows(g_rows) if W != D else g_rows.contiguous().clone()
        st.gld = torch.zeros(N, dtype=torch.float32, device=device) if g_logdet is None else g_logdet.contiguous()
        st.grads_per_step = grads_per_step = [[] for _ in plan]
        if fb is not None:
            st.out_all = out_all = torch.empty(maps["n_ext"], dtype=torch.float32, device=device)
            out_all[-1:].zero_()
        else:
            st.out_all = out_all = (torch.empty(packs.n_out_total, dtype=torch.float32, device=device)
                                    if packs.fused[_AFFINE] else None)
        for i in range(len(plan) - 1, -1, -1):
            _STEPS[packs.routes[i]][1](st, i, plan[i][0], plan[i][1])

        def input_grad():
            return None if not ctx.needs_input_grad[1] else (st.g if W == D else packs.unpad_rows(st.g))
        if fb is not None:
            # ONE gather: accumulator layout of every layer -> the layout of the parameter buffer; the gradients leave
            # as slices of it (what FlatAdamW.step looks for)
            G = out_all.index_select(0, maps["grad_src"])
            if ctx.l2vec is not None and g_reg is not None:
                if fb.P._version != ctx.flat_version:
                    raise RuntimeError("the parameter buffer was modified between the forward and the backward pass")
                G.addcmul_(fb.P, ctx.l2vec * g_reg, value=2.0)
            fb.last_grad = G
            pieces = G.split_with_sizes(fb.split_sizes)
            flat = [None if r is None else pieces[r[0]].view(r[1]) for r in maps["ret"]]
            assert len(flat) == ctx.n_params
            return (None, input_grad(), *flat)
        if packs.fused[_AFFINE]:                # accumulator layout -> parameter layout, all layers at once
            pieces = out_all[packs.grad_index]
            lo = 0
            for rec in packs.fused[_AFFINE]:
                sizes = rec.pack.sizes
                grads = (t.view(shp) for t, shp in zip(pieces[lo:lo + sum(sizes)].split(sizes), rec.pack.shapes))
                lo += sum(sizes)
                grads_per_step[rec.step] = _mlp_param_grads(_module_params(plan[rec.step][0].conditioner_transform),
                                                            rec.lin1, rec.lin2, *grads)
        flat = [gp for gs in grads_per_step for gp in gs]
        assert len(flat) == ctx.n_params
        return (None, input_grad(), *flat)


class GaussLogProbFunction(torch.autograd.Function):
    """``DiagonalGaussian.log_prob(rows) [+ log_det]`` (gaussian.py:46-54, flows.py:647-648) with
    fixed loc / scale: one forward and one reverse-mode launch."""

    @staticmethod
    def forward(ctx, rows, loc, log_scale, log_det):
        out = torch.empty(rows.shape[0], dtype=torch.float32, device=rows.device)
        native.diag_gauss_logprob(rows, loc, log_scale, log_det, out)
        ctx.save_for_backward(rows, loc, log_scale)
        ctx.has_ld = log_det is not None
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, glp):
        rows, loc, log_scale = ctx.saved_tensors
        glp = glp.contiguous()
        g = None
        if ctx.needs_input_grad[0]:
            g = torch.empty_like(rows)
            native.diag_gauss_logprob_bwd(rows, loc, log_scale, glp, g)
        return g, None, None, (glp if ctx.has_ld and ctx.needs_input_grad[3] else None)


def run(composition, plan, x: torch.Tensor, context=None) -> Tuple[torch.Tensor, torch.Tensor]:
    from torchflows_amd.utils import as_rows
    rows, batch = as_rows(x, composition.event_shape)
    if context is not None:
        # (a hand-built composition takes its context_shape from its FIRST layer, which may have none: the layers that
        # do take a context reshape the flat rows themselves)
        cs = composition.context_shape
        plan.context = (context.reshape(rows.shape[0], *cs) if cs is not None
                        else context.reshape(rows.shape[0], -1)).contiguous()
    params = [p for layer, _, kind in plan for p in _layer_params(layer, kind)]
    outs = ChainFunction.apply(plan, rows, *params)
    out, ld = outs[0], outs[1]
    if plan.l2:                      # the caller asked for the L2 penalty in the same node: hand it over (or None)
        composition.__dict__["_tfk_l2_out"] = outs[2] if len(outs) == 3 else None
    return out.view(x.shape), ld.view(batch)
