"""Host-side compiler from a ``BijectiveComposition`` to libtfk *flow programs*.

``tfk_flow_run`` (csrc/tfk_flow.hip) keeps each row in registers and applies a list of ops
to it, with the conditioner MLP evaluated in-kernel -- one launch for a whole chain of
layers.  This module turns the reference-shaped layer objects into that
list:

* permutation layers emit nothing: the compiler tracks ``pos[l]`` = physical position of
  logical element ``l`` and packs every later layer's parameters in physical order;
* ElementwiseAffine / ActNorm become ``alpha*x+beta`` / ``(x-beta)/alpha`` ops with
  ``alpha = exp(u/2 + log(1-1e-10)) + 1e-10`` and ``sum log alpha`` evaluated once per
  compilation (they are batch-constant; the reference recomputes them per row);
* Affine / Shift couplings on the HalfSplit mask whose conditioner is the default
  ``FeedForward`` (Linear, Tanh, Linear) become coupling ops; after the folded reversals
  the conditioner's input must still be exactly one half ("plane") of the physical row.

* RQ-spline couplings (8 bins) and the parallel map of MADE-based affine / RQ-spline layers have
  ops of their own on the matrix-core kernel (``tfk_flow_run_mfma``: event sizes 64 / 128 / 256);
* other event sizes ride on the same kernel padded: even sizes with each half at the head of its
  plane, odd sizes (HalfSplit moves one element across the halves at every reversal) with every
  element owning an index in both planes and ``OP_PLANE_SWAP`` ops in front of the couplings --
  padding elements see zero weights, i.e. the identity with log-det 0.

Anything else (other masks, context, deeper / non-tanh conditioners, ActNorm that still has to
initialise itself from data) makes ``compile_chain`` return ``None`` and the composition runs
layer by layer (bijections/base.py).  The cache of compiled programs and their launch are ``fused``'s, the operand
layouts ``flow_pack``'s, the op codes and the table of lean kinds ``flow_ops``'s.
"""
from __future__ import annotations

import math
from typing import List, Optional

import numpy as np
import torch
import torch.nn as nn

from torchflows_amd import flow_ops, fused, native
from torchflows_amd.flow_ops import (
    FMT_BF16X3, FMT_F16X2, FORWARD, INVERSE, LDS_LIMIT, LEAN_KINDS, MAX_CONTEXT, MAX_HIDDEN_RQS, N_BINS,
    OP_AFFINE_FWD, OP_AFFINE_INV, OP_EWC_MULADD, OP_EWC_SUBDIV, OP_EW_FMA, OP_EW_MULADD, OP_EW_SUBDIV, OP_MADE_FWD,
    OP_MADE_INV, OP_MADE_RQS, OP_PLANE_SWAP, OP_RQS_FWD, OP_RQS_INV, OP_SHIFT_FWD, OP_SHIFT_INV, RQS_PAD, lean_kind)
from torchflows_amd.flow_pack import (
    _affine_scale, _lanes, _pack_lean, _pack_lean_made, _pack_lean_made_spline, _pack_lean_rqs, _pack_mfma, _pad4,
    lean_bf16x3_enabled, lean_enabled, lean_f16x2_enabled, odd_lean_enabled, padded_enabled, rows16_enabled,
    rqs_bf16x3_enabled, stream_chain_enabled)
from torchflows_amd.fused import CompiledChain, Segment
from torchflows_amd.utils import debug_switch


def _flatten(layers, attr: str):
    """[(layer, direction)] with nested compositions expanded; None if a layer's bound
    forward/inverse is not one of the tagged implementations."""
    from torchflows_amd.bijections.base import BijectiveComposition, method_direction
    out = []
    for layer in layers:
        d = method_direction(getattr(layer, attr))
        if d is None:
            return None
        if isinstance(layer, BijectiveComposition):
            inner = layer.layers if d == FORWARD else list(layer.layers)[::-1]
            sub = _flatten(inner, "forward" if d == FORWARD else "inverse")
            if sub is None:
                return None
            out.extend(sub)
        else:
            out.append((layer, d))
    return out


def _constant_elementwise(layer, d: int, D: int):
    """(alpha, beta, divide) of an ElementwiseAffine / ActNorm with global parameters in LOGICAL order, fp32 as the
    reference computes them -- ``z = alpha x + beta`` or, with ``divide``, ``z = (x - beta) / alpha`` -- or None."""
    from torchflows_amd.bijections.finite.autoregressive.layers import ActNorm
    kind = layer.transformer.native_kind
    if kind not in ("affine", "inverse_affine") or not layer.use_global_parameters:
        return None
    if isinstance(layer, ActNorm) and layer.training and layer.first_training_batch_pass:
        return None                       # must see a batch first (layers.py:58-68)
    value = layer.value.detach().reshape(D, 2)
    return layer.transformer.constrain_scale(value[:, 0]), value[:, 1], (d == INVERSE) != (kind == "inverse_affine")


def _elementwise_op(layer, d: int, pos: torch.Tensor, D: int, Dp: Optional[int] = None):
    got = _constant_elementwise(layer, d, D)
    if got is None:
        return None
    alpha, beta, subdiv = got
    ld = torch.log(alpha).sum()
    ld = -ld if subdiv else ld
    Dp = D if Dp is None else Dp
    alpha_p = alpha.new_ones(Dp)               # padding elements: alpha = 1, beta = 0 (identity, log alpha = 0)
    beta_p = beta.new_zeros(Dp)
    alpha_p[pos] = alpha
    beta_p[pos] = beta
    parts = [alpha_p, beta_p, ld.reshape(1), ld.new_zeros(3)]
    if subdiv:
        parts.append(1.0 / alpha_p)           # correctly rounded reciprocal for the in-kernel quotient
    return (OP_EW_SUBDIV if subdiv else OP_EW_MULADD, 0, 0), torch.cat(parts)


def _halfsplit_coupling(layer, pos: torch.Tensor, D: int, Dp: int, max_context: int):
    """What every coupling op asks of its layer -- an affine / shift / spline transformer (8 bins) on the HalfSplit mask,
    the default FeedForward(tanh) conditioner, at most ``max_context`` context elements, after the folded reversals the
    sources in one plane of the ``Dp``-wide physical row and the targets in the other -- and its weights in physical
    order: (kind, C, H, source plane, W1t (H, hp), b1, W2p (hp, P, H), b2p (hp, P), W1c (H, C) or None), or None."""
    # padding elements: zero weights => h = 0 => alpha = exp(c0) + 1e-10 = 1, beta = 0, log alpha = 0 exactly (a padded
    # RQ-spline element has all-zero parameters: equal bins, unit derivatives -- the identity at its value 0, log-det 0 up
    # to the 1 ulp of softplus(c) + 1e-5 vs 1)
    from torchflows_amd.bijections.finite.autoregressive.conditioning.transforms import FeedForward
    from torchflows_amd.utils import event_size as _esize
    kind = layer.transformer.native_kind
    if kind not in ("affine", "inverse_affine", "shift", "rqs", "lrs"):
        return None
    C = _esize(layer.context_shape) if layer.context_shape is not None else 0
    if C > max_context or (kind in ("rqs", "lrs") and layer.transformer.n_bins != N_BINS):
        return None
    c = layer.coupling
    S, T = c.source_event_size, c.target_event_size        # HalfSplit: D // 2 and D - D // 2 (coupling_masks.py:78-81)
    if not (c.source_is_head and c.target_is_tail and S == D // 2 and S + T == D):
        return None
    ct = layer.conditioner_transform
    if type(ct) is not FeedForward or ct.n_global_parameters != 0:
        return None
    if ct.output_lower_bound != float("-inf") or ct.output_upper_bound != float("inf"):
        return None
    mods = list(ct.sequential)
    if not (len(mods) == 4 and isinstance(mods[0], nn.Linear) and isinstance(mods[1], nn.Tanh)
            and isinstance(mods[2], nn.Linear) and isinstance(mods[3], nn.Unflatten)):
        return None
    P = {"shift": 1, "rqs": 23, "lrs": 32}.get(kind, 2)
    W1, b1 = mods[0].weight.detach(), mods[0].bias.detach()          # (H, S + C), (H,)
    W2, b2 = mods[2].weight.detach(), mods[2].bias.detach()          # (T*P, H), (T*P,)
    H = W1.shape[0]
    if W1.shape[1] != S + C or W2.shape[0] != T * P or W2.shape[1] != H:
        return None
    W1c = W1[:, S:] if C else None            # [x_A || context]: the context's columns (conditioning/context.py:46-60)
    W1 = W1[:, :S]
    hp = Dp // 2                              # plane width the kernel sees (> D // 2 when padded)
    src_pos, tgt_pos = pos[:S], pos[S:]
    plane = int(src_pos[0].item()) // hp
    if not bool(((src_pos // hp) == plane).all()) or not bool(((tgt_pos // hp) == 1 - plane).all()):
        return None
    W1t = W1.new_zeros(H, hp)
    W1t[:, src_pos - plane * hp] = W1
    m_t = tgt_pos - (1 - plane) * hp
    W2p = W2.new_zeros(hp, P, H)
    W2p[m_t] = W2.reshape(T, P, H)
    b2p = b2.new_zeros(hp, P)
    b2p[m_t] = b2.reshape(T, P)
    return kind, C, H, plane, W1t, b1, W2p, b2p, W1c


def _coupling_op(layer, d: int, pos: torch.Tensor, D: int, mfma: bool = False, Dp: Optional[int] = None):
    if (Dp is None or Dp == D or not mfma) and D % 2:
        return None                           # odd event sizes: padded matrix-core programs only
    Dp = D if Dp is None else Dp
    if Dp != D and not mfma:
        return None                           # padded planes: matrix-core path only
    # (a context: matrix-core interpreter only, tfk_flow_run_mfma_ctx)
    got = _halfsplit_coupling(layer, pos, D, Dp, MAX_CONTEXT if mfma else 0)
    if got is None or got[0] == "lrs":
        return None
    kind, C, H, plane, W1t, b1, W2p, b2p, W1c = got
    if C and H > 16:
        return None
    half, P = D // 2, W2p.shape[1]
    if mfma:
        if H > (16 if kind == "rqs" else 128) or (kind == "rqs" and Dp > 128):
            return None
        head, block = _pack_mfma(kind, d, plane, H, Dp, W1t, b1, W2p, b2p)
        if C:                                 # further GEMM-1 k-steps: A1c[cs][64], lane (q, i) <-> context element 4 s + q
            cs = (C + 3) // 4
            W1cp = W1c.new_zeros(16, 4 * cs)
            W1cp[:H, :C] = W1c
            L = _lanes(W1c.device)
            A1c = torch.stack([W1cp[L.unit1, 4 * s_ + L.ql] for s_ in range(cs)])
            block = torch.cat([block, A1c.reshape(-1).to(block.dtype)])
            head = (head[0], head[1] | (cs << 4)) + tuple(head[2:])
        if kind == "rqs":
            head = head + _rqs_extra(layer.transformer)
        return head, block
    if kind == "rqs":
        if H > MAX_HIDDEN_RQS:
            return None
        G = D // 8
        # physical target m = 4*j + e  ->  [k][e][j][24] (23 parameters + 1 pad)
        W2q = W2p.new_zeros(half, RQS_PAD, H)
        W2q[:, :P] = W2p
        b2q = b2p.new_zeros(half, RQS_PAD)
        b2q[:, :P] = b2p
        W2t = W2q.reshape(G, 4, RQS_PAD, H).permute(3, 1, 0, 2).reshape(-1)
        b2t = b2q.reshape(G, 4, RQS_PAD).permute(1, 0, 2).reshape(-1)
        block = torch.cat([W1t.reshape(-1), _pad4(b1), W2t, b2t])
        return (OP_RQS_FWD if d == FORWARD else OP_RQS_INV, plane, H) + _rqs_extra(layer.transformer), block
    block = torch.cat([W1t.reshape(-1), _pad4(b1), W2p.permute(2, 0, 1).reshape(-1), b2p.reshape(-1)])
    if kind == "shift":
        op = OP_SHIFT_FWD if d == FORWARD else OP_SHIFT_INV
    else:
        op = OP_AFFINE_FWD if (d == FORWARD) != (kind == "inverse_affine") else OP_AFFINE_INV
    return (op, plane, H), block


def _elementwise_ctx_op(layer, d: int, pos: torch.Tensor, D: int, Dp: int, lean: bool = False):
    """An elementwise affine layer whose parameters come from the CONTEXT through the default Linear conditioner
    (layers_base.py:300-318) as a TFK_OP_EWC_* op: Ac[EPL][cs][64] | bc[EPL][4][4] (csrc/tfk_flow_mfma.h: ewc_m)."""
    from torchflows_amd.bijections.finite.autoregressive.conditioning.transforms import Linear
    from torchflows_amd.utils import event_size as _esize
    kind = layer.transformer.native_kind
    ct = layer.conditioner_transform
    if kind not in ("affine", "inverse_affine") or layer.use_global_parameters or type(ct) is not Linear:
        return None
    if ct.n_global_parameters != 0 or ct.output_lower_bound != float("-inf") or ct.output_upper_bound != float("inf"):
        return None
    lin = ct.sequential[0]
    C = _esize(layer.context_shape)
    if not isinstance(lin, nn.Linear) or lin.in_features != C or lin.out_features != 2 * D or C > MAX_CONTEXT:
        return None
    cs = (C + 3) // 4
    EPL, hp = Dp // 8, Dp // 2
    dev = lin.weight.device
    W = torch.zeros(Dp, 2, 4 * cs, dtype=lin.weight.dtype, device=dev)      # physical element, parameter, context column
    W[pos, :, :C] = lin.weight.detach().view(D, 2, C)
    bq = torch.zeros(Dp, 2, dtype=lin.bias.dtype, device=dev)               # padding: zero logits = the identity
    bq[pos] = lin.bias.detach().view(D, 2)
    if lean:      # inside a lean program (csrc/tfk_flow_chain.h: ewc_lean): alpha = exp2(.) + 1e-10, as the lean couplings
        W, bq = W.double(), bq.double()
        _affine_scale(W, bq)
    L = _lanes(dev)
    ql, q2, r2, qq, rr = L.ql, L.q2, L.r2, L.qq, L.rr
    A, bm = [], []
    for t in range(EPL):
        plane, tt = (0, t) if t < EPL // 2 else (1, t - EPL // 2)
        m_l = plane * hp + EPL * q2 + 2 * tt + (r2 >> 1)
        for s_ in range(cs):
            A.append(W[m_l, r2 & 1, 4 * s_ + ql])
        bm.append(bq[plane * hp + EPL * qq + 2 * tt + (rr >> 1), rr & 1])
    block = torch.cat([torch.stack(A).reshape(-1), torch.stack(bm).reshape(-1)])
    subdiv = (d == INVERSE) != (kind == "inverse_affine")
    return (OP_EWC_SUBDIV if subdiv else OP_EWC_MULADD, cs << 4, 0), block


def _plane_swap(layer, pos: torch.Tensor, Dp: int):
    """Odd event sizes run in a layout where logical element l owns index l of BOTH planes (Dp >= 2 D), so an
    element changes planes by a swap with the zero that sits at its index in the other plane.  Returns
    ``(item or None, new pos)`` such that the coupling's source elements share one plane and its targets the
    other (the assignment that needs fewer swaps)."""
    hp = Dp // 2
    S = layer.coupling.source_event_size
    plane = pos // hp
    src, tgt = plane[:S], plane[S:]
    cost0 = int((src != 0).sum() + (tgt != 1).sum())        # sources in plane 0, targets in plane 1
    cost1 = int((src != 1).sum() + (tgt != 0).sum())
    want_src = 0 if cost0 <= cost1 else 1
    want = torch.cat([torch.full_like(src, want_src), torch.full_like(tgt, 1 - want_src)])
    wrong = plane != want
    if not bool(wrong.any()):
        return None, pos
    slot = pos % hp
    mask = torch.zeros(hp, dtype=torch.float32, device=pos.device)
    mask[slot[wrong]] = 1.0
    new_pos = torch.where(wrong, want * hp + slot, pos)
    return ((OP_PLANE_SWAP, 0, 0), mask), new_pos


def _made_layers(layer, d: int, D: int):
    """The modules (MaskedLinear, Tanh, MaskedLinear) of the conditioner of a MADE-based layer whose map in direction ``d``
    is the PARALLEL one; None for the sequential map, deeper MADEs, a context."""
    from torchflows_amd.bijections.finite.autoregressive.conditioning.transforms import MADE
    ct = layer.conditioner_transform
    if d == layer._sequential_when or layer.context_shape is not None or ct.n_global_parameters != 0:
        return None
    if ct.output_lower_bound != float("-inf") or ct.output_upper_bound != float("inf"):
        return None
    mods = list(ct.sequential)
    if not (len(mods) == 3 and isinstance(mods[0], MADE.MaskedLinear) and isinstance(mods[1], nn.Tanh)
            and isinstance(mods[2], MADE.MaskedLinear)) or mods[0].in_features != D:
        return None
    return mods


def _made_op(layer, d: int, pos: torch.Tensor, D: int, Dp: Optional[int] = None):
    """A MADE-based affine layer's PARALLEL map as one matrix-core op (tfk_flow_mfma.hip: made_m).
    None for the sequential map, other transformers, deeper MADEs, a context."""
    kind = layer.transformer.native_kind
    mods = _made_layers(layer, d, D)
    if kind not in ("affine", "inverse_affine", "rqs") or mods is None:
        return None
    H = mods[0].out_features
    Dp = D if Dp is None else Dp              # padded row width: padding elements get zero weights (identity)
    if H > 128 or (Dp == 256 and H > 16):
        return None
    if kind == "rqs":
        return _made_rqs_op(layer, mods, pos, D, H, Dp)
    half, EPL = Dp // 2, Dp // 8
    T2 = EPL // 2
    steps2 = (H + 3) // 4
    HT = 1 if steps2 <= 4 else (2 if steps2 <= 8 else (4 if steps2 <= 16 else 8))
    W1 = (mods[0].weight * mods[0].mask).detach()                       # (H, D) logical columns
    W2 = (mods[2].weight * mods[2].mask).detach().view(D, 2, H)        # logical element, parameter, unit
    dev, dt = W1.device, W1.dtype
    W1p = torch.zeros(16 * HT, Dp, dtype=dt, device=dev)
    W1p[:H, pos] = W1                                                   # physical columns
    b1p = torch.zeros(16 * HT, dtype=dt, device=dev)
    b1p[:H] = mods[0].bias.detach()
    W2p = torch.zeros(Dp, 2, 16 * HT, dtype=dt, device=dev)
    W2p[pos, :, :H] = W2                                                # physical elements
    b2p = torch.zeros(Dp, 2, dtype=dt, device=dev)
    b2p[pos] = mods[2].bias.detach().view(D, 2)
    _, ql, _, unit1, q2, r2, qq, rr = _lanes(dev)
    A1 = torch.stack([W1p[16 * t + unit1, plane * half + EPL * ql + s]
                      for plane in range(2) for s in range(EPL) for t in range(HT)])
    b1m = torch.stack([b1p[16 * t + 4 * rr + qq] for t in range(HT)])
    A2, b2m = [], []
    for plane in range(2):
        for t in range(T2):
            for r1 in range(steps2):
                A2.append(W2p[plane * half + EPL * q2 + 2 * t + (r2 >> 1), r2 & 1, 4 * r1 + ql])
            b2m.append(b2p[plane * half + EPL * qq + 2 * t + (rr >> 1), rr & 1])
    block = torch.cat([A1.reshape(-1), b1m.reshape(-1), torch.stack(A2).reshape(-1), torch.stack(b2m).reshape(-1)])
    divide = (kind == "inverse_affine")                # the parallel map uses transformer.forward
    return (OP_MADE_INV if divide else OP_MADE_FWD, 0, steps2), block


def _made_rqs_op(layer, mods, pos: torch.Tensor, D: int, H: int, Dp: Optional[int] = None):
    """The parallel map of a MADE-based RQ-spline layer (8 bins, hidden <= 16, D <= 128) as one matrix-core
    op (tfk_flow_mfma.h: made_rqs_m): A1[2 EPL][64] | b1[4][4] | A2[2 EPL 6][steps2][64] | b2[2 EPL 6][4][4]."""
    tr = layer.transformer
    Dp = D if Dp is None else Dp
    if tr.n_bins != N_BINS or H > 16 or Dp > 128:
        return None
    half, EPL = Dp // 2, Dp // 8
    steps2 = (H + 3) // 4
    W1 = (mods[0].weight * mods[0].mask).detach()                       # (H, D) logical columns
    W2 = (mods[2].weight * mods[2].mask).detach().view(D, 23, H)       # logical element, parameter, unit
    dev, dt = W1.device, W1.dtype
    W1p = torch.zeros(16, Dp, dtype=dt, device=dev)
    W1p[:H, pos] = W1                                                   # physical columns
    b1p = torch.zeros(16, dtype=dt, device=dev)
    b1p[:H] = mods[0].bias.detach()
    W2p = torch.zeros(Dp, 24, 16, dtype=dt, device=dev)
    W2p[pos, :23, :H] = W2                                              # physical elements, 23 + 1 pad
    b2p = torch.zeros(Dp, 24, dtype=dt, device=dev)
    b2p[pos, :23] = mods[2].bias.detach().view(D, 23)
    _, ql, _, unit1, q2, r2, qq, rr = _lanes(dev)
    A1 = torch.stack([W1p[unit1, plane * half + EPL * ql + s] for plane in range(2) for s in range(EPL)])
    b1m = b1p[4 * rr + qq]
    A2, b2m = [], []
    for plane in range(2):
        for e in range(EPL):
            for c in range(6):
                for r1 in range(steps2):
                    A2.append(W2p[plane * half + EPL * q2 + e, 4 * c + r2, 4 * r1 + ql])
                b2m.append(b2p[plane * half + EPL * qq + e, 4 * c + rr])
    block = torch.cat([A1.reshape(-1), b1m.reshape(-1), torch.stack(A2).reshape(-1), torch.stack(b2m).reshape(-1)])
    return (OP_MADE_RQS, 0, steps2) + _rqs_extra(tr), block


def _rqs_extra(tr) -> tuple:
    """Fields 5..8 of an interpreter RQ-spline op: (bins, boundary, 1 - min_bin_size * n_bins, the derivative logits' offset)."""
    return (N_BINS, float(tr.boundary), float(np.float32(1.0 - tr.min_bin_size * tr.n_bins)),
            float(np.float32(math.log(math.expm1(1 - tr.min_delta)))))


def _lean_spline_extra(tr, lrs: bool, fmt: int) -> tuple:
    """Fields 5..8 of a lean spline op: (bins | operand format, boundary, 1 - min_bin * n_bins, delta), delta being the
    fp32 constant under the derivative logits (RQ: ``boundary_u_delta``; linear rational: ``const``)."""
    width, delta = (tr.min_bin_width, tr.const) if lrs else (tr.min_bin_size, tr.boundary_u_delta)
    return (N_BINS | fmt, float(tr.boundary), float(np.float32(1.0 - width * tr.n_bins)), float(np.float32(delta)))


# ---------------------------------------------------------------------------------------------
# lean chains (csrc/tfk_flow_chain.h): couplings of one kind, elementwise layers deferred
# ---------------------------------------------------------------------------------------------
def _lean_elementwise(layer, d: int, D: int):
    """``_constant_elementwise`` in fp64 (of the fp32 scale the reference uses), or None."""
    got = _constant_elementwise(layer, d, D)
    return None if got is None else (got[0].double(), got[1].double(), got[2])


def _lean_coupling(layer, d: int, pos: torch.Tensor, D: int, Dp: int, allow_ctx: bool = False):
    """``_halfsplit_coupling`` for the lean programs, hidden width <= 16 (splines: 31): (lean kind ``lk`` of
    flow_ops.LEAN_KINDS, source plane, H, W1t (H, hp), b1, W2p (hp, P, H), b2p (hp, P)) in fp64 -- with ``allow_ctx`` also
    the context's columns W1c (further GEMM-1 k-steps) or None --, or None.  (T = S + 1: odd event sizes.)"""
    got = _halfsplit_coupling(layer, pos, D, Dp, MAX_CONTEXT if allow_ctx else 0)
    if got is None:
        return None
    kind, _, H, plane = got[:4]
    lk = lean_kind("affine" if kind == "inverse_affine" else kind, (d == INVERSE) != (kind == "inverse_affine"))
    if H > LEAN_KINDS[lk].max_hidden:
        return None
    weights = tuple(None if w is None else w.double() for w in got[4:])
    return (lk, plane, H) + (weights if allow_ctx else weights[:4])


def _lean_made(layer, d: int, pos: torch.Tensor, D: int, Dp: int):
    """Physical-order weights of a MADE-based affine / spline layer's PARALLEL map (the checks of ``_made_op``), fp64:
    (lean kind, H, W1p (H, Dp), b1, W2p (Dp, P, H), b2p (Dp, P)) or None."""
    kind = layer.transformer.native_kind
    mods = _made_layers(layer, d, D)
    if kind not in ("affine", "inverse_affine", "rqs", "lrs") or mods is None:
        return None
    if kind in ("rqs", "lrs") and layer.transformer.n_bins != N_BINS:
        return None
    lk = lean_kind("made_" + kind) if kind in ("rqs", "lrs") else lean_kind("made", kind == "inverse_affine")
    P, H = LEAN_KINDS[lk].params, mods[0].out_features
    if H > LEAN_KINDS[lk].max_hidden:
        return None
    W1 = (mods[0].weight * mods[0].mask).detach().double()                     # (H, D) logical columns
    W2 = (mods[2].weight * mods[2].mask).detach().double().view(D, P, H)       # logical element, parameter, unit
    W1p = W1.new_zeros(H, Dp)
    W1p[:, pos] = W1
    W2p = W2.new_zeros(Dp, P, H)
    W2p[pos] = W2
    b2p = W2.new_zeros(Dp, P)
    b2p[pos] = mods[2].bias.detach().double().view(D, P)
    return lk, H, W1p, mods[0].bias.detach().double(), W2p, b2p


class _PendingMap:
    """The deferred elementwise layers of a lean program (``_compile_lean``, ``fused_wide.compile_wide``): physical column c
    carries a pending map x -> s[c] x + t[c], fp64 on the host, and ``ld_const`` the sum of the constant log-dets."""

    def __init__(self, width: int, device):
        self.s = torch.ones(width, dtype=torch.float64, device=device)
        self.t = torch.zeros(width, dtype=torch.float64, device=device)
        self.ld_const = torch.zeros((), dtype=torch.float64, device=device)

    def compose(self, pos: torch.Tensor, alpha: torch.Tensor, beta: torch.Tensor, divide: bool) -> None:
        """An elementwise layer (``_lean_elementwise``) behind what is pending, logical element l at column pos[l]."""
        s, t = self.s, self.t
        if divide:
            s[pos] = s[pos] / alpha
            t[pos] = (t[pos] - beta) / alpha
            self.ld_const = self.ld_const - torch.log(alpha).sum()
        else:
            s[pos] = alpha * s[pos]
            t[pos] = alpha * t[pos] + beta
            self.ld_const = self.ld_const + torch.log(alpha).sum()

    def fold(self, W1: torch.Tensor, b1: torch.Tensor, cols=None):
        """(W1, b1) of a conditioner that reads ``cols`` (None: the whole row) with their maps folded in:
        W1 (s x + t) + b1 = (W1 s) x + (W1 t + b1)."""
        s, t = (self.s, self.t) if cols is None else (self.s[cols], self.t[cols])
        return W1 * s, b1 + W1 @ t

    def take(self, cols=None):
        """(s, t) of the columns a layer transforms -- its pre-affine --, which then carry nothing."""
        cols = slice(None) if cols is None else cols
        pre = self.s[cols].clone(), self.t[cols].clone()
        self.s[cols] = 1.0
        self.t[cols] = 0.0
        return pre

    def move(self, old: int, new: int) -> None:
        """The map of column ``old`` goes to column ``new`` (the middle element of an odd event size changes planes)."""
        self.s[new], self.t[new] = self.s[old].clone(), self.t[old].clone()
        self.s[old], self.t[old] = 1.0, 0.0

    def is_identity(self, ignore_logdet: bool = False) -> bool:
        return (bool((self.s == 1).all()) and bool((self.t == 0).all())
                and (ignore_logdet or float(self.ld_const) == 0.0))

    def flush(self) -> torch.Tensor:
        """The TFK_OP_EW_FMA block s | t | ld | 0 0 0 (fp32) of what is pending, which is then the identity."""
        block = torch.cat([self.s, self.t, self.ld_const.reshape(1), self.ld_const.new_zeros(3)]).float()
        self.s.fill_(1.0)
        self.t.fill_(0.0)
        self.ld_const = torch.zeros_like(self.ld_const)
        return block


_SIDE_OPS = (OP_EW_FMA, OP_EWC_MULADD, OP_EWC_SUBDIV)     # elementwise ops inside a lean program
_SMALL_OPS = (OP_EW_MULADD, OP_EW_SUBDIV, OP_PLANE_SWAP, OP_EWC_MULADD, OP_EWC_SUBDIV)


def _cut_segments(items, mfma: bool, budget: Optional[int] = None, max_ops: int = 0, may_cut=None, riders=()):
    """``items`` [(op, src_plane, steps, block, extra)] as launches whose parameter blocks fit ``budget`` bytes of LDS and
    that hold ``max_ops`` ops at most; ``budget`` None: one launch whatever its size (streamed operands, a few elementwise
    ops).  ``may_cut(op, n_ops)``: a launch of ``n_ops`` ops may end in front of ``op`` (None: anywhere); ``riders``: ops
    that ride along past the budget as long as the launch fits the LDS at all.  None if one block alone does not fit it."""
    segments: List[Segment] = []
    ops, blocks, used = [], [], 0
    for op, plane, steps, block, extra in items:
        n = block.numel()
        if budget is not None:
            if n * 4 > LDS_LIMIT:
                return None
            over = (used + n) * 4 > budget and not (op in riders and (used + n) * 4 <= LDS_LIMIT)
            if ops and (over or len(ops) >= max_ops) and (may_cut is None or may_cut(op, len(ops))):
                segments.append(Segment(ops, torch.cat(blocks).contiguous(), mfma))
                ops, blocks, used = [], [], 0
        ops.append((op, plane, steps, used) + tuple(extra))
        blocks.append(block.float())
        used += n
    if ops:
        segments.append(Segment(ops, torch.cat(blocks).contiguous(), mfma))
    return segments


def _interpreter_items(pairs):
    """[(op head (kind, src_plane, H, *extra), block)] of the interpreter op builders as items of ``_cut_segments``."""
    return [(head[0], head[1], head[2], block, tuple(head[3:])) for head, block in pairs]


def _lean_budget(Dp: int, kind, bf16x3: bool) -> int:
    """LDS bytes one launch of a lean program of ``kind`` (a LeanKind, or None for a chain without couplings) may stage."""
    budget = max(flow_ops.MAX_PARAM_BYTES_MFMA, flow_ops.MFMA_BUDGET_WIDE.get(Dp, 0))
    if bf16x3:
        budget = LDS_LIMIT          # bf16 x 3 operands: one 1024-thread workgroup per CU holds the whole chain
    if Dp == 64 and kind is not None and kind.family in ("affine", "shift"):
        # the 64-wide chain kernel is register-bound at 4 waves per SIMD = TWO 512-thread workgroups per CU: up to
        # 76 KB of operands per launch cost no occupancy (12 couplings, or 8 with their context columns)
        budget = max(budget, flow_ops.LEAN_BUDGET_64)
    if Dp == 128:
        # the 128-wide chain kernel runs one 768-thread workgroup per CU whatever the block's size: RealNVP(128, 8 layers)
        # = 90.6 KB is ONE launch (at the interpreter's 76 KB budget it was two, and the rows' trip through HBM between
        # them -- 0.9 GB per launch at 2.8 TB/s -- bound both: 2 x 316 us)
        budget = LDS_LIMIT
    return budget


def _lean_formats(plan, Dp: int, context: bool, odd: bool):
    """The operand formats of GEMM 2 to try for an affine / shift chain, in order: split f16 where eligible, then bf16 x 3
    where eligible, then fp32 (0), which every chain has.  (Spline chains carry their format in ``rqs_bf16x3``.)"""
    from torchflows_amd.bijections.finite.autoregressive.layers_base import CouplingBijection
    formats = []
    # split-f16 operands (lean_f16x2_enabled): resident blocks of ONE launch, no context, even event sizes, H <= 10, and only
    # while lean_bf16x3 is left at "auto" (0 asks for fp32 operands, 1 for bf16 x 3); whatever does not fit -- a weight that
    # is not representable, a chain that would need a second launch -- is packed again in the fp32 format
    if (lean_f16x2_enabled(Dp) and debug_switch("lean_bf16x3", "auto") == "auto" and not odd and not context
            and Dp in (32, 64, 128)):
        formats.append(FMT_F16X2)
    # bf16 x 3 operands: D = 64 only where the whole chain stays ONE launch (10.6 KB of operands per coupling instead of
    # 5.7) -- decided by a dry count of the couplings --, and D = 256 (round 4: the streamed chain takes the format too --
    # 42 KB per coupling, two blocks resident)
    n_couplings = sum(isinstance(layer, CouplingBijection) for layer, _ in plan)
    if lean_bf16x3_enabled(Dp) and not odd and ((Dp == 64 and 0 < n_couplings <= 13)
                                                or (Dp == 256 and not context and stream_chain_enabled())):
        formats.append(FMT_BF16X3)
    return formats + [0]


_ABANDON = object()       # an attempt in one operand format gives up: the next format of ``_lean_formats`` is tried


class _LeanWalk:
    """One attempt at a lean program in one operand format ``fmt``: what the layers of the plan share while they are walked."""

    def __init__(self, plan, device, D: int, Dp: int, pos: torch.Tensor, context: bool, odd: bool, fmt: int):
        from torchflows_amd.bijections.finite.autoregressive.layers_base import (
            CouplingBijection, ElementwiseBijection, MaskedAutoregressiveBijection)
        self.device, self.D, self.Dp, self.pos, self.context, self.odd, self.fmt = device, D, Dp, pos, context, odd, fmt
        self.pending = _PendingMap(Dp, device)
        self.items = []                                      # (op, src_plane, steps2, block, extra)
        self.kind0 = self.steps0 = None                      # lean kind and GEMM-2 steps of the program's layers
        self.extra = ()                                      # fields 5.. of its op records (operand format, spline constants)
        self.ctx_bits = 0
        self.head, self.tail, self.closed_flush = [], [], None   # (context) interpreter ops around the chain
        self.pre_items, self.post_items = [], []                 # (context) elementwise ops inside the lean launch
        # (context) if a context-conditioned elementwise layer precedes the first coupling, every elementwise layer before
        # that coupling is an interpreter op of the launch in front of the chain (the inverse direction starts with a
        # constant ActNorm followed by the context-conditioned layer)
        self.first_c = next((i for i, (layer, _) in enumerate(plan)
                             if isinstance(layer, (CouplingBijection, MaskedAutoregressiveBijection))), len(plan))
        self.head_mode = context and any(isinstance(layer, ElementwiseBijection) and not layer.use_global_parameters
                                         for layer, _ in plan[:self.first_c])
        # affine / shift chains take those elementwise layers INSIDE the lean launch (csrc/tfk_flow_chain.h: side_op): in front
        # of the couplings and behind the closing TFK_OP_EW_FMA, up to 3 ops per side -- one launch per conditional log_prob
        self.kind_c = (plan[self.first_c][0].transformer.native_kind
                       if self.first_c < len(plan) and isinstance(plan[self.first_c][0], CouplingBijection) else None)
        self.inline = context and (self.kind_c in ("affine", "inverse_affine", "shift")
                                   or (self.kind_c in ("rqs", "lrs") and Dp <= 128 and rqs_bf16x3_enabled()))

    def run(self, plan):
        """The segments of the lean chain, None where a layer has no place in one, ``_ABANDON`` where only the format fails."""
        from torchflows_amd.bijections.finite.autoregressive.layers_base import (
            CouplingBijection, ElementwiseBijection, MaskedAutoregressiveBijection)
        from torchflows_amd.bijections.finite.matrix.permutation import PermutationMatrix
        if self.inline and self.Dp == 256 and self.kind_c not in ("rqs", "lrs"):
            # the context variant of the 256-wide chain kernel spills (660 B of scratch at the 256-VGPR cap): measured
            # 1.8e8 evals/s against the interpreter's 3.5e8 on a conditional RealNVP(256) -- the interpreter keeps that size
            return None
        with torch.no_grad():
            for li, (layer, d) in enumerate(plan):
                if isinstance(layer, PermutationMatrix):
                    ok = self.permutation(layer, d)
                elif isinstance(layer, ElementwiseBijection) and self.context and not layer.use_global_parameters:
                    ok = self.context_elementwise(layer, d)
                elif isinstance(layer, ElementwiseBijection):
                    ok = self.constant_elementwise(layer, d, li)
                elif isinstance(layer, MaskedAutoregressiveBijection):
                    ok = self.made(layer, d)
                elif isinstance(layer, CouplingBijection):
                    ok = self.coupling(layer, d)
                else:
                    ok = None
                if ok is not True:
                    return ok
        return self.segments()

    def permutation(self, layer, d: int):
        self.pos = self.pos[(layer._fwd_index if d == FORWARD else layer._inv_index).to(self.device)]
        return True

    def _ew_fma(self):
        return (OP_EW_FMA, 0, 0, self.pending.flush(), ())

    def _same_program(self, lk: int, steps2: int) -> bool:
        """A program holds layers of ONE kind and hidden width (couplings and MADE layers do not share one)."""
        if self.kind0 is None:
            self.kind0, self.steps0 = lk, steps2
        return (lk, steps2) == (self.kind0, self.steps0)

    def context_elementwise(self, layer, d: int):
        """An elementwise layer whose parameters are a Linear map of the context: a TFK_OP_EWC_* op inside the lean launch
        (``inline``) or in an interpreter launch of its own in front of / behind the chain."""
        before = not self.items and self.closed_flush is None
        item = _elementwise_ctx_op(layer, d, self.pos, self.D, self.Dp, lean=self.inline)
        if item is None:
            return None
        if self.inline:
            ewc = (item[0][0], item[0][1], 0, item[1].float(), ())
            if before:                                       # in front of the couplings: what is pending goes first
                if not self.pending.is_identity():
                    self.pre_items.append(self._ew_fma())
                self.pre_items.append(ewc)
            else:                                            # behind them: close the chain (once), then the op
                if self.closed_flush is None:
                    self.closed_flush = self.pending.flush()
                elif not self.pending.is_identity():
                    self.post_items.append(self._ew_fma())
                self.post_items.append(ewc)
            return True if len(self.pre_items) <= 3 and len(self.post_items) <= 2 else None
        if before:                                           # before the chain: nothing may be pending
            if not self.pending.is_identity(ignore_logdet=True):
                return None
            self.head.append(item)
        else:                                                # after it: the chain ends here, pending maps flushed
            if self.closed_flush is None:
                self.closed_flush = self.pending.flush()
            self.tail.append(item)
        return True

    def constant_elementwise(self, layer, d: int, li: int):
        """An elementwise layer with global parameters: deferred (composed into the pending maps), or -- beside
        context-conditioned layers that run on the interpreter -- an interpreter op of the same launch as those."""
        if not self.inline and ((self.head_mode and li < self.first_c) or self.closed_flush is not None):
            item = _elementwise_op(layer, d, self.pos, self.D, self.Dp)
            if item is None:
                return None
            (self.head if self.closed_flush is None else self.tail).append(item)
            return True
        got = _lean_elementwise(layer, d, self.D)
        if got is None:
            return None
        self.pending.compose(self.pos, *got)
        return True

    def made(self, layer, d: int):
        """MAF density / IAF sampling: the parallel map of a MADE layer."""
        # (odd event sizes: any layout serves a MADE layer -- the conditioner reads and transforms every element; no moves)
        if self.context or self.Dp < 32:
            return None
        got = _lean_made(layer, d, self.pos, self.D, self.Dp)
        if got is None:
            return None
        lk, H, W1p, b1, W2p, b2p = got
        kind = LEAN_KINDS[lk]
        steps2, extra = (H + 3) // 4, ()
        if kind.spline:                                      # MADE spline layers: the single-launch spline chain kernel
            if not rqs_bf16x3_enabled() or self.Dp not in (64, 128):
                return None
            steps2 = (H + 1 + 3) // 4
            extra = _lean_spline_extra(layer.transformer, kind.family == "made_lrs", FMT_BF16X3)
        if not self._same_program(lk, steps2) or (self.items and self.extra != extra):
            return None
        W1f, b1f = self.pending.fold(W1p, b1)
        pre_s, pre_t = self.pending.take()
        if kind.spline:
            block = _pack_lean_made_spline(H, self.Dp, W1f, b1f, W2p, b2p, pre_s, pre_t, extra[3], kind.family == "made_lrs")
        else:
            block = _pack_lean_made(H, self.Dp, W1f, b1f, W2p, b2p, pre_s, pre_t)
        self.items.append((kind.op, 0, steps2, block, extra))
        self.extra = extra
        return True

    def _move_middle(self, layer):
        """The move bit of a coupling at an odd event size (0: nothing to move), or None."""
        # ODD event sizes: HalfSplit has one target more than sources, and with the reversals the MIDDLE element is a target
        # of every coupling -- it has to sit in whichever plane is being transformed.  Both planes reserve their last column
        # for it (the caller's layout puts it there); before a coupling that finds it in its SOURCE plane the kernel takes it
        # over (bit 2 of the op's src_plane, csrc/tfk_flow_chain.h: move_middle), and its pending map moves with it here.
        hp = self.Dp // 2
        S_ = layer.coupling.source_event_size
        src_plane = int(self.pos[0].item()) // hp
        wrong = ((self.pos[S_:] // hp) == src_plane).nonzero().flatten()
        if wrong.numel() > 1:
            return None
        if wrong.numel() == 0:
            return 0
        l_mid = S_ + int(wrong[0].item())
        old, new = int(self.pos[l_mid].item()), (1 - src_plane) * hp + hp - 1
        if old != src_plane * hp + hp - 1:
            return None
        self.pos[l_mid] = new
        self.pending.move(old, new)
        return 4

    def coupling(self, layer, d: int):
        Dp, hp = self.Dp, self.Dp // 2
        if self.closed_flush is not None:
            return None                                      # (a coupling behind a context-conditioned elementwise layer)
        moved = 0
        if self.odd:
            moved = self._move_middle(layer)
            if moved is None:
                return None
        got = _lean_coupling(layer, d, self.pos, self.D, Dp, allow_ctx=self.context)
        if got is None:
            return None
        lk, plane, H, W1t, b1, W2p, b2p = got[:7]
        W1c = got[7] if self.context else None
        kind = LEAN_KINDS[lk]
        fmt3 = rqs_bf16x3_enabled()
        if self.context:
            if kind.spline and not fmt3:
                return None                                  # (lean context spline programs: bf16 x 3 operands)
            cs_l = 0 if W1c is None else (W1c.shape[1] + 3) // 4
            if self.items and (cs_l << 4) != self.ctx_bits:
                return None
            self.ctx_bits = cs_l << 4
        steps2 = (H + 3) // 4
        if kind.spline:
            if Dp < 32:
                return None                                  # (16-wide rows: affine / shift chains only)
            if (self.odd or kind.family == "lrs") and not fmt3:
                return None                                  # (odd event sizes, linear rational splines: bf16 x 3 operands only)
            if fmt3:
                steps2 = (H + 1 + 3) // 4                    # bf16 x 3 operands: counts the bias unit; > 4 = two hidden tiles
        if not self._same_program(lk, steps2) or (self.items and plane != 1 - (self.items[-1][1] & 1)):
            return None                                      # (the source planes of a program's couplings alternate)
        src = torch.arange(plane * hp, (plane + 1) * hp, device=self.device)
        tgt = torch.arange((1 - plane) * hp, (2 - plane) * hp, device=self.device)
        W1f, b1f = self.pending.fold(W1t, b1, src)
        if kind.spline:                                      # one launch for the chain, operands streamed
            lrs = kind.family == "lrs"                       # (as the RQ spline, 32 parameters)
            # (fp32 operands: chunks of 8 elements per lane group; bf16 x 3: the last hidden unit carries the bias, H <= 31)
            if not fmt3 and (H > 16 or Dp < 64):
                return None
            extra = _lean_spline_extra(layer.transformer, lrs, FMT_BF16X3 if fmt3 else 0)
            if self.items and self.extra != extra:
                return None
            pre_s, pre_t = self.pending.take(tgt)
            block = _pack_lean_rqs(H, Dp, W1f, b1f, W2p, b2p, pre_s, pre_t, extra[3], bf16x3=fmt3, lrs=lrs, W1c=W1c)
        else:
            use3 = self.fmt == FMT_BF16X3 and H <= 15 and not self.context
            useh = self.fmt == FMT_F16X2 and H <= 10
            extra = (FMT_BF16X3,) if use3 else ((FMT_F16X2,) if useh else ())
            if self.items and self.extra != extra:           # (formats mixed in one chain)
                return _ABANDON if self.fmt == FMT_F16X2 else None
            pre_s, pre_t = self.pending.take(tgt)
            block = _pack_lean(lk, H, Dp, W1f, b1f, W2p, b2p, pre_s, pre_t, bf16x3=use3, W1c=W1c, f16x2=useh)
            if block is None:                                # (a weight the split-f16 format cannot hold)
                return _ABANDON
        self.items.append((kind.op, plane | moved, steps2, block, extra))
        self.extra = extra
        return True

    def segments(self):
        """Close the chain and cut it into launches."""
        if self.inline and self.closed_flush is not None and not self.pending.is_identity():
            self.post_items.append(self._ew_fma())           # constant layers behind the last context op
        flush = self.closed_flush if self.closed_flush is not None else self.pending.flush()
        if self.context and not self.items:
            return None
        Dp, kind = self.Dp, LEAN_KINDS.get(self.kind0)
        affine_shift = kind is not None and kind.family in ("affine", "shift")
        streamed = kind is not None and kind.streamed        # spline chains read their operands from global memory
        n_pre = len(self.pre_items)
        items = self.pre_items + self.items + [(OP_EW_FMA, 0, 0, flush, ())] + self.post_items
        # affine / shift chains whose blocks do not fit the LDS together (D = 256: 22 KB per coupling): ONE launch with the
        # operands streamed block by block (csrc/tfk_flow_chain.h: chain_layers_stream) instead of one launch per LDS-full
        total = sum(block.numel() for _, _, _, block, _ in items) * 4
        if (affine_shift and not self.context and not self.odd and Dp >= 128 and stream_chain_enabled() and len(items) <= 61
                and total > 158 * 1024 and (self.extra == () or (Dp == 256 and self.extra == (FMT_BF16X3,)))):
            streamed = True
        elif Dp == 256 and self.extra == (FMT_BF16X3,):
            # bf16 x 3 blocks at D = 256 exist as STREAMED operands only: a chain short enough to keep its blocks resident
            # (three couplings) is packed again in the fp32 format
            return _ABANDON
        # a launch never ends in front of an elementwise op of the chain or inside the ops in front of the couplings
        items = [(op, plane | (0 if op in _SIDE_OPS else self.ctx_bits), steps2, block, extra)
                 for op, plane, steps2, block, extra in items]
        segments = _cut_segments(items, True, None if streamed else _lean_budget(Dp, kind, self.extra == (FMT_BF16X3,)),
                                 flow_ops.MAX_OPS_LEAN, may_cut=lambda op, n_ops: op not in _SIDE_OPS and n_ops > n_pre)
        if segments is None:
            return None
        if len(segments) > 1 and self.extra == (FMT_F16X2,):
            return _ABANDON                                  # (split-f16 blocks are a little larger: never at the price of a launch)
        if self.head:                                        # a few interpreter ops (elementwise layers) as one launch
            segments = _cut_segments(_interpreter_items(self.head), True) + segments
        if self.tail:
            segments = segments + _cut_segments(_interpreter_items(self.tail), True)
        return segments


def _compile_lean(composition, plan, device, D: int, Dp: int, pos: torch.Tensor, pos_in: torch.Tensor,
                  context: bool = False, odd: bool = False):
    """The chain as LEAN flow programs (csrc/tfk_flow_chain.h), or None: elementwise layers with global parameters,
    folded reversals and affine / shift couplings of one kind and one hidden width <= 16 whose source plane
    alternates -- every RealNVP / NICE preset.  The elementwise layers are deferred (``_PendingMap``): physical column c
    carries a pending map x -> s[c] x + t[c] (fp64 on the host) that is folded into W1 / b1 where c feeds a conditioner,
    applied by the coupling that transforms c (its pre-affine), and flushed by one TFK_OP_EW_FMA at the end together
    with the sum of the constant log-dets.
    ``context`` (conditional flows; spline chains only): the couplings' conditioners read [x_A | context] -- the
    context's columns of W1 are further k-steps of GEMM 1 --, and the elementwise layers whose parameters are a Linear map
    of the context (the presets' first and second-to-last layer) run as interpreter ops (TFK_OP_EWC_*) in a launch of
    their own before / after the lean chain: 3 launches for a conditional CouplingRQNSF instead of one per coupling.
    ``odd``: odd event sizes (affine / shift and spline chains), the middle element in the last column of a plane
    (``_LeanWalk._move_middle``).
    The plan is walked once per operand format of ``_lean_formats`` until one yields a chain."""
    if odd and (context or (D + 1) // 2 > Dp // 2):
        return None
    segments = _ABANDON
    for fmt in _lean_formats(plan, Dp, context, odd):
        walk = _LeanWalk(plan, device, D, Dp, pos.clone(), context, odd, fmt)
        segments = walk.run(plan)
        if segments is not _ABANDON:
            break
    if segments is None:
        return None
    return CompiledChain(Dp, segments, walk.pos, bool(torch.equal(walk.pos, pos_in)), fused._params_version(composition),
                         D_log=D, pos_in=pos_in if Dp != D else None)


def compile_chain(composition, direction: int, device: torch.device,
                  mfma: Optional[bool] = None, context: bool = False) -> Optional[CompiledChain]:
    """Flow programs for ``composition.forward`` (direction 0) or ``.inverse`` (1), or None.
    ``mfma`` None: use the matrix-core kernel when the chain qualifies (D in {64, 128}, affine /
    shift couplings, hidden width <= 16), else the vector-ALU one."""
    from torchflows_amd.bijections.finite.autoregressive.layers_base import (
        CouplingBijection, ElementwiseBijection, MaskedAutoregressiveBijection)
    from torchflows_amd.bijections.finite.matrix.permutation import PermutationMatrix

    D = composition.n_dim
    if not fused.enabled():
        return None
    # even event sizes that are not 64 / 128 / 256: both halves are padded to the next supported plane width
    # (the rows are padded on the way in, run_chain) -- matrix-core programs with affine / shift couplings only
    Dp = D
    if not native.lib().tfk_flow_mfma_supported(D) and D % 2 == 0 and 4 <= D < 256:
        Dp = 64 if D < 64 else (128 if D < 128 else 256)
    # even event sizes above 256: the wide-row chain kernel (csrc/tfk_flow_wide.h), one launch for the chain -- tried first,
    # so that D = 512 only falls to the vector-ALU interpreter with TORCHFLOWS_AMD_MFMA=0 or TORCHFLOWS_AMD_DEBUG=wide=0
    if mfma is None and fused.mfma_enabled() and not context and D % 2 == 0 and D > 256:
        from torchflows_amd import fused_wide
        if fused_wide.enabled():
            order_w = composition.layers if direction == FORWARD else list(composition.layers)[::-1]
            chain = fused_wide.compile_wide(composition, _flatten(order_w, "forward" if direction == FORWARD else "inverse"),
                                            device, D, direction)
            if chain is not None:
                return chain
    # odd event sizes: HalfSplit moves one element across the halves at every reversal, so every element gets
    # its own index in both planes (plane width >= D) and changes planes by TFK_OP_PLANE_SWAP
    slots = D % 2 == 1 and 3 <= D <= 64          # (the swap op is not built for 256-wide rows)
    if slots:
        Dp = 64 if D <= 32 else 128
    # odd event sizes above 64: the straight-line kernels only (the middle element changes planes there, _compile_lean)
    odd_wide = D % 2 == 1 and 64 < D < 256
    if odd_wide:
        Dp = 128 if D < 128 else 256
    if mfma is None:
        if fused.mfma_enabled() and native.lib().tfk_flow_mfma_supported(Dp) and padded_enabled(D, Dp):
            chain = compile_chain(composition, direction, device, mfma=True, context=context)
            if chain is not None:
                return chain
        mfma = False
    if context and not mfma:
        return None                              # context-conditioned programs: matrix-core interpreter only
    if not mfma:
        Dp = D
    elif Dp != D and not padded_enabled(D, Dp):
        return None
    if not native.lib().tfk_flow_supported(Dp):
        return None
    order = composition.layers if direction == FORWARD else list(composition.layers)[::-1]
    plan = _flatten(order, "forward" if direction == FORWARD else "inverse")
    if plan is None:
        return None
    def planes(width):                           # logical element -> physical column of a row of `width`
        p_ = torch.arange(D, device=device)
        if width != D and not slots:             # second half of the row starts at the padded plane boundary
            p_ = torch.where(p_ < D // 2, p_, p_ - D // 2 + width // 2)
        return p_
    if mfma and not slots and lean_enabled():
        # event sizes <= 32: the straight-line kernels exist at row width 32 as well (half the work of a 64-wide row)
        # (conditional flows: the elementwise layers around the chain are interpreter launches -- 64 columns at least)
        narrow = D % 2 == 0 and not context
        widths = (([16] if (narrow and 4 <= D <= 16 and rows16_enabled()) else [])
                  + ([32] if (narrow and 4 <= D <= 32) else []) + [Dp])
        for w in widths:
            if w != D and not padded_enabled(D, w):
                continue
            chain = _compile_lean(composition, plan, device, D, w, planes(w), planes(w), context=context)
            if chain is not None:
                return chain
    if mfma and D % 2 == 1 and 3 <= D < 256 and lean_enabled() and odd_lean_enabled() and not context:
        # odd event sizes on the straight-line kernels (affine / shift chains): sources at the head of plane A, the
        # targets behind the middle element at the head of plane B, the middle element in plane B's last column
        h_ = D // 2
        for w in (16, 32, 64, 128, 256):
            if (D + 1) // 2 > w // 2 or (w == 16 and not rows16_enabled()) or not padded_enabled(D, w):
                continue
            l_ = torch.arange(D, device=device)
            lay = torch.where(l_ < h_, l_, torch.where(l_ == h_, torch.full_like(l_, w - 1), w // 2 + l_ - h_ - 1))
            chain = _compile_lean(composition, plan, device, D, w, lay, lay.clone(), context=False, odd=True)
            if chain is not None:
                return chain
            if w >= 32:
                break                            # (a wider row would not make a chain lean that is not lean here; 16-wide
                                                 # rows are for affine / shift chains only: a spline chain gets 32)
    if odd_wide:
        return None                              # (no interpreter route at these sizes)
    pos = planes(Dp)
    pos_in = pos.clone()                         # (odd sizes: the whole row enters in plane 0, element l at index l)
    items = []                                   # [(op triple, block)]
    with torch.no_grad():
        for layer, d in plan:
            if isinstance(layer, PermutationMatrix):
                perm = (layer._fwd_index if d == FORWARD else layer._inv_index).to(device)
                pos = pos[perm]                  # new logical j = old logical perm[j]
                continue
            if isinstance(layer, ElementwiseBijection):
                if context and not layer.use_global_parameters:
                    item = _elementwise_ctx_op(layer, d, pos, D, Dp)
                else:
                    item = _elementwise_op(layer, d, pos, D, Dp)
            elif isinstance(layer, CouplingBijection):
                if slots and Dp != D:
                    swap, pos = _plane_swap(layer, pos, Dp)
                    if swap is not None:
                        items.append(swap)
                item = _coupling_op(layer, d, pos, D, mfma=mfma, Dp=Dp)
            elif isinstance(layer, MaskedAutoregressiveBijection):
                item = _made_op(layer, d, pos, D, Dp) if mfma else None
            else:
                item = None
            if item is None:
                return None
            items.append(item)
    # pack into launches whose parameter block fits the LDS budget: a launch holds as many ops as fit; a coupling op too
    # big for the budget gets a launch of its own, and the small elementwise ops around it ride along
    budget = (max(flow_ops.MAX_PARAM_BYTES_MFMA, flow_ops.MFMA_BUDGET_WIDE.get(Dp, 0)) if mfma
              else flow_ops.MAX_PARAM_BYTES)
    segments = _cut_segments(_interpreter_items(items), mfma, budget, flow_ops.MAX_OPS, riders=_SMALL_OPS)
    if segments is None:
        return None                              # a single op larger than LDS: not fusable here
    identity = bool(torch.equal(pos, pos_in))
    if Dp != D and not segments:
        return None
    return CompiledChain(Dp, segments, pos, identity, fused._params_version(composition), D_log=D,
                         pos_in=pos_in if Dp != D else None)
