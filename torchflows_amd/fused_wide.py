"""Flow programs for event sizes above 256: the packer of the wide-row chain kernel (csrc/tfk_flow_wide.h).

Chains of affine / shift HalfSplit couplings (RealNVP, NICE, InverseRealNVP ...) on EVEN event sizes 256 < D <= 2048 whose
conditioner is ``Linear(S, H) -> Tanh -> Linear(H, P)`` with H <= 16 become ONE ``tfk_flow_run_wide`` launch.  As in
``flow_compile._compile_lean``: reversals are folded into the column order, elementwise layers with global parameters are
deferred (a pending map x -> s x + t per physical column, folded into W1 / b1 where the column feeds a conditioner,
applied as the pre-affine of the coupling that transforms it, flushed by the closing TFK_OP_EW_FMA together with the sum
of the constant log-dets).  The rows stay at their logical width D in memory; only the parameter blocks know the padded
plane width ``hp`` (the next multiple of 64 above D / 2).

Training does not go through this packer: with gradients enabled ``autograd.ChainFunction`` runs one coupling per launch of
the same kernel, on operands ``train_packs._WideTrainPack`` gathers from the live weights (the block of ``pack_coupling`` with
pre_s = 1, pre_t = 0), and its reverse mode on csrc/tfk_wide_bwd.h.
"""
from __future__ import annotations

from typing import Optional

import torch

from torchflows_amd import flow_compile, fused, native
from torchflows_amd.flow_ops import FORWARD, LEAN_KINDS, OP_EW_FMA
from torchflows_amd.flow_pack import _gemm1_operands, _gemm2_operands, _lanes
from torchflows_amd.utils import debug_switch

WAVES = 4                 # waves of a workgroup = column groups of a plane (csrc/tfk_flow_wide.h)
MAX_COUPLINGS = 64        # kWideMaxOps


def enabled() -> bool:
    """TORCHFLOWS_AMD_DEBUG=wide=0: the routes of the releases before this kernel (layer by layer above 256; the
    vector-ALU interpreter at 512)."""
    return debug_switch("wide", "1") != "0"


def plane_width(D: int) -> int:
    return (D // 2 + 63) // 64 * 64


def layout(D: int, device) -> torch.Tensor:
    """Physical column of logical element l on entry: each half at the head of its plane."""
    half, hp = D // 2, plane_width(D)
    l_ = torch.arange(D, device=device)
    return torch.where(l_ < half, l_, l_ - half + hp)


def pack_coupling(lk: int, H: int, hp: int, W1f, b1f, W2p, b2p, pre_s, pre_t) -> torch.Tensor:
    """Parameter block of one coupling (layout: csrc/tfk_flow_wide.h).  Inputs fp64 in physical order, pending
    elementwise maps of the source plane already folded into W1f / b1f; the pre-scaling is the lean format's."""
    dev = W1f.device
    E = hp // 16                                               # columns per lane and plane
    P = W2p.shape[1]
    W1pad, b1pad, _ = _gemm1_operands(H, W1f, b1f)
    W2pad, b2q = _gemm2_operands(H, W2p, b2p, affine=LEAN_KINDS[lk].family == "affine")
    _, ql, _, unit1, q2, r2, qq, rr = _lanes(dev)
    w_ = torch.arange(WAVES, device=dev)
    k_ = torch.arange(4, device=dev)
    # A1[w][g][l][k]: hidden unit unit1(i), source column (4 w + q) E + 4 g + k
    g_ = torch.arange(E // 4, device=dev)
    cols = ((4 * w_.view(-1, 1, 1, 1) + ql.view(1, 1, 64, 1)) * E + 4 * g_.view(1, -1, 1, 1) + k_.view(1, 1, 1, 4))
    A1 = W1pad[unit1.view(1, 1, 64, 1).expand_as(cols), cols]
    b1m = b1pad[4 * rr + qq]                                   # [q][r]
    # A2[w][t][l][k]: hidden unit 4 k + (l >> 4), output row i = 4 q2 + r2 of tile t of wave w
    # (P = 2, affine: tile t holds both parameters of 2 columns per lane group; P = 1, shift: 4 columns)
    T2 = E * P // 4
    t_ = torch.arange(T2, device=dev)
    col = lambda q, r: (4 * w_.view(-1, 1, 1, 1) + q) * E + (4 // P) * t_.view(1, -1, 1, 1) + r // P
    m_l, p_l = col(q2.view(1, 1, 64, 1), r2.view(1, 1, 64, 1)), (r2 % P).view(1, 1, 64, 1)
    m_b = col(qq.view(1, 1, 4, 4), rr.view(1, 1, 4, 4))
    p_b = (rr % P).view(1, 1, 4, 4).expand_as(m_b)
    shape = (WAVES, T2, 64, 4)
    A2 = W2pad[m_l.expand(shape), p_l.expand(shape), (4 * k_.view(1, 1, 1, 4) + ql.view(1, 1, 64, 1)).expand(shape)]
    b2m = b2q[m_b, p_b]                                        # [w][t][q][r]
    return torch.cat([A1.reshape(-1), b1m.reshape(-1), A2.reshape(-1), b2m.reshape(-1), pre_s, pre_t]).float()


def block_floats(hp: int, affine: bool) -> int:
    E = hp // 16
    T2 = E // 2 if affine else E // 4
    return 256 * E + 16 + WAVES * T2 * 256 + WAVES * T2 * 16 + 2 * hp


def compile_wide(composition, plan, device, D: int, direction: int) -> Optional["fused.CompiledChain"]:
    """``plan`` (``flow_compile._flatten`` of the composition in ``direction``) as one wide segment, or None."""
    from torchflows_amd.bijections.finite.autoregressive.layers_base import CouplingBijection, ElementwiseBijection
    from torchflows_amd.bijections.finite.matrix.permutation import PermutationMatrix
    if plan is None or D % 2 or D <= 256 or not native.lib().tfk_flow_wide_supported(D, 1):
        return None
    hp = plane_width(D)
    Dp = 2 * hp
    pos_in = layout(D, device)
    pos = pos_in.clone()
    pending = flow_compile._PendingMap(Dp, device)
    ops, blocks, used, kind0 = [], [], 0, None
    with torch.no_grad():
        for layer, d in plan:
            if isinstance(layer, PermutationMatrix):
                perm = (layer._fwd_index if d == FORWARD else layer._inv_index).to(device)
                pos = pos[perm]
            elif isinstance(layer, ElementwiseBijection):
                got = flow_compile._lean_elementwise(layer, d, D)
                if got is None:
                    return None
                pending.compose(pos, *got)
            elif isinstance(layer, CouplingBijection):
                got = flow_compile._lean_coupling(layer, d, pos, D, Dp)
                if got is None:
                    return None
                lk, plane, H, W1t, b1, W2p, b2p = got
                if (LEAN_KINDS[lk].family not in ("affine", "shift") or not native.lib().tfk_flow_wide_supported(D, H)
                        or len(ops) == MAX_COUPLINGS):
                    return None
                if kind0 is None:
                    kind0 = lk
                elif lk != kind0:
                    return None                               # (a program holds couplings of one kind)
                src = torch.arange(plane * hp, (plane + 1) * hp, device=device)
                tgt = torch.arange((1 - plane) * hp, (2 - plane) * hp, device=device)
                W1f, b1f = pending.fold(W1t, b1, src)
                block = pack_coupling(lk, H, hp, W1f, b1f, W2p, b2p, *pending.take(tgt))
                ops.append((LEAN_KINDS[lk].op, plane, H, used))
                blocks.append(block)
                used += block.numel()
            else:
                return None
    if not ops:
        return None
    ops.append((OP_EW_FMA, 0, 0, used))
    blocks.append(pending.flush())
    seg = fused.Segment(ops, torch.cat(blocks).contiguous(), True, wide=True)
    return fused.CompiledChain(Dp, [seg], pos, bool(torch.equal(pos, pos_in)), fused._params_version(composition),
                               D_log=D, pos_in=pos_in)


def is_wide(chain) -> bool:
    return chain is not None and len(chain.segments) == 1 and chain.segments[0].wide


def _reversed_out(chain) -> bool:
    """The rows come out exactly reversed: the kernel's store writes logical column c to D - 1 - c (flag bit 1)."""
    hit = chain.__dict__.get("_wide_reversed")
    if hit is None:
        hit = chain.__dict__["_wide_reversed"] = (not chain.identity_out
                                                  and bool(torch.equal(chain.pos, chain.pos_in.flip(0))))
    return hit


def _base_physical(chain, base, of_input: bool):
    """Base parameters in the kernel's physical order (2 hp entries), cached.  Pad columns hold 0 throughout: loc 0 and
    log_scale = -0.5 log(2 pi) make their density term vanish exactly."""
    key = (of_input, base[0].data_ptr(), base[0]._version, base[1].data_ptr(), base[1]._version)
    hit = chain.__dict__.get("_base_cache")
    if hit is None or hit[0] != key:
        where = chain.pos_in if of_input else chain.pos
        loc_p = base[0].new_zeros(chain.D)
        ls_p = base[1].new_full((chain.D,), -0.9189385332046727)
        loc_p[where] = base[0]
        ls_p[where] = base[1]
        chain.__dict__["_base_cache"] = hit = (key, loc_p, ls_p)
    return hit[1], hit[2]


def run_wide(chain, rows: torch.Tensor, want_rows: bool, base=None, base_of_input: bool = False):
    """``fused.run_chain`` for a wide chain: one launch, plus a row reorder where the chain leaves the rows permuted
    other than reversed."""
    N, D = rows.shape
    dev = rows.device
    seg = chain.segments[0]
    logprob = torch.empty(N, dtype=torch.float32, device=dev) if base is not None else None
    logdet = torch.empty(N, dtype=torch.float32, device=dev) if base is None else None
    out = torch.empty_like(rows) if want_rows else None
    if N == 0:
        return out, logdet, logprob
    loc_p = ls_p = None
    if base is not None:
        loc_p, ls_p = _base_physical(chain, base, base_of_input)
    rev = want_rows and _reversed_out(chain)
    native.flow_run_wide(rows, out, logdet, loc_p, ls_p, logprob, seg.packed_ops(), seg.params,
                         reverse_out=rev, base_of_input=base_of_input)
    if want_rows and not chain.identity_out and not rev:
        idx = chain.__dict__.get("_wide_gather")
        if idx is None:                                        # column of the stored row that holds logical element l
            hp, half = chain.D // 2, D // 2
            idx = torch.where(chain.pos < hp, chain.pos, chain.pos - hp + half).to(torch.int32)
            chain.__dict__["_wide_gather"] = idx
        cur, out = out, torch.empty_like(out)
        native.permute(cur, idx, out)
    return out, logdet, logprob
