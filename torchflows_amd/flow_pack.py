"""Operand packers of the flow programs: physical-order conditioner weights -> the per-lane blocks the MFMA kernels read
(csrc/tfk_flow_mfma.hip, tfk_flow_chain.h, tfk_flow_rqs_chain.h; the wide-row kernel's packer is
``fused_wide.pack_coupling``), and the route / format switches only the compiler and these packers read."""
from __future__ import annotations

from collections import namedtuple
from typing import Optional

import torch

from torchflows_amd.flow_ops import (AFF_C0, FORWARD, LEAN_KINDS, LOG2E, OP_AFFINE_FWD, OP_AFFINE_INV, OP_RQS_FWD, OP_RQS_INV,
                                     OP_SHIFT_FWD, OP_SHIFT_INV)
from torchflows_amd.utils import debug_switch


def lean_enabled() -> bool:
    return debug_switch("lean", "1") != "0"


def lean_bf16x3_enabled(Dp: int = 64) -> bool:
    """bf16 x 3 operands for GEMM 2 of affine / shift chains (TORCHFLOWS_AMD_DEBUG=lean_bf16x3=0 / 1; default "auto").
    D = 64: OFF unless forced -- measured on RealNVP-64 (2^20 rows): 252.0 us per launch against 255.8 us with fp32
    operands.  The 12 f32 MFMAs it removes (384 matrix cycles per wave-layer) come back as 12 bf16 MFMAs (~192) + 22 vector
    instructions for the split + a 1024-thread workgroup per CU (85 KB of operands).
    D = 256 (streamed operands): ON -- round 4, RealNVP-256 on 2^19 rows, same box, alternating: 617 -> 545 us per launch
    (8.25 -> 9.34e8 evals/s, +13 %): 48 f32 MFMAs per wave-layer (1 536 matrix cycles of the layer's 2 560) become 48 bf16
    ones (~770) for the same 22-instruction split; parity unchanged (tests/test_gpu_fused.py)."""
    mode = debug_switch("lean_bf16x3", "auto")
    return mode == "1" or (mode == "auto" and Dp == 256)


def lean_f16x2_enabled(Dp: int = 64) -> bool:
    """Split-f16 operands for GEMM 2 of affine / shift chains of hidden width <= 10 (csrc/tfk_flow_chain.h: couple_lean_h;
    TORCHFLOWS_AMD_DEBUG=lean_f16x2=0 / 1; default "auto"): every weight and every tanh output as hi = f16(v),
    lo = f16(v - hi), the three piece products of a tile in ONE v_mfma_f32_16x16x32_f16 where the fp32 format takes
    ceil(H / 4) v_mfma_f32_16x16x4_f32.  ``1`` turns it on wherever the format exists (Dp in 32 / 64 / 128, resident
    operands, no context, even event size, H <= 10, every weight representable, ``lean_bf16x3`` not forced); ``auto``
    where it was measured faster by more than three times the spread of the runs it replaces (round 5, same box, the
    two libraries alternating, five plain ``bench.py`` runs each, per launch / per step):
    D = 64:  ON  -- RealNVP-64, 2^20 rows: 250.5 us (249.0 .. 253.0) -> 195.2 us (193.2 .. 196.9), 267.7 -> 213.1 us per step
             (3.92 -> 4.92e9 evals/s): 12 f32 MFMAs per wave-layer (384 matrix cycles) become 4 f16 ones (~64) + 13 vector
             instructions for the split; 106 VGPRs, two 512-thread workgroups per CU as before.
    D = 128: ON  -- RealNVP-128, 2^20 rows: 501.1 us (499.5 .. 502.1) -> 365.1 us (356.9 .. 367.3), 518.9 -> 382.9 us per step.
    D = 32:  OFF unless forced -- RealNVP(32, 8), 2^20 rows: 121.6 us (119.0 .. 122.1) -> 116.2 us (115.3 .. 116.8): 5.4 us
             against a bar of 9.3; that launch moves 268 MB in 116 us and is no longer bound by the matrix pipe.
    Parity: log_prob within 3e-7 of the fp32 operand format and of the host's fp64 value (tests/test_gpu_lean_f16.py)."""
    mode = debug_switch("lean_f16x2", "auto")
    return mode == "1" or (mode == "auto" and Dp in _F16X2_AUTO)


_F16X2_AUTO = (64, 128)    # row widths at which "auto" selects the split-f16 format


def rqs_bf16x3_enabled() -> bool:
    return debug_switch("rqs_bf16x3", "1") != "0"


def stream_chain_enabled() -> bool:
    """One launch with streamed operands for affine / shift chains that do not fit the LDS (TORCHFLOWS_AMD_DEBUG=stream_chain=0:
    one launch per LDS-full of couplings, as before)."""
    return debug_switch("stream_chain", "1") != "0"


def odd_lean_enabled() -> bool:
    """Odd event sizes on the straight-line chain kernels (TORCHFLOWS_AMD_DEBUG=odd_lean=0: the interpreter with a plane per
    element, as before round 3)."""
    return debug_switch("odd_lean", "1") != "0"


def rows16_enabled() -> bool:
    """Row width 16 for affine / shift chains on event sizes <= 16 (TORCHFLOWS_AMD_DEBUG=rows16=0: width 32 as before)."""
    return debug_switch("rows16", "1") != "0"


def padded_enabled(D: int, Dp: int) -> bool:
    return Dp == D or debug_switch("fused_pad", "1") != "0"


def _pad4(t: torch.Tensor) -> torch.Tensor:
    r = (-t.numel()) % 4
    return t if r == 0 else torch.cat([t, t.new_zeros(r)])


# Index vectors of a wave's 64 lanes, lane l = (q = l >> 4, i = l & 15), as every MFMA operand layout uses them: (64,)
# lane, ql = q, il = i, unit1 = 4 (i & 3) + (i >> 2) (the hidden unit of D-row i in GEMM 1), q2 = i >> 2, r2 = i & 3; and
# (4, 4) qq, rr: [q][r] -> q, r (the bias tiles)
Lanes = namedtuple("Lanes", "lane ql il unit1 q2 r2 qq rr")


def _lanes(dev) -> Lanes:
    lane = torch.arange(64, device=dev)
    ql, il = lane >> 4, lane & 15
    qq, rr = torch.meshgrid(torch.arange(4, device=dev), torch.arange(4, device=dev), indexing="ij")
    return Lanes(lane, ql, il, 4 * (il & 3) + (il >> 2), il >> 2, il & 3, qq, rr)


def _gemm1_operands(H: int, W1, b1, units: int = 16, W1c=None):
    """GEMM 1 of a lean op, fp64: ``W1pad`` (units, columns) and ``b1pad`` (units,) zero-padded to the kernel's hidden units
    and multiplied by 2 log2(e) (tanh through exp2), and likewise the context's columns ``W1cp`` (units, 16) or None."""
    W1pad = torch.zeros(units, W1.shape[1], dtype=torch.float64, device=W1.device)
    W1pad[:H] = W1 * (2.0 * LOG2E)
    b1pad = torch.zeros(units, dtype=torch.float64, device=W1.device)
    b1pad[:H] = b1 * (2.0 * LOG2E)
    W1cp = None
    if W1c is not None:
        W1cp = torch.zeros(units, 16, dtype=torch.float64, device=W1.device)
        W1cp[:H, :W1c.shape[1]] = W1c * (2.0 * LOG2E)
    return W1pad, b1pad, W1cp


def _affine_scale(W, b) -> None:
    """In place, parameter 0 (the scale logit u) of ``W`` (element, parameter, ...) and ``b`` (element, parameter):
    alpha = exp(u / 2 + c0) + 1e-10 = exp2((u / 2 + c0) log2 e) + 1e-10."""
    W[:, 0] *= 0.5 * LOG2E
    b[:, 0] = (b[:, 0] * 0.5 + AFF_C0) * LOG2E


def _gemm2_operands(H: int, W2p, b2p, affine: bool):
    """GEMM 2 of a lean affine / shift op, fp64: ``W2pad`` (element, parameter, 16) zero-padded to 16 hidden units and a
    copy of ``b2p``, the scale-logit rows pre-scaled (``_affine_scale``) for ``affine``."""
    W2pad = torch.zeros(W2p.shape[0], W2p.shape[1], 16, dtype=torch.float64, device=W2p.device)
    W2pad[:, :, :H] = W2p
    b2q = b2p.clone()
    if affine:
        _affine_scale(W2pad, b2q)
    return W2pad, b2q


def _pack_mfma(kind: str, d: int, plane: int, H: int, D: int, W1t, b1, W2p, b2p):
    """Parameter block of one affine / shift coupling for tfk_flow_run_mfma
    (csrc/tfk_flow_mfma.hip): A1[EPL][HT][64] | b1[HT][4][4] | A2[T2][steps2][64] | b2[T2][4][4]
    (HT = 1, 2, 4 or 8 tiles of 16 hidden units; RQS: HT = 1).
    Lane l = (q = l >> 4, i = l & 15).  GEMM 1: D-row i <-> hidden unit 4*(i & 3) + (i >> 2),
    k-step s of lane-group q <-> physical source element EPL*q + s.  GEMM 2, tile t: D-row
    i = 4*q2 + r <-> parameter (r & 1) of target element EPL*q2 + 2t + (r >> 1) (affine) or
    target element EPL*q2 + 4t + r (shift); k-step r' of lane-group q <-> hidden unit 4r' + q."""
    half, EPL = D // 2, D // 8
    dev, dt = W1t.device, W1t.dtype
    P = W2p.shape[1]
    steps2 = (H + 3) // 4
    HT = 1 if steps2 <= 4 else (2 if steps2 <= 8 else (4 if steps2 <= 16 else 8))       # 16-unit tiles of the hidden layer
    W1pad = torch.zeros(16 * HT, half, dtype=dt, device=dev)
    W1pad[:H] = W1t
    b1pad = torch.zeros(16 * HT, dtype=dt, device=dev)
    b1pad[:H] = b1
    W2pad = torch.zeros(half, P, 16 * HT, dtype=dt, device=dev)
    W2pad[:, :, :H] = W2p
    L = _lanes(dev)
    ql, unit1, q2, r2, qq, rr = L.ql, L.unit1, L.q2, L.r2, L.qq, L.rr
    # A1[s][t][lane]: tile t holds hidden units 16t .. 16t+15 (D-row i <-> unit 16t + unit1(i))
    A1 = torch.stack([W1pad[16 * t + unit1, EPL * ql + s] for s in range(EPL) for t in range(HT)])
    b1m = torch.stack([b1pad[16 * t + 4 * rr + qq] for t in range(HT)])           # [t][q][r]
    if kind == "rqs":
        # 23 spline parameters per element padded to 24: tile 6e + c holds parameters 4c .. 4c+3
        # of target element EPL*q2 + e
        W2q = torch.zeros(half, 24, 16, dtype=dt, device=dev)
        W2q[:, :P] = W2pad
        b2q = torch.zeros(half, 24, dtype=dt, device=dev)
        b2q[:, :P] = b2p
        A2, b2m = [], []
        for e in range(EPL):
            for c in range(6):
                for r1 in range(steps2):
                    A2.append(W2q[EPL * q2 + e, 4 * c + r2, 4 * r1 + ql])
                b2m.append(b2q[EPL * qq + e, 4 * c + rr])
        block = torch.cat([A1.reshape(-1), b1m.reshape(-1), torch.stack(A2).reshape(-1),
                           torch.stack(b2m).reshape(-1)])
        return (OP_RQS_FWD if d == FORWARD else OP_RQS_INV, plane, steps2), block
    T2 = EPL // 2 if P == 2 else EPL // 4
    A2, b2m = [], []
    for t in range(T2):
        m_l, p_l, m_b, p_b = _tile_rows(L, EPL, P, t)
        for r1 in range(steps2):
            A2.append(W2pad[m_l, p_l, 4 * r1 + ql])                               # (64,)
        b2m.append(b2p[m_b, p_b])                                                  # (4, 4)
    block = torch.cat([A1.reshape(-1), b1m.reshape(-1), torch.stack(A2).reshape(-1),
                       torch.stack(b2m).reshape(-1)])
    if kind == "shift":
        op = OP_SHIFT_FWD if d == FORWARD else OP_SHIFT_INV
    else:
        op = OP_AFFINE_FWD if (d == FORWARD) != (kind == "inverse_affine") else OP_AFFINE_INV
    return (op, plane, steps2), block


def _f16_pieces(w: torch.Tensor):
    """fp64 -> (hi, lo) float16 with hi + lo ~ w, and whether every element passes the representability check of the
    split-f16 format: |w| <= 65 504 and hi + lo within 2^-22 relative or 2^-24 absolute of w."""
    ok = bool((w.abs() <= 65504.0).all())
    hi = w.clamp(-65504.0, 65504.0).to(torch.float16)
    lo = (w - hi.double()).to(torch.float16)
    err = (hi.double() + lo.double() - w).abs()
    ok = ok and bool(((err <= 2.0 ** -22 * w.abs()) | (err <= 2.0 ** -24)).all())
    return hi, lo, ok


def _bf16_pieces(w: torch.Tensor):
    """fp32 -> three bf16 pieces by truncation (hi = w & 0xffff0000, mid and lo likewise from the exact remainders),
    each returned as the int32 holding its 16 significant bits in the LOW half."""
    w = w.float().contiguous()
    mask = torch.tensor(-65536, dtype=torch.int32, device=w.device)             # 0xffff0000
    hi = (w.view(torch.int32) & mask).view(torch.float32)
    r1 = w - hi
    mid = (r1.view(torch.int32) & mask).view(torch.float32)
    r2 = (r1 - mid).contiguous()
    lo = (r2.view(torch.int32) & mask).view(torch.float32)
    return [(t.contiguous().view(torch.int32) >> 16) & 0xFFFF for t in (hi, mid, lo)]


def _tile_rows(L: Lanes, EPL: int, P: int, t: int):
    """GEMM-2 tile t of an affine (P = 2) / shift (P = 1) coupling: (target element, parameter) of the output row of every
    lane, (64,) each, and of every bias slot [q][r], (4, 4) each."""
    n = 4 // P                                   # target elements per lane group and tile
    return EPL * L.q2 + n * t + L.r2 // P, L.r2 % P, EPL * L.qq + n * t + L.rr // P, L.rr % P


def _context_operand(W1cp, L: Lanes, HT: int = 1) -> torch.Tensor:
    """The context's columns of W1 as further GEMM-1 k-steps: A1c[t][lane][k] = W1c[unit 16 t + unit1(i), context 4 k + q]."""
    kk = torch.arange(4, device=W1cp.device)
    return torch.stack([W1cp[(16 * t + L.unit1).view(64, 1), 4 * kk.view(1, 4) + L.ql.view(64, 1)]
                        for t in range(HT)]).reshape(-1)


def _pack_lean(lk: int, H: int, Dp: int, W1t, b1, W2p, b2p, pre_s, pre_t, bf16x3: bool = False, W1c=None,
               f16x2: bool = False) -> Optional[torch.Tensor]:
    """Parameter block of a lean coupling op (csrc/tfk_flow_chain.h): lane-major MFMA A-operands
    A1[EPL/4][64][4] | b1[4][4] | A2[nA2/4][64][4] | b2[T2][4][4] | pre_s[hp] | pre_t[hp], with W1 / b1 multiplied by
    2 log2(e) and (affine) the scale-logit rows of W2 / b2 by log2(e) / 2, b2 += c0 log2(e).  Inputs fp64, physical
    order, the pending elementwise maps of the source plane already folded into W1t / b1.
    ``f16x2``: the split-f16 format (H <= 10), or None if a weight of W2 is not representable in it."""
    EPL = Dp // 8
    L = _lanes(W1t.device)
    W1pad, b1pad, W1cp = _gemm1_operands(H, W1t, b1, W1c=W1c)
    W2pad, b2q = _gemm2_operands(H, W2p, b2p, affine=LEAN_KINDS[lk].family == "affine")
    if f16x2:
        assert H <= 10 and EPL >= 4 and W1c is None
        return _lean_block_f16x2(L, EPL, W1pad, b1pad, W2pad, b2q, pre_s, pre_t)
    A1 = torch.stack([W1pad[L.unit1, EPL * L.ql + s] for s in range(EPL)])             # (EPL, 64)
    VW = min(EPL, 4)                                                                   # (16-wide rows: A1[64][2])
    A1 = A1.reshape(EPL // VW, VW, 64).permute(0, 2, 1)                                # lane-major groups of 4 k-steps
    b1m = b1pad[4 * L.rr + L.qq]                                                       # [q][r]
    if bf16x3:
        return torch.cat([A1.reshape(-1).float(), b1m.reshape(-1).float(), _lean_gemm2_bf16x3(L, EPL, W2pad, b2q),
                          pre_s.float(), pre_t.float()])
    tail_ = [] if W1cp is None else [_context_operand(W1cp, L)]
    return torch.cat([A1.reshape(-1), b1m.reshape(-1)] + _lean_gemm2_fp32(L, EPL, (H + 3) // 4, W2pad, b2q)
                     + [pre_s, pre_t] + tail_).float()


def _lean_gemm2_fp32(L: Lanes, EPL: int, steps2: int, W2pad, b2q):
    """[A2[nA2/4][64][4], b2[T2][4][4]] in fp64: one k-step of 4 hidden units per fp32 MFMA."""
    hp, P = W2pad.shape[0], W2pad.shape[1]
    T2 = EPL // 2 if P == 2 else (EPL + 3) // 4
    A2, b2m = [], []
    for t in range(T2):
        ok_l = ok_b = None
        m_l, p_l, m_b, p_b = _tile_rows(L, EPL, P, t)
        if P != 2 and EPL < 4:                       # 16-wide rows: rows r >= EPL of every group belong to no element
            ok_l, ok_b = (L.r2 < EPL).to(torch.float64), (L.rr < EPL).to(torch.float64)
            m_l, m_b = m_l.clamp(max=hp - 1), m_b.clamp(max=hp - 1)
        for r1 in range(steps2):
            A2.append(W2pad[m_l, p_l, 4 * r1 + L.ql] if ok_l is None else W2pad[m_l, p_l, 4 * r1 + L.ql] * ok_l)
        b2m.append(b2q[m_b, p_b] if ok_b is None else b2q[m_b, p_b] * ok_b)
    nA2 = (T2 * steps2 + 3) & ~3
    A2 = torch.stack(A2 + [torch.zeros(64, dtype=torch.float64, device=W2pad.device)] * (nA2 - T2 * steps2))
    A2 = A2.reshape(nA2 // 4, 4, 64).permute(0, 2, 1)
    return [A2.reshape(-1), torch.stack(b2m).reshape(-1)]


def _lean_gemm2_bf16x3(L: Lanes, EPL: int, W2pad, b2q) -> torch.Tensor:
    """GEMM 2 in the bf16 x 3 operand format (csrc/tfk_flow_chain.h: couple_lean3): per tile and lane
    [W_hi | W_mid] and [W_lo | W_hi], 4 bf16 each (slot i <-> hidden unit 4 i + q); b2 = the weight of unit 15."""
    P = W2pad.shape[1]
    W2b = W2pad.clone()
    W2b[:, :, 15] = b2q
    Af = []
    for t in range(EPL // 2 if P == 2 else (EPL + 3) // 4):
        m_l, p_l, _, _ = _tile_rows(L, EPL, P, t)
        Af.append(torch.stack([W2b[m_l, p_l, 4 * i + L.ql] for i in range(4)], dim=1))         # (64, 4)
    hi, mid, lo = _bf16_pieces(torch.stack(Af))                                                # (T2, 64, 4)
    return _bf16x3_dwords(hi, mid, lo, dim=1).reshape(-1).view(torch.float32)                  # (T2, 2, 64, 4)


def _bf16x3_dwords(hi, mid, lo, dim: int) -> torch.Tensor:
    """The two A-operands [W_hi | W_mid] and [W_lo | W_hi] of the three bf16 pieces, two per dword, stacked along ``dim``."""
    pack2 = lambda v: (v[..., 0::2] | (v[..., 1::2] << 16))
    return torch.stack([torch.cat([pack2(hi), pack2(mid)], dim=-1),
                        torch.cat([pack2(lo), pack2(hi)], dim=-1)], dim=dim).to(torch.int32)


def _lean_block_f16x2(L: Lanes, EPL: int, W1pad, b1pad, W2pad, b2q, pre_s, pre_t) -> Optional[torch.Tensor]:
    """The split-f16 format (couple_lean_h): M-row 4 q + r of GEMM 1 = hidden unit 2 q + r (r < 2), 8 + (q >> 1) (r = 2: units
    8 and 9 are computed twice), none (r = 3) -- so that every lane group holds all pieces of "its" units."""
    dev, P = W1pad.device, W2pad.shape[1]
    lane, ql, q2, r2, qq, rr = L.lane, L.ql, L.q2, L.r2, L.qq, L.rr
    live = (r2 < 3).to(torch.float64)
    unit_h = torch.where(r2 < 2, 2 * q2 + r2, 8 + (q2 >> 1))                       # (64,): unit of M-row il
    A1 = torch.stack([W1pad[unit_h, EPL * ql + s] * live for s in range(EPL)])
    A1 = A1.reshape(EPL // 4, 4, 64).permute(0, 2, 1)
    b1m = b1pad[torch.where(rr < 2, 2 * qq + rr, 8 + (qq >> 1))] * (rr < 3).to(torch.float64)
    u0, u1, u2 = 2 * ql, 2 * ql + 1, 8 + (ql >> 1)
    first = (ql & 1) == 0                        # unit 8 / 9: (W_hi, W_hi) in the even group, (W_lo, 0) in the odd one
    A2h, b2m, ok = [], [], True
    for t in range(EPL // 2 if P == 2 else EPL // 4):
        m_l, p_l, m_b, p_b = _tile_rows(L, EPL, P, t)
        hi, lo, ok_t = _f16_pieces(W2pad[m_l, p_l])                                # (64, 16): the lane's row of W2
        ok = ok and ok_t
        g = lambda v, u: v[lane, u]
        zero = torch.zeros(64, dtype=torch.float16, device=dev)
        # against the lane's B-operand [hi0 lo0 hi0 hi1 | lo1 hi1 hi2 lo2]
        A2h.append(torch.stack([g(hi, u0), g(hi, u0), g(lo, u0), g(hi, u1), g(hi, u1), g(lo, u1),
                                torch.where(first, g(hi, u2), g(lo, u2)), torch.where(first, g(hi, u2), zero)], dim=1))
        b2m.append(b2q[m_b, p_b])
    if not ok:
        return None
    A2h = torch.stack(A2h).contiguous().view(torch.int32)                          # (T2, 64, 4 dwords)
    return torch.cat([A1.reshape(-1).float(), b1m.reshape(-1).float(), A2h.reshape(-1).view(torch.float32),
                      torch.stack(b2m).reshape(-1).float(), pre_s.float(), pre_t.float()])


def _pack_lean_rqs(H: int, Dp: int, W1t, b1, W2p, b2p, pre_s, pre_t, c_delta: float, bf16x3: bool = False,
                   lrs: bool = False, W1c=None) -> torch.Tensor:
    """Parameter block of a lean RQ-spline coupling op (csrc/tfk_flow_rqs_chain.h), fp64 in, fp32 out.
    fp32 operands (hidden width <= 16): head A1[EPL/4][64][4] | b1[4][4] | pre_s[hp] | pre_t[hp], then EPL/8 chunks
    A2[48][64][4] | b2[48][4][4].  bf16 x 3 operands (hidden width <= 15, or <= 31 with HT = 2 hidden tiles): head
    A1[EPL/4][HT][64][4] | b1[HT][4][4] | pre_s | pre_t, then EPL HT / 4 chunks A[4/HT][6][HT][2][64][4 dwords].
    Per target element 24 parameters, all times log2(e): [0, 8) u_x, [8, 16) u_x + u_y / 1000 (the reference's height
    logits, rational_quadratic.py:76), [16, 23) c + u_d / 1000 (:77, c = boundary_u_delta), pad.
    ``lrs`` (bf16 x 3 only): linear rational spline, 32 parameters = 8 tiles per element (linear_rational.py:49-58):
    [0, 8) u_x, [8, 16) u_x + u_y / 100, [16, 24) -u_lambda, [24, 31) c + u_d / 100, [31] u_w0, times log2(e)."""
    hp, EPL = Dp // 2, Dp // 8
    dev = W1t.device
    HT = 2 if (bf16x3 and H > 15) else 1
    HU = 16 * HT                                                   # hidden units the kernel sees
    W1pad, b1pad, W1cp = _gemm1_operands(H, W1t, b1, units=HU, W1c=W1c)
    TPE = 8 if lrs else 6                                          # tiles of 4 parameters per element
    Q = torch.zeros(hp, 4 * TPE, HU, dtype=torch.float64, device=dev)
    bq = torch.zeros(hp, 4 * TPE, dtype=torch.float64, device=dev)
    if lrs:
        assert bf16x3
        for dst, w in ((Q[:, :, :H], W2p), (bq, b2p)):
            dst[:, 0:8] = w[:, 0:8] * LOG2E
            dst[:, 8:16] = (w[:, 0:8] + w[:, 8:16] / 100.0) * LOG2E
            dst[:, 16:24] = -w[:, 16:24] * LOG2E
            dst[:, 24:31] = w[:, 24:31] / 100.0 * LOG2E
            dst[:, 31] = w[:, 31] * LOG2E
        bq[:, 24:31] += c_delta * LOG2E
    else:
        Q[:, 0:8, :H] = W2p[:, 0:8] * LOG2E
        Q[:, 8:16, :H] = (W2p[:, 0:8] + W2p[:, 8:16] / 1000.0) * LOG2E
        Q[:, 16:23, :H] = W2p[:, 16:23] / 1000.0 * LOG2E
        bq[:, 0:8] = b2p[:, 0:8] * LOG2E
        bq[:, 8:16] = (b2p[:, 0:8] + b2p[:, 8:16] / 1000.0) * LOG2E
        bq[:, 16:23] = (c_delta + b2p[:, 16:23] / 1000.0) * LOG2E
    L = _lanes(dev)
    ql, unit1, q2, r2, qq, rr = L.ql, L.unit1, L.q2, L.r2, L.qq, L.rr
    # A1[g][t][lane][k]: source k-step 4 g + k, hidden tile t, D-row i <-> unit 16 t + unit1(i)
    A1 = torch.stack([torch.stack([W1pad[16 * t + unit1, EPL * ql + s_] for t in range(HT)]) for s_ in range(EPL)])
    A1 = A1.reshape(EPL // 4, 4, HT, 64).permute(0, 2, 3, 1)                          # (EPL/4, HT, 64, 4)
    b1m = torch.stack([b1pad[16 * t + 4 * rr + qq] for t in range(HT)])                # [t][q][r]
    parts = [A1.reshape(-1), b1m.reshape(-1), pre_s, pre_t]
    if W1cp is not None:
        assert bf16x3
        parts.append(_context_operand(W1cp, L, HT))
    e_all = torch.arange(EPL, device=dev).view(EPL, 1, 1, 1, 1)                        # the lane-group's element index
    c = torch.arange(TPE, device=dev).view(1, TPE, 1, 1, 1)
    m = EPL * q2.view(1, 1, 1, 64, 1) + e_all                                          # physical target element
    if bf16x3:
        Q[:, :, HU - 1] = bq                                   # the bias as the weight of the last hidden unit (= 1)
        th = torch.arange(HT, device=dev).view(1, 1, HT, 1, 1)
        i4 = torch.arange(4, device=dev).view(1, 1, 1, 1, 4)
        Wf = Q[m, 4 * c + r2.view(1, 1, 1, 64, 1), 16 * th + 4 * i4 + ql.view(1, 1, 1, 64, 1)]   # (EPL, TPE, HT, 64, 4)
        A3 = _bf16x3_dwords(*_bf16_pieces(Wf), dim=3)                                  # (EPL, TPE, HT, 2, 64, 4)
        return torch.cat([torch.cat(parts).float(), A3.reshape(-1).view(torch.float32)])
    r1 = torch.arange(4, device=dev).view(1, 1, 1, 1, 4)
    A2 = Q[m, 4 * c + r2.view(1, 1, 1, 64, 1), 4 * r1 + ql.view(1, 1, 1, 64, 1)][:, :, 0]   # (EPL, 6, 64, 4)
    mb = EPL * qq.view(1, 1, 4, 4) + torch.arange(EPL, device=dev).view(EPL, 1, 1, 1)
    b2 = bq[mb, 4 * torch.arange(6, device=dev).view(1, 6, 1, 1) + rr.view(1, 1, 4, 4)]       # (EPL, 6, 4, 4)
    for k in range(EPL // 8):
        parts += [A2[8 * k:8 * k + 8].reshape(-1), b2[8 * k:8 * k + 8].reshape(-1)]
    return torch.cat(parts).float()


def _pack_lean_made_spline(H: int, Dp: int, W1f, b1f, W2p, b2p, pre_s, pre_t, c_delta: float, lrs: bool) -> torch.Tensor:
    """Parameter block of a lean MADE spline op (csrc/tfk_flow_rqs_chain.h: rqs_made_layer3), bf16 x 3 operands, hidden
    width <= 15: head A1[2 EPL / 4][64][4] (plane A's k-steps, then plane B's) | b1[4][4] | pre_s[Dp] | pre_t[Dp], then the
    chunks of plane A's elements and of plane B's, each exactly as a lean spline coupling's (``_pack_lean_rqs``)."""
    hp, EPL = Dp // 2, Dp // 8
    dev = W1f.device
    head_len = EPL * 64 + 16 + 2 * hp                    # a coupling block's head (dropped below)
    zero_w1 = torch.zeros(H, hp, dtype=torch.float64, device=dev)
    chunks = []
    for plane in (0, 1):
        sl = slice(plane * hp, (plane + 1) * hp)
        blk = _pack_lean_rqs(H, Dp, zero_w1, b1f, W2p[sl], b2p[sl], pre_s[sl], pre_t[sl], c_delta, bf16x3=True, lrs=lrs)
        chunks.append(blk[head_len:])
    head = torch.cat(_made_gemm1(_lanes(dev), H, Dp, W1f, b1f) + [pre_s, pre_t]).float()
    return torch.cat([head] + chunks)


def _made_gemm1(L: Lanes, H: int, Dp: int, W1f, b1f):
    """[A1[2 EPL / 4][64][4], b1[4][4]] of a lean MADE op, fp64: GEMM 1 reads the whole row, plane A's k-steps first."""
    hp, EPL = Dp // 2, Dp // 8
    W1pad, b1pad, _ = _gemm1_operands(H, W1f, b1f)
    A1 = torch.stack([W1pad[L.unit1, plane * hp + EPL * L.ql + s_] for plane in range(2) for s_ in range(EPL)])
    A1 = A1.reshape(2 * EPL // 4, 4, 64).permute(0, 2, 1)
    return [A1.reshape(-1), b1pad[4 * L.rr + L.qq].reshape(-1)]


def _pack_lean_made(H: int, Dp: int, W1f, b1f, W2p, b2p, pre_s, pre_t) -> torch.Tensor:
    """Parameter block of a lean MADE op (csrc/tfk_flow_chain.h: made_lean): A1[2 EPL / 4][64][4] (plane A's k-steps,
    then plane B's) | b1[4][4] | A2[nA2 / 4][64][4] | b2[EPL][4][4] | pre_s[Dp] | pre_t[Dp], weights pre-scaled as
    for the lean couplings.  Inputs fp64, physical order, pending elementwise maps already folded into W1f / b1f."""
    hp, EPL = Dp // 2, Dp // 8
    dev = W1f.device
    steps2 = (H + 3) // 4
    W2pad, b2q = _gemm2_operands(H, W2p, b2p, affine=True)
    L = _lanes(dev)
    ql, q2, r2, qq, rr = L.ql, L.q2, L.r2, L.qq, L.rr
    A2, b2m = [], []
    for t in range(EPL):
        plane, tt = (0, t) if t < EPL // 2 else (1, t - EPL // 2)
        for r1 in range(steps2):
            A2.append(W2pad[plane * hp + EPL * q2 + 2 * tt + (r2 >> 1), r2 & 1, 4 * r1 + ql])
        b2m.append(b2q[plane * hp + EPL * qq + 2 * tt + (rr >> 1), rr & 1])
    nA2 = (EPL * steps2 + 3) & ~3
    A2 = torch.stack(A2 + [torch.zeros(64, dtype=torch.float64, device=dev)] * (nA2 - EPL * steps2))
    A2 = A2.reshape(nA2 // 4, 4, 64).permute(0, 2, 1)
    return torch.cat(_made_gemm1(L, H, Dp, W1f, b1f) + [A2.reshape(-1), torch.stack(b2m).reshape(-1), pre_s, pre_t]).float()
