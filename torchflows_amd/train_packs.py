"""Index maps between a coupling layer's weights and the operand / accumulator layouts of the fused training launches
(csrc/tfk_bwd.hip, csrc/tfk_wide_bwd.h, include/tfk.h), built once per geometry and device, and the padded training layout of
the rows.  The user is ``torchflows_amd/autograd.py``."""
from __future__ import annotations

from typing import List, Optional

import torch

from torchflows_amd import native


def training_layout(D: int, W: int, device) -> torch.Tensor:
    """Physical column of logical element l on rows padded from D to W: l for the first D // 2 (the sources of a
    HalfSplit coupling), W - D + l for the others (its targets) -- for even D reversing the D logical columns is then
    reversing the W physical ones; for odd D it is not (the middle element is a target before AND after a reversal, so
    it has to change planes): those plans run their reversals as the general column gather ``reversal_index``."""
    key = (D, W, str(device))
    hit = _LAYOUTS.get(key)
    if hit is None:
        l = torch.arange(D, device=device)
        hit = _LAYOUTS[key] = torch.where(l < D // 2, l, l + (W - D))
    return hit


_LAYOUTS = {}


def reversal_index(D: int, W: int, device) -> torch.Tensor:
    """int32 (W,): out[:, c] = in[:, index[c]] reverses the D logical columns of rows in the padded training layout and
    leaves the padding where it is (an involution: the backward pass uses the same index)."""
    key = (D, W, str(device), "rev")
    hit = _LAYOUTS.get(key)
    if hit is None:
        phys = training_layout(D, W, "cpu")
        idx = torch.arange(W)
        idx[phys] = phys.flip(0)                     # the column of logical j takes the column of logical D - 1 - j
        hit = _LAYOUTS[key] = idx.to(torch.int32).to(device)
    return hit


class _TrainPack:
    """Index maps between a coupling layer's (W1, b1, W2, b2) and the operand / accumulator layouts
    of tfk_affine_coupling_train_bwd (csrc/tfk_bwd.hip), built once per (D, H, device).
    Lane l = (q = l >> 4, i = l & 15); hidden unit of D-row i: u(i) = 4 (i & 3) + (i >> 2)."""

    _cache = {}

    @classmethod
    def get(cls, D: int, H: int, device, D_log: Optional[int] = None, shift: bool = False) -> "_TrainPack":
        key = (D, H, str(device), D_log or D, shift)
        if key not in cls._cache:
            cls._cache[key] = cls(D, H, device, D_log or D, shift)
        return cls._cache[key]

    def __init__(self, D: int, H: int, device, D_log: Optional[int] = None, shift: bool = False):
        """``D``: the row width the kernels see; ``D_log`` <= D: the layer's event size when its rows are padded
        (training_layout: the source half at the head of plane A, the target half at the TAIL of plane B, zeros between) --
        the weights of the padding are the appended zero, its accumulators are not mapped back.
        ``shift``: a Shift coupling (NICE, affine.py:137-159) run as the affine coupling it is with a scale logit of
        zero -- alpha = exp(0 / 2 + c0) + 1e-10 = 1 exactly, log alpha = 0: the conditioner's one output per element is the
        shift row of GEMM 2, the logit rows are the appended zero, and their accumulators are not mapped back."""
        D_log = D_log or D
        half, EPL = D // 2, D // 8
        h = D_log // 2                                    # sources (HalfSplit: the first D // 2 elements, coupling_masks)
        ht = D_log - h                                    # targets: one more when the event size is odd
        pad = half - ht                                   # plane B: padding first, then the targets
        T2, T1 = EPL // 2, EPL // 4
        self.steps2 = (H + 3) // 4
        TP = ht if shift else 2 * ht                      # rows of the real W2 / b2
        off_b1 = H * h
        off_W2 = off_b1 + H
        off_b2 = off_W2 + TP * H
        Z = off_b2 + TP                                   # index of the appended zero
        ar = torch.arange
        W1idx = torch.full((16, half), Z, dtype=torch.long)
        W1idx[:H, :h] = (ar(H)[:, None] * h + ar(h)[None, :])
        b1idx = torch.full((16,), Z, dtype=torch.long)
        b1idx[:H] = off_b1 + ar(H)
        W2idx = torch.full((half, 2, 16), Z, dtype=torch.long)
        b2idx = torch.full((half, 2), Z, dtype=torch.long)
        if shift:
            W2idx[pad:, 1, :H] = off_W2 + (ar(ht)[:, None] * H + ar(H)[None, :])
            b2idx[pad:, 1] = off_b2 + ar(ht)
        else:
            W2idx[pad:, :, :H] = off_W2 + ((ar(ht)[:, None, None] * 2 + ar(2)[None, :, None]) * H + ar(H)[None, None, :])
            b2idx[pad:] = off_b2 + (ar(ht)[:, None] * 2 + ar(2)[None, :])
        lane = ar(64)
        ql, il = lane >> 4, lane & 15
        unit = 4 * (il & 3) + (il >> 2)
        q2, r2 = il >> 2, il & 3
        qq, rr = torch.meshgrid(ar(4), ar(4), indexing="ij")
        parts = [torch.stack([W1idx[unit, EPL * ql + s] for s in range(EPL)]).reshape(-1),        # A1
                 b1idx[4 * rr + qq].reshape(-1)]                                                  # b1[q][r]
        A2, b2m, A2T, A1T = [], [], [], []
        for t in range(T2):
            for r1 in range(self.steps2):
                A2.append(W2idx[EPL * q2 + 2 * t + (r2 >> 1), r2 & 1, 4 * r1 + ql])
            b2m.append(b2idx[EPL * qq + 2 * t + (rr >> 1), rr & 1].reshape(-1))
            for r in range(4):
                A2T.append(W2idx[EPL * ql + 2 * t + (r >> 1), r & 1, unit])
        for t in range(T1):
            for r in range(4):
                A1T.append(W1idx[4 * r + ql, EPL * (il >> 2) + 4 * t + (il & 3)])
        parts += [torch.stack(A2).reshape(-1), torch.stack(b2m).reshape(-1),
                  torch.stack(A2T).reshape(-1), torch.stack(A1T).reshape(-1)]
        self.param_index = torch.cat(parts).to(device)
        self.n_flat = Z + 1
        # accumulator layout -> [dW1 (H, half) | db1 (H) | dW2 (TP, H) | db2 (TP)]
        u = ar(H)
        e = ar(h)                                         # (physical = logical source element)
        off1 = T2 * 256
        dW1 = off1 + (((e // 16)[None, :] * 64 + 16 * ((e % 16) // 4)[None, :] + u[:, None]) * 4 + (e % 4)[None, :])
        db1 = off1 + T1 * 256 + 4 * (u % 4) + (u // 4)
        if shift:
            m, pbit = pad + ar(ht), torch.ones(ht, dtype=torch.long)  # (the shift rows only)
        else:
            m = (pad + ar(ht))[:, None].expand(ht, 2).reshape(-1)    # physical target element of logical target t
            pbit = ar(2)[None, :].expand(ht, 2).reshape(-1)
        q_m, rem = m // EPL, m % EPL
        T_m, r_m = rem // 2, 2 * (rem % 2) + pbit
        dW2 = ((T_m * 64 + 16 * q_m)[:, None] + u[None, :]) * 4 + r_m[:, None]
        db2 = (T_m * 64 + 16 * q_m + 15) * 4 + r_m
        self.grad_index = torch.cat([dW1.reshape(-1), db1, dW2.reshape(-1), db2]).to(device)
        self.sizes = (H * h, H, TP * H, TP)
        self.shapes = ((H, h), (H,), (TP, H), (TP,))
        self.zero = torch.zeros(1, dtype=torch.float32, device=device)
        n_out = int(native.lib().tfk_coupling_train_bwd_out_floats(D))
        self.n_out = n_out
        self.workspace = torch.empty(int(native.lib().tfk_coupling_train_bwd_workspace_bytes(D)) // 4,
                                     dtype=torch.float32, device=device)


class _RqsTrainPack:
    """Index maps for tfk_rqs_coupling_train_bwd (D = 64, 8 bins, hidden width H <= 16): operand
    block from (W1, b1, W2, b2), and the un-permutations of its accumulator-order outputs."""

    _cache = {}

    @classmethod
    def get(cls, H: int, device, D_log: int = 64) -> "_RqsTrainPack":
        key = (H, str(device), D_log)
        if key not in cls._cache:
            cls._cache[key] = cls(H, device, D_log)
        return cls._cache[key]

    def __init__(self, H: int, device, D_log: int = 64):
        """``D_log`` < 64: the layer's event size on rows in the padded training layout (its h = D_log / 2 sources at the
        head of plane A, its h targets at the tail of plane B); a padding element's 23 spline parameters are the appended
        zero -- equal bins, unit derivatives: the identity at its value 0 (a knot)."""
        half, EPL, P = 32, 8, 23
        h = D_log // 2                                    # sources
        ht = D_log - h                                    # targets (one more when the event size is odd)
        pad = half - ht
        self.H = H
        self.steps2 = (H + 3) // 4
        off_b1 = H * h
        off_W2 = off_b1 + H
        off_b2 = off_W2 + ht * P * H
        Z = off_b2 + ht * P
        ar = torch.arange
        W1idx = torch.full((16, half), Z, dtype=torch.long)
        W1idx[:H, :h] = ar(H)[:, None] * h + ar(h)[None, :]
        b1idx = torch.full((16,), Z, dtype=torch.long)
        b1idx[:H] = off_b1 + ar(H)
        W2idx = torch.full((half, 24, 16), Z, dtype=torch.long)
        W2idx[pad:, :P, :H] = off_W2 + ((ar(ht)[:, None, None] * P + ar(P)[None, :, None]) * H + ar(H)[None, None, :])
        b2idx = torch.full((half, 24), Z, dtype=torch.long)
        b2idx[pad:, :P] = off_b2 + ar(ht)[:, None] * P + ar(P)[None, :]
        lane = ar(64)
        ql, il = lane >> 4, lane & 15
        unit = 4 * (il & 3) + (il >> 2)
        q2, r2 = il >> 2, il & 3
        qq, rr = torch.meshgrid(ar(4), ar(4), indexing="ij")
        A1 = torch.stack([W1idx[unit, EPL * ql + s] for s in range(EPL)])
        b1m = b1idx[4 * rr + qq]
        A2, b2m, A2T = [], [], []
        for e in range(EPL):
            for c in range(6):
                for r1 in range(self.steps2):
                    A2.append(W2idx[EPL * q2 + e, 4 * c + r2, 4 * r1 + ql])
                b2m.append(b2idx[EPL * qq + e, 4 * c + rr].reshape(-1))
                for r in range(4):
                    A2T.append(W2idx[EPL * ql + e, 4 * c + r, unit])
        A1T = [W1idx[4 * r + ql, EPL * (il >> 2) + 4 * t + (il & 3)] for t in range(2) for r in range(4)]
        self.param_index = torch.cat([A1.reshape(-1), b1m.reshape(-1), torch.stack(A2).reshape(-1),
                                      torch.stack(b2m).reshape(-1), torch.stack(A2T).reshape(-1),
                                      torch.stack(A1T).reshape(-1)]).to(device)
        self.n_fwd = EPL * 64 + 16 + 48 * self.steps2 * 64 + 48 * 16
        # column of gh_perm that holds parameter p of (physical) target element m = pad + logical target
        m = (pad + ar(ht))[:, None]
        pp = ar(P)[None, :]
        e_, q_ = m % EPL, m // EPL
        self.gh_col = ((6 * e_ + pp // 4) * 16 + 4 * q_ + pp % 4).reshape(-1).to(device)     # (736,)
        u = ar(H)
        self.gpre_col = (4 * (u % 4) + u // 4).to(device)                                   # (H,)
        self.zero = torch.zeros(1, dtype=torch.float32, device=device)
        # tfk_rows_outer route (hidden width <= 15): three products in accumulator order, one buffer
        #   [gh_perm^T hid_perm (768 x 16) | x_A^T gpre_perm (32 x 16) | gpre_perm^T hid_perm (16 x 16)]
        # and ONE gather to [dW1 (H, 32) | db1 (H) | dW2 (736, H) | db2 (736)]
        self.n_acc = 768 * 16 + 32 * 16 + 16 * 16
        if H <= 15:
            slot = 4 * (u % 4) + u // 4                                   # column of hid_perm / gpre_perm that holds unit u
            c = ((6 * e_ + pp // 4) * 16 + 4 * q_ + pp % 4).reshape(-1)  # gh_perm column of (target m, parameter p)
            t1 = 4 * (c // 64) + (c % 64) % 4                             # its tile and M-index (include/tfk.h)
            i1 = (c % 64) // 4
            idx1 = lambda j: ((t1 * 64 + 16 * (i1 // 4))[:, None] + j[None, :]) * 4 + (i1 % 4)[:, None]
            dW2 = idx1(slot)                                              # (736, H)
            db2 = idx1(torch.tensor([15]))[:, 0]
            e = ar(h)
            base2 = 768 * 16
            dW1 = base2 + (((e // 16) * 64 + 16 * ((e % 16) // 4))[None, :] + slot[:, None]) * 4 + ((e % 16) % 4)[None, :]
            base3 = base2 + 32 * 16
            db1 = base3 + (16 * (slot // 4) + 15) * 4 + slot % 4
            self.acc_index = torch.cat([dW1.reshape(-1), db1, dW2.reshape(-1), db2]).to(device)
            self.acc_sizes = (H * h, H, ht * P * H, ht * P)
            self.acc_shapes = ((H, h), (H,), (ht * P, H), (ht * P,))

    def pack(self, lin1, lin2) -> torch.Tensor:
        flat = torch.cat([lin1.weight.detach().reshape(-1), lin1.bias.detach(),
                          lin2.weight.detach().reshape(-1), lin2.bias.detach(), self.zero])
        return flat[self.param_index]


class _WideTrainPack:
    """Index maps between a coupling layer's [W1 | b1 | W2 | b2 | 0] and the layouts of the wide training launches (event
    sizes 256 < D <= 1024, D % 8 == 0), built once per (D, H, device, shift):

    (a) ``fwd_index`` / ``fwd_mul`` / ``fwd_add``: the operand block ``tfk_flow_run_wide`` reads for a one-coupling program
        (csrc/tfk_flow_wide.h; ``fused_wide.pack_coupling`` with pre_s = 1, pre_t = 0) as ONE gather and ONE multiply-add in
        float64 -- the lean pre-scaling (W1 / b1 times 2 log2 e, the logit rows times log2(e) / 2, + c0 log2 e) --, so the
        block is bit for bit the inference packer's;
    (b) behind it, in the module's own scale, the transposed operands A2T | A1T of ``tfk_wide_coupling_train_bwd``
        (csrc/tfk_wide_bwd.h): ``param_index`` = (a) + (b), ``n_bwd`` floats -- the head of a layer's packed block; the
        closing TFK_OP_EW_FMA block (4 hp + 4 floats) follows at offset ``n_bwd``;
    (c) ``acc_index``: from the three ``tfk_rows_outer`` outputs [gh_rec^T hid_rec (GH x 16) | x^T gpre_rec (hp x 16) |
        gpre_rec^T hid_rec (16 x 16)], accumulator order (include/tfk.h), to [dW1 (H, D/2) | db1 (H) | dW2 (TP, H) | db2 (TP)].
    Pad columns (D / 2 <= c < hp) and hidden units >= H read the appended zero; their accumulators are never mapped back.
    The record buffers and the accumulator block live here: nothing is allocated per step."""

    _cache = {}

    @classmethod
    def get(cls, D: int, H: int, device, shift: bool = False) -> "_WideTrainPack":
        key = (D, H, str(device), shift)
        if key not in cls._cache:
            cls._cache[key] = cls(D, H, device, shift)
        return cls._cache[key]

    def __init__(self, D: int, H: int, device, shift: bool = False):
        from torchflows_amd import flow_ops
        half = D // 2
        hp = (half + 63) // 64 * 64
        E = hp // 16
        P = 1 if shift else 2
        T2, G1 = (E // 4 if shift else E // 2), E // 4
        TP = P * half
        self.D, self.H, self.hp, self.E, self.shift, self.device = D, H, hp, E, shift, device
        off_b1 = H * half
        off_W2 = off_b1 + H
        off_b2 = off_W2 + TP * H
        Z = off_b2 + TP                                   # index of the appended zero
        self.n_flat = Z + 1
        ar = torch.arange
        W1idx = torch.full((16, hp), Z, dtype=torch.long)
        W1idx[:H, :half] = ar(H)[:, None] * half + ar(half)[None, :]
        b1idx = torch.full((16,), Z, dtype=torch.long)
        b1idx[:H] = off_b1 + ar(H)
        W2idx = torch.full((hp, P, 16), Z, dtype=torch.long)
        W2idx[:half, :, :H] = off_W2 + ((ar(half)[:, None, None] * P + ar(P)[None, :, None]) * H + ar(H)[None, None, :])
        b2idx = torch.full((hp, P), Z, dtype=torch.long)
        b2idx[:half] = off_b2 + ar(half)[:, None] * P + ar(P)[None, :]
        lane = ar(64)
        ql, il = lane >> 4, lane & 15
        unit1 = 4 * (il & 3) + (il >> 2)
        q2, r2 = il >> 2, il & 3
        w_, k_ = ar(4), ar(4)
        qq, rr = torch.meshgrid(ar(4), ar(4), indexing="ij")
        g_ = ar(G1)
        t_ = ar(T2)
        # A1[w][g][l][k]: hidden unit unit1(i), source column (4 w + q) E + 4 g + k
        cols = (4 * w_.view(4, 1, 1, 1) + ql.view(1, 1, 64, 1)) * E + 4 * g_.view(1, -1, 1, 1) + k_.view(1, 1, 1, 4)
        A1 = W1idx[unit1.view(1, 1, 64, 1).expand_as(cols), cols]
        b1m = b1idx[4 * rr + qq]                          # [q][r]
        # output row i = 4 q2 + r of GEMM-2 tile t of wave w: (target column, parameter)
        if shift:
            col_of = lambda qv, rv: (4 * w_.view(4, 1, 1, 1) + qv) * E + 4 * t_.view(1, -1, 1, 1) + rv
            par_of = lambda rv: torch.zeros_like(rv)
        else:
            col_of = lambda qv, rv: (4 * w_.view(4, 1, 1, 1) + qv) * E + 2 * t_.view(1, -1, 1, 1) + (rv >> 1)
            par_of = lambda rv: rv & 1
        shape = (4, T2, 64, 4)
        # A2[w][t][l][k]: hidden unit 4 k + (l >> 4) for output row i = l & 15
        m_l = col_of(q2.view(1, 1, 64, 1), r2.view(1, 1, 64, 1)).expand(shape)
        p_l = par_of(r2).view(1, 1, 64, 1).expand(shape)
        A2 = W2idx[m_l, p_l, (4 * k_.view(1, 1, 1, 4) + ql.view(1, 1, 64, 1)).expand(shape)]
        m_b = col_of(qq.view(1, 1, 4, 4), rr.view(1, 1, 4, 4)).expand(4, T2, 4, 4)
        p_b = par_of(rr).view(1, 1, 4, 4).expand(4, T2, 4, 4)
        b2m = b2idx[m_b, p_b]                             # [w][t][q][r]
        # A2T[w][t][l][r]: hidden unit unit1(i) in output row r of tile t for lane group l >> 4
        m_t = col_of(ql.view(1, 1, 64, 1), k_.view(1, 1, 1, 4)).expand(shape)
        p_t = par_of(k_).view(1, 1, 1, 4).expand(shape)
        A2T = W2idx[m_t, p_t, unit1.view(1, 1, 64, 1).expand(shape)]
        # A1T[w][g][l][r]: hidden unit 4 r + (l >> 4) for source column (4 w + (i >> 2)) E + 4 g + (i & 3)
        cols_t = ((4 * w_.view(4, 1, 1, 1) + (il >> 2).view(1, 1, 64, 1)) * E + 4 * g_.view(1, -1, 1, 1)
                  + (il & 3).view(1, 1, 64, 1)).expand(4, G1, 64, 4)
        A1T = W1idx[(4 * k_.view(1, 1, 1, 4) + ql.view(1, 1, 64, 1)).expand(4, G1, 64, 4), cols_t]
        pre = torch.full((2 * hp,), Z, dtype=torch.long)
        index = torch.cat([A1.reshape(-1), b1m.reshape(-1), A2.reshape(-1), b2m.reshape(-1), pre,
                           A2T.reshape(-1), A1T.reshape(-1)])
        # the pre-scaling of the forward block (fused_wide.pack_coupling), float64
        mul = torch.ones(index.numel(), dtype=torch.float64)
        add = torch.zeros(index.numel(), dtype=torch.float64)
        n_A1, n_A2, n_b2 = A1.numel(), A2.numel(), b2m.numel()
        mul[:n_A1 + 16] = 2.0 * flow_ops.LOG2E
        if not shift:
            lo = n_A1 + 16
            logit_l = (p_l == 0).reshape(-1)
            mul[lo:lo + n_A2][logit_l] = 0.5 * flow_ops.LOG2E
            lo += n_A2
            logit_b = (p_b == 0).reshape(-1)
            mul[lo:lo + n_b2][logit_b] = 0.5 * flow_ops.LOG2E
            add[lo:lo + n_b2][logit_b] = flow_ops.AFF_C0 * flow_ops.LOG2E
        lo = n_A1 + 16 + n_A2 + n_b2
        add[lo:lo + hp] = 1.0                             # pre_s = 1 (pre_t = 0)
        self.n_fwd = lo + 2 * hp
        self.n_bwd = int(index.numel())
        assert self.n_bwd == int(native.lib().tfk_wide_coupling_train_bwd_param_floats(D, 1 if shift else 0))
        self.param_index = index.to(device)
        self.param_mul, self.param_add = mul.to(device), add.to(device)
        self.zero = torch.zeros(1, dtype=torch.float32, device=device)
        # the closing TFK_OP_EW_FMA block of a coupling nothing rides along with: s = 1, t = 0, no constant log-det
        self.ew_identity = torch.cat([torch.ones(2 * hp), torch.zeros(2 * hp + 4)]).to(device)
        self.n_ew = 4 * hp + 4
        # one-coupling programs per lean kind (0 affine, 1 dividing affine, 2 shift forward, 3 shift inverse)
        self.ops = {lk: ((flow_ops.LEAN_KINDS[lk].op, 0, H, 0), (flow_ops.OP_EW_FMA, 0, 0, self.n_bwd)) for lk in range(4)}
        # (c) accumulator order of tfk_rows_outer for M >= 64: column m of A, column j of B
        self.GH = GH = P * hp
        u = ar(H)
        slot = 4 * (u % 4) + u // 4                       # column of hid_rec / gpre_rec that holds unit u

        def acc(m, j):                                    # (len(m), len(j)) positions of out[m][j]
            t = 4 * (m // 64) + m % 4
            i = (m % 64) // 4
            return ((t * 64 + 16 * (i // 4))[:, None] + j[None, :]) * 4 + (i % 4)[:, None]
        m2 = (ar(half)[:, None] * P + ar(P)[None, :]).reshape(-1)          # gh_rec column of (target c, parameter p)
        dW2 = acc(m2, slot)                                                 # (TP, H)
        db2 = acc(m2, torch.tensor([15]))[:, 0]
        base2 = GH * 16
        dW1 = base2 + acc(ar(half), slot).t()                               # (H, half)
        base3 = base2 + hp * 16
        db1 = base3 + (16 * (slot // 4) + 15) * 4 + slot % 4
        self.acc_index = torch.cat([dW1.reshape(-1), db1, dW2.reshape(-1), db2]).to(device)
        self.acc_sizes = (H * half, H, TP * H, TP)
        self.acc_shapes = ((H, half), (H,), (TP, H), (TP,))
        self.n_acc = base3 + 256
        self.acc_out = torch.empty(self.n_acc, dtype=torch.float32, device=device)
        self._rec = None
        self._retired = []                                # (a captured step keeps the addresses of the buffers it saw)

    def flat_of(self, lin1, lin2) -> List[torch.Tensor]:
        return [lin1.weight.detach().reshape(-1), lin1.bias.detach(), lin2.weight.detach().reshape(-1),
                lin2.bias.detach(), self.zero]

    def pack(self, lin1, lin2) -> torch.Tensor:
        """The ``n_bwd`` floats of (a) + (b) for the current weights (one layer; _PlanPacks packs a plan's at once)."""
        flat = torch.cat(self.flat_of(lin1, lin2)).double()
        return torch.addcmul(self.param_add, flat.index_select(0, self.param_index), self.param_mul).float()

    def records(self, N: int):
        """(gh_rec, gpre_rec, hid_rec) with N rows: views of buffers that only ever grow, and are never freed."""
        if self._rec is None or self._rec[0] < N:
            if self._rec is not None:
                self._retired.append(self._rec)
            cap = max(N, 2 * self._rec[0] if self._rec is not None else N)
            mk = lambda w: torch.empty(cap, w, dtype=torch.float32, device=self.device)
            self._rec = (cap, mk(self.GH), mk(16), mk(16))
        _, gh, gpre, hid = self._rec
        return gh[:N], gpre[:N], hid[:N]

    def unpack_grads(self, acc: torch.Tensor):
        """(dW1, db1, dW2, db2) from the three products' outputs."""
        return tuple(t.view(shp) for t, shp in zip(acc.index_select(0, self.acc_index).split(self.acc_sizes),
                                                   self.acc_shapes))
