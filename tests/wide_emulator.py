"""fp64 emulator of the wide-row chain kernel (csrc/tfk_flow_wide.h) for host-side tests: decodes the packed parameter
blocks exactly as the kernel reads them -- planes padded to a multiple of 64 columns, per-wave column ownership, split-K
partials of GEMM 1 added in wave order, lane-major MFMA A-operands, pre-affine, closing fma, base-2 log-det -- so that the
packer in torchflows_amd/fused_wide.py can be checked without a GPU."""
import math

import torch

from lean_emulator import _mfma

LN2 = math.log(2.0)
WAVES = 4


def run_wide(ops, params, rows, D, reverse_out=False):
    """rows (N, D) fp64 at the logical width -> (rows out (N, D), logdet (N,)) of one wide segment, as
    tfk_flow_run_wide stores them (each plane's logical columns; reversed with ``reverse_out``)."""
    N = rows.shape[0]
    half = D // 2
    hp = (half + 63) // 64 * 64
    E = hp // 16
    T = (N + 15) // 16
    x = torch.zeros(T * 16, 2 * hp, dtype=torch.float64)        # rows past the end and pad columns: zeros
    x[:N, :half] = rows[:, :half]
    x[:N, hp:hp + half] = rows[:, half:]
    x = x.reshape(T, 16, 2 * hp)
    lane = torch.arange(64)
    q, j = lane >> 4, lane & 15
    # lane registers of wave w: a[w][l, e, tile] = row j, column (4 w + q) E + e of plane A
    col = lambda w: ((4 * w + q) * E)[:, None] + torch.arange(E)[None, :]                   # (64, E)
    a = [x[:, j][:, lane[:, None], col(w)].permute(1, 2, 0).clone() for w in range(WAVES)]
    b = [x[:, j][:, lane[:, None], hp + col(w)].permute(1, 2, 0).clone() for w in range(WAVES)]
    prm = params.double()
    ld2 = [torch.zeros(64, T, dtype=torch.float64) for _ in range(WAVES)]
    sign = 0.0
    assert ops[-1][0] == 16 and all(op[0] == ops[0][0] for op in ops[:-1]) and 12 <= ops[0][0] <= 15
    for kind, plane, _, off in [op[:4] for op in ops[:-1]]:
        lk = kind - 12
        affine = lk < 2
        T2 = E // 2 if affine else E // 4
        o_b1 = 256 * E
        o_a2 = o_b1 + 16
        o_b2 = o_a2 + WAVES * T2 * 256
        o_pre = o_b2 + WAVES * T2 * 16
        A1 = prm[off:off + o_b1].reshape(WAVES, E // 4, 64, 4)
        b1 = prm[off + o_b1:off + o_a2]
        A2 = prm[off + o_a2:off + o_b2].reshape(WAVES, T2, 64, 4)
        b2 = prm[off + o_b2:off + o_pre].reshape(WAVES, T2, 16)
        pre = prm[off + o_pre:off + o_pre + 2 * hp]
        src, tgt = (a, b) if plane == 0 else (b, a)
        # GEMM 1: one partial per wave over its own K-slice, then the sum in wave order on top of b1
        parts = []
        for w in range(WAVES):
            acc = torch.zeros(64, 4, T, dtype=torch.float64)
            for s_ in range(E):
                acc = _mfma(A1[w, s_ // 4, :, s_ % 4], src[w][:, s_], acc)
            parts.append(acc)
        h = b1[(4 * q)[:, None] + torch.arange(4)[None, :]][:, :, None].expand(64, 4, T).clone()
        for w in range(WAVES):
            h = h + parts[w]
        hid = 1.0 - 2.0 / (torch.exp2(h) + 1.0)                                              # (64, 4, T)
        for w in range(WAVES):
            tw = (pre[col(w)][:, :, None] * tgt[w] + pre[hp + col(w)][:, :, None]).clone()
            for t_ in range(T2):
                o = b2[w, t_][(4 * q)[:, None] + torch.arange(4)[None, :]][:, :, None].expand(64, 4, T).clone()
                for k in range(4):
                    o = _mfma(A2[w, t_, :, k], hid[:, k], o)
                if affine:
                    for i in range(2):
                        e = 2 * t_ + i
                        al = torch.exp2(o[:, 2 * i]) + 1e-10
                        ld2[w] = ld2[w] + torch.log2(al)
                        tw[:, e] = al * tw[:, e] + o[:, 2 * i + 1] if lk == 0 else (tw[:, e] - o[:, 2 * i + 1]) / al
                    sign = 1.0 if lk == 0 else -1.0
                else:
                    for i in range(4):
                        e = 4 * t_ + i
                        tw[:, e] = tw[:, e] + o[:, i] if lk == 2 else tw[:, e] - o[:, i]
            tgt[w] = tw
    off = ops[-1][3]                                                                         # TFK_OP_EW_FMA
    s, t = prm[off:off + 2 * hp], prm[off + 2 * hp:off + 4 * hp]
    ld_row = torch.full((16, T), float(prm[off + 4 * hp]), dtype=torch.float64)
    out = torch.zeros(T, 16, 2 * hp, dtype=torch.float64)
    for w in range(WAVES):
        aw = s[col(w)][:, :, None] * a[w] + t[col(w)][:, :, None]
        bw = s[hp + col(w)][:, :, None] * b[w] + t[hp + col(w)][:, :, None]
        ld_row.index_add_(0, j, sign * LN2 * ld2[w])
        for e in range(E):
            out[:, j, (4 * w + q) * E + e] = aw[:, e].t()
            out[:, j, hp + (4 * w + q) * E + e] = bw[:, e].t()
    out = out.reshape(T * 16, 2 * hp)[:N]
    z = torch.cat([out[:, :half], out[:, hp:hp + half]], dim=1)                              # logical width, pads dropped
    if reverse_out:
        z = z.flip(1)
    return z, ld_row.t().reshape(T * 16)[:N]
