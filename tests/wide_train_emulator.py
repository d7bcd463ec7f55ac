"""fp64 emulator of the wide training launches for host-side tests: ``run_wide_bwd`` decodes the parameter block exactly as
csrc/tfk_wide_bwd.h indexes it (per-wave column ownership, split-K partials of GEMM 1 and of W2^T dL/dh added in wave
order, lane-major MFMA A-operands, the records' column order), ``rows_outer`` restates tfk_rows_outer's accumulator order
(include/tfk.h) -- so that torchflows_amd/autograd.py:_WideTrainPack can be checked without a GPU."""
import torch

from lean_emulator import _mfma

WAVES = 4


def run_wide_bwd(params, x, g, gld, D, shift=False, inverse_form=False, gscale=None, g_reversed=False):
    """x, g (N, D), gld (N,) -> (g out (N, D), gh_rec (N, 2 hp | hp), gpre_rec (N, 16), hid_rec (N, 16)), all float64."""
    N = x.shape[0]
    half = D // 2
    hp = (half + 63) // 64 * 64
    E = hp // 16
    T = (N + 15) // 16
    T2, G1 = (E // 4 if shift else E // 2), E // 4
    GHL = E if shift else 2 * E
    prm = params.double()
    o_b1 = 256 * E
    o_a2 = o_b1 + 16
    o_b2 = o_a2 + WAVES * T2 * 256
    o_a2t = o_b2 + WAVES * T2 * 16 + 2 * hp
    o_a1t = o_a2t + WAVES * T2 * 256
    assert prm.numel() == o_a1t + 256 * E
    A1 = prm[:o_b1].reshape(WAVES, G1, 64, 4)
    b1 = prm[o_b1:o_a2]
    A2 = prm[o_a2:o_b2].reshape(WAVES, T2, 64, 4)
    b2 = prm[o_b2:o_b2 + WAVES * T2 * 16].reshape(WAVES, T2, 16)
    A2T = prm[o_a2t:o_a1t].reshape(WAVES, T2, 64, 4)
    A1T = prm[o_a1t:].reshape(WAVES, G1, 64, 4)

    gin = g.double()
    if g_reversed:
        gin = gin.flip(1)
    if gscale is not None:
        gin = gin * gscale.double()[None, :]

    def planes(rows):
        p = torch.zeros(T * 16, 2 * hp, dtype=torch.float64)            # rows past the end and pad columns: zeros
        p[:N, :half] = rows[:, :half]
        p[:N, hp:hp + half] = rows[:, half:]
        return p.reshape(T, 16, 2 * hp)
    xp, gp = planes(x.double()), planes(gin)
    glp = torch.zeros(T * 16, dtype=torch.float64)
    glp[:N] = gld.double()
    lane = torch.arange(64)
    q, j = lane >> 4, lane & 15
    gl = glp.reshape(T, 16)[:, j].t()                                    # (64, T)
    col = lambda w: ((4 * w + q) * E)[:, None] + torch.arange(E)[None, :]                   # (64, E)
    regs = lambda p, w, base: p[:, j][:, lane[:, None], base + col(w)].permute(1, 2, 0).clone()   # (64, E, T)
    xa = [regs(xp, w, 0) for w in range(WAVES)]
    xb = [regs(xp, w, hp) for w in range(WAVES)]
    ga = [regs(gp, w, 0) for w in range(WAVES)]
    gb = [regs(gp, w, hp) for w in range(WAVES)]
    quad = (4 * q)[:, None] + torch.arange(4)[None, :]
    # GEMM 1: split-K partials, summed in wave order on top of b1
    h = b1[quad][:, :, None].expand(64, 4, T).clone()
    for w in range(WAVES):
        acc = torch.zeros(64, 4, T, dtype=torch.float64)
        for s_ in range(E):
            acc = _mfma(A1[w, s_ // 4, :, s_ % 4], xa[w][:, s_], acc)
        h = h + acc
    hid = 1.0 - 2.0 / (torch.exp2(h) + 1.0)                              # (64, 4, T): unit 4 r + q
    gh_rec = torch.zeros(T, 16, 16 * GHL, dtype=torch.float64)
    gha = torch.zeros(64, 4, T, dtype=torch.float64)
    for w in range(WAVES):
        part = torch.zeros(64, 4, T, dtype=torch.float64)
        for t_ in range(T2):
            o = b2[w, t_][quad][:, :, None].expand(64, 4, T).clone()
            for k in range(4):
                o = _mfma(A2[w, t_, :, k], hid[:, k], o)
            ghv = torch.zeros(64, 4, T, dtype=torch.float64)
            if not shift:
                for i in range(2):
                    e = 2 * t_ + i
                    ex = torch.exp2(o[:, 2 * i])
                    beta = o[:, 2 * i + 1]
                    alpha = ex + 1e-10
                    gz = gb[w][:, e].clone()
                    if not inverse_form:
                        gx, gbeta, galpha = gz * alpha, gz, gz * xb[w][:, e] + gl / alpha
                    else:
                        r_ = gz / alpha
                        gx, gbeta, galpha = r_, -r_, -r_ * ((xb[w][:, e] - beta) / alpha) - gl / alpha
                    gb[w][:, e] = gx
                    ghv[:, 2 * i] = galpha * ex * 0.5
                    ghv[:, 2 * i + 1] = gbeta
            else:
                for i in range(4):
                    ghv[:, i] = -gb[w][:, 4 * t_ + i] if inverse_form else gb[w][:, 4 * t_ + i]
            for r in range(4):
                gh_rec[:, j, (4 * w + q) * GHL + 4 * t_ + r] = ghv[:, r].t()
                part = _mfma(A2T[w, t_, :, r], ghv[:, r], part)
        gha = gha + part
    gpre = gha * (1.0 - hid * hid)
    out = torch.zeros(T, 16, 2 * hp, dtype=torch.float64)
    for w in range(WAVES):
        for s_ in range(G1):
            d = torch.zeros(64, 4, T, dtype=torch.float64)
            for r in range(4):
                d = _mfma(A1T[w, s_, :, r], gpre[:, r], d)
            for r in range(4):
                ga[w][:, 4 * s_ + r] = ga[w][:, 4 * s_ + r] + d[:, r]
        for e in range(E):
            out[:, j, (4 * w + q) * E + e] = ga[w][:, e].t()
            out[:, j, hp + (4 * w + q) * E + e] = gb[w][:, e].t()
    out = out.reshape(T * 16, 2 * hp)[:N]
    g_out = torch.cat([out[:, :half], out[:, hp:hp + half]], dim=1)
    hid_rec = torch.zeros(T, 16, 16, dtype=torch.float64)
    gpre_rec = torch.zeros(T, 16, 16, dtype=torch.float64)
    for r in range(4):
        hv = hid[:, r].clone()
        if r == 3:
            hv[q == 3] = 1.0                                              # the bias column
        hid_rec[:, j, 4 * q + r] = hv.t()
        gpre_rec[:, j, 4 * q + r] = gpre[:, r].t()
    return (g_out, gh_rec.reshape(T * 16, -1)[:N], gpre_rec.reshape(T * 16, 16)[:N], hid_rec.reshape(T * 16, 16)[:N])


def rows_outer(A, M, B):
    """tfk_rows_outer's output for A (N, lda), its first M columns, and B (N, 16): M * 16 floats in accumulator order."""
    full = A[:, :M].double().t() @ B.double()                             # (M, 16)
    t, q, j, r = torch.meshgrid(torch.arange(M // 16), torch.arange(4), torch.arange(16), torch.arange(4), indexing="ij")
    i = 4 * q + r
    col = 64 * (t >> 2) + 4 * i + (t & 3) if M >= 64 else 16 * t + i
    return full[col, j].reshape(-1)


def coupling_backward(pack, params, x, g, gld, D, shift=False, inverse_form=False, gscale=None, g_reversed=False):
    """The whole reverse mode of one wide coupling as ChainFunction.backward issues it: the launch, the three products,
    the un-permute -> (g out, dW1, db1, dW2, db2)."""
    g_out, gh_rec, gpre_rec, hid_rec = run_wide_bwd(params, x, g, gld, D, shift, inverse_form, gscale, g_reversed)
    acc = torch.cat([rows_outer(gh_rec, pack.GH, hid_rec), rows_outer(x, pack.hp, gpre_rec), rows_outer(gpre_rec, 16, hid_rec)])
    return (g_out,) + pack.unpack_grads(acc)
