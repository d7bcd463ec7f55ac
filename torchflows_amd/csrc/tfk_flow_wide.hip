// tfk_flow_wide.hip -- tfk_flow_run_wide: chains of affine / shift couplings on event sizes 256 < D <= 2048 as ONE launch
// (kernel and parameter-block layout: tfk_flow_wide.h).
#include "tfk_flow_wide.h"

namespace tfk {

template <int KIND>
static int launch_wide(int eplw, const float *x, float *z, float *logdet, const float *loc, const float *log_scale,
                       float *logprob, int64_t N, int D, const float *params, const WideProg &prog, int flags, int vec,
                       hipStream_t s, const char *fn)
{
#define TFK_W(E_) case E_: return launch_wide_k<E_, KIND>(x, z, logdet, loc, log_scale, logprob, N, D, params, prog, flags, vec, s, fn)
    switch (eplw) {
    TFK_W(12); TFK_W(16); TFK_W(20); TFK_W(24); TFK_W(28); TFK_W(32); TFK_W(36); TFK_W(40);
    TFK_W(44); TFK_W(48); TFK_W(52); TFK_W(56); TFK_W(60); TFK_W(64);
    default: return fail(TFK_EINVAL, "%s: no kernel for %d columns per lane", fn, eplw);
    }
#undef TFK_W
}

}  // namespace tfk

using namespace tfk;

extern "C" {

int tfk_flow_wide_supported(int32_t D, int32_t H)
{
    return (D % 2 == 0 && D > 256 && D <= 2048 && H >= 1 && H <= 16) ? 1 : 0;
}

int tfk_flow_run_wide(const float *x, float *z, float *logdet, const float *gauss_loc, const float *gauss_log_scale,
                      float *logprob, int64_t N, int32_t D, const int32_t *ops, int32_t n_ops,
                      const float *params, int64_t n_params, int32_t flags, void *stream)
{
    const char *fn = "tfk_flow_run_wide";
    if (!tfk_flow_wide_supported(D, 1))
        return fail(TFK_EINVAL, "%s: event size %d (even sizes in (256, 2048])", fn, (int)D);
    if (N < 0 || !x || !ops || !params) return fail(TFK_EINVAL, "%s: null argument or negative N", fn);
    if (logprob && (!gauss_loc || !gauss_log_scale)) return fail(TFK_EINVAL, "%s: logprob needs the base parameters", fn);
    if ((flags & 4) && !logprob) return fail(TFK_EINVAL, "%s: flag bit 2 (base of the input) needs logprob", fn);
    if ((flags & 1) && !logdet) return fail(TFK_EINVAL, "%s: flag bit 0 (accumulate) needs logdet", fn);
    if (flags & ~7) return fail(TFK_EINVAL, "%s: unknown flag bits %d", fn, (int)flags);
    const int half = D / 2;
    const int hp = (half + 63) / 64 * 64;                    // plane width the blocks are packed for
    const int eplw = hp / 16;
    if (n_ops < 2 || n_ops > kWideMaxOps + 1)
        return fail(TFK_EINVAL, "%s: a program is 1..%d couplings and the closing TFK_OP_EW_FMA", fn, kWideMaxOps);
    WideProg prog = {};
    int kind = -1;
    for (int i = 0; i < n_ops; ++i) {
        const int32_t *rec = ops + 8 * i;
        const int k = rec[0], src = rec[1];
        const int64_t off = rec[3];
        if (off < 0 || (off & 3)) return fail(TFK_EINVAL, "%s: op %d: offset %lld is not a multiple of 4 floats", fn, i, (long long)off);
        if (i == n_ops - 1) {
            if (k != TFK_OP_EW_FMA) return fail(TFK_EINVAL, "%s: the last op must be TFK_OP_EW_FMA", fn);
            if (off + 4 * hp + 4 > n_params) return fail(TFK_EINVAL, "%s: op %d: parameters outside the block", fn, i);
            prog.ew_offset = (int)off;
            break;
        }
        if (k < TFK_OP_AFFINE_FWD_LEAN || k > TFK_OP_SHIFT_INV_LEAN)
            return fail(TFK_EINVAL, "%s: op %d: kind %d (affine / shift couplings, TFK_OP_*_LEAN)", fn, i, k);
        if (kind < 0) kind = k - TFK_OP_AFFINE_FWD_LEAN;
        else if (kind != k - TFK_OP_AFFINE_FWD_LEAN) return fail(TFK_EINVAL, "%s: op %d: a program holds couplings of one kind", fn, i);
        if (src != 0 && src != 1) return fail(TFK_EINVAL, "%s: op %d: src_plane %d", fn, i, src);
        if (rec[2] < 1 || rec[2] > 16) return fail(TFK_EINVAL, "%s: op %d: hidden width %d not in [1, 16]", fn, i, (int)rec[2]);
        if (off + wide_block_floats(eplw, kind < 2) > n_params)
            return fail(TFK_EINVAL, "%s: op %d: parameters outside the block", fn, i);
        prog.offset[prog.n_c] = (int)off;
        if (src) prog.src_mask |= 1ull << prog.n_c;
        ++prog.n_c;
    }
    // widest access every plane start and row start allows (rows are read at their logical width, in place)
    int vec = (half % 4 == 0) ? 4 : ((half % 2 == 0) ? 2 : 1);
    const uintptr_t align = reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(z);
    while (vec > 1 && (align & (uintptr_t)(4 * vec - 1))) vec >>= 1;
    if ((align & 3) || !aligned16(params)) return fail(TFK_EINVAL, "%s: x / z must be 4-byte and params 16-byte aligned", fn);
    if (N == 0) return TFK_OK;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    switch (kind) {
    case 0: return launch_wide<0>(eplw, x, z, logdet, gauss_loc, gauss_log_scale, logprob, N, D, params, prog, flags, vec, s, fn);
    case 1: return launch_wide<1>(eplw, x, z, logdet, gauss_loc, gauss_log_scale, logprob, N, D, params, prog, flags, vec, s, fn);
    case 2: return launch_wide<2>(eplw, x, z, logdet, gauss_loc, gauss_log_scale, logprob, N, D, params, prog, flags, vec, s, fn);
    default: return launch_wide<3>(eplw, x, z, logdet, gauss_loc, gauss_log_scale, logprob, N, D, params, prog, flags, vec, s, fn);
    }
}

}  // extern "C"
