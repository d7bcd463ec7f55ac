// tfk_wide_bwd.hip -- tfk_wide_coupling_train_bwd: reverse mode of one affine / shift coupling on event sizes
// 256 < D <= 1024, D % 8 == 0 (kernel, geometry and parameter-block layout: tfk_wide_bwd.h).
#include "tfk_wide_bwd.h"

namespace tfk {

// EPLW = 12 .. 32: planes of 192 .. 512 columns, i.e. every D % 8 == 0 in (256, 1024]
#define TFK_WB_ALL(X_) X_(12) X_(16) X_(20) X_(24) X_(28) X_(32)

template <bool SHIFT>
static int launch_wide_bwd(int eplw, const float *x, float *g, const float *gld, const float *params, float *gh_rec,
                           float *gpre_rec, float *hid_rec, int64_t N, int D, int inverse_form, const float *gscale,
                           int g_reversed, hipStream_t s, const char *fn)
{
#define TFK_WB(E_) case E_: return launch_wide_bwd_k<E_, SHIFT>(x, g, gld, params, gh_rec, gpre_rec, hid_rec, N, D, inverse_form, gscale, g_reversed, s, fn);
    switch (eplw) {
    TFK_WB_ALL(TFK_WB)
    default: return fail(TFK_EINVAL, "%s: no kernel for %d columns per lane", fn, eplw);
    }
#undef TFK_WB
}

template <bool SHIFT>
static int grid_cap(int eplw)
{
#define TFK_WB(E_) case E_: return wide_bwd_grid_cap<E_, SHIFT>();
    switch (eplw) {
    TFK_WB_ALL(TFK_WB)
    default: return 0;
    }
#undef TFK_WB
}

}  // namespace tfk

using namespace tfk;

extern "C" {

int tfk_wide_coupling_train_bwd_supported(int32_t D, int32_t H)
{
    return (D % 8 == 0 && D > 256 && D <= 1024 && H >= 1 && H <= 15) ? 1 : 0;
}

int64_t tfk_wide_coupling_train_bwd_param_floats(int32_t D, int32_t shift)
{
    if (!tfk_wide_coupling_train_bwd_supported(D, 1)) return 0;
    return wide_bwd_block_floats((D / 2 + 63) / 64 * 4, !shift);
}

int64_t tfk_wide_coupling_train_bwd_grid_cap(int32_t D, int32_t shift)
{
    if (!tfk_wide_coupling_train_bwd_supported(D, 1)) return 0;
    const int eplw = (D / 2 + 63) / 64 * 4;
    return shift ? grid_cap<true>(eplw) : grid_cap<false>(eplw);
}

int tfk_wide_coupling_train_bwd(const float *x, float *g, const float *gld, const float *params, int64_t n_params,
                                float *gh_rec, float *gpre_rec, float *hid_rec, int64_t N, int32_t D, int32_t shift,
                                int32_t inverse_form, const float *gscale, int32_t g_reversed, void *stream)
{
    const char *fn = "tfk_wide_coupling_train_bwd";
    if (N < 1) return fail(TFK_EINVAL, "%s: N = %lld < 1", fn, (long long)N);
    if (!tfk_wide_coupling_train_bwd_supported(D, 1))
        return fail(TFK_EINVAL, "%s: event size %d (multiples of 8 in (256, 1024])", fn, (int)D);
    const int64_t need = tfk_wide_coupling_train_bwd_param_floats(D, shift);
    if (n_params != need) return fail(TFK_EINVAL, "%s: parameter block has %lld floats, expected %lld", fn,
                                      (long long)n_params, (long long)need);
    if (!x || !g || !gld || !params || !gh_rec || !gpre_rec || !hid_rec) return fail(TFK_EINVAL, "%s: null pointer", fn);
    if (!aligned16(x) || !aligned16(g) || !aligned16(params) || !aligned16(gh_rec) || !aligned16(gpre_rec)
        || !aligned16(hid_rec) || (gscale && !aligned16(gscale)))
        return fail(TFK_EINVAL, "%s: x, g, params, the records and gscale must be 16-byte aligned", fn);
    const int eplw = (D / 2 + 63) / 64 * 4;
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (shift)
        return launch_wide_bwd<true>(eplw, x, g, gld, params, gh_rec, gpre_rec, hid_rec, N, D, inverse_form ? 1 : 0, gscale,
                                     g_reversed ? 1 : 0, s, fn);
    return launch_wide_bwd<false>(eplw, x, g, gld, params, gh_rec, gpre_rec, hid_rec, N, D, inverse_form ? 1 : 0, gscale,
                                  g_reversed ? 1 : 0, s, fn);
}

}  // extern "C"
