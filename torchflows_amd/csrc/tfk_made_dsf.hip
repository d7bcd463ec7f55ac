// tfk_made_dsf.hip -- the SEQUENTIAL map of a MADE-based deep sigmoidal layer in one launch.
//
// Replaces MaskedAutoregressiveBijection.inverse (MaskedAutoregressiveDeepSF sampling) and, with the maps exchanged,
// InverseMaskedAutoregressiveBijection.forward (InverseAutoregressiveDeepSF density) around Sigmoid / DeepSigmoid
// (transformers/combination/sigmoid.py): the host loop of D passes, each a whole MADE conditioner on ATen and one
// tfk_dsf_coupling_inv launch that bisects all D elements of every row to keep one of them.  The walk is the one of
// tfk_made.hip (k_made_rqs_sequential): the H hidden pre-activations of a row are kept and updated with column i of the
// first masked weight once element i is known, element i's record of P = 3 K C raw parameters is row block i of the second
// masked weight applied to tanh(a).  The transform is the one of tfk_dsf.hip (k_dsf_coupling<K, true>): tfk_dsf.h's
// extraction, its logit and its bisection on [-10, 10] (bracket moved on f(c) < y, until the fp32 midpoint stops moving,
// at most kDsfMaxTrips times), components last to first.
//   log-det: the one the reference returns, that of its LAST pass (layers_base.py: _sequential): for j < D-1 the
//   transformer's inverse evaluated at the already inverted x_j -- a second bisection, minus the forward log-det at the
//   point it returns --, for j = D-1 at z_{D-1} (tfk_made.hip does the same with its second spline evaluation).
//
// How the work is split.  The serial chain per element is long (two bisections x C components x up to 64 trips x K
// sigmoids) and sampling batches are small, so a row is NOT one lane's: it is owned by a group of G = 4, 8 or 16 adjacent
// lanes, the smallest not below K.
//   * lane g of a group owns hidden unit g of every component: its three dot products against tanh(a), its (a, b, w), its
//     sigmoid in every bisection trip (lanes g >= K idle along: a = b = w = 0);
//   * the softmax maximum and sum, the two mixture sums of a trip and the log-det sum cross the group as DPP all-reduces
//     (quad_perm, row_half_mirror, row_mirror: every lane of the group ends with the same bits, so the group takes every
//     branch of the bisection together); no LDS round trip and no barrier among them;
//   * the H hidden pre-activations are split over the group's lanes for the rank-one update; tanh(a) is handed round the
//     group by lane shuffles once per element.
// A workgroup of BLOCK lanes takes BLOCK / G rows, staged in the LDS at stride D + 1.  W1t, b1 and b2 live in the LDS; W2
// too when everything fits beside 256 lanes' rows, otherwise element i + 1's slice of P HP floats is brought in by the
// LDS-DMA (global_load_lds_dwordx4, no registers) into the other of two buffers while element i is being bisected, and
// one barrier per element publishes it.
// Dynamic LDS (floats): W1t[D][HP] | b1[HP] | b2[D][P] | rows[BLOCK / G][D + 1], up to a multiple of 4 | W2[D][P][HP] or
// 2 x [P][HP].  No matrix instructions: the P x HP product is under 5 % of an element's instructions.
#include "tfk_dsf.h"

namespace tfk {

template <int CTRL>
__device__ __forceinline__ float dpp_move(float v)
{
    return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), CTRL, 0xF, 0xF, false));
}

// Sum / maximum over the G (4, 8 or 16) adjacent lanes of a group, left in every one of them.  Step by step the two sides
// add the same two numbers, so all G lanes end with identical bits.
template <int G>
__device__ __forceinline__ float made_group_sum(float v)
{
    v += dpp_move<0xB1>(v);                                         // quad_perm [1, 0, 3, 2]
    v += dpp_move<0x4E>(v);                                         // quad_perm [2, 3, 0, 1]
    if (G >= 8) v += dpp_move<0x141>(v);                            // row_half_mirror: the other quad of 8
    if (G >= 16) v += dpp_move<0x140>(v);                           // row_mirror: the other half of 16
    return v;
}
template <int G>
__device__ __forceinline__ float made_group_max(float v)
{
    v = fmaxf(v, dpp_move<0xB1>(v));
    v = fmaxf(v, dpp_move<0x4E>(v));
    if (G >= 8) v = fmaxf(v, dpp_move<0x141>(v));
    if (G >= 16) v = fmaxf(v, dpp_move<0x140>(v));
    return v;
}

// d = sum_j w_j sigmoid(c_j) and its complement (dsf_value / dsf_forward of tfk_dsf.h, one hidden unit per lane); e: exp(-|c|)
template <int G, bool LEAN>
__device__ __forceinline__ void made_dsf_mix(float a, float b, float w, float x, float &d, float &cd, float &ac, float &e)
{
    const float c = a * x + b;
    ac = __builtin_fabsf(c);
    e = LEAN ? exp_lean(-ac) : exp_noovf(-ac);
    const float r = div_fast(1.0f, 1.0f + e);
    const float er = e * r;
    d = made_group_sum<G>(w * (c >= 0.0f ? r : er));
    cd = made_group_sum<G>(w * (c >= 0.0f ? er : r));
}

// The transformer's inverse at y for the group's row: record rows of W2 (w2i: [P][HP]) applied to tanh(a) (hk), extracted
// (dsf_extract), bisected (dsf_step<K, true>), components last to first.  Every lane of the group returns the same x and
// log-det.
template <int K, int G, int HP>
__device__ __forceinline__ void made_dsf_invert(const float *w2i, const float *b2i, const float (&hk)[HP], int C, int g,
                                                float y, float &x_out, float &ld_out)
{
    const bool act = g < K;
    const int gg = act ? g : 0;                                     // (idle lanes read lane 0's rows)
    float v = y, total = 0.0f;
    for (int c = C - 1; c >= 0; --c) {
        const int row = c * 3 * K + gg;
        float p[3];
#pragma unroll
        for (int t = 0; t < 3; ++t) {
            const float4 *wr = reinterpret_cast<const float4 *>(w2i + (row + t * K) * HP);
            float acc = b2i[row + t * K];
#pragma unroll
            for (int q = 0; q < HP / 4; ++q) {
                const float4 w4 = wr[q];
                acc = fmaf(w4.x, hk[4 * q], acc);
                acc = fmaf(w4.y, hk[4 * q + 1], acc);
                acc = fmaf(w4.z, hk[4 * q + 2], acc);
                acc = fmaf(w4.w, hk[4 * q + 3], acc);
            }
            p[t] = acc;
        }
        // sigmoid.py: extract_parameters (dsf_extract, hidden unit g)
        const float a_full = softplus20(kDsfDefaultUa + div_1000(p[0])) + kDsfMinScale;
        const float a = act ? a_full : 0.0f;
        const float b = act ? div_1000(p[1]) : 0.0f;
        const float wp = 0.0f + div_1000(p[2]);
        const float m = made_group_max<G>(act ? wp : -__builtin_inff());
        const float ew = act ? exp_noovf(wp - m) : 0.0f;
        const float s = made_group_sum<G>(ew);
        const float w = ew * (1.0f / s);
        const float lse = m + log_normal(s);
        const float cs = act ? (wp - lse) + log_normal(a_full) : 0.0f;      // this unit's log w + log a
        // numerical_inversion.py: bisection_no_gradient
        float lo = -10.0f, hi = 10.0f, mid = 0.0f;
        float d, cd, ac, e, lg, lc;
        for (int it = 0; it < kDsfMaxTrips; ++it) {
            made_dsf_mix<G, true>(a, b, w, mid, d, cd, ac, e);
            const bool below = dsf_logit(d, cd, lg, lc) < v;
            lo = below ? mid : lo;
            hi = below ? hi : mid;
            const float next = (lo + hi) / 2.0f;
            const bool done = (next == mid);
            mid = next;
            if (done) break;
        }
        // minus the forward log-det at the returned x (dsf_forward)
        made_dsf_mix<G, false>(a, b, w, mid, d, cd, ac, e);
        const float t3 = act ? -(ac + 2.0f * log1p_pos(e)) : 0.0f;
        const float rest = made_group_sum<G>(cs + t3);
        const float zf = dsf_logit(d, cd, lg, lc);
        total -= (float)K * zf + rest;
        v = mid;
    }
    x_out = v;
    ld_out = total;
}

// this wave's share of one [P][HP] slice of W2, global -> LDS without registers (nbytes: a multiple of 16)
__device__ __forceinline__ void made_dsf_issue(const float *src_f, float *dst_f, int nbytes, int wave, int lane, int waves)
{
    typedef __attribute__((address_space(1))) const void *gptr_t;
    typedef __attribute__((address_space(3))) void *lptr_t;
    const char *src = reinterpret_cast<const char *>(src_f);
    for (int c = wave; c * 1024 < nbytes; c += waves) {
        const int off = c * 1024 + lane * 16;
        if (off < nbytes)
            __builtin_amdgcn_global_load_lds((gptr_t)(src + off), (lptr_t)(reinterpret_cast<char *>(dst_f) + c * 1024), 16, 0, 0);
    }
}

template <int K, int G, int HP>
__global__ __launch_bounds__(256) void k_made_dsf_sequential(
    const float *z, float *x, float *logdet, long long N, int D, const float *__restrict__ W1t,
    const float *__restrict__ b1, const float *__restrict__ W2, const float *__restrict__ b2, int C, int stream_w2,
    int accumulate)
{
    constexpr int AK = HP >= G ? HP / G : 1;                        // hidden pre-activations a lane keeps
    const int P = 3 * K * C;
    const int B = blockDim.x, R = B / G, RS = D + 1;
    extern __shared__ __attribute__((aligned(16))) float lds[];
    float *w1 = lds;                                                // [D][HP]
    float *bb1 = w1 + D * HP;
    float *bb2 = bb1 + HP;                                          // [D][P]
    float *rows = bb2 + D * P;                                      // [R][D + 1]
    float *w2 = lds + ((D * HP + HP + D * P + R * RS + 3) & ~3);    // [D][P][HP], or two slices of [P][HP]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int r = tid / G, g = tid & (G - 1);
    for (int i = tid; i < D * HP; i += B) w1[i] = W1t[i];
    for (int i = tid; i < HP; i += B) bb1[i] = b1[i];
    for (int i = tid; i < D * P; i += B) bb2[i] = b2[i];
    if (!stream_w2)
        for (int i = tid; i < D * P * HP; i += B) w2[i] = W2[i];
    const int slice = P * HP;
    const long long n_tiles = (N + R - 1) / R;
    for (long long tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const long long base = tile * R;
        const int nrows = (int)((N - base) < (long long)R ? (N - base) : (long long)R);
        __syncthreads();                                            // the previous tile's rows and slices are done with
        for (int e = tid; e < R * D; e += B) {                      // coalesced load, parked at stride D + 1; idle rows: 0
            const int rr = e / D;
            rows[rr * RS + (e - rr * D)] = rr < nrows ? z[base * D + e] : 0.0f;
        }
        if (stream_w2) made_dsf_issue(W2, w2, slice * 4, wave, lane, B >> 6);
        else __syncthreads();
        float a[AK];
#pragma unroll
        for (int j = 0; j < AK; ++j) a[j] = bb1[(g + j * G) & (HP - 1)];
        float ld = 0.0f;
        float *mine = rows + r * RS;
        for (int i = 0; i < D; ++i) {
            const float *w2i = w2 + (size_t)i * slice;
            if (stream_w2) {
                asm volatile("s_waitcnt vmcnt(0)" ::: "memory");    // this wave's share of slice i has landed
                __syncthreads();                                    // ... everybody's has, and element i - 1 is done with
                w2i = w2 + (i & 1) * slice;
                if (i + 1 < D) made_dsf_issue(W2 + (size_t)(i + 1) * slice, w2 + ((i + 1) & 1) * slice, slice * 4, wave, lane, B >> 6);
            }
            float th[AK], hk[HP];
#pragma unroll
            for (int j = 0; j < AK; ++j) {
                const float e2 = __builtin_amdgcn_exp2f(a[j] * 2.8853900817779268f);
                th[j] = fmaf(-2.0f, __builtin_amdgcn_rcpf(e2 + 1.0f), 1.0f);                  // tanh
            }
#pragma unroll
            for (int k = 0; k < HP; ++k) hk[k] = __shfl(th[HP >= G ? k / G : 0], k & (G - 1), G);
            const float y = mine[i];
            float xi, l;
            made_dsf_invert<K, G, HP>(w2i, bb2 + i * P, hk, C, g, y, xi, l);
            if (i < D - 1) {                                        // what the reference's last pass sees
                float x2;
                made_dsf_invert<K, G, HP>(w2i, bb2 + i * P, hk, C, g, xi, x2, l);
            }
            ld += l;
            if (g == 0) mine[i] = xi;
            const float *col = w1 + i * HP;
#pragma unroll
            for (int j = 0; j < AK; ++j) a[j] = fmaf(col[(g + j * G) & (HP - 1)], xi, a[j]);
        }
        if (g == 0 && r < nrows) {
            const long long row = base + r;
            logdet[row] = accumulate ? logdet[row] + ld : ld;
        }
        __syncthreads();
        for (int e = tid; e < nrows * D; e += B) {
            const int rr = e / D;
            x[base * D + e] = rows[rr * RS + (e - rr * D)];
        }
    }
}

// ---- host ----

constexpr int64_t kMadeDsfLdsMax = 160 * 1024;

__host__ __device__ constexpr int made_dsf_group(int K) { return K <= 4 ? 4 : (K <= 8 ? 8 : 16); }

// bytes of the layout above at `block` lanes
static int64_t made_dsf_lds(int D, int HP, int C, int K, int block, bool stream_w2)
{
    const int64_t P = 3 * (int64_t)K * C, R = block / made_dsf_group(K);
    const int64_t head = ((int64_t)D * HP + HP + D * P + R * (D + 1) + 3) & ~(int64_t)3;
    return 4 * (head + (stream_w2 ? 2 * P * HP : D * P * HP));
}

int64_t made_dsf_sequential_lds_bytes(int32_t D, int32_t hidden_padded, int32_t code)
{
    const int C = (code >> 8) & 0xFF, K = code & 0xFF;
    if (!made_is_dsf(code) || !dsf_supported(C, K) || (hidden_padded != 8 && hidden_padded != 16) || D < 1 || D > 1024)
        return (int64_t)1 << 40;                                    // no kernel: above every LDS
    return made_dsf_lds(D, hidden_padded, C, K, 64, true);          // the smallest workgroup, W2 streamed
}

template <int K, int HP>
static void made_dsf_launch(int grid, int block, size_t lds, hipStream_t s, const float *z, float *x, float *logdet, int64_t N,
                            int D, const float *W1t, const float *b1, const float *W2, const float *b2, int C, int stream_w2,
                            int accumulate, bool &attr_ok)
{
    constexpr int G = made_dsf_group(K);
    attr_ok = true;
    if (lds > 64 * 1024 &&
        hipFuncSetAttribute(reinterpret_cast<const void *>(&k_made_dsf_sequential<K, G, HP>),
                            hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess) {
        (void)hipGetLastError();
        attr_ok = false;
        return;
    }
    hipLaunchKernelGGL((k_made_dsf_sequential<K, G, HP>), dim3(grid), dim3(block), lds, s, z, x, logdet, (long long)N, D, W1t,
                       b1, W2, b2, C, stream_w2, accumulate);
}

#define TFK_MADE_DSF_FOR_EACH_K(X) \
    X(1) X(2) X(3) X(4) X(5) X(6) X(7) X(8) X(9) X(10) X(11) X(12) X(13) X(14) X(15) X(16)

int made_dsf_sequential(const float *z, float *x, float *logdet, int64_t N, int32_t D, const float *W1t, const float *b1,
                        const float *W2, const float *b2, int32_t hidden_padded, int32_t code, float boundary,
                        int32_t accumulate, void *stream, const char *fn)
{
    const int C = (code >> 8) & 0xFF, K = code & 0xFF, HP = hidden_padded;
    if (N < 0) return fail(TFK_EINVAL, "%s: N = %lld < 0", fn, (long long)N);
    if (D < 1 || D > 1024) return fail(TFK_EINVAL, "%s: D = %d not in [1, 1024]", fn, D);
    if (HP != 8 && HP != 16) return fail(TFK_EINVAL, "%s: hidden_padded = %d must be 8 or 16", fn, HP);
    if (!dsf_supported(C, K))
        return fail(TFK_EINVAL, "%s: n_bins = 0x%x: n_components = %d, hidden_dim = %d (kernels exist for hidden_dim <= 16 "
                    "with <= 2 components and hidden_dim <= 8 with <= 4: tfk_dsf_supported)", fn, code, C, K);
    if (boundary != 10.0f)
        return fail(TFK_EINVAL, "%s: boundary = %g: the deep sigmoidal bisection runs on [-10, 10]", fn, (double)boundary);
    if (N == 0) return TFK_OK;
    if (!z || !x || !logdet || !W1t || !b1 || !W2 || !b2) return fail(TFK_EINVAL, "%s: null pointer", fn);
    if (!aligned16(W2)) return fail(TFK_EINVAL, "%s: W2 must be 16-byte aligned", fn);
    int block = 256, stream_w2 = 0;
    if (made_dsf_lds(D, HP, C, K, 256, false) > kMadeDsfLdsMax) {
        stream_w2 = 1;
        while (block > 64 && made_dsf_lds(D, HP, C, K, block, true) > kMadeDsfLdsMax) block >>= 1;
    }
    const size_t lds = (size_t)made_dsf_lds(D, HP, C, K, block, stream_w2 != 0);
    if ((int64_t)lds > kMadeDsfLdsMax)
        return fail(TFK_EINVAL, "%s: D = %d, %d x %d parameters, hidden <= %d needs %zu bytes of LDS", fn, D, C, 3 * K, HP, lds);
    const int R = block / made_dsf_group(K);
    int per_cu = (int)(kMadeDsfLdsMax / (int64_t)lds);
    if (per_cu > 8) per_cu = 8;
    const int64_t n_tiles = (N + R - 1) / R;
    const int grid = (int)(n_tiles < (int64_t)cu_count() * per_cu ? n_tiles : (int64_t)cu_count() * per_cu);
    hipStream_t s = static_cast<hipStream_t>(stream);
    bool attr_ok = true;
    switch (HP * 32 + K) {
#define TFK_MADE_DSF_CASE(K_)                                                                                                  \
    case 8 * 32 + K_:                                                                                                          \
        made_dsf_launch<K_, 8>(grid, block, lds, s, z, x, logdet, N, D, W1t, b1, W2, b2, C, stream_w2, accumulate, attr_ok);  \
        break;                                                                                                                 \
    case 16 * 32 + K_:                                                                                                         \
        made_dsf_launch<K_, 16>(grid, block, lds, s, z, x, logdet, N, D, W1t, b1, W2, b2, C, stream_w2, accumulate, attr_ok); \
        break;
        TFK_MADE_DSF_FOR_EACH_K(TFK_MADE_DSF_CASE)
#undef TFK_MADE_DSF_CASE
    }
    if (!attr_ok) return fail(TFK_ELAUNCH, "%s: cannot reserve %zu bytes of LDS", fn, lds);
    return check_launch(fn);
}

}  // namespace tfk
