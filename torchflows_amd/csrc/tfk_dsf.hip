// tfk_dsf.hip -- deep sigmoidal flow coupling (Huang et al. 2018, neural autoregressive flows).
//
// Replaces CouplingBijection.forward / inverse (layers_base.py) around Sigmoid / DeepSigmoid
// (transformers/combination/sigmoid.py, combination/base.py) and, for the inverse, the host-driven bisection of
// bijections/numerical_inversion.py.  h is (N, T, 3 K C): C components of [da (K) | db (K) | dw (K)] per element:
//     a = softplus(log(e - 1 - 1e-3) + da / 1000) + 1e-3,  b = db / 1000,  w = softmax(dw / 1000)
//     d = clip(sum_j w_j sigmoid(a_j x + b_j), 1e-6, 1 - 1e-6),  z = log d - log1p(-d)      (1 - d: dsf_logit below)
//     log-det (as the reference has it) = K (log d - log(1 - d)) + sum_j [log w_j + log a_j + log sigmoid(c_j) + log sigmoid(-c_j)]
//   * a workgroup takes R = BLOCK / T rows = up to BLOCK records, loads them with coalesced non-temporal reads and
//     stores them in LDS at an odd stride, so that the per-lane reads of "my record" are bank-conflict-free
//     (BLOCK = 256 for K <= 4, 128 above: at most 50 KB of records either way);
//   * one lane = one element; K is a template parameter, so a component's (a, b, w) sit in registers; the components
//     are walked in a loop (forward: first to last, inverse: last to first), each extracted once;
//   * inverse: the reference's bisection on [-10, 10] (bracket moved on f(c) < y, result = the last midpoint) runs per
//     element until the fp32 midpoint stops moving, at most kDsfMaxTrips times (loop body: the value only, lean exp); the
//     log-det is evaluated at the returned x;
//   * per-row log-det: __shfl_xor inside the T-lane group when T is a power of two <= 64, LDS otherwise; rows longer than
//     the tile are walked in chunks.  Deterministic.
#include "tfk_common.h"
#include "tfk_spline.h"

namespace tfk {

constexpr int kDsfMaxTrips = 64;            // 20 * 2^-64 is far below one ulp of any fp32 midpoint
constexpr float kDsfEps = 1e-6f;            // the clip of d (python doubles rounded once to fp32, as ATen does)
constexpr float kDsfOneMinusEps = (float)(1.0 - 1e-6);
constexpr float kDsfMinScale = 1e-3f;
constexpr float kDsfDefaultUa = 0.5407427084918718f;     // log(e - 1 - 1e-3)

__host__ __device__ constexpr int dsf_block(int K) { return K <= 4 ? 256 : 128; }

template <int K>
struct DsfComp {
    float a[K], b[K], w[K];
    float csum;                              // sum_j (log w_j + log a_j)
};

// log1p(-d) for 0 < d < 1: log(u) + ((1 - u) - d) / u with u = fl(1 - d) (tfk_common.h: log1p_pos)
__device__ __forceinline__ float log1p_neg(float d) {
    const float u = 1.0f - d;
    const float lost = (1.0f - u) - d;
    return log_normal(u) + lost * __builtin_amdgcn_rcpf(u);
}

// z = log d - log(1 - d) with the reference's clip of d = sum_j w_j sigmoid(c_j).  Inside the clip 1 - d is taken as the
// complement sum cd = sum_j w_j sigmoid(-c_j): fl(1 - d) knows 1 - d only to ulp(1) / (1 - d) relative (4e-5 at
// 1 - d = 1.5e-3, 6 % beside the clip), which is the noise of z, of the root the bisection finds and of 1 / (d (1 - d)) in
// the reverse mode there; cd keeps 1e-7 relative (d + cd = sum_j w_j = 1 to a rounding).  cd is held at or above the
// clip's own 1 - d, so that z stays monotone across the clip's edge.  lg, lc: log d and log(1 - d).
__device__ __forceinline__ float dsf_complement(float cd) { return fmaxf(cd, 1.0f - kDsfOneMinusEps); }
__device__ __forceinline__ float dsf_logit(float d0, float cd, float &lg, float &lc)
{
    const bool inside = (d0 >= kDsfEps) && (d0 <= kDsfOneMinusEps);
    const float d = fminf(fmaxf(d0, kDsfEps), kDsfOneMinusEps);
    lg = log_normal(d);
    lc = inside ? log_normal(dsf_complement(cd)) : log1p_neg(d);
    return lg - lc;
}

// sigmoid.py: extract_parameters.  log_softmax goes through the log-sum-exp, softmax is e * (1 / sum) (ATen's CPU form).
template <int K>
__device__ __forceinline__ void dsf_extract(const float *p, DsfComp<K> &q)
{
    float wp[K];
    float m = 0.0f;
#pragma unroll
    for (int j = 0; j < K; ++j) {
        q.a[j] = softplus20(kDsfDefaultUa + div_1000(p[j])) + kDsfMinScale;
        q.b[j] = div_1000(p[K + j]);
        wp[j] = 0.0f + div_1000(p[2 * K + j]);
        m = j ? fmaxf(m, wp[j]) : wp[j];
    }
    float s = 0.0f;
#pragma unroll
    for (int j = 0; j < K; ++j) {
        q.w[j] = exp_noovf(wp[j] - m);
        s += q.w[j];
    }
    const float r = 1.0f / s;
    const float lse = m + log_normal(s);
    float cs = 0.0f;
#pragma unroll
    for (int j = 0; j < K; ++j) {
        q.w[j] = q.w[j] * r;
        cs += (wp[j] - lse) + log_normal(q.a[j]);
    }
    q.csum = cs;
}

// forward_1d: the value only.  LEAN (the bisection's loop body, which only compares the value): exp in 5 ops (within
// 1 ulp of the other, tfk_common.h) -- the search then settles within that ulp's worth of x, far inside the fp32 noise of
// f around the root that any fp32 bisection has.
template <int K, bool LEAN>
__device__ __forceinline__ float dsf_value(const DsfComp<K> &q, float x)
{
    float d = 0.0f, cd = 0.0f;
#pragma unroll
    for (int j = 0; j < K; ++j) {
        const float c = q.a[j] * x + q.b[j];
        const float ac = __builtin_fabsf(c);                        // e in (0, 1]: no overflow for any c
        const float e = LEAN ? exp_lean(-ac) : exp_noovf(-ac);
        const float r = div_fast(1.0f, 1.0f + e);                   // (1 + e in [1, 2]: within half an ulp, tfk_common.h)
        const float er = e * r;
        d += q.w[j] * (c >= 0.0f ? r : er);
        cd += q.w[j] * (c >= 0.0f ? er : r);                        // sigmoid(-c)
    }
    float lg, lc;
    return dsf_logit(d, cd, lg, lc);
}

// forward_1d: value and the reference's log-det
template <int K>
__device__ __forceinline__ float dsf_forward(const DsfComp<K> &q, float x, float &ld)
{
    float d = 0.0f, cd = 0.0f, t3 = 0.0f;
#pragma unroll
    for (int j = 0; j < K; ++j) {
        const float c = q.a[j] * x + q.b[j];
        const float ac = __builtin_fabsf(c);
        const float e = exp_noovf(-ac);
        const float r = div_fast(1.0f, 1.0f + e);
        const float er = e * r;
        d += q.w[j] * (c >= 0.0f ? r : er);
        cd += q.w[j] * (c >= 0.0f ? er : r);
        t3 -= ac + 2.0f * log1p_pos(e);                             // log sigmoid(c) + log sigmoid(-c)
    }
    float lg, lc;
    const float z = dsf_logit(d, cd, lg, lc);
    ld = (float)K * z + q.csum + t3;
    return z;
}

// One element through all C components.  p: its record (3 K C floats, LDS).
template <int K, bool INVERSE>
__device__ __forceinline__ void dsf_eval(const float *p, int C, float v, float &out, float &ld)
{
    DsfComp<K> q;
    float total = 0.0f;
    if (!INVERSE) {
        for (int c = 0; c < C; ++c) {
            dsf_extract<K>(p + c * 3 * K, q);
            float l;
            v = dsf_forward<K>(q, v, l);
            total += l;
        }
    } else {
        for (int c = C - 1; c >= 0; --c) {
            dsf_extract<K>(p + c * 3 * K, q);
            float lo = -10.0f, hi = 10.0f, mid = 0.0f;
            for (int it = 0; it < kDsfMaxTrips; ++it) {             // numerical_inversion.py: bisection_no_gradient
                const bool below = dsf_value<K, true>(q, mid) < v;
                lo = below ? mid : lo;
                hi = below ? hi : mid;
                const float next = (lo + hi) / 2.0f;
                const bool done = (next == mid);
                mid = next;
                if (done) break;
            }
            float l;
            dsf_forward<K>(q, mid, l);
            v = mid;
            total -= l;
        }
    }
    out = v;
    ld = total;
}

// Dynamic LDS: [BLOCK records x PS floats | BLOCK log-dets | D bytes of target mask]
template <int K, bool INVERSE>
__global__ __launch_bounds__(dsf_block(K)) void k_dsf_coupling(
    const float *x, const float *__restrict__ h, float *z, float *logdet, long long N, int D,
    const int *__restrict__ tgt_idx, int T, int T_shift, int C, int PS, int accumulate, int inplace)
{
    constexpr int BLOCK = dsf_block(K);
    const int P = 3 * K * C;
    extern __shared__ __attribute__((aligned(16))) float lds[];
    float *rec = lds;
    float *ld_s = lds + BLOCK * PS;
    unsigned char *is_tgt = reinterpret_cast<unsigned char *>(ld_s + BLOCK);
    const int tid = threadIdx.x;
    const bool use_mask = (tgt_idx != nullptr) && !inplace;
    if (use_mask) {
        for (int e = tid; e < D; e += BLOCK) is_tgt[e] = 0;
        __syncthreads();
        for (int t = tid; t < T; t += BLOCK) is_tgt[tgt_idx[t]] = 1;
    }
    const int R = T <= BLOCK ? BLOCK / T : 1;
    const int chunks = T <= BLOCK ? 1 : (T + BLOCK - 1) / BLOCK;
    const long long n_tiles = (N + R - 1) / R;
    const bool shfl_reduce = (T_shift >= 0) && (T <= kWave);
    // float i of a tile goes to record i / P, slot i % P; a lane's next float is BLOCK further
    const int r_first = tid / P, j_first = tid - r_first * P;
    const int r_step = BLOCK / P, j_step = BLOCK - r_step * P;

    for (long long tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const long long row0 = tile * R;
        const int rows = (int)((N - row0) < (long long)R ? (N - row0) : (long long)R);
        float ld_thread = 0.0f;
        for (int ch = 0; ch < chunks; ++ch) {
            const int cbase = ch * BLOCK;
            const int E = (chunks == 1) ? rows * T : ((T - cbase) < BLOCK ? (T - cbase) : BLOCK);
            const float *src = h + (row0 * (long long)T + cbase) * P;
            __syncthreads();                    // previous tile's readers are done
            int r = r_first, j = j_first;
            for (int i = tid; i < E * P; i += BLOCK) {
                rec[r * PS + j] = nt_load(src + i);                 // h is read once
                r += r_step;
                j += j_step;
                if (j >= P) { j -= P; ++r; }
            }
            __syncthreads();
            float ld = 0.0f;
            long long row = row0;
            int t = cbase + tid;
            if (chunks == 1) {
                const int rr = T_shift >= 0 ? (tid >> T_shift) : (tid / T);
                t = tid - rr * T;
                row = row0 + rr;
            }
            if (tid < E) {
                const int idx = tgt_idx ? tgt_idx[t] : D - T + t;
                const float v = x[row * D + idx];
                float o;
                dsf_eval<K, INVERSE>(rec + tid * PS, C, v, o, ld);
                z[row * D + idx] = o;
            }
            if (chunks > 1) {
                ld_thread += ld;
            } else if (shfl_reduce) {
                const float sum = group_sum(ld, T);
                if (tid < E && t == 0) logdet[row] = accumulate ? logdet[row] + sum : sum;
            } else {
                ld_s[tid] = ld;
                __syncthreads();
                if (tid < rows) {
                    float sum = 0.0f;
                    for (int jj = 0; jj < T; ++jj) sum += ld_s[tid * T + jj];
                    logdet[row0 + tid] = accumulate ? logdet[row0 + tid] + sum : sum;
                }
            }
        }
        if (chunks > 1) {
            __syncthreads();
            ld_s[tid] = ld_thread;
            __syncthreads();
            for (int o = BLOCK / 2; o > 0; o >>= 1) {
                if (tid < o) ld_s[tid] += ld_s[tid + o];
                __syncthreads();
            }
            if (tid == 0) logdet[row0] = accumulate ? logdet[row0] + ld_s[0] : ld_s[0];
        }
        if (!inplace) {                                            // clone, layers_base.py
            const int total = rows * D;
            for (int e = tid; e < total; e += BLOCK) {
                const int rr = e / D;
                const int c = e - rr * D;
                const bool tgt = tgt_idx ? (is_tgt[c] != 0) : (c >= D - T);
                if (!tgt) z[(row0 + rr) * D + c] = x[(row0 + rr) * D + c];
            }
        }
    }
}

// ---------------------------------------------------------------------------------------------
// Reverse mode of the forward direction, recomputed from x and h (what torch.autograd derives from sigmoid.py).
// For one component with input x, A = dL/d out, B = dL/d log-det, D0 = sum_j w_j s_j, s_j = sigmoid(c_j):
//     dL/dD0 = (A + K B) / (d (1 - d)) inside the clip, 0 where it is active
//     dL/dc_j = dL/dD0 w_j s_j (1 - s_j) + B (1 - 2 s_j);   dL/dx = sum_j dL/dc_j a_j
//     dL/da_j = dL/dc_j x + B / a_j;  dL/db_j = dL/dc_j
//     dL/dwp_i = w_i (dL/dD0 s_i - sum_j dL/dD0 s_j w_j) + B (1 - K w_i)       (softmax and log_softmax)
// 1 - d, 1 - s_j and, for D0 above one half, s_j - sum_i w_i s_i are taken from t_j = sigmoid(-c_j) and cd = sum_j w_j t_j
// (dsf_logit), which do not cancel where D0 approaches 1.
// p holds the component's 3 K parameters on entry and their gradients on exit.
// ---------------------------------------------------------------------------------------------
template <int K>
__device__ __forceinline__ float dsf_bwd_comp(float *p, float x, float A, float B)
{
    DsfComp<K> q;
    dsf_extract<K>(p, q);
    float s[K], t[K];                                              // sigmoid(c_j), sigmoid(-c_j)
    float d0 = 0.0f, cd = 0.0f;
#pragma unroll
    for (int j = 0; j < K; ++j) {
        const float c = q.a[j] * x + q.b[j];
        const float e = exp_noovf(-__builtin_fabsf(c));
        const float r = 1.0f / (1.0f + e);
        const float er = e * r;
        s[j] = c >= 0.0f ? r : er;
        t[j] = c >= 0.0f ? er : r;
        d0 += q.w[j] * s[j];
        cd += q.w[j] * t[j];
    }
    const float d = fminf(fmaxf(d0, kDsfEps), kDsfOneMinusEps);
    const bool inside = (d0 >= kDsfEps) && (d0 <= kDsfOneMinusEps);      // clamp passes the gradient on its bounds
    const float g_d0 = inside ? (A + (float)K * B) / (d * dsf_complement(cd)) : 0.0f;      // (dsf_logit: 1 - d)
    // s_j - sum_i s_i w_i, which cancels where one weight is close to 1: from the small side, cd - t_j above one half
    const bool high = d0 > 0.5f;
    float gx = 0.0f;
#pragma unroll
    for (int j = 0; j < K; ++j) {
        const float g_c = g_d0 * q.w[j] * (s[j] * t[j]) + B * (1.0f - 2.0f * s[j]);
        gx += g_c * q.a[j];
        const float g_a = g_c * x + B / q.a[j];
        const float ta = kDsfDefaultUa + div_1000(p[j]);
        const float sp = ta > 20.0f ? 1.0f : 1.0f / (1.0f + exp_noovf(-ta));     // softplus'
        const float g_wp = q.w[j] * (g_d0 * (high ? cd - t[j] : s[j] - d0)) + B * (1.0f - (float)K * q.w[j]);
        p[j] = g_a * sp / 1000.0f;
        p[K + j] = g_c / 1000.0f;
        p[2 * K + j] = g_wp / 1000.0f;
    }
    return gx;
}

// Flat map over the N*T elements, BLOCK per workgroup; records go through LDS at an odd stride with C extra slots that
// keep the inputs of the components, gradients back the same way.
template <int K>
__global__ __launch_bounds__(dsf_block(K)) void k_dsf_coupling_bwd(
    const float *__restrict__ x, const float *__restrict__ h, float *g, const float *__restrict__ gld,
    float *__restrict__ gh, long long N, int D, const int *__restrict__ tgt_idx, int T, int C, int PS)
{
    constexpr int BLOCK = dsf_block(K);
    const int P = 3 * K * C;
    extern __shared__ __attribute__((aligned(16))) float rec[];
    const int tid = threadIdx.x;
    const long long total = N * (long long)T;
    const long long n_tiles = (total + BLOCK - 1) / BLOCK;
    const int r_first = tid / P, j_first = tid - r_first * P;
    const int r_step = BLOCK / P, j_step = BLOCK - r_step * P;
    for (long long tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const long long e0 = tile * BLOCK;
        const int E = (int)((total - e0) < (long long)BLOCK ? (total - e0) : (long long)BLOCK);
        __syncthreads();
        int r = r_first, j = j_first;
        for (int i = tid; i < E * P; i += BLOCK) {
            rec[r * PS + j] = h[e0 * P + i];
            r += r_step;
            j += j_step;
            if (j >= P) { j -= P; ++r; }
        }
        __syncthreads();
        if (tid < E) {
            const long long e = e0 + tid;
            const long long row = e / T;
            const int t = (int)(e - row * T);
            const int idx = tgt_idx ? tgt_idx[t] : D - T + t;
            float *p = rec + tid * PS;
            float v = x[row * D + idx];
            DsfComp<K> q;
            for (int c = 0; c < C; ++c) {                           // the components' inputs
                p[P + c] = v;
                if (c + 1 < C) {
                    dsf_extract<K>(p + c * 3 * K, q);
                    v = dsf_value<K, false>(q, v);
                }
            }
            float A = g[row * D + idx];
            const float B = gld[row];
            for (int c = C - 1; c >= 0; --c) {
                float pc[3 * K];
#pragma unroll
                for (int jj = 0; jj < 3 * K; ++jj) pc[jj] = p[c * 3 * K + jj];
                A = dsf_bwd_comp<K>(pc, p[P + c], A, B);
#pragma unroll
                for (int jj = 0; jj < 3 * K; ++jj) p[c * 3 * K + jj] = pc[jj];
            }
            g[row * D + idx] = A;
        }
        __syncthreads();
        r = r_first;
        j = j_first;
        for (int i = tid; i < E * P; i += BLOCK) {
            gh[e0 * P + i] = rec[r * PS + j];
            r += r_step;
            j += j_step;
            if (j >= P) { j -= P; ++r; }
        }
    }
}

static bool dsf_supported(int C, int K)
{
    return K >= 1 && C >= 1 && ((K <= 16 && C <= 2) || (K <= 8 && C <= 4));
}

static int dsf_check(const char *fn, int64_t N, int32_t D, int32_t T, int32_t C, int32_t K)
{
    if (N < 0) return fail(TFK_EINVAL, "%s: N = %lld < 0", fn, (long long)N);
    if (D < 1 || T < 1 || T > D) return fail(TFK_EINVAL, "%s: need 1 <= T <= D (T = %d, D = %d)", fn, T, D);
    if (!dsf_supported(C, K))
        return fail(TFK_EINVAL, "%s: n_components = %d, hidden_dim = %d (kernels exist for hidden_dim <= 16 with <= 2 "
                    "components and hidden_dim <= 8 with <= 4: tfk_dsf_supported)", fn, C, K);
    return TFK_OK;
}

#define TFK_DSF_FOR_EACH_K(X) \
    X(1) X(2) X(3) X(4) X(5) X(6) X(7) X(8) X(9) X(10) X(11) X(12) X(13) X(14) X(15) X(16)

template <bool INVERSE>
static int dsf_coupling(const float *x, const float *h, float *z, float *logdet, int64_t N, int32_t D,
                        const int32_t *tgt_idx, int32_t T, int32_t C, int32_t K, int32_t accumulate,
                        void *stream, const char *fn)
{
    if (const int rc = dsf_check(fn, N, D, T, C, K)) return rc;
    if (N == 0) return TFK_OK;
    if (!x || !h || !z || !logdet) return fail(TFK_EINVAL, "%s: null pointer", fn);
    const bool inplace = (x == z);
    int T_shift = -1;
    if ((T & (T - 1)) == 0) {
        T_shift = 0;
        while ((1 << T_shift) < T) ++T_shift;
    }
    const int BLOCK = dsf_block(K);
    const int P = 3 * K * C, PS = P | 1;
    const int R = T <= BLOCK ? BLOCK / T : 1;
    const int64_t n_tiles = (N + R - 1) / R;
    const size_t lds = ((size_t)BLOCK * PS + BLOCK) * sizeof(float) + ((tgt_idx && !inplace) ? (size_t)D : 0);
    if (lds > 64 * 1024)
        return fail(TFK_EINVAL, "%s: an index list over D = %d columns does not fit the workgroup's LDS", fn, D);
    int per_cu = (int)((160 * 1024) / lds);
    if (per_cu > 8) per_cu = 8;
    const int64_t grid = n_tiles < (int64_t)cu_count() * per_cu ? n_tiles : (int64_t)cu_count() * per_cu;
    hipStream_t s = static_cast<hipStream_t>(stream);
    switch (K) {
#define TFK_DSF_CASE(K_)                                                                                          \
    case K_:                                                                                                      \
        hipLaunchKernelGGL((k_dsf_coupling<K_, INVERSE>), dim3((unsigned)grid), dim3(dsf_block(K_)), lds, s, x, h, z, \
                           logdet, (long long)N, D, tgt_idx, T, T_shift, C, PS, accumulate, inplace ? 1 : 0);     \
        break;
        TFK_DSF_FOR_EACH_K(TFK_DSF_CASE)
#undef TFK_DSF_CASE
    }
    return check_launch(fn);
}

}  // namespace tfk

extern "C" {

int tfk_dsf_supported(int32_t n_components, int32_t hidden_dim)
{
    return tfk::dsf_supported(n_components, hidden_dim) ? 1 : 0;
}

int tfk_dsf_coupling_fwd(const float *x, const float *h, float *z, float *logdet, int64_t N, int32_t D,
                         const int32_t *tgt_idx, int32_t T, int32_t n_components, int32_t hidden_dim,
                         int32_t accumulate, void *stream)
{
    return tfk::dsf_coupling<false>(x, h, z, logdet, N, D, tgt_idx, T, n_components, hidden_dim, accumulate, stream,
                                    "tfk_dsf_coupling_fwd");
}

int tfk_dsf_coupling_inv(const float *z, const float *h, float *x, float *logdet, int64_t N, int32_t D,
                         const int32_t *tgt_idx, int32_t T, int32_t n_components, int32_t hidden_dim,
                         int32_t accumulate, void *stream)
{
    return tfk::dsf_coupling<true>(z, h, x, logdet, N, D, tgt_idx, T, n_components, hidden_dim, accumulate, stream,
                                   "tfk_dsf_coupling_inv");
}

int tfk_dsf_coupling_bwd(const float *x, const float *h, float *g, const float *gld, float *gh,
                         int64_t N, int32_t D, const int32_t *tgt_idx, int32_t T, int32_t n_components,
                         int32_t hidden_dim, int32_t inverse, void *stream)
{
    using namespace tfk;
    const char *fn = "tfk_dsf_coupling_bwd";
    const int C = n_components, K = hidden_dim;
    if (const int rc = dsf_check(fn, N, D, T, C, K)) return rc;
    if (inverse)
        return fail(TFK_EINVAL, "%s: the inverse direction is a bisection without gradient; differentiate it on the ATen "
                    "path", fn);
    if (N == 0) return TFK_OK;
    if (!x || !h || !g || !gld || !gh) return fail(TFK_EINVAL, "%s: null pointer", fn);
    const int BLOCK = dsf_block(K);
    const int PS = (3 * K * C + C) | 1;
    const size_t lds = (size_t)BLOCK * PS * sizeof(float);
    const int64_t n_tiles = (N * (int64_t)T + BLOCK - 1) / BLOCK;
    int per_cu = (int)((160 * 1024) / lds);
    if (per_cu > 8) per_cu = 8;
    const int grid = (int)(n_tiles < (int64_t)cu_count() * per_cu ? n_tiles : (int64_t)cu_count() * per_cu);
    hipStream_t s = static_cast<hipStream_t>(stream);
    switch (K) {
#define TFK_DSF_CASE(K_)                                                                                          \
    case K_:                                                                                                      \
        hipLaunchKernelGGL((k_dsf_coupling_bwd<K_>), dim3(grid), dim3(dsf_block(K_)), lds, s, x, h, g, gld, gh,   \
                           (long long)N, D, tgt_idx, T, C, PS);                                                   \
        break;
        TFK_DSF_FOR_EACH_K(TFK_DSF_CASE)
#undef TFK_DSF_CASE
    }
    return check_launch(fn);
}

}  // extern "C"
