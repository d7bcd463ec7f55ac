// tfk_dsf.h -- the arithmetic of one deep sigmoidal component (transformers/combination/sigmoid.py), shared by the
// coupling kernels that read their parameters from HBM (tfk_dsf.hip) and the image kernel that makes them on the matrix
// cores (tfk_glow_dsf.hip); below it the pieces of a coupling tile (target mask, per-row log-det, pass-through copy) that
// tfk_dsf.hip shares with the dense sigmoidal kernel (tfk_dense_dsf.hip).  Per element a component takes 3 K parameters [da (K) | db (K) | dw (K)]:
//     a = softplus(log(e - 1 - 1e-3) + da / 1000) + 1e-3,  b = db / 1000,  w = softmax(dw / 1000)
//     d = clip(sum_j w_j sigmoid(a_j x + b_j), 1e-6, 1 - 1e-6),  z = log d - log1p(-d)      (1 - d: dsf_logit below)
//     log-det (as the reference has it) = K (log d - log(1 - d)) + sum_j [log w_j + log a_j + log sigmoid(c_j) + log sigmoid(-c_j)]
#pragma once

#include "tfk_common.h"
#include "tfk_spline.h"

namespace tfk {

constexpr int kDsfMaxTrips = 64;            // 20 * 2^-64 is far below one ulp of any fp32 midpoint
constexpr float kDsfEps = 1e-6f;            // the clip of d (python doubles rounded once to fp32, as ATen does)
constexpr float kDsfOneMinusEps = (float)(1.0 - 1e-6);
constexpr float kDsfMinScale = 1e-3f;
constexpr float kDsfDefaultUa = 0.5407427084918718f;     // log(e - 1 - 1e-3)

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

// One element through one extracted component, either way: v becomes its image (forward) or its pre-image (inverse: the
// reference's bisection on [-10, 10], bracket moved on f(c) < y, result = the last midpoint, until the fp32 midpoint
// stops moving and at most kDsfMaxTrips times); total gains the log-det, minus the forward one at the returned x for the
// inverse.
template <int K, bool INVERSE>
__device__ __forceinline__ void dsf_step(const DsfComp<K> &q, float &v, float &total)
{
    float l;
    if (!INVERSE) {
        v = dsf_forward<K>(q, v, l);
        total += l;
    } else {
        float lo = -10.0f, hi = 10.0f, mid = 0.0f;
        for (int it = 0; it < kDsfMaxTrips; ++it) {                 // numerical_inversion.py: bisection_no_gradient
            const bool below = dsf_value<K, true>(q, mid) < v;
            lo = below ? mid : lo;
            hi = below ? hi : mid;
            const float next = (lo + hi) / 2.0f;
            const bool done = (next == mid);
            mid = next;
            if (done) break;
        }
        dsf_forward<K>(q, mid, l);
        v = mid;
        total -= l;
    }
}

// ---- a coupling tile: `block` lanes, one element each, R = block / T rows per tile (rows longer than a tile: in chunks) ----

// is_tgt[c] = column c is transformed (the pass-through copy leaves it alone)
__device__ __forceinline__ void dsf_mark_targets(unsigned char *is_tgt, const int *__restrict__ tgt_idx, int T, int D, int block)
{
    const int tid = threadIdx.x;
    for (int e = tid; e < D; e += block) is_tgt[e] = 0;
    __syncthreads();
    for (int t = tid; t < T; t += block) is_tgt[tgt_idx[t]] = 1;
}

// Per-row log-det of a tile of whole rows: inside the T-lane group (T a power of two <= 64) or through ld_s (block floats).
// `first`: this lane holds element 0 of a live row `row`.  Every lane of the workgroup calls it.
__device__ __forceinline__ void dsf_row_logdet(float ld, float *ld_s, float *logdet, long long row0, long long row, int rows,
                                               int T, bool first, bool shfl_reduce, int accumulate)
{
    const int tid = threadIdx.x;
    if (shfl_reduce) {
        const float sum = group_sum(ld, T);
        if (first) logdet[row] = accumulate ? logdet[row] + sum : sum;
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

// ... of ONE row longer than the tile: the lanes' sums over its chunks, added in a tree (block: a power of two)
__device__ __forceinline__ void dsf_long_row_logdet(float ld_thread, float *ld_s, float *logdet, long long row0, int block,
                                                    int accumulate)
{
    const int tid = threadIdx.x;
    __syncthreads();
    ld_s[tid] = ld_thread;
    __syncthreads();
    for (int o = block / 2; o > 0; o >>= 1) {
        if (tid < o) ld_s[tid] += ld_s[tid + o];
        __syncthreads();
    }
    if (tid == 0) logdet[row0] = accumulate ? logdet[row0] + ld_s[0] : ld_s[0];
}

// the columns that are no targets, copied (clone, layers_base.py); is_tgt: dsf_mark_targets, unused for a tail (no tgt_idx)
__device__ __forceinline__ void dsf_copy_passthrough(const float *x, float *z, long long row0, int rows, int D, int T,
                                                     const int *tgt_idx, const unsigned char *is_tgt, int block)
{
    const int total = rows * D;
    for (int e = threadIdx.x; e < total; e += block) {
        const int rr = e / D;
        const int c = e - rr * D;
        const bool tgt = tgt_idx ? (is_tgt[c] != 0) : (c >= D - T);
        if (!tgt) z[(row0 + rr) * D + c] = x[(row0 + rr) * D + c];
    }
}

// ---- the dense sigmoidal family (tfk_dense_dsf.hip) behind tfk_dsf_supported / tfk_dsf_coupling_fwd / _inv: n_components
// carries C | (L + 1) << 8 (include/tfk.h) ----
inline bool dsf_is_dense(int32_t n_components) { return (n_components >> 8) != 0; }
bool dense_dsf_supported(int32_t n_components, int32_t hidden);
int dense_dsf_coupling(bool inverse, const float *x, const float *pred, float *z, float *logdet, int64_t N, int32_t D,
                       const int32_t *desc, int32_t T, int32_t n_components, int32_t hidden, int32_t accumulate,
                       void *stream, const char *fn);
// ... and behind tfk_dsf_coupling_bwd: gh = [dL/dbase (T CP) | kDenseBwdSlices x T CP of workspace | dL/dpred (N stride)]
constexpr int kDenseBwdSlices = 256;        // the most workgroups the reverse-mode launch runs (include/tfk.h states it)
int dense_dsf_coupling_bwd(const float *x, const float *pred, float *g, const float *gld, float *gh, int64_t N, int32_t D,
                           const int32_t *desc, int32_t T, int32_t n_components, int32_t hidden, int32_t inverse,
                           void *stream, const char *fn);

// the (C, K) the coupling kernels of tfk_dsf.hip and the sequential MADE kernel of tfk_made_dsf.hip are instantiated for
inline bool dsf_supported(int C, int K) { return K >= 1 && C >= 1 && ((K <= 16 && C <= 2) || (K <= 8 && C <= 4)); }

// ---- the sequential map of a MADE-based deep sigmoidal layer (tfk_made_dsf.hip) behind tfk_made_rqs_sequential /
// tfk_made_rqs_sequential_lds_bytes: n_bins carries 1 << 16 | C << 8 | K (include/tfk.h) ----
inline bool made_is_dsf(int32_t n_bins) { return (n_bins >> 16) == 1; }
int64_t made_dsf_sequential_lds_bytes(int32_t D, int32_t hidden_padded, int32_t code);
int made_dsf_sequential(const float *z, float *x, float *logdet, int64_t N, int32_t D, const float *W1t, const float *b1,
                        const float *W2, const float *b2, int32_t hidden_padded, int32_t code, float boundary,
                        int32_t accumulate, void *stream, const char *fn);

}  // namespace tfk
