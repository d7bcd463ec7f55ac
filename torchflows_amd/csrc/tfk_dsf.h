// tfk_dsf.h -- the arithmetic of one deep sigmoidal component (transformers/combination/sigmoid.py), shared by the
// coupling kernels that read their parameters from HBM (tfk_dsf.hip) and the image kernel that makes them on the matrix
// cores (tfk_glow_dsf.hip).  Per element a component takes 3 K parameters [da (K) | db (K) | dw (K)]:
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

}  // namespace tfk
