// tfk_dense_dsf.hip -- dense sigmoidal flow coupling (Huang et al. 2018): DenseSigmoid / DeepDenseSigmoid
// (transformers/combination/dense_sigmoid.py) inside CouplingBijection / MaskedAutoregressiveBijection, both directions, behind
// tfk_dsf_coupling_fwd / _inv with n_components = C | (L + 1) << 8 (include/tfk.h).
//
// Per element a component is L + 2 inner transforms (i inputs -> o outputs): 1 -> H, L x (H -> H), H -> 1, each taking
// [da (o) | db (o) | dw (o o) | du (o i)]:
//     u = softmax_rows(du / 1000)  a = softplus(log(e - 1 - 1e-3) + da / 1000) + 1e-3  b = db / 1000  w = softmax_rows(dw / 1000)
//     c_j = a_j (u_j . v) + b_j     d_p = clip(sum_j w_pj sigmoid(c_j), 1e-6, 1 - 1e-6)     v'_p = log d_p - log(1 - d_p)
//     log-det (as the reference has it: the SUM of log_dot(m1, log u) over all its entries)
//         = i o [sum_p v'_p + sum_j (log sigmoid(c_j) + log sigmoid(-c_j))]                            (depends on x)
//         + i [sum_pj log w_pj + o sum_j log a_j] + o^2 sum_k log sum_l u_lk                           (does not)
// The first transform has i = 1: u = 1 whatever du holds, and the last term is o^2 log o.
//   * the parameter tensor h (N, T, C P) is never materialised: the launch takes the conditioner's predicted block
//     (N, stride) and a descriptor [col (T C P) | base (T C P)] -- record entry j of target t is pred[n, col] where
//     col >= 0 and the learned constant base otherwise -- and composes the records while it fills the LDS (predicted columns
//     ascend with (t, j): consecutive lanes read ascending addresses, non-temporal);
//   * one lane = one element = one record of C P floats at an odd stride (conflict-free per-lane reads);  the lane turns
//     its record into (a, b, w, u) IN PLACE, one softmax row at a time (H template parameter: a row sits in registers),
//     and folds every x-independent log-det term of all components into one scalar;
//   * one evaluation of a transform is then two small mat-vecs from LDS, o sigmoids and o logits; the inverse is the
//     reference's bisection per component, last to first (tfk_dsf.h: dsf_step), values only, the log-det once at the result;
//   * lanes per workgroup: the largest of 256 / 128 / 64 whose records fit the 160 KB LDS; tiles, chunks, log-det
//     reduction and pass-through copy are those of k_dsf_coupling (tfk_dsf.h);
//   * no matrix instructions: every element has its own u and w, there is no operand two elements share.
#include <math.h>

#include "tfk_dsf.h"

namespace tfk {

constexpr int kDenseMaxFloats = 512;        // C P: the record of one element
constexpr size_t kDenseLdsBytes = 160 * 1024;

__host__ __device__ constexpr int dense_p_first(int H) { return H * H + 3 * H; }         // 1 -> H
__host__ __device__ constexpr int dense_p_mid(int H) { return 2 * H * H + 2 * H; }       // H -> H
__host__ __device__ constexpr int dense_p_last(int H) { return H + 3; }                  // H -> 1
static int dense_p(int H, int L) { return dense_p_first(H) + L * dense_p_mid(H) + dense_p_last(H); }

// softmax of r[0..M) / 1000 in place (dsf_extract's form); returns sum_j log softmax_j; col (or null) gains the row
template <int M>
__device__ __forceinline__ float dense_softmax_row(float *r, float *col)
{
    float wp[M], e[M];
    float m = 0.0f;
#pragma unroll
    for (int j = 0; j < M; ++j) {
        wp[j] = 0.0f + div_1000(r[j]);
        m = j ? fmaxf(m, wp[j]) : wp[j];
    }
    float s = 0.0f;
#pragma unroll
    for (int j = 0; j < M; ++j) {
        e[j] = exp_noovf(wp[j] - m);
        s += e[j];
    }
    const float inv = 1.0f / s;
    const float lse = m + log_normal(s);
    float lsum = 0.0f;
#pragma unroll
    for (int j = 0; j < M; ++j) {
        const float v = e[j] * inv;
        r[j] = v;
        if (col) col[j] += v;
        lsum += wp[j] - lse;
    }
    return lsum;
}

// One inner transform's raw parameters -> (a, b, w, u) in place; returns its x-independent log-det term.
template <int I, int O>
__device__ __forceinline__ float dense_extract(float *q)
{
    float la = 0.0f;
#pragma unroll
    for (int j = 0; j < O; ++j) {
        const float a = softplus20(kDsfDefaultUa + div_1000(q[j])) + kDsfMinScale;
        q[j] = a;
        la += log_normal(a);
        q[O + j] = div_1000(q[O + j]);
    }
    float lw = 0.0f;
    if (O > 1) {                                                   // (a 1 x 1 softmax is 1, its log 0: never read)
        for (int p = 0; p < O; ++p) lw += dense_softmax_row<O>(q + 2 * O + p * O, nullptr);
    }
    float lu;
    if (I == 1) {
        lu = (float)(O * O) * __builtin_logf((float)O);            // u = 1: o rows of log 1 (folded at compile time)
    } else {
        float col[I];
#pragma unroll
        for (int k = 0; k < I; ++k) col[k] = 0.0f;
        for (int j = 0; j < O; ++j) dense_softmax_row<I>(q + 2 * O + O * O + j * I, col);
        lu = 0.0f;
#pragma unroll
        for (int k = 0; k < I; ++k) lu += log_normal(fmaxf(col[k], 1.17549435e-38f));    // log sum_l u_lk
        lu *= (float)(O * O);
    }
    return (float)I * (lw + (float)O * la) + lu;
}

// One extracted inner transform: vin[I] -> vout[O]; WITH_LD: ld gains the x-dependent part of its log-det.
// LEAN: the bisection's loop body (tfk_dsf.h: dsf_value).
template <int I, int O, bool WITH_LD, bool LEAN>
__device__ __forceinline__ void dense_inner(const float *q, const float *vin, float *vout, float &ld)
{
    float s[O], t[O];
    float t3 = 0.0f;
#pragma unroll
    for (int j = 0; j < O; ++j) {
        float ux = vin[0];
        if (I > 1) {
            ux = 0.0f;
#pragma unroll
            for (int k = 0; k < I; ++k) ux += q[2 * O + O * O + j * I + k] * vin[k];
        }
        const float c = q[j] * ux + q[O + j];
        const float ac = __builtin_fabsf(c);
        const float e = LEAN ? exp_lean(-ac) : exp_noovf(-ac);
        const float r = div_fast(1.0f, 1.0f + e);
        const float er = e * r;
        s[j] = c >= 0.0f ? r : er;
        t[j] = c >= 0.0f ? er : r;                                  // sigmoid(-c)
        if (WITH_LD) t3 -= ac + 2.0f * log1p_pos(e);                // log sigmoid(c) + log sigmoid(-c)
    }
    float sl = 0.0f;
#pragma unroll
    for (int p = 0; p < O; ++p) {
        float d = s[0], cd = t[0];
        if (O > 1) {
            d = 0.0f;
            cd = 0.0f;
#pragma unroll
            for (int j = 0; j < O; ++j) {
                const float w = q[2 * O + p * O + j];
                d += w * s[j];
                cd += w * t[j];
            }
        }
        float lg, lc;
        vout[p] = dsf_logit(d, cd, lg, lc);
        sl += vout[p];
    }
    if (WITH_LD) ld += (float)(I * O) * (sl + t3);
}

// All of an element's components, raw -> extracted in place; returns the folded x-independent log-det.
template <int H>
__device__ __forceinline__ float dense_extract_record(float *q, int C, int L)
{
    float cst = 0.0f;
    for (int c = 0; c < C; ++c) {
        cst += dense_extract<1, H>(q);
        q += dense_p_first(H);
        for (int l = 0; l < L; ++l) {
            cst += dense_extract<H, H>(q);
            q += dense_p_mid(H);
        }
        cst += dense_extract<H, 1>(q);
        q += dense_p_last(H);
    }
    return cst;
}

// One extracted component at x
template <int H, bool WITH_LD, bool LEAN>
__device__ __forceinline__ float dense_comp(const float *q, int L, float x, float &ld)
{
    float v[H], w[H];
    dense_inner<1, H, WITH_LD, LEAN>(q, &x, v, ld);
    q += dense_p_first(H);
    for (int l = 0; l < L; ++l) {
        dense_inner<H, H, WITH_LD, LEAN>(q, v, w, ld);
#pragma unroll
        for (int j = 0; j < H; ++j) v[j] = w[j];
        q += dense_p_mid(H);
    }
    float out;
    dense_inner<H, 1, WITH_LD, LEAN>(q, v, &out, ld);
    return out;
}

// One element through its C extracted components (P floats each): forward first to last; inverse last to first, each by
// the bisection of dsf_step.  ld: the x-dependent log-det, negated for the inverse.
template <int H, bool INVERSE>
__device__ __forceinline__ float dense_eval(const float *q, int C, int L, int P, float v, float &ld)
{
    float total = 0.0f;
    for (int i = 0; i < C; ++i) {
        const float *qc = q + (INVERSE ? C - 1 - i : i) * P;
        if (!INVERSE) {
            v = dense_comp<H, true, false>(qc, L, v, total);
        } else {
            float unused = 0.0f;
            float lo = -10.0f, hi = 10.0f, mid = 0.0f;
            for (int it = 0; it < kDsfMaxTrips; ++it) {             // numerical_inversion.py: bisection_no_gradient
                const bool below = dense_comp<H, false, true>(qc, L, mid, unused) < v;
                lo = below ? mid : lo;
                hi = below ? hi : mid;
                const float next = (lo + hi) / 2.0f;
                const bool done = (next == mid);
                mid = next;
                if (done) break;
            }
            float l = 0.0f;
            dense_comp<H, true, false>(qc, L, mid, l);
            v = mid;
            total -= l;
        }
    }
    ld = total;
    return v;
}

// desc: [T target columns | stride | col (T CP) | base (T CP, float bits)].
// Dynamic LDS: [block records x PS floats | block log-dets | D bytes of target mask]; block = blockDim.x.
template <int H, bool INVERSE>
__global__ __launch_bounds__(256) void k_dense_dsf_coupling(
    const float *x, const float *__restrict__ pred, float *z, float *logdet, long long N, int D,
    const int *__restrict__ desc, int T, int T_shift, int C, int L, int P, int PS, int accumulate, int inplace)
{
    const int block = blockDim.x;
    const int CP = C * P;
    extern __shared__ __attribute__((aligned(16))) float lds[];
    float *rec = lds;
    float *ld_s = lds + block * PS;
    unsigned char *is_tgt = reinterpret_cast<unsigned char *>(ld_s + block);
    const int *tgt_idx = desc;
    const long long stride = desc[T];
    const int *col = desc + T + 1;
    const float *base = reinterpret_cast<const float *>(col + (long long)T * CP);
    const int tid = threadIdx.x;
    if (!inplace) dsf_mark_targets(is_tgt, tgt_idx, T, D, block);
    const int R = T <= block ? block / T : 1;
    const int chunks = T <= block ? 1 : (T + block - 1) / block;
    const long long n_tiles = (N + R - 1) / R;
    const bool shfl_reduce = (T_shift >= 0) && (T <= kWave);
    // float i of a tile goes to record r = i / CP, slot j = i % CP; record r is target t = r % T of row r / T; a lane's
    // next float is `block` further
    const int r_first = tid / CP, j_first = tid - r_first * CP;
    const int r_step = block / CP, j_step = block - r_step * CP;
    const int rr_first = r_first / T, t_first = r_first - rr_first * T;
    const int rr_step = r_step / T, t_step = r_step - rr_step * T;

    for (long long tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const long long row0 = tile * R;
        const int rows = (int)((N - row0) < (long long)R ? (N - row0) : (long long)R);
        float ld_thread = 0.0f;
        for (int ch = 0; ch < chunks; ++ch) {
            const int cbase = ch * block;
            const int E = (chunks == 1) ? rows * T : ((T - cbase) < block ? (T - cbase) : block);
            __syncthreads();                    // previous tile's readers are done
            int r = r_first, j = j_first, rr = rr_first, t = cbase + t_first;
            for (int i = tid; i < E * CP; i += block) {
                const int dj = t * CP + j;
                const int cc = col[dj];
                rec[r * PS + j] = cc >= 0 ? nt_load(pred + (row0 + rr) * stride + cc) : base[dj];
                r += r_step;
                rr += rr_step;
                t += t_step;
                j += j_step;
                if (j >= CP) { j -= CP; ++r; ++t; }
                if (chunks == 1 && t >= T) { t -= T; ++rr; }
            }
            __syncthreads();
            float ld = 0.0f;
            long long row = row0;
            int te = cbase + tid;
            if (chunks == 1) {
                const int re = T_shift >= 0 ? (tid >> T_shift) : (tid / T);
                te = tid - re * T;
                row = row0 + re;
            }
            if (tid < E) {
                float *q = rec + tid * PS;
                const float cst = dense_extract_record<H>(q, C, L);
                const int idx = tgt_idx[te];
                const float v = x[row * D + idx];
                z[row * D + idx] = dense_eval<H, INVERSE>(q, C, L, P, v, ld);
                ld = INVERSE ? ld - cst : ld + cst;
            }
            if (chunks > 1) ld_thread += ld;
            else dsf_row_logdet(ld, ld_s, logdet, row0, row, rows, T, tid < E && te == 0, shfl_reduce, accumulate);
        }
        if (chunks > 1) dsf_long_row_logdet(ld_thread, ld_s, logdet, row0, block, accumulate);
        if (!inplace) dsf_copy_passthrough(x, z, row0, rows, D, T, tgt_idx, is_tgt, block);
    }
}

bool dense_dsf_supported(int32_t n_components, int32_t hidden)
{
    const int C = n_components & 0xff, L = (n_components >> 8) - 1, H = hidden;
    return H >= 1 && H <= 8 && L >= 0 && L <= 2 && C >= 1 && C <= 2 && C * dense_p(H, L) <= kDenseMaxFloats;
}

#define TFK_DENSE_FOR_EACH_H(X) X(1) X(2) X(3) X(4) X(5) X(6) X(7) X(8)

template <bool INVERSE>
static int dense_launch(const float *x, const float *pred, float *z, float *logdet, int64_t N, int32_t D,
                        const int32_t *desc, int32_t T, int32_t C, int32_t L, int32_t H, int32_t accumulate,
                        void *stream, const char *fn)
{
    const bool inplace = (x == z);
    int T_shift = -1;
    if ((T & (T - 1)) == 0) {
        T_shift = 0;
        while ((1 << T_shift) < T) ++T_shift;
    }
    const int P = dense_p(H, L), PS = (C * P) | 1;
    int block = 256;
    size_t lds = 0;
    for (; block >= 64; block >>= 1) {
        lds = ((size_t)block * PS + block) * sizeof(float) + (inplace ? 0 : (size_t)D);
        if (lds <= kDenseLdsBytes) break;
    }
    if (block < 64)
        return fail(TFK_EINVAL, "%s: a target mask over D = %d columns does not fit the workgroup's LDS", fn, D);
    const int R = T <= block ? block / T : 1;
    const int64_t n_tiles = (N + R - 1) / R;
    int per_cu = (int)(kDenseLdsBytes / lds);
    if (per_cu > 8) per_cu = 8;
    const int64_t grid = n_tiles < (int64_t)cu_count() * per_cu ? n_tiles : (int64_t)cu_count() * per_cu;
    hipStream_t s = static_cast<hipStream_t>(stream);
    switch (H) {
#define TFK_DENSE_CASE(H_)                                                                                          \
    case H_: {                                                                                                      \
        auto kern = &k_dense_dsf_coupling<H_, INVERSE>;                                                             \
        if (lds > 64 * 1024 && hipFuncSetAttribute(reinterpret_cast<const void *>(kern),                            \
                                                   hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess) { \
            (void)hipGetLastError();                                                                                \
            return fail(TFK_ELAUNCH, "%s: cannot reserve %zu bytes of LDS", fn, lds);                               \
        }                                                                                                           \
        hipLaunchKernelGGL(kern, dim3((unsigned)grid), dim3(block), lds, s, x, pred, z, logdet, (long long)N, D, desc, T, \
                           T_shift, C, L, P, PS, accumulate, inplace ? 1 : 0);                                      \
    } break;
        TFK_DENSE_FOR_EACH_H(TFK_DENSE_CASE)
#undef TFK_DENSE_CASE
    }
    return check_launch(fn);
}

int dense_dsf_coupling(bool inverse, const float *x, const float *pred, float *z, float *logdet, int64_t N, int32_t D,
                       const int32_t *desc, int32_t T, int32_t n_components, int32_t hidden, int32_t accumulate,
                       void *stream, const char *fn)
{
    if (N < 0) return fail(TFK_EINVAL, "%s: N = %lld < 0", fn, (long long)N);
    if (D < 1 || T < 1 || T > D) return fail(TFK_EINVAL, "%s: need 1 <= T <= D (T = %d, D = %d)", fn, T, D);
    if (!dense_dsf_supported(n_components, hidden))
        return fail(TFK_EINVAL, "%s: dense sigmoidal kernels exist for 1 <= hidden size <= 8, 0 <= dense layers <= 2, 1 or 2 "
                    "components and at most %d parameters per element (n_components = 0x%x, hidden_dim = %d)", fn,
                    kDenseMaxFloats, (unsigned)n_components, hidden);
    if (N == 0) return TFK_OK;
    if (!x || !z || !logdet || !desc)                              // (pred may be null: every parameter a learned constant)
        return fail(TFK_EINVAL, "%s: null pointer (the dense family always takes its descriptor block in tgt_idx)", fn);
    const int C = n_components & 0xff, L = (n_components >> 8) - 1;
    return inverse ? dense_launch<true>(x, pred, z, logdet, N, D, desc, T, C, L, hidden, accumulate, stream, fn)
                   : dense_launch<false>(x, pred, z, logdet, N, D, desc, T, C, L, hidden, accumulate, stream, fn);
}

// ---------------------------------------------------------------------------------------------
// Reverse mode of the forward map, recomputed from x, the predicted block and the descriptor (what torch.autograd derives
// from dense_sigmoid.py).  For one inner transform (i inputs v, o outputs), A_p = dL/dv'_p, B = dL/dlog-det:
//     G_p     = dL/dD0_p = (A_p + i o B) / (d_p (1 - d_p)) inside the clip, 0 where it is active (ATen's clamp)
//     dL/dc_j = (sum_p G_p w_pj) s_j (1 - s_j) + i o B (1 - 2 s_j)
//     dL/da_j = dL/dc_j (u_j . v) + i o B / a_j       dL/db_j = dL/dc_j
//     dL/dwp_pj = w_pj G_p (s_j - D0_p) + i B (1 - o w_pj)                                  (softmax and log_softmax of row p)
//     dL/du_jk = dL/dc_j a_j v_k + o^2 B / sum_l u_lk;   dL/dup_jk = u_jk (dL/du_jk - sum_m dL/du_jm u_jm)    (i > 1)
//     dL/dv_k = sum_j dL/dc_j a_j u_jk
// and raw parameters are the pre-activations x 1000: da gains softplus' = 1 - exp(-(a - 1e-3)), everything 1 / 1000.
// 1 - d, 1 - s and s_j - D0_p above one half come from the complements, as in dsf_bwd_comp (tfk_dsf.hip).
//   * the forward kernel's layout: one lane = one element, its record of C P floats in the LDS at an odd stride, extracted
//     in place; a component's L + 1 hidden activations are recomputed once into registers, then its transforms are walked
//     last to first and the gradient of every raw parameter OVERWRITES the extracted one it belongs to (a softmax row's
//     backward needs the row and its gradient only);
//   * dL/dpred: the record floats with col >= 0 go back the way they came, plain stores -- the descriptor names every
//     predicted column at most once (layers_base.py: _dense_inputs).  Columns it does not name are NOT written: the
//     caller zero-fills dL/dpred (native.dense_coupling_bwd);
//   * dL/dbase: the tile's records still lie in the LDS; lane i sums entries dj = i (mod block) over the tile's rows in row
//     order and adds the sum to slice blockIdx.x of the workspace, tile after tile (a persistent workgroup; the same
//     lane owns dj throughout, so the slice needs no synchronisation).  k_dense_bwd_sum then adds the slices in slice
//     order: no atomics, two calls give the same bits.
// ---------------------------------------------------------------------------------------------
template <int I, int O>
__device__ __forceinline__ void dense_inner_bwd(float *q, const float *vin, const float *A, float B, float *gv)
{
    constexpr float IO = (float)(I * O);
    constexpr int W0 = 2 * O, U0 = 2 * O + O * O;
    float s[O], t[O], ux[O], gs[O];
#pragma unroll
    for (int j = 0; j < O; ++j) {
        float u = vin[0];
        if (I > 1) {
            u = 0.0f;
#pragma unroll
            for (int k = 0; k < I; ++k) u += q[U0 + j * I + k] * vin[k];
        }
        ux[j] = u;
        const float c = q[j] * u + q[O + j];
        const float e = exp_noovf(-__builtin_fabsf(c));
        const float r = 1.0f / (1.0f + e);
        const float er = e * r;
        s[j] = c >= 0.0f ? r : er;
        t[j] = c >= 0.0f ? er : r;
        gs[j] = 0.0f;
    }
#pragma unroll
    for (int p = 0; p < O; ++p) {
        float d0 = s[0], cd = t[0];
        if (O > 1) {
            d0 = 0.0f;
            cd = 0.0f;
#pragma unroll
            for (int j = 0; j < O; ++j) {
                const float w = q[W0 + p * O + j];
                d0 += w * s[j];
                cd += w * t[j];
            }
        }
        const float d = fminf(fmaxf(d0, kDsfEps), kDsfOneMinusEps);
        const bool inside = (d0 >= kDsfEps) && (d0 <= kDsfOneMinusEps);      // clamp passes the gradient on its bounds
        const float G = inside ? (A[p] + IO * B) / (d * dsf_complement(cd)) : 0.0f;
        if (O > 1) {
            const bool high = d0 > 0.5f;
#pragma unroll
            for (int j = 0; j < O; ++j) {
                const float w = q[W0 + p * O + j];
                gs[j] += G * w;
                q[W0 + p * O + j] = (w * (G * (high ? cd - t[j] : s[j] - d0)) + B * ((float)I * (1.0f - (float)O * w))) / 1000.0f;
            }
        } else {
            gs[0] += G;
            q[W0] = 0.0f;                                           // (a 1 x 1 softmax is constant)
        }
    }
    float colsum[I];                                               // sum_l u_lk, then o^2 B over it
#pragma unroll
    for (int k = 0; k < I; ++k) {
        colsum[k] = 0.0f;
        gv[k] = 0.0f;
    }
    if (I > 1) {
#pragma unroll
        for (int j = 0; j < O; ++j) {
#pragma unroll
            for (int k = 0; k < I; ++k) colsum[k] += q[U0 + j * I + k];
        }
#pragma unroll
        for (int k = 0; k < I; ++k) colsum[k] = B * (float)(O * O) / fmaxf(colsum[k], 1.17549435e-38f);
    }
#pragma unroll
    for (int j = 0; j < O; ++j) {
        const float g_c = gs[j] * (s[j] * t[j]) + IO * B * (t[j] - s[j]);
        const float a = q[j];
        const float g_ux = g_c * a;
        const float sp = 1.0f - exp_noovf(kDsfMinScale - a);        // softplus' = sigmoid = 1 - exp(-softplus)
        q[j] = (g_c * ux[j] + IO * B / a) * sp / 1000.0f;
        q[O + j] = g_c / 1000.0f;
        if (I == 1) {
            gv[0] += g_ux;
            q[U0 + j] = 0.0f;                                       // (u = 1 whatever du holds)
        } else {
            float gu[I];
            float dot = 0.0f;
#pragma unroll
            for (int k = 0; k < I; ++k) {
                const float u = q[U0 + j * I + k];
                gu[k] = g_ux * vin[k] + colsum[k];
                dot += gu[k] * u;
                gv[k] += g_ux * u;
            }
#pragma unroll
            for (int k = 0; k < I; ++k) q[U0 + j * I + k] = q[U0 + j * I + k] * (gu[k] - dot) / 1000.0f;
        }
    }
}

// One extracted component at x: its record becomes the raw parameters' gradients; returns dL/dx.
template <int H>
__device__ __forceinline__ float dense_comp_bwd(float *q, int L, float x, float A, float B)
{
    float *q1 = q + dense_p_first(H), *q2 = q1 + dense_p_mid(H), *qlast = q1 + L * dense_p_mid(H);
    float act[3][H];                                               // what the first L + 1 transforms give
#pragma unroll
    for (int j = 0; j < H; ++j) act[1][j] = act[2][j] = 0.0f;
    float unused = 0.0f;
    dense_inner<1, H, false, false>(q, &x, act[0], unused);
    if (L > 0) dense_inner<H, H, false, false>(q1, act[0], act[1], unused);
    if (L > 1) dense_inner<H, H, false, false>(q2, act[1], act[2], unused);
    float last[H], gv[H], gw[H];
#pragma unroll
    for (int j = 0; j < H; ++j) last[j] = L == 0 ? act[0][j] : (L == 1 ? act[1][j] : act[2][j]);
    dense_inner_bwd<H, 1>(qlast, last, &A, B, gv);
    if (L > 1) {
        dense_inner_bwd<H, H>(q2, act[1], gv, B, gw);
#pragma unroll
        for (int j = 0; j < H; ++j) gv[j] = gw[j];
    }
    if (L > 0) {
        dense_inner_bwd<H, H>(q1, act[0], gv, B, gw);
#pragma unroll
        for (int j = 0; j < H; ++j) gv[j] = gw[j];
    }
    float gx;
    dense_inner_bwd<1, H>(q, &x, gv, B, &gx);
    return gx;
}

// ws: gridDim.x slices of T CP floats.  Dynamic LDS: block records x PS floats.
template <int H>
__global__ __launch_bounds__(256) void k_dense_dsf_coupling_bwd(
    const float *__restrict__ x, const float *__restrict__ pred, float *g, const float *__restrict__ gld,
    float *__restrict__ dpred, float *__restrict__ ws, long long N, int D, const int *__restrict__ desc, int T, int T_shift,
    int C, int L, int P, int PS)
{
    const int block = blockDim.x;
    const int CP = C * P;
    extern __shared__ __attribute__((aligned(16))) float rec[];
    const int *tgt_idx = desc;
    const long long stride = desc[T];
    const int *col = desc + T + 1;
    const float *base = reinterpret_cast<const float *>(col + (long long)T * CP);
    const int tid = threadIdx.x;
    const long long TCP = (long long)T * CP;
    float *slice = ws + blockIdx.x * TCP;
    for (long long i = tid; i < TCP; i += block) slice[i] = 0.0f;  // (entry dj belongs to lane dj % block, here and below)
    const int R = T <= block ? block / T : 1;
    const int chunks = T <= block ? 1 : (T + block - 1) / block;
    const long long n_tiles = (N + R - 1) / R;
    const int r_first = tid / CP, j_first = tid - r_first * CP;
    const int r_step = block / CP, j_step = block - r_step * CP;
    const int rr_first = r_first / T, t_first = r_first - rr_first * T;
    const int rr_step = r_step / T, t_step = r_step - rr_step * T;

    for (long long tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const long long row0 = tile * R;
        const int rows = (int)((N - row0) < (long long)R ? (N - row0) : (long long)R);
        for (int ch = 0; ch < chunks; ++ch) {
            const int cbase = ch * block;
            const int E = (chunks == 1) ? rows * T : ((T - cbase) < block ? (T - cbase) : block);
            __syncthreads();                    // previous tile's readers are done
            int r = r_first, j = j_first, rr = rr_first, t = cbase + t_first;
            for (int i = tid; i < E * CP; i += block) {             // (k_dense_dsf_coupling's walk)
                const int dj = t * CP + j;
                const int cc = col[dj];
                rec[r * PS + j] = cc >= 0 ? nt_load(pred + (row0 + rr) * stride + cc) : base[dj];
                r += r_step;
                rr += rr_step;
                t += t_step;
                j += j_step;
                if (j >= CP) { j -= CP; ++r; ++t; }
                if (chunks == 1 && t >= T) { t -= T; ++rr; }
            }
            __syncthreads();
            if (tid < E) {
                long long row = row0;
                int te = cbase + tid;
                if (chunks == 1) {
                    const int re = T_shift >= 0 ? (tid >> T_shift) : (tid / T);
                    te = tid - re * T;
                    row = row0 + re;
                }
                float *q = rec + tid * PS;
                (void)dense_extract_record<H>(q, C, L);
                const long long at = row * D + tgt_idx[te];
                const float v = x[at];
                float A = g[at];
                const float B = gld[row];
                if (C == 2) {
                    float unused = 0.0f;
                    const float mid = dense_comp<H, false, false>(q, L, v, unused);
                    A = dense_comp_bwd<H>(q + P, L, mid, A, B);
                }
                g[at] = dense_comp_bwd<H>(q, L, v, A, B);
            }
            __syncthreads();
            if (dpred) {
                r = r_first, j = j_first, rr = rr_first, t = cbase + t_first;
                for (int i = tid; i < E * CP; i += block) {
                    const int cc = col[t * CP + j];
                    if (cc >= 0) dpred[(row0 + rr) * stride + cc] = rec[r * PS + j];
                    r += r_step;
                    rr += rr_step;
                    t += t_step;
                    j += j_step;
                    if (j >= CP) { j -= CP; ++r; ++t; }
                    if (chunks == 1 && t >= T) { t -= T; ++rr; }
                }
            }
            // the learned constants: this tile's rows in row order, onto the workgroup's slice
            const int Tc = chunks == 1 ? T : E, rows_c = chunks == 1 ? rows : 1;
            int tl = r_first;
            j = j_first;
            for (int i = tid; i < Tc * CP; i += block) {
                const long long dj = (long long)cbase * CP + i;
                if (col[dj] < 0) {
                    float sum = 0.0f;
                    for (int k = 0; k < rows_c; ++k) sum += rec[(k * T + tl) * PS + j];
                    slice[dj] += sum;
                }
                tl += r_step;
                j += j_step;
                if (j >= CP) { j -= CP; ++tl; }
            }
        }
    }
}

// dbase[dj] = the slices' entries dj in slice order (0 where the parameter is predicted)
__global__ __launch_bounds__(256) void k_dense_bwd_sum(const float *__restrict__ ws, const int *__restrict__ col,
                                                       float *__restrict__ dbase, long long TCP, int slices)
{
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= TCP) return;
    float sum = 0.0f;
    if (col[i] < 0) {
        for (int k = 0; k < slices; ++k) sum += ws[k * TCP + i];
    }
    dbase[i] = sum;
}

int dense_dsf_coupling_bwd(const float *x, const float *pred, float *g, const float *gld, float *gh, int64_t N, int32_t D,
                           const int32_t *desc, int32_t T, int32_t n_components, int32_t hidden, int32_t inverse,
                           void *stream, const char *fn)
{
    if (N < 0) return fail(TFK_EINVAL, "%s: N = %lld < 0", fn, (long long)N);
    if (D < 1 || T < 1 || T > D) return fail(TFK_EINVAL, "%s: need 1 <= T <= D (T = %d, D = %d)", fn, T, D);
    if (!dense_dsf_supported(n_components, hidden))
        return fail(TFK_EINVAL, "%s: dense sigmoidal kernels exist for 1 <= hidden size <= 8, 0 <= dense layers <= 2, 1 or 2 "
                    "components and at most %d parameters per element (n_components = 0x%x, hidden_dim = %d)", fn,
                    kDenseMaxFloats, (unsigned)n_components, hidden);
    if (inverse)
        return fail(TFK_EINVAL, "%s: the inverse direction is a bisection without gradient; differentiate it on the ATen "
                    "path", fn);
    if (N == 0) return TFK_OK;                                      // (nothing is written; with null pointers: the probe)
    if (!x || !g || !gld || !gh || !desc)                           // (pred may be null: every parameter a learned constant)
        return fail(TFK_EINVAL, "%s: null pointer (the dense family always takes its descriptor block in tgt_idx)", fn);
    const int C = n_components & 0xff, L = (n_components >> 8) - 1, H = hidden;
    int T_shift = -1;
    if ((T & (T - 1)) == 0) {
        T_shift = 0;
        while ((1 << T_shift) < T) ++T_shift;
    }
    const int P = dense_p(H, L), PS = (C * P) | 1;
    int block = 256;                                               // (64 records of 513 floats fit)
    while (block > 64 && (size_t)block * PS * sizeof(float) > kDenseLdsBytes) block >>= 1;
    const size_t lds = (size_t)block * PS * sizeof(float);
    const int R = T <= block ? block / T : 1;
    const int64_t n_tiles = (N + R - 1) / R;
    int per_cu = (int)(kDenseLdsBytes / lds);
    if (per_cu > 8) per_cu = 8;
    int64_t grid = (int64_t)cu_count() * per_cu;
    if (grid > kDenseBwdSlices) grid = kDenseBwdSlices;
    if (grid > n_tiles) grid = n_tiles;
    const size_t TCP = (size_t)T * C * P;
    float *dbase = gh, *ws = gh + TCP;
    float *dpred = pred ? gh + (size_t)(1 + kDenseBwdSlices) * TCP : nullptr;
    hipStream_t s = static_cast<hipStream_t>(stream);
    switch (H) {
#define TFK_DENSE_CASE(H_)                                                                                          \
    case H_: {                                                                                                      \
        auto kern = &k_dense_dsf_coupling_bwd<H_>;                                                                  \
        if (lds > 64 * 1024 && hipFuncSetAttribute(reinterpret_cast<const void *>(kern),                            \
                                                   hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess) { \
            (void)hipGetLastError();                                                                                \
            return fail(TFK_ELAUNCH, "%s: cannot reserve %zu bytes of LDS", fn, lds);                               \
        }                                                                                                           \
        hipLaunchKernelGGL(kern, dim3((unsigned)grid), dim3(block), lds, s, x, pred, g, gld, dpred, ws, (long long)N, D, desc, \
                           T, T_shift, C, L, P, PS);                                                                \
    } break;
        TFK_DENSE_FOR_EACH_H(TFK_DENSE_CASE)
#undef TFK_DENSE_CASE
    }
    if (const int rc = check_launch(fn)) return rc;
    hipLaunchKernelGGL(k_dense_bwd_sum, dim3((unsigned)((TCP + 255) / 256)), dim3(256), 0, s, ws, desc + T + 1, dbase,
                       (long long)TCP, (int)grid);
    return check_launch(fn);
}

}  // namespace tfk
