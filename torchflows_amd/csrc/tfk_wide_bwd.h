// tfk_wide_bwd.h -- reverse mode of ONE affine / shift coupling on event sizes above 256, the row spread over four waves
// (template; instantiated and dispatched in tfk_wide_bwd.hip behind tfk_wide_coupling_train_bwd).
//
// Geometry, loads and stores are those of the forward kernel (tfk_flow_wide.h): a workgroup of 4 waves owns a tile of 16
// rows; lane (q, j) of wave w holds columns c0 .. c0 + EPLW - 1, c0 = (4 w + q) EPLW, of BOTH planes of row j, planes padded
// in registers to HP = 16 EPLW (pad columns are zero and have zero weights), rows read and written at their logical width
// D (D % 8 == 0: 16-byte accesses only).  Per tile:
//   1. x (both planes) and g (both planes; column c from D - 1 - c with `g_reversed`, times gscale[c]) -> 4 EPLW registers
//   2. GEMM 1 split-K over the waves exactly as wide_couple does it: the four 16 x 16 partials meet in the LDS behind
//      barrier A, every wave adds them in wave order -- all four hold bit-identical hidden units -- and takes the tanh
//   3. GEMM 2 on the wave's own target columns -> (scale logit, shift) -> alpha
//   4. the transform backwards in registers (k_affine_coupling_bwd's formulas, tfk_bwd.hip; the log-det term gld / alpha,
//      d alpha / d u = (alpha - 1e-10) / 2): dL/dx_target and dL/dh with respect to the module's OWN conditioner outputs.
//      A shift coupling is the affine one with logit 0: alpha = 1, no logit row
//   5. dL/dhidden = W2^T dL/dh: each wave contracts over its own target columns, one MFMA per owned column and parameter --
//      the B operand of lane (q, j) is the dL/dh it already holds, the k index is the lane group, A2T is packed so that the
//      result lands on the lane / register that holds the unit; the four partials meet in the LDS behind barrier B and are
//      added in wave order
//   6. dL/dpre = dL/dhidden (1 - hidden^2)
//   7. dL/dx_source += W1^T dL/dpre on the wave's own source columns (EPLW / 4 tiles x 4 k-steps; A1T packed so that
//      accumulator (q, r) is a column the lane owns)
//   8. g stored in place, un-reversed
//   9. three records for the products that contract over the batch rows (tfk_rows_outer), 16-byte stores:
//        gh_rec[row][2 c + p]  affine: dL/d(parameter p of target column c), c < HP        (N, 2 HP)
//        gh_rec[row][c]        shift                                                       (N, HP)
//        gpre_rec[row][4 q + r] = dL/dpre of hidden unit 4 r + q                           (N, 16)
//        hid_rec[row][4 q + r]  = hidden unit 4 r + q, column 15 == 1 (the bias column)    (N, 16)
//      (every wave holds the same 16 hidden values: wave 0 writes the last two)
// Rows >= N of the last tile are computed on zeros; their g and record rows are not written.  The trip count of the tile
// loop is the same for every wave of the workgroup: no wave leaves before the last barrier.  The two barriers use distinct
// LDS buffers, two sets alternating by tile parity: a wave that runs ahead never overwrites what a slower one still reads.
//
// `g` is read at the top of a tile and written at its end by OTHER waves of the workgroup when it is read reversed: the
// loaded values are pinned in registers before barrier A, so every load has returned before any wave stores.
//
// Parameter block (floats): the forward block of tfk_flow_wide.h, pre-scaled as there (pre_s / pre_t are not read: the
// training node runs one coupling per launch on plain rows), followed by the transposed operands in the module's own scale:
//   A1[4][EPLW/4][64][4] | b1[4][4] | A2[4][T2][64][4] | b2[4][T2][4][4] | pre_s[HP] | pre_t[HP] |
//   A2T[4][T2][64][4] | A1T[4][EPLW/4][64][4]
//   A2T[w][t][l][r]: weight of hidden unit 4 (i & 3) + (i >> 2), i = l & 15, in GEMM-2 output row r of tile t of wave w for
//                    lane group l >> 4 (affine: parameter r & 1 of target column (4 w + (l >> 4)) EPLW + 2 t + (r >> 1);
//                    shift: target column (4 w + (l >> 4)) EPLW + 4 t + r)
//   A1T[w][g][l][r]: weight of hidden unit 4 r + (l >> 4) for source column (4 w + (i >> 2)) EPLW + 4 g + (i & 3)
#pragma once
#include "tfk_flow_wide.h"

namespace tfk {

constexpr int wide_bwd_block_floats(int eplw, bool affine)
{
    const int t2 = affine ? eplw / 2 : eplw / 4;
    return wide_block_floats(eplw, affine) + 4 * t2 * 256 + 256 * eplw;
}

// EPLW columns of one plane of a row whose logical column c sits at D - 1 - c (p0 = 0: plane A, half: plane B)
template <int EPLW>
__device__ __forceinline__ void wide_load_rev(const float *row, int p0, int c0, int half, int D, bool live, float (&v)[EPLW])
{
#pragma unroll
    for (int i = 0; i < EPLW; i += 4) {
        wf32x4 t = {0.0f, 0.0f, 0.0f, 0.0f};
        if (live && c0 + i < half) t = *reinterpret_cast<const wf32x4 *>(row + (D - p0 - c0 - i - 4));
        v[i] = t[3]; v[i + 1] = t[2]; v[i + 2] = t[1]; v[i + 3] = t[0];
    }
}

template <int EPLW, bool SHIFT>
__global__ __launch_bounds__(kWideBlock) void k_wide_coupling_train_bwd(
    const float *__restrict__ x, float *g, const float *__restrict__ gld, const float *__restrict__ params,
    float *__restrict__ gh_rec, float *__restrict__ gpre_rec, float *__restrict__ hid_rec, long long N, int D,
    int inverse_form, const float *__restrict__ gscale, int g_reversed)
{
    constexpr int T2 = SHIFT ? EPLW / 4 : EPLW / 2, G1 = EPLW / 4;
    constexpr int GHL = SHIFT ? EPLW : 2 * EPLW;                           // dL/dh values of a lane = its stretch of gh_rec
    constexpr int OFF_B1 = 256 * EPLW, OFF_A2 = OFF_B1 + 16, OFF_B2 = OFF_A2 + 4 * T2 * 256;
    constexpr int OFF_A2T = wide_block_floats(EPLW, !SHIFT), OFF_A1T = OFF_A2T + 4 * T2 * 256;
    __shared__ __attribute__((aligned(16))) wf32x4 part_s[2 * 2 * 256];    // [tile parity][barrier A / B][wave][lane]

    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int q = lane >> 4, j = lane & 15;
    const int half = D >> 1;
    const int c0_ = (4 * wave + q) * EPLW;
    const long long n_tiles = (N + 15) >> 4;
    const wf32x4 *A1 = reinterpret_cast<const wf32x4 *>(params) + wave * G1 * 64;
    const wf32x4 *A2 = reinterpret_cast<const wf32x4 *>(params + OFF_A2) + wave * T2 * 64;
    const float *b2 = params + OFF_B2 + wave * T2 * 16;
    const wf32x4 *A2T = reinterpret_cast<const wf32x4 *>(params + OFF_A2T) + wave * T2 * 64;
    const wf32x4 *A1T = reinterpret_cast<const wf32x4 *>(params + OFF_A1T) + wave * G1 * 64;
    int par = 0;
    // (the trip count is the same for every wave of the workgroup: no wave leaves before the last barrier)
    for (long long tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const long long row = tile * 16 + j;
        int c0 = c0_;
        asm volatile("" : "+v"(c0));                                  // (opaque per tile, as in k_flow_wide)
        const bool live = row < N;                                    // rows past the end: zeros in, nothing out
        const long long ro = (live ? row : 0) * (long long)D;
        wf32x4 *partA = part_s + par * 512, *partB = partA + 256;
        par ^= 1;

        // 1. the rows
        float xa[EPLW], xb[EPLW], ga[EPLW], gb[EPLW];
        wide_load<EPLW, 4>(x + ro, c0, half, live, xa);
        wide_load<EPLW, 4>(x + ro + half, c0, half, live, xb);
        if (!g_reversed) {
            wide_load<EPLW, 4>(g + ro, c0, half, live, ga);
            wide_load<EPLW, 4>(g + ro + half, c0, half, live, gb);
        } else {
            wide_load_rev<EPLW>(g + ro, 0, c0, half, D, live, ga);
            wide_load_rev<EPLW>(g + ro, half, c0, half, D, live, gb);
        }
        if (gscale) {                                                 // a fixed elementwise scale followed the layer
#pragma unroll
            for (int i = 0; i < EPLW; i += 4) {
                if (c0 + i < half) {
                    const wf32x4 sa = *reinterpret_cast<const wf32x4 *>(gscale + c0 + i);
                    const wf32x4 sb = *reinterpret_cast<const wf32x4 *>(gscale + half + c0 + i);
#pragma unroll
                    for (int k = 0; k < 4; ++k) {
                        ga[i + k] *= sa[k];
                        gb[i + k] *= sb[k];
                    }
                }
            }
        }
        const float gl = live ? gld[row] : 0.0f;
        // every load of g has returned before barrier A: another wave stores these addresses at the end of the tile
#pragma unroll
        for (int i = 0; i < EPLW; ++i) asm volatile("" : "+v"(ga[i]), "+v"(gb[i]));
        __builtin_amdgcn_sched_barrier(0);

        // 2. GEMM 1, this wave's K-slice (weights pre-scaled by 2 log2 e), operands in stages as in wide_couple
        wf32x4 acc = {0.0f, 0.0f, 0.0f, 0.0f};
        {
            wf32x4 w1[2][kWideStage];
#pragma unroll
            for (int s = 0; s < kWideStage; ++s)
                if (s < G1) w1[0][s] = A1[s * 64 + lane];
#pragma unroll
            for (int g0 = 0; g0 < G1; g0 += kWideStage) {
                const int cur = (g0 / kWideStage) & 1;
#pragma unroll
                for (int s = 0; s < kWideStage; ++s)
                    if (g0 + kWideStage + s < G1) w1[cur ^ 1][s] = A1[(g0 + kWideStage + s) * 64 + lane];
                __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                for (int s = 0; s < kWideStage; ++s)
                    if (g0 + s < G1) {
#pragma unroll
                        for (int k = 0; k < 4; ++k)
                            acc = __builtin_amdgcn_mfma_f32_16x16x4f32(w1[cur][s][k], xa[4 * (g0 + s) + k], acc, 0, 0, 0);
                    }
                __builtin_amdgcn_sched_barrier(0);
            }
        }
        partA[wave * 64 + lane] = acc;
        __builtin_amdgcn_sched_barrier(0);
        __syncthreads();                                              // barrier A
        wf32x4 h = *reinterpret_cast<const wf32x4 *>(params + OFF_B1 + 4 * q);
#pragma unroll
        for (int w = 0; w < 4; ++w) h = h + partA[w * 64 + lane];     // wave order: the same sum in every wave
        float hid[4];
#pragma unroll
        for (int r = 0; r < 4; ++r)                                   // tanh, transforms.py:293-304
            hid[r] = fmaf(-2.0f, __builtin_amdgcn_rcpf(__builtin_amdgcn_exp2f(h[r]) + 1.0f), 1.0f);

        // 3. + 4. GEMM 2 on the wave's own target columns, the transform backwards; dL/dh stays in ghv and goes to gh_rec
        wf32x4 ghv[T2];
        float *ghr = gh_rec + (live ? row : 0) * (long long)(16 * GHL) + (4 * wave + q) * GHL;
        {
            wf32x4 w2[2][kWideStage], o2[2][kWideStage];
#pragma unroll
            for (int s = 0; s < kWideStage; ++s)
                if (s < T2) {
                    w2[0][s] = A2[s * 64 + lane];
                    o2[0][s] = *reinterpret_cast<const wf32x4 *>(b2 + (s * 4 + q) * 4);
                }
#pragma unroll
            for (int t0 = 0; t0 < T2; t0 += kWideStage) {
                const int cur = (t0 / kWideStage) & 1;
#pragma unroll
                for (int s = 0; s < kWideStage; ++s)
                    if (t0 + kWideStage + s < T2) {
                        w2[cur ^ 1][s] = A2[(t0 + kWideStage + s) * 64 + lane];
                        o2[cur ^ 1][s] = *reinterpret_cast<const wf32x4 *>(b2 + ((t0 + kWideStage + s) * 4 + q) * 4);
                    }
                __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                for (int s = 0; s < kWideStage; ++s) {
                    const int t = t0 + s;
                    if (t < T2) {
                        wf32x4 o = o2[cur][s];
#pragma unroll
                        for (int k = 0; k < 4; ++k)
                            o = __builtin_amdgcn_mfma_f32_16x16x4f32(w2[cur][s][k], hid[k], o, 0, 0, 0);
                        if constexpr (!SHIFT) {
#pragma unroll
                            for (int i = 0; i < 2; ++i) {
                                const int e = 2 * t + i;
                                // affine.py:33-34 with the logit row pre-scaled: o = (u / 2 + c0) log2 e
                                const float ex = __builtin_amdgcn_exp2f(o[2 * i]);
                                const float beta = o[2 * i + 1];
                                const float alpha = ex + kAffMinScale;
                                const float ra = __builtin_amdgcn_rcpf(alpha);
                                const float gz = gb[e];
                                float gx, gbeta, galpha;
                                if (!inverse_form) {                  // out = alpha x + beta, ld = +sum log alpha
                                    gx = gz * alpha;
                                    gbeta = gz;
                                    galpha = gz * xb[e] + gl * ra;
                                } else {                              // out = (x - beta) / alpha, ld = -sum log alpha
                                    const float r_ = gz * ra;
                                    gx = r_;
                                    gbeta = -r_;
                                    galpha = -r_ * ((xb[e] - beta) * ra) - gl * ra;
                                }
                                gb[e] = gx;
                                ghv[t][2 * i] = galpha * ex * 0.5f;
                                ghv[t][2 * i + 1] = gbeta;
                            }
                        } else {                                      // out = x +/- h, log-det 0 (affine.py:137-159)
#pragma unroll
                            for (int i = 0; i < 4; ++i) ghv[t][i] = inverse_form ? -gb[4 * t + i] : gb[4 * t + i];
                        }
                        if (live) *reinterpret_cast<wf32x4 *>(ghr + 4 * t) = ghv[t];
                    }
                }
                __builtin_amdgcn_sched_barrier(0);
            }
        }

        // 5. dL/dhidden = W2^T dL/dh over this wave's target columns (two accumulators in turn: the MFMA's own latency)
        wf32x4 gha0 = {0.0f, 0.0f, 0.0f, 0.0f}, gha1 = {0.0f, 0.0f, 0.0f, 0.0f};
        {
            wf32x4 wt[2][kWideStage];
#pragma unroll
            for (int s = 0; s < kWideStage; ++s)
                if (s < T2) wt[0][s] = A2T[s * 64 + lane];
#pragma unroll
            for (int t0 = 0; t0 < T2; t0 += kWideStage) {
                const int cur = (t0 / kWideStage) & 1;
#pragma unroll
                for (int s = 0; s < kWideStage; ++s)
                    if (t0 + kWideStage + s < T2) wt[cur ^ 1][s] = A2T[(t0 + kWideStage + s) * 64 + lane];
                __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                for (int s = 0; s < kWideStage; ++s) {
                    const int t = t0 + s;
                    if (t < T2) {
#pragma unroll
                        for (int r = 0; r < 4; ++r) {
                            if (r & 1) gha1 = __builtin_amdgcn_mfma_f32_16x16x4f32(wt[cur][s][r], ghv[t][r], gha1, 0, 0, 0);
                            else gha0 = __builtin_amdgcn_mfma_f32_16x16x4f32(wt[cur][s][r], ghv[t][r], gha0, 0, 0, 0);
                        }
                    }
                }
                __builtin_amdgcn_sched_barrier(0);
            }
        }
        partB[wave * 64 + lane] = gha0 + gha1;
        __builtin_amdgcn_sched_barrier(0);
        __syncthreads();                                              // barrier B
        wf32x4 gha = partB[lane];
#pragma unroll
        for (int w = 1; w < 4; ++w) gha = gha + partB[w * 64 + lane]; // wave order
        // 6. times tanh'
        float gpre[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) gpre[r] = gha[r] * (1.0f - hid[r] * hid[r]);

        // 7. dL/dx_source += W1^T dL/dpre: column c0 + 4 s + r lands in register r of tile s
        {
            wf32x4 wt[2][kWideStage];
#pragma unroll
            for (int s = 0; s < kWideStage; ++s)
                if (s < G1) wt[0][s] = A1T[s * 64 + lane];
#pragma unroll
            for (int g0 = 0; g0 < G1; g0 += kWideStage) {
                const int cur = (g0 / kWideStage) & 1;
#pragma unroll
                for (int s = 0; s < kWideStage; ++s)
                    if (g0 + kWideStage + s < G1) wt[cur ^ 1][s] = A1T[(g0 + kWideStage + s) * 64 + lane];
                __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                for (int s = 0; s < kWideStage; ++s) {
                    const int t = g0 + s;
                    if (t < G1) {
                        wf32x4 d = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
                        for (int r = 0; r < 4; ++r)
                            d = __builtin_amdgcn_mfma_f32_16x16x4f32(wt[cur][s][r], gpre[r], d, 0, 0, 0);
#pragma unroll
                        for (int r = 0; r < 4; ++r) ga[4 * t + r] += d[r];
                    }
                }
                __builtin_amdgcn_sched_barrier(0);
            }
        }

        // 8. + 9. the gradient rows in place, the records of the hidden layer
        if (live) {
            float *gr = g + row * (long long)D;
            wide_store<EPLW, 4>(gr, 0, c0, half, D, false, ga);
            wide_store<EPLW, 4>(gr, half, c0, half, D, false, gb);
            if (wave == 0) {
                wf32x4 hv, pv;
                hv[0] = hid[0]; hv[1] = hid[1]; hv[2] = hid[2]; hv[3] = q == 3 ? 1.0f : hid[3];
                pv[0] = gpre[0]; pv[1] = gpre[1]; pv[2] = gpre[2]; pv[3] = gpre[3];
                *reinterpret_cast<wf32x4 *>(hid_rec + row * 16 + 4 * q) = hv;
                *reinterpret_cast<wf32x4 *>(gpre_rec + row * 16 + 4 * q) = pv;
            }
        }
    }
}

// workgroups the launch uses at most: resident sets as for k_flow_wide
template <int EPLW, bool SHIFT>
static int wide_bwd_grid_cap()
{
    int per_cu = 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, k_wide_coupling_train_bwd<EPLW, SHIFT>, kWideBlock, 0) != hipSuccess
        || per_cu < 1) {
        (void)hipGetLastError();
        per_cu = 1;
    }
    if (per_cu > 8) per_cu = 8;
    return cu_count() * per_cu * kGridOversubscribe;
}

template <int EPLW, bool SHIFT>
static int launch_wide_bwd_k(const float *x, float *g, const float *gld, const float *params, float *gh_rec,
                             float *gpre_rec, float *hid_rec, int64_t N, int D, int inverse_form, const float *gscale,
                             int g_reversed, hipStream_t s, const char *fn)
{
    const int64_t want = (N + 15) / 16;
    const int64_t cap = wide_bwd_grid_cap<EPLW, SHIFT>();
    const int grid = (int)(want < cap ? want : cap);
    hipLaunchKernelGGL((k_wide_coupling_train_bwd<EPLW, SHIFT>), dim3(grid), dim3(kWideBlock), 0, s, x, g, gld, params,
                       gh_rec, gpre_rec, hid_rec, (long long)N, D, inverse_form, gscale, g_reversed);
    return check_launch(fn);
}

}  // namespace tfk
