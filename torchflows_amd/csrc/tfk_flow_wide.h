// tfk_flow_wide.h -- wide-row chain kernel: chains of affine / shift couplings on event sizes 256 < D <= 2048
// (template; instantiated and dispatched in tfk_flow_wide.hip behind tfk_flow_run_wide).
//
// The straight-line chain kernels of tfk_flow_chain.h keep a row in ONE wave (D / 8 floats per lane and plane); above
// D = 256 a row no longer fits.  Here a workgroup of 4 waves owns a tile of 16 rows for the whole chain:
//
//   * each plane (the source half / the target half of the HalfSplit mask) is padded to HP = 16 * EPLW columns, HP a
//     multiple of 64; lane l = (q = l >> 4, j = l & 15) of wave w holds, of row j of the tile, the EPLW contiguous
//     columns c0 .. c0 + EPLW - 1 of BOTH planes, c0 = (4 w + q) EPLW -- wave w owns HP / 4 contiguous columns.  Pad
//     columns are zero in registers and have zero weights (alpha = 1, beta = 0, log alpha = 0 exactly);
//   * GEMM 1 is split-K over the waves: every wave runs v_mfma_f32_16x16x4_f32 over its own source columns into one
//     16 x 16 partial, the four partials meet in the LDS (ONE barrier per coupling, two buffers in turn), and every
//     wave adds them in wave order to b1 and takes the tanh -- all four hold the same 16 hidden units afterwards;
//   * GEMM 2 and the transform run on the wave's own target columns (tiles of 8 (affine) / 16 (shift) targets never
//     straddle waves: EPLW is a multiple of 4), always 4 k-steps: hidden widths below 16 are zero-padded;
//   * the operands are read from global memory where they stay in L2 across workgroups (a coupling's block is 48 HP
//     floats: 86 KB at D = 784 -- a chain's blocks do not fit the LDS);
//   * rows are read and written at their LOGICAL width D, in place (no padded copy): 16-byte accesses when D % 8 == 0,
//     8-byte ones when D % 4 == 0, 4-byte ones otherwise (plane B then starts at an odd column);
//   * rows >= N of the last tile are computed on zeros and not stored: every wave reaches every barrier.
//
// Conventions carried over from the lean format (tfk_flow_chain.h): W1 / b1 arrive times 2 log2(e), the scale-logit
// rows of W2 / b2 times log2(e) / 2 (+ c0 log2(e)): tanh = 1 - 2 / (exp2(.) + 1), alpha = exp2(.) + 1e-10, the log-det
// is summed in base 2 and scaled by ln 2 once per row; the elementwise layers are deferred by the packer (folded into
// W1 / b1, a pre-affine on the target plane, one closing fma per element + one constant log-det).
//
// Parameter block of a coupling (floats; W = 4 waves, T2 = EPLW / 2 (affine) or EPLW / 4 (shift) tiles per wave):
//   A1[W][EPLW/4][64][4] | b1[4][4] | A2[W][T2][64][4] | b2[W][T2][4][4] | pre_s[HP] | pre_t[HP]
//   A1[w][g][l][k]: weight of hidden unit 4 (i & 3) + (i >> 2), i = l & 15, for source column (4 w + (l >> 4)) EPLW + 4 g + k
//   b1[q][r]:       bias of hidden unit 4 r + q
//   A2[w][t][l][k]: weight of hidden unit 4 k + (l >> 4) for output row i = l & 15 = 4 q2 + r of tile t of wave w:
//                   affine: parameter r & 1 (0 scale logit, 1 shift) of target column (4 w + q2) EPLW + 2 t + (r >> 1)
//                   shift:  the shift of target column (4 w + q2) EPLW + 4 t + r
//   b2[w][t][q2][r]: the bias of that output row
//   pre_s / pre_t:  pending elementwise map of the target plane, z = fma(pre_s, x, pre_t), applied before the transform
// Closing TFK_OP_EW_FMA block: s[2 HP] | t[2 HP] | logdet_const | pad[3]   (plane A's columns, then plane B's)
#pragma once
#include "tfk_common.h"

namespace tfk {

constexpr int kWideMaxOps = 64;
constexpr int kWideBlock = 256;        // 4 waves: the column split above
constexpr int kWideStage = 2;          // 16-byte operand loads per pipeline stage of the two GEMMs (4: +56 VGPRs at D = 784)

struct WideProg {
    int n_c;                           // couplings (>= 1)
    int ew_offset;                     // the closing TFK_OP_EW_FMA block
    unsigned long long src_mask;       // bit o: coupling o reads plane B (and transforms plane A)
    int offset[kWideMaxOps];
};

typedef float wf32x4 __attribute__((ext_vector_type(4)));
typedef float wf32x2 __attribute__((ext_vector_type(2)));

// floats of one coupling's block
constexpr int wide_block_floats(int eplw, bool affine)
{
    const int t2 = affine ? eplw / 2 : eplw / 4;
    return 256 * eplw + 16 + 4 * t2 * 256 + 4 * t2 * 16 + 32 * eplw;
}

// EPLW columns of one plane of one row, starting at column c0 of the plane (`half` logical columns, zeros behind them and
// in rows past the end).  VEC divides half, c0 and EPLW: a vector lies inside the plane or outside as a whole.
template <int EPLW, int VEC>
__device__ __forceinline__ void wide_load(const float *plane, int c0, int half, bool live, float (&v)[EPLW])
{
#pragma unroll
    for (int i = 0; i < EPLW; i += VEC) {
        const bool ok = live && c0 + i < half;
        if constexpr (VEC == 4) {
            wf32x4 t = {0.0f, 0.0f, 0.0f, 0.0f};
            if (ok) t = *reinterpret_cast<const wf32x4 *>(plane + c0 + i);
            v[i] = t[0]; v[i + 1] = t[1]; v[i + 2] = t[2]; v[i + 3] = t[3];
        } else if constexpr (VEC == 2) {
            wf32x2 t = {0.0f, 0.0f};
            if (ok) t = *reinterpret_cast<const wf32x2 *>(plane + c0 + i);
            v[i] = t[0]; v[i + 1] = t[1];
        } else {
            v[i] = ok ? plane[c0 + i] : 0.0f;
        }
    }
}

// ... and the store: logical column p0 + c (p0 = 0 for plane A, half for plane B), or D - 1 - (p0 + c) with `rev`
// (a ReversePermutationMatrix behind the program, folded into the store)
template <int EPLW, int VEC>
__device__ __forceinline__ void wide_store(float *row, int p0, int c0, int half, int D, bool rev, const float (&v)[EPLW])
{
#pragma unroll
    for (int i = 0; i < EPLW; i += VEC) {
        const int c = c0 + i;
        if (c < half) {
            float *dst = rev ? row + (D - p0 - c - VEC) : row + p0 + c;
            if constexpr (VEC == 4) {
                wf32x4 t;
                t[0] = rev ? v[i + 3] : v[i]; t[1] = rev ? v[i + 2] : v[i + 1];
                t[2] = rev ? v[i + 1] : v[i + 2]; t[3] = rev ? v[i] : v[i + 3];
                *reinterpret_cast<wf32x4 *>(dst) = t;
            } else if constexpr (VEC == 2) {
                wf32x2 t;
                t[0] = rev ? v[i + 1] : v[i]; t[1] = rev ? v[i] : v[i + 1];
                *reinterpret_cast<wf32x2 *>(dst) = t;
            } else {
                *dst = v[i];
            }
        }
    }
}

// One coupling.  KIND: 0 affine fwd, 1 affine inv, 2 shift fwd, 3 shift inv.  `part`: this coupling's LDS buffer for the
// four GEMM-1 partials.  Contains the coupling's ONE barrier: called by every wave of the workgroup, unconditionally.
template <int EPLW, int KIND>
__device__ __forceinline__ void wide_couple(const float *__restrict__ blk, wf32x4 *part, int lane, int q, int wave,
                                            const float (&src)[EPLW], float (&tgt)[EPLW], float &ld2)
{
    constexpr bool affine = KIND < 2;
    constexpr int HP = 16 * EPLW;
    constexpr int T2 = affine ? EPLW / 2 : EPLW / 4;
    constexpr int OFF_B1 = 256 * EPLW, OFF_A2 = OFF_B1 + 16, OFF_B2 = OFF_A2 + 4 * T2 * 256, OFF_PRE = OFF_B2 + 4 * T2 * 16;
    const int c0 = (4 * wave + q) * EPLW;

    // GEMM 1, this wave's K-slice (weights pre-scaled by 2 log2 e)
    const wf32x4 *A1 = reinterpret_cast<const wf32x4 *>(blk) + wave * (EPLW / 4) * 64;
    wf32x4 acc = {0.0f, 0.0f, 0.0f, 0.0f};
    // operands in stages of kWideStage 16-byte loads, the next stage in flight while this one feeds the matrix core; the
    // scheduling fences keep the compiler from hoisting EVERY load of the coupling to its top (512 VGPRs and scratch)
    constexpr int G1 = EPLW / 4;
    wf32x4 w1[2][kWideStage];
#pragma unroll
    for (int g = 0; g < kWideStage; ++g)
        if (g < G1) w1[0][g] = A1[g * 64 + lane];
#pragma unroll
    for (int g0 = 0; g0 < G1; g0 += kWideStage) {
        const int cur = (g0 / kWideStage) & 1;
#pragma unroll
        for (int g = 0; g < kWideStage; ++g)
            if (g0 + kWideStage + g < G1) w1[cur ^ 1][g] = A1[(g0 + kWideStage + g) * 64 + lane];
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int g = 0; g < kWideStage; ++g)
            if (g0 + g < G1) {
#pragma unroll
                for (int k = 0; k < 4; ++k)
                    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(w1[cur][g][k], src[4 * (g0 + g) + k], acc, 0, 0, 0);
            }
        __builtin_amdgcn_sched_barrier(0);
    }
    part[wave * 64 + lane] = acc;
    // the elements about to be transformed take their pending elementwise layers now (one fma)
    const float *pre = blk + OFF_PRE;
#pragma unroll
    for (int i = 0; i < EPLW / 4; ++i) {
        const wf32x4 s = *reinterpret_cast<const wf32x4 *>(pre + c0 + 4 * i);
        const wf32x4 t = *reinterpret_cast<const wf32x4 *>(pre + HP + c0 + 4 * i);
#pragma unroll
        for (int k = 0; k < 4; ++k) tgt[4 * i + k] = fmaf(s[k], tgt[4 * i + k], t[k]);
        if ((i & 3) == 3) __builtin_amdgcn_sched_barrier(0);
    }
    __builtin_amdgcn_sched_barrier(0);
    __syncthreads();
    wf32x4 h = *reinterpret_cast<const wf32x4 *>(blk + OFF_B1 + 4 * q);
#pragma unroll
    for (int w = 0; w < 4; ++w) h = h + part[w * 64 + lane];        // wave order: the same sum in every wave
    float hid[4];
#pragma unroll
    for (int r = 0; r < 4; ++r)                                      // tanh, transforms.py:293-304
        hid[r] = fmaf(-2.0f, __builtin_amdgcn_rcpf(__builtin_amdgcn_exp2f(h[r]) + 1.0f), 1.0f);

    // GEMM 2 + transform on this wave's target columns
    const wf32x4 *A2 = reinterpret_cast<const wf32x4 *>(blk + OFF_A2) + wave * T2 * 64;
    const float *b2 = blk + OFF_B2 + wave * T2 * 16;
    wf32x4 w2[2][kWideStage], o2[2][kWideStage];
#pragma unroll
    for (int g = 0; g < kWideStage; ++g)
        if (g < T2) {
            w2[0][g] = A2[g * 64 + lane];
            o2[0][g] = *reinterpret_cast<const wf32x4 *>(b2 + (g * 4 + q) * 4);
        }
#pragma unroll
    for (int t0 = 0; t0 < T2; t0 += kWideStage) {
        const int cur = (t0 / kWideStage) & 1;
#pragma unroll
        for (int g = 0; g < kWideStage; ++g)
            if (t0 + kWideStage + g < T2) {
                w2[cur ^ 1][g] = A2[(t0 + kWideStage + g) * 64 + lane];
                o2[cur ^ 1][g] = *reinterpret_cast<const wf32x4 *>(b2 + ((t0 + kWideStage + g) * 4 + q) * 4);
            }
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int g = 0; g < kWideStage; ++g) {
            const int t = t0 + g;
            if (t < T2) {
                wf32x4 o = o2[cur][g];
#pragma unroll
                for (int k = 0; k < 4; ++k)
                    o = __builtin_amdgcn_mfma_f32_16x16x4f32(w2[cur][g][k], hid[k], o, 0, 0, 0);
                if constexpr (affine) {
                    // affine.py:33-34 with the logit row pre-scaled: o = (u / 2 + c0) log2 e
                    const float al[2] = {__builtin_amdgcn_exp2f(o[0]) + kAffMinScale, __builtin_amdgcn_exp2f(o[2]) + kAffMinScale};
                    ld2 += __builtin_amdgcn_logf(al[0]) + __builtin_amdgcn_logf(al[1]);        // log2 alpha; affine.py:42
#pragma unroll
                    for (int i = 0; i < 2; ++i) {
                        const int e = 2 * t + i;
                        if constexpr (KIND == 0) tgt[e] = fmaf(al[i], tgt[e], o[2 * i + 1]);    // affine.py:48
                        else tgt[e] = (tgt[e] - o[2 * i + 1]) * __builtin_amdgcn_rcpf(al[i]);   // affine.py:59
                    }
                } else {
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        const int e = 4 * t + i;
                        if constexpr (KIND == 2) tgt[e] = tgt[e] + o[i];                        // affine.py:150
                        else tgt[e] = tgt[e] - o[i];                                            // affine.py:158
                    }
                }
            }
        }
        __builtin_amdgcn_sched_barrier(0);
    }
}

template <int EPLW, int KIND>
__global__ __launch_bounds__(kWideBlock) void k_flow_wide(
    const float *__restrict__ x, float *z, float *logdet, const float *__restrict__ gauss_loc,
    const float *__restrict__ gauss_log_scale, float *logprob, long long N, int D,
    const float *__restrict__ params, WideProg prog, int flags, int vec)
{
    constexpr int HP = 16 * EPLW;
    __shared__ __attribute__((aligned(16))) wf32x4 part_s[2 * 4 * 64];     // GEMM-1 partials, two couplings in flight
    __shared__ float red_s[2 * 4 * 16];                                    // per-wave log-det / squared-norm shares
    // base density as  -0.5 sum ((z - loc) / scale)^2 - sum (log scale + 0.5 log 2 pi):  loc[2 HP] | 1/scale[2 HP] | const
    __shared__ __attribute__((aligned(16))) float base_s[4 * HP + 4];
    __shared__ __attribute__((aligned(16))) float ew_s[4 * HP + 4];        // the closing TFK_OP_EW_FMA block
    const bool accumulate = (flags & 1) != 0;
    const bool reverse_out = (flags & 2) != 0;
    const bool base_of_input = (flags & 4) != 0;
    for (int e = threadIdx.x; e < 4 * HP + 4; e += kWideBlock) ew_s[e] = params[prog.ew_offset + e];
    if (logprob) {
        for (int e = threadIdx.x; e < 2 * HP; e += kWideBlock) {
            base_s[e] = gauss_loc[e];
            base_s[2 * HP + e] = expf(-gauss_log_scale[e]);
        }
        if (threadIdx.x < 64) {
            float c = 0.0f;
            for (int e = threadIdx.x; e < 2 * HP; e += 64) c += gauss_log_scale[e] + kHalfLog2Pi;
            c = group_sum(c, 64);
            if (threadIdx.x == 0) base_s[4 * HP] = c;
        }
    }
    __syncthreads();

    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int q = lane >> 4, j = lane & 15;
    const int half = D >> 1;
    const int c0_ = (4 * wave + q) * EPLW;
    const long long n_tiles = (N + 15) >> 4;
    const float base_const = logprob ? base_s[4 * HP] : 0.0f;
    const float *ew = ew_s;
    int par = 0;
    // (the trip count is the same for every wave of the workgroup: no wave leaves before the last barrier)
    for (long long tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const long long row = tile * 16 + j;
        // (opaque per tile: as a loop invariant the compiler keeps every element's load / store offset of the 4- and 8-byte
        // paths in a register of its own across the whole chain -- 4 EPLW VGPRs and scratch above D = 1400)
        int c0 = c0_;
        asm volatile("" : "+v"(c0));
        const bool live = row < N;                                    // rows past the end: zeros in, nothing out
        const float *xr = x + (live ? row : 0) * (long long)D;
        float a[EPLW], b[EPLW];
        if (vec == 4) {
            wide_load<EPLW, 4>(xr, c0, half, live, a);
            wide_load<EPLW, 4>(xr + half, c0, half, live, b);
        } else if (vec == 2) {
            wide_load<EPLW, 2>(xr, c0, half, live, a);
            wide_load<EPLW, 2>(xr + half, c0, half, live, b);
        } else {
            wide_load<EPLW, 1>(xr, c0, half, live, a);
            wide_load<EPLW, 1>(xr + half, c0, half, live, b);
        }
        float sq = 0.0f;                                              // sum of squared standardised elements
        auto base_terms = [&]() {                                     // gaussian.py:46-54
#pragma unroll
            for (int i = 0; i < EPLW / 4; ++i) {
                const wf32x4 la = *reinterpret_cast<const wf32x4 *>(base_s + c0 + 4 * i);
                const wf32x4 lb = *reinterpret_cast<const wf32x4 *>(base_s + HP + c0 + 4 * i);
                const wf32x4 ia = *reinterpret_cast<const wf32x4 *>(base_s + 2 * HP + c0 + 4 * i);
                const wf32x4 ib = *reinterpret_cast<const wf32x4 *>(base_s + 3 * HP + c0 + 4 * i);
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const float ta = (a[4 * i + k] - la[k]) * ia[k];
                    const float tb = (b[4 * i + k] - lb[k]) * ib[k];
                    sq = fmaf(ta, ta, sq);
                    sq = fmaf(tb, tb, sq);
                }
                if (i & 1) __builtin_amdgcn_sched_barrier(0);
            }
        };
        if (logprob && base_of_input) base_terms();                   // Flow.sample (flows.py:699-707)

        float ld2 = 0.0f;                                             // this lane's share of the log-det, in base 2
#pragma unroll 1
        for (int o = 0; o < prog.n_c; ++o) {
            const float *blk = params + prog.offset[o];
            if (((prog.src_mask >> o) & 1ull) == 0) wide_couple<EPLW, KIND>(blk, part_s + par * 256, lane, q, wave, a, b, ld2);
            else wide_couple<EPLW, KIND>(blk, part_s + par * 256, lane, q, wave, b, a, ld2);
            par ^= 1;
        }
        float ld = 0.0f;
        if constexpr (KIND == 0) ld = ld2 * __int_as_float(0x3f317218);                  // ln 2
        else if constexpr (KIND == 1) ld = ld2 * -__int_as_float(0x3f317218);

        // what is still pending of the elementwise layers, one fma per element
#pragma unroll
        for (int i = 0; i < EPLW / 4; ++i) {
            const wf32x4 sa = *reinterpret_cast<const wf32x4 *>(ew + c0 + 4 * i);
            const wf32x4 sb = *reinterpret_cast<const wf32x4 *>(ew + HP + c0 + 4 * i);
            const wf32x4 ta = *reinterpret_cast<const wf32x4 *>(ew + 2 * HP + c0 + 4 * i);
            const wf32x4 tb = *reinterpret_cast<const wf32x4 *>(ew + 3 * HP + c0 + 4 * i);
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                a[4 * i + k] = fmaf(sa[k], a[4 * i + k], ta[k]);
                b[4 * i + k] = fmaf(sb[k], b[4 * i + k], tb[k]);
            }
            if (i & 1) __builtin_amdgcn_sched_barrier(0);
        }
        if (logprob && !base_of_input) base_terms();

        ld += __shfl_xor(ld, 16, kWave);
        ld += __shfl_xor(ld, 32, kWave);
        sq += __shfl_xor(sq, 16, kWave);
        sq += __shfl_xor(sq, 32, kWave);
        if (q == 0) {
            red_s[wave * 16 + j] = ld;
            red_s[64 + wave * 16 + j] = sq;
        }
        if (z && live) {
            float *zr = z + row * (long long)D;
            if (vec == 4) {
                wide_store<EPLW, 4>(zr, 0, c0, half, D, reverse_out, a);
                wide_store<EPLW, 4>(zr, half, c0, half, D, reverse_out, b);
            } else if (vec == 2) {
                wide_store<EPLW, 2>(zr, 0, c0, half, D, reverse_out, a);
                wide_store<EPLW, 2>(zr, half, c0, half, D, reverse_out, b);
            } else {
                wide_store<EPLW, 1>(zr, 0, c0, half, D, reverse_out, a);
                wide_store<EPLW, 1>(zr, half, c0, half, D, reverse_out, b);
            }
        }
        __syncthreads();
        // (the next write to red_s lies behind the next tile's first coupling barrier, which wave 0 reaches after these reads)
        if (wave == 0 && q == 0 && live) {
            float ldt = ((red_s[j] + red_s[16 + j]) + red_s[32 + j]) + red_s[48 + j];
            ldt += ew[4 * HP];
            if (accumulate && logdet) ldt += logdet[row];
            if (logdet) logdet[row] = ldt;
            if (logprob) {
                const float sqt = ((red_s[64 + j] + red_s[80 + j]) + red_s[96 + j]) + red_s[112 + j];
                logprob[row] = (fmaf(-0.5f, sqt, -base_const)) + ldt;                   // flows.py:648
            }
        }
    }
}

template <int EPLW, int KIND>
static int launch_wide_k(const float *x, float *z, float *logdet, const float *loc, const float *log_scale,
                         float *logprob, int64_t N, int D, const float *params, const WideProg &prog, int flags, int vec,
                         hipStream_t s, const char *fn)
{
    auto kern = &k_flow_wide<EPLW, KIND>;
    int per_cu = 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kern, kWideBlock, 0) != hipSuccess || per_cu < 1) {
        (void)hipGetLastError();
        per_cu = 1;
    }
    if (per_cu > 8) per_cu = 8;
    const int64_t want = (N + 15) / 16;
    const int64_t cap = (int64_t)cu_count() * per_cu * kGridOversubscribe;
    const int grid = (int)(want < cap ? want : cap);
    hipLaunchKernelGGL(kern, dim3(grid), dim3(kWideBlock), 0, s, x, z, logdet, loc, log_scale, logprob, (long long)N, D,
                       params, prog, flags, vec);
    return check_launch(fn);
}

}  // namespace tfk
