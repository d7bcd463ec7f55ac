// tfk_glow_dsf.hip -- one launch per DEEP SIGMOIDAL coupling of the image / multiscale flows (kind 3 of tfk_glow_coupling:
// MultiscaleDeepSigmoid, DeepSigmoidGlow, MultiscaleBijection(transformer_class=DeepSigmoid)).
//
// The stages up to the 16 numbers per sample that feed the Linear layer are tfk_glow.hip's (tfk_glow.h: glow_background,
// glow_conditioner16); the arithmetic of a sigmoidal component is tfk_dsf.hip's (tfk_dsf.h).  New here is what lies
// between them.  The conditioner's output for one coupling is h (N, T, 3 K C) -- 90 floats per target element at the
// reference's K = 15, C = 2, i.e. 553 KB per sample for a checkerboard coupling of a (3, 32, 32) image whose row is
// 12 KB.  The layer-by-layer route writes it, bounds it and reads it back through HBM; here it never leaves the
// registers:
//
//  * Parameter generation.  Per group of 16 targets (neighbours in the row: the host sorts them by position) there are
//    P = 3 K C v_mfma_f32_16x16x4_f32 tiles of 16 samples x 16 targets, 4 k-steps each (K_gemm = 16), ordered
//    [component][da (K) | db (K) | dw (K)].  Lane (q, j) receives parameter p of target 16 m + j for the samples
//    4 q .. 4 q + 3, exactly where the affine kind receives (u, beta): every row access of a wave instruction is 4 rows x
//    16 neighbouring targets, whole 128-byte lines.  The bounded output -2 + 4 sigmoid(h) is applied to each accumulator
//    as it leaves the matrix core (W_eff / b_eff arrive times log2 e: one v_exp_f32).
//  * Register budget.  A component needs its 3 K parameters together (softmax over K), so a lane that kept all four
//    samples would hold 12 K raw parameters (180 VGPRs at K = 15) besides the extracted (a, b, w) and the unrolled
//    arithmetic of tfk_dsf.h, which alone wants about 10 K.  The tiles are cheap (4 MFMAs and one 1 KB operand that the
//    L2 serves), so above K = kGlowDsfAll4 the component's tiles are walked TWICE, each pass keeping two of the four
//    accumulator rows; up to it all four rows are kept in one pass.  NS (samples per pass) and the occupancy the register
//    allocator aims at (glow_dsf_waves: 3 waves per SIMD up to K = 5, 2 up to K = 10, 1 above) follow from K at compile
//    time; no instantiation uses scratch (DESIGN.md 3.3e lists VGPRs and occupancy for each).  No LDS staging: 16 samples x
//    16 targets x 3 K floats per wave (46 KB at K = 15) would take the room of the conv stages' slots.
//  * Components run first to last (inverse: last to first, the reference's bisection per element, bounded by
//    kDsfMaxTrips; its log-det is minus the forward one at the returned x).  A wave walks the target groups m = wave,
//    wave + nw, ...; nothing in that loop is a barrier, so partial groups and tiles (targets >= T, rows >= N: computed on
//    clamped inputs, not stored) leave every wave on the same barriers.
//  * Log-det per sample: __shfl_xor inside the 16-lane group, then across the waves through ldpart in wave order.
//
// Built without packed fp32 instructions (Makefile): the conv stages' float2 fmas are scalar pairs in this translation
// unit.
#include "tfk_dsf.h"
#include "tfk_glow.h"

namespace tfk {

constexpr int kGlowDsfAll4 = 4;                     // largest K whose four samples per lane are kept in one pass (image_program.layer_cost counts the second pass above it)
constexpr int kGlowDsfBlock = 256;                  // threads per workgroup at most (the register budget below assumes it)
__host__ __device__ constexpr int glow_dsf_ns(int K) { return K <= kGlowDsfAll4 ? 4 : 2; }
// waves per SIMD the register allocation aims at (the LDS allows three workgroups of four waves per CU)
__host__ __device__ constexpr int glow_dsf_waves(int K) { return K <= 5 ? 3 : (K <= 10 ? 2 : 1); }

template <int K, bool INV>
__global__ __launch_bounds__(kGlowDsfBlock) __attribute__((amdgpu_waves_per_eu(glow_dsf_waves(K)))) void k_glow_dsf(float *rows, float *logdet, long long N, GlowGeom g,
                                                            const int *__restrict__ src_idx,
                                                            const float2 *__restrict__ src_st,
                                                            const int *__restrict__ tgt_idx,
                                                            const float2 *__restrict__ tgt_st,
                                                            const float *__restrict__ wts, const float *__restrict__ bg1,
                                                            const float *__restrict__ bg2, const float4 *__restrict__ w_eff,
                                                            const float *__restrict__ b_eff)
{
    constexpr int NS = glow_dsf_ns(K), P1 = 3 * K;     // samples per pass; tiles (= parameters) of one component
    extern __shared__ float4 lds4[];
    float *lds = reinterpret_cast<float *>(lds4);
    float *V = lds;                                   // [16 samples][16]
    float *ldpart = lds + 256;                        // [waves][16 samples]
    float *slot0 = lds + g.fixed_floats;
    const int tid = threadIdx.x;
    // (the wave index as a scalar: the target group m, its tiles' addresses and the loops over them are then wave-uniform --
    // SGPR bases with the lane's offset as the only VGPR, instead of a 64-bit VGPR address per unrolled tile)
    const int lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6), nw = blockDim.x >> 6;
    const int D = g.D, C = g.n_ch;
    const int n_groups = (g.T + 15) >> 4;

    glow_background(g, slot0, wts, bg1, bg2);

    const long long n_tiles_rows = (N + g.tile_rows - 1) / g.tile_rows;
    for (long long tile = blockIdx.x; tile < n_tiles_rows; tile += gridDim.x) {
        const long long row_base = tile * g.tile_rows;
        const int nrows = (int)((N - row_base) < (long long)g.tile_rows ? (N - row_base) : (long long)g.tile_rows);

        glow_conditioner16(g, rows, N, row_base, slot0, V, src_idx, src_st, wts);

        const int j = lane & 15, q = lane >> 4;
        float bq[4];
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) bq[ks] = V[j * 16 + 4 * ks + q];
        float ldr[4] = {0.0f, 0.0f, 0.0f, 0.0f};
        float *xr0 = rows + (row_base + 4 * q) * D;
        bool ok[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) ok[r] = 4 * q + r < nrows;
        for (int m = (g.skip & 4) ? n_groups : wave; m < n_groups; m += nw) {
            const int ph = tgt_idx[16 * m + j];                      // (tables padded to whole groups of 16)
            const float2 pst = tgt_st[16 * m + j];
            float v[4], ld[4];
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                v[r] = fmaf(pst.x, ok[r] ? xr0[(long long)r * D + ph] : 0.0f, pst.y);
                ld[r] = 0.0f;
            }
            for (int i = 0; i < C; ++i) {
                const int comp = INV ? C - 1 - i : i;
                const size_t t0 = ((size_t)m * C + comp) * P1;      // the component's first tile
                const float4 *wt = w_eff + t0 * 64;
                const float *bt = b_eff + t0 * 16;
                // A ROLLED loop over the passes: unrolled, the second pass's operand loads and MFMAs are the first's, the
                // compiler merges them and keeps all four rows after all.  The samples of the pass are v[0 .. NS); the
                // arrays are rotated by NS behind it (back in place after the last pass).
#pragma unroll 1
                for (int pass = 0; pass < 4 / NS; ++pass) {
                    float p[NS][P1];
#pragma unroll
                    for (int t = 0; t < P1; ++t) {
                        const float4 a = wt[t * 64 + lane];
                        const float b = bt[t * 16 + j];
                        gf32x4 acc = {0.0f, 0.0f, 0.0f, 0.0f};
                        acc = __builtin_amdgcn_mfma_f32_16x16x4f32(bq[0], a.x, acc, 0, 0, 0);
                        acc = __builtin_amdgcn_mfma_f32_16x16x4f32(bq[1], a.y, acc, 0, 0, 0);
                        acc = __builtin_amdgcn_mfma_f32_16x16x4f32(bq[2], a.z, acc, 0, 0, 0);
                        acc = __builtin_amdgcn_mfma_f32_16x16x4f32(bq[3], a.w, acc, 0, 0, 0);
                        // The bounded parameter is made HERE: left to itself the compiler sinks it to its use inside
                        // dsf_extract and keeps the tile's four accumulator rows (12 K VGPRs) instead of the pass's NS.
                        if (NS == 4) {
#pragma unroll
                            for (int s = 0; s < 4; ++s) p[s][t] = bounded4(acc[s] + b);
                        } else {
                            p[0][t] = bounded4((pass ? acc[2] : acc[0]) + b);
                            p[1][t] = bounded4((pass ? acc[3] : acc[1]) + b);
                        }
#pragma unroll
                        for (int s = 0; s < NS; ++s) asm volatile("" : "+v"(p[s][t]));
                        // (and four tiles' operands in flight, not all 3 K of them: 15 K VGPRs hoisted to the top)
                        if ((t & 3) == 3) __builtin_amdgcn_sched_barrier(0);
                    }
#pragma unroll
                    for (int s = 0; s < NS; ++s) {
                        DsfComp<K> qc;
                        dsf_extract<K>(p[s], qc);
                        dsf_step<K, INV>(qc, v[s], ld[s]);
                        asm volatile("" : "+v"(v[s]), "+v"(ld[s]));     // one sample's (a, b, w) at a time
                    }
                    if (NS < 4) {                                  // rotate left by NS
                        float tv[NS], tl[NS];
#pragma unroll
                        for (int s = 0; s < NS; ++s) tv[s] = v[s], tl[s] = ld[s];
#pragma unroll
                        for (int r = 0; r < 4 - NS; ++r) v[r] = v[r + NS], ld[r] = ld[r + NS];
#pragma unroll
                        for (int s = 0; s < NS; ++s) v[4 - NS + s] = tv[s], ld[4 - NS + s] = tl[s];
                    }
                }
            }
            const bool tgt_ok = 16 * m + j < g.T;
#pragma unroll
            for (int r = 0; r < 4; ++r)
                if (tgt_ok && ok[r]) {
                    xr0[(long long)r * D + ph] = v[r];
                    ldr[r] += ld[r];
                }
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) {
#pragma unroll
            for (int o = 1; o < 16; o <<= 1) ldr[r] += __shfl_xor(ldr[r], o, kWave);
            if (j == 0) ldpart[wave * 16 + 4 * q + r] = ldr[r];
        }
        __syncthreads();
        if (tid < nrows) {
            float s = 0.0f;
            for (int w = 0; w < nw; ++w) s += ldpart[w * 16 + tid];
            logdet[row_base + tid] += s;
        }
        __syncthreads();                                        // V, ldpart are free again
    }
}

#define TFK_GLOW_DSF_FOR_EACH_K(X) \
    X(1) X(2) X(3) X(4) X(5) X(6) X(7) X(8) X(9) X(10) X(11) X(12) X(13) X(14) X(15) X(16)

template <int K, bool INV>
static int glow_dsf_launch_k(float *rows, float *logdet, int64_t N, const GlowGeom &g, int block, size_t lds,
                             const tfk_glow_layer *layer, hipStream_t s, const char *fn)
{
    auto kern = k_glow_dsf<K, INV>;
    const void *kp = reinterpret_cast<const void *>(kern);
    // The LDS limit (an attribute per DEVICE) and the workgroups per CU -- what registers AND the LDS allow; the LDS alone
    // would promise three where K = 15 fits one -- are asked once per (device, block, LDS size) of this instantiation.
    thread_local int c_dev = -1, c_block = 0, c_per_cu = 0;
    thread_local size_t c_lds = 0;
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) return fail(TFK_ENODEV, "%s: %s", fn, hipGetErrorString(hipGetLastError()));
    if (dev != c_dev || block != c_block || lds != c_lds) {
        if (hipFuncSetAttribute(kp, hipFuncAttributeMaxDynamicSharedMemorySize, kGlowLdsBytes) != hipSuccess)
            return fail(TFK_ELAUNCH, "%s: cannot raise the dynamic LDS limit: %s", fn, hipGetErrorString(hipGetLastError()));
        int n = 0;
        if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, kp, block, lds) != hipSuccess || n < 1) {
            (void)hipGetLastError();
            n = imax(1, imin((int)(kGlowLdsBytes / lds), 2048 / block));
        }
        c_dev = dev, c_block = block, c_lds = lds, c_per_cu = n;
    }
    const int per_cu = c_per_cu;
    const int64_t tiles = (N + g.tile_rows - 1) / g.tile_rows;
    int64_t grid = layer->grid > 0 ? layer->grid : (int64_t)cu_count() * per_cu;
    if (grid > tiles) grid = tiles;
    hipLaunchKernelGGL(kern, dim3((unsigned)grid), dim3(block), lds, s, rows, logdet, (long long)N, g, layer->src_idx,
                       reinterpret_cast<const float2 *>(layer->src_st), layer->tgt_idx,
                       reinterpret_cast<const float2 *>(layer->tgt_st), layer->weights, layer->bg1, layer->bg2,
                       reinterpret_cast<const float4 *>(layer->w_eff), layer->b_eff);
    return check_launch(fn);
}

int glow_dsf_launch(float *rows, float *logdet, int64_t N, const GlowGeom &g, int block, size_t lds,
                    const tfk_glow_layer *layer, int inverse, hipStream_t s, const char *fn)
{
    if (block > kGlowDsfBlock)
        return fail(TFK_EINVAL, "%s: a deep sigmoidal coupling runs in workgroups of at most %d threads, got %d", fn,
                    kGlowDsfBlock, block);
    switch (g.hw) {
#define TFK_GLOW_DSF_CASE(K_)                                                                               \
    case K_:                                                                                                \
        return inverse ? glow_dsf_launch_k<K_, true>(rows, logdet, N, g, block, lds, layer, s, fn)         \
                       : glow_dsf_launch_k<K_, false>(rows, logdet, N, g, block, lds, layer, s, fn);
        TFK_GLOW_DSF_FOR_EACH_K(TFK_GLOW_DSF_CASE)
#undef TFK_GLOW_DSF_CASE
    }
    return fail(TFK_EINVAL, "%s: no deep sigmoidal kernel for hidden_dim %d", fn, g.hw);
}

}  // namespace tfk
