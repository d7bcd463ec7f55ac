// tfk_glow_resnet.hip -- one launch per AFFINE or SHIFT coupling whose conditioner is the ResNet (kinds 4 and 6 of
// tfk_glow_coupling: MultiscaleBijection(use_resnet=True) and every image preset that forwards the keyword).
//
// Replaces, for one coupling, in place on the rows (same tables, pending maps and log-det convention as kinds 0 and 2):
//   x_A = x[..., source_mask].view(constant_shape)
//   ConvModifier -> (4, 32, 32)                                             multiscale/conditioning/resnet.py:83
//   3 x [ x + relu(bn2(conv2(relu(bn1(conv1(x))))))  (C -> 16 -> C),  conv3x3 stride 2 (C -> 2 C) ]   C = 4, 8, 16     :85-92
//   Linear(512, 100), leaky_relu, Linear(100, n_params)                      :94-118
//   h = -2 + 4 sigmoid(h);  Affine / Shift forward or inverse;  z[..., target_mask] = ...
// BatchNorm sits in front of the ReLU, so the host folds it into the convolutions: the kernel sees nine plain
// convolutions, three residual adds and two Linear layers (image_program._pack_resnet_conditioner).
//
// Work split.  A workgroup of 256 lanes owns a tile of 16 samples (= the MFMA's N).  The trunk runs for G <= 3 resident
// samples at a time (a slot is two buffers of 4 x 34 x 34 floats, 37 KB: G = 3 is what the 160 KB of LDS hold besides the
// park) and leaves each sample's 512 features in a park of 16 x 516 floats; the head then runs ONCE per tile on the matrix
// cores.  Full frames are computed: this conditioner only ever sees the outermost block's images, which fill most of
// the 32 x 32 frame, so there is no receptive-field window and the LDS need does not depend on the layer.
//
// Trunk.  An activation lives in the LDS with a one-pixel zero halo, so no tap tests its bounds.  The two buffers A and B
// of a slot change roles from stage to stage:
//   stage 1   x (4, 34, 34) in A        hidden group (4, 34, 34) in B
//   down 1    A -> B as (8, 18, 18)
//   stage 2   x in B[0, 2592)           hidden group (4, 18, 18) in B[2592, 3888)
//   down 2    B -> A as (16, 10, 10)
//   stage 3   x in A[0, 1600)           hidden group (4, 10, 10) in A[1600, 2000)
//   down 3    A -> park[sample][c * 16 + y * 4 + x]
// The 16 hidden channels of a residual block are produced FOUR AT A TIME into the hidden buffer; conv2 accumulates over
// the four groups in registers (a lane owns the same (sample, pixel, 4 output channels) tasks in every group: 12, 6 and 3
// tasks per lane at G = 3), so the 16-channel hidden image -- 74 KB per sample at stage 1 -- never exists.  x + relu(.)
// is written back over x behind a barrier; the same phase zeroes the cells the next stage's halos need.  Lane task =
// one pixel x 4 output channels; a wave's 64 tasks share the channel group, so the weights ([ci][ky][kx][co]) are
// wave-uniform scalar loads.  The stride-2 convolutions read x[2 y + k - 1] from the same haloed buffer.
//
// Head.  linear1 (M = 100 in 7 tiles of 16, rows of padding zero; K = 512): v_mfma_f32_16x16x4_f32 with the weight tiles
// as A (global memory, one float4 = four k-steps per lane) and the park as B (one ds_read_b128 = four k-steps); the four
// waves split K (eight 16-wide blocks each) and keep all seven tiles' accumulators, the partial sums meet in the LDS.
// Every wave then builds its 25 B operands of linear2 (bias, sum of the four parts, leaky_relu) in registers and walks
// its target groups exactly as kinds 0 and 2 do (tfk_glow.hip): kGlowPB groups per step, K = 100 in 25 k-steps, the
// bounded output, the transform, the log-det reduction, the store.
//
// Deviations from the first plan, and why: (1) built WITHOUT packed fp32 instructions, like tfk_glow_dsf.hip (new code
// here is; the channel pairs are scalar fmas), (2) the transform tail is restated here, not shared through tfk_glow.h, so
// that tfk_glow.hip's kernels are byte for byte the parent's.
#include "tfk_glow.h"

namespace tfk {

constexpr int kRnBuf = 4 * 34 * 34;                // one of the two buffers of a slot
constexpr int kRnSlot = 2 * kRnBuf;                // floats per resident sample
constexpr int kRnMaxSlots = 3;
constexpr int kRnBlock = 256;                      // four waves: the K split of linear1 and the task tables assume it
constexpr int kRnPark = 516;                       // floats per sample in the park (512 + 4: float4 reads, rows on different banks)
constexpr int kRnHidTiles = 7, kRnHidRows = 16 * kRnHidTiles;       // linear1's 100 rows in tiles of 16
constexpr int kRnK2 = 25, kRnKB2 = 7;              // linear2: k-steps of 4, float4 blocks of four k-steps
constexpr int kRnFixed = kGlowMaxRows * kRnPark + 64;               // park + ldpart

// float offsets of the folded trunk inside `weights`, behind the modifier (tfk.h): per stage of C channels
// conv1 [C][9][16], b1 (16), conv2 [16][9][C], b2 (C), down [C][9][2 C], bd (2 C)
__host__ __device__ constexpr int rn_stage_floats(int C) { return 18 * C * C + 291 * C + 16; }
__host__ __device__ constexpr int rn_trunk_floats() { return rn_stage_floats(4) + rn_stage_floats(8) + rn_stage_floats(16); }

// A: bias inside the frame, zero halo; B: zero.  Ends WITHOUT a barrier.
__device__ __forceinline__ void rn_fill(float *slot0, int Gr, const float *__restrict__ bm)
{
    for (int t = threadIdx.x; t < Gr * kRnSlot; t += kRnBlock) {
        const int e = t % kRnSlot;
        float v = 0.0f;
        if (e < kRnBuf) {
            const int ch = e / 1156, r = e - ch * 1156, y = r / 34, x = r - y * 34;
            if (y >= 1 && y <= 32 && x >= 1 && x <= 32) v = bm[ch];
        }
        slot0[t] = v;
    }
}

// x <- x + relu(conv2(relu(conv1(x)))) for Gr resident samples; x (C, S + 2, S + 2) at X, the hidden group (4, S + 2, S + 2)
// at H (halo already zero), both offsets into a slot.  Behind it zero_n floats from zero_at of every slot are cleared.
// Ends with a barrier.
template <int C, int S>
__device__ __forceinline__ void rn_res_block(float *X, float *H, int Gr, const float *__restrict__ w1,
                                             const float *__restrict__ b1, const float *__restrict__ w2,
                                             const float *__restrict__ b2, float *zero_at, int zero_n)
{
    constexpr int P = S + 2, PL = P * P, NPIX = S * S, NGO = C / 4;
    constexpr int MAXI = (((kRnMaxSlots * NPIX + 63) / 64) * NGO + 3) / 4;      // conv2 tasks per lane at most
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int n = Gr * NPIX, chunks = (n + 63) >> 6, total = chunks * NGO;
    float acc[MAXI][4];
#pragma unroll
    for (int i = 0; i < MAXI; ++i) acc[i][0] = acc[i][1] = acc[i][2] = acc[i][3] = 0.0f;
#pragma unroll 1
    for (int hg = 0; hg < 4; ++hg) {
        // conv1 + ReLU: hidden channels 4 hg .. 4 hg + 3
        for (int t = threadIdx.x; t < n; t += kRnBlock) {
            const int slot = t / NPIX, pix = t - slot * NPIX, y = pix / S, x = pix - y * S;
            const float *ip = X + slot * kRnSlot + y * P + x;           // the 3x3 patch's first cell (halo coordinates)
            float a[4] = {b1[4 * hg], b1[4 * hg + 1], b1[4 * hg + 2], b1[4 * hg + 3]};
#pragma unroll 2
            for (int ci = 0; ci < C; ++ci) {
                const float *wc = w1 + ci * 144 + 4 * hg;
#pragma unroll
                for (int k = 0; k < 9; ++k) {
                    const float v = ip[ci * PL + (k / 3) * P + k % 3];
#pragma unroll
                    for (int o = 0; o < 4; ++o) a[o] = fmaf(wc[k * 16 + o], v, a[o]);
                }
            }
            float *hp = H + slot * kRnSlot + (y + 1) * P + x + 1;
#pragma unroll
            for (int o = 0; o < 4; ++o) hp[o * PL] = fmaxf(a[o], 0.0f);
        }
        __syncthreads();
        // conv2: this group's four input channels into the lane's accumulators
#pragma unroll
        for (int i = 0; i < MAXI; ++i) {
            const int c = wave + 4 * i;
            if (c < total) {
                const int cgi = c / chunks;
                int t = (c - cgi * chunks) * 64 + lane;
                t = t < n ? t : n - 1;
                const int slot = t / NPIX, pix = t - slot * NPIX, y = pix / S, x = pix - y * S;
                const float *hp = H + slot * kRnSlot + y * P + x;
#pragma unroll
                for (int cl = 0; cl < 4; ++cl) {
                    const float *wc = w2 + (4 * hg + cl) * 9 * C + 4 * cgi;
#pragma unroll
                    for (int k = 0; k < 9; ++k) {
                        const float v = hp[cl * PL + (k / 3) * P + k % 3];
#pragma unroll
                        for (int o = 0; o < 4; ++o) acc[i][o] = fmaf(wc[k * C + o], v, acc[i][o]);
                    }
                }
            }
        }
        __syncthreads();
    }
#pragma unroll
    for (int i = 0; i < MAXI; ++i) {
        const int c = wave + 4 * i;
        if (c < total) {
            const int cgi = c / chunks;
            const int t = (c - cgi * chunks) * 64 + lane;
            if (t < n) {
                const int slot = t / NPIX, pix = t - slot * NPIX, y = pix / S, x = pix - y * S;
                float *xp = X + slot * kRnSlot + (4 * cgi) * PL + (y + 1) * P + x + 1;
#pragma unroll
                for (int o = 0; o < 4; ++o) xp[o * PL] += fmaxf(acc[i][o] + b2[4 * cgi + o], 0.0f);
            }
        }
    }
    for (int t = threadIdx.x; t < Gr * zero_n; t += kRnBlock) {
        const int slot = t / zero_n;
        zero_at[slot * kRnSlot + (t - slot * zero_n)] = 0.0f;
    }
    __syncthreads();
}

// conv3x3, stride 2, padding 1, C -> 2 C channels: (C, S + 2, S + 2) at `in` to (2 C, S / 2 + 2, S / 2 + 2) at `out` (halo
// already zero), or, PARK, to the sample's 512 features in (c, y, x) order.  Ends with a barrier.
template <int C, int S, bool PARK>
__device__ __forceinline__ void rn_down(const float *in, float *out, int Gr, const float *__restrict__ w,
                                        const float *__restrict__ bias)
{
    constexpr int P = S + 2, PL = P * P, SO = S / 2, NPO = SO * SO, PO = SO + 2, PLO = PO * PO, CO = 2 * C, NGO = CO / 4;
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int n = Gr * NPO, chunks = (n + 63) >> 6, total = chunks * NGO;
    for (int c = wave; c < total; c += 4) {
        const int cgi = c / chunks;
        const int t = (c - cgi * chunks) * 64 + lane;
        const int tt = t < n ? t : n - 1;
        const int slot = tt / NPO, pix = tt - slot * NPO, y = pix / SO, x = pix - y * SO;
        const float *ip = in + slot * kRnSlot + 2 * y * P + 2 * x;      // x[2 y + k - 1] in halo coordinates
        float a[4] = {bias[4 * cgi], bias[4 * cgi + 1], bias[4 * cgi + 2], bias[4 * cgi + 3]};
#pragma unroll 2
        for (int ci = 0; ci < C; ++ci) {
            const float *wc = w + ci * 9 * CO + 4 * cgi;
#pragma unroll
            for (int k = 0; k < 9; ++k) {
                const float v = ip[ci * PL + (k / 3) * P + k % 3];
#pragma unroll
                for (int o = 0; o < 4; ++o) a[o] = fmaf(wc[k * CO + o], v, a[o]);
            }
        }
        if (t < n) {
#pragma unroll
            for (int o = 0; o < 4; ++o) {
                if (PARK) out[slot * kRnPark + (4 * cgi + o) * NPO + pix] = a[o];
                else out[slot * kRnSlot + (4 * cgi + o) * PLO + (y + 1) * PO + x + 1] = a[o];
            }
        }
    }
    __syncthreads();
}

template <bool SHIFT, bool INV>
__global__ __launch_bounds__(kRnBlock) void k_glow_resnet(float *rows, float *logdet, long long N, GlowGeom g,
                                                          const int *__restrict__ src_idx,
                                                          const float2 *__restrict__ src_st,
                                                          const int *__restrict__ tgt_idx,
                                                          const float2 *__restrict__ tgt_st,
                                                          const float *__restrict__ wts,
                                                          const float4 *__restrict__ w1t, const float *__restrict__ bias1,
                                                          const float4 *__restrict__ w_eff,
                                                          const float *__restrict__ b_eff)
{
    extern __shared__ float4 lds4[];
    float *lds = reinterpret_cast<float *>(lds4);
    float *park = lds;                                // [16 samples][kRnPark]
    float *ldpart = lds + kGlowMaxRows * kRnPark;     // [4 waves][16 samples]
    float *slot0 = lds + kRnFixed;                    // G slots; the head's partial sums [4 waves][112][16] afterwards
    float *A = slot0, *B = slot0 + kRnBuf;
    const int tid = threadIdx.x;
    const int lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int D = g.D, G = g.slots;
    // the folded trunk behind the modifier
    const float *s1 = wts + gw_bm(g.cm) + 4, *s2 = s1 + rn_stage_floats(4), *s3 = s2 + rn_stage_floats(8);

    const long long n_tiles_rows = (N + kGlowMaxRows - 1) / kGlowMaxRows;
    for (long long tile = blockIdx.x; tile < n_tiles_rows; tile += gridDim.x) {
        const long long row_base = tile * kGlowMaxRows;
        const int nrows = (int)((N - row_base) < (long long)kGlowMaxRows ? (N - row_base) : (long long)kGlowMaxRows);

        // ---- trunk: G samples per round; rounds past the tile's last row are skipped (their park rows feed MFMA columns
        //      that nothing stores) ----
        for (int r0 = 0; r0 < nrows; r0 += G) {
            const int Gr = G < kGlowMaxRows - r0 ? G : kGlowMaxRows - r0;
            rn_fill(slot0, Gr, wts + gw_bm(g.cm));
            __syncthreads();
            if (g.kh * g.kw == 1) s0_modifier<true>(g, rows, N, row_base + r0, Gr, slot0, src_idx, src_st, wts);
            else s0_modifier<false>(g, rows, N, row_base + r0, Gr, slot0, src_idx, src_st, wts);
            __syncthreads();
            rn_res_block<4, 32>(A, B, Gr, s1, s1 + 576, s1 + 592, s1 + 1168, B, 3888);
            rn_down<4, 32, false>(A, B, Gr, s1 + 1172, s1 + 1460);
            rn_res_block<8, 16>(B, B + 2592, Gr, s2, s2 + 1152, s2 + 1168, s2 + 2320, A, 2000);
            rn_down<8, 16, false>(B, A, Gr, s2 + 2328, s2 + 3480);
            rn_res_block<16, 8>(A, A + 1600, Gr, s3, s3 + 2304, s3 + 2320, s3 + 4624, A, 0);
            rn_down<16, 8, true>(A, park + r0 * kRnPark, Gr, s3 + 4640, s3 + 9248);
        }

        // ---- linear1 on the matrix cores: wave w takes K blocks 8 w .. 8 w + 7 of all seven tiles ----
        const int j = lane & 15, q = lane >> 4;
        {
            gf32x4 h1[kRnHidTiles];
#pragma unroll
            for (int t = 0; t < kRnHidTiles; ++t) h1[t] = gf32x4{0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll 2
            for (int kb = 8 * wave; kb < 8 * wave + 8; ++kb) {
                const float4 b = *reinterpret_cast<const float4 *>(park + j * kRnPark + 16 * kb + 4 * q);
#pragma unroll
                for (int t = 0; t < kRnHidTiles; ++t) {
                    const float4 a = w1t[(t * 32 + kb) * 64 + lane];
                    h1[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(a.x, b.x, h1[t], 0, 0, 0);
                    h1[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(a.y, b.y, h1[t], 0, 0, 0);
                    h1[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(a.z, b.z, h1[t], 0, 0, 0);
                    h1[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(a.w, b.w, h1[t], 0, 0, 0);
                }
            }
            // (the slots were last read by down 3, one barrier ago)
#pragma unroll
            for (int t = 0; t < kRnHidTiles; ++t)
#pragma unroll
                for (int r = 0; r < 4; ++r) slot0[wave * (16 * kRnHidRows) + (16 * t + 4 * q + r) * 16 + j] = h1[t][r];
        }
        __syncthreads();
        // ---- linear2's B operands: hidden unit 4 ks + q of sample j ----
        float bq[kRnK2];
#pragma unroll
        for (int ks = 0; ks < kRnK2; ++ks) {
            const int m = 4 * ks + q;
            float v = bias1[m];
#pragma unroll
            for (int w = 0; w < 4; ++w) v += slot0[w * (16 * kRnHidRows) + m * 16 + j];
            bq[ks] = v > 0.0f ? v : 0.01f * v;                          // leaky_relu, slope 0.01
        }
        // ---- linear2 + bounded output + transform: tfk_glow.hip's loop with K = 100 ----
        constexpr int TPG = SHIFT ? 1 : 2;                              // MFMA tiles per group of 16 targets
        const int n_pairs = g.n_tiles / TPG;
        float ldr[4] = {0.0f, 0.0f, 0.0f, 0.0f};
        float *xr0 = rows + (row_base + 4 * q) * D;
        bool ok[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) ok[r] = 4 * q + r < nrows;
        for (int pb = kGlowPB * wave; pb < n_pairs; pb += kGlowPB * 4) {
            float4 au[kGlowPB][kRnKB2], ab[kGlowPB][kRnKB2];
            float bu[kGlowPB], bb[kGlowPB], x[kGlowPB][4];
            float2 pst[kGlowPB];
            int ph[kGlowPB];
#pragma unroll
            for (int u = 0; u < kGlowPB; ++u) {
                const int m = pb + u < n_pairs ? pb + u : n_pairs - 1;
#pragma unroll
                for (int kb = 0; kb < kRnKB2; ++kb) {
                    au[u][kb] = SHIFT ? float4{0.0f, 0.0f, 0.0f, 0.0f} : w_eff[((size_t)(TPG * m) * kRnKB2 + kb) * 64 + lane];
                    ab[u][kb] = w_eff[((size_t)(TPG * m + TPG - 1) * kRnKB2 + kb) * 64 + lane];
                }
                bu[u] = b_eff[16 * TPG * m + j];
                bb[u] = b_eff[16 * TPG * m + 16 * (TPG - 1) + j];
                ph[u] = tgt_idx[16 * m + j];                            // (tables padded to whole groups of 16)
                pst[u] = tgt_st[16 * m + j];
            }
#pragma unroll
            for (int u = 0; u < kGlowPB; ++u)
#pragma unroll
                for (int r = 0; r < 4; ++r) x[u][r] = ok[r] ? xr0[(long long)r * D + ph[u]] : 0.0f;
#pragma unroll
            for (int u = 0; u < kGlowPB; ++u) {
                gf32x4 hu = {bu[u], bu[u], bu[u], bu[u]}, hb = {bb[u], bb[u], bb[u], bb[u]};
#pragma unroll
                for (int kb = 0; kb < kRnKB2; ++kb) {
                    const float ua[4] = {au[u][kb].x, au[u][kb].y, au[u][kb].z, au[u][kb].w};
                    const float ba[4] = {ab[u][kb].x, ab[u][kb].y, ab[u][kb].z, ab[u][kb].w};
#pragma unroll
                    for (int ks = 0; ks < 4; ++ks)
                        if (4 * kb + ks < kRnK2) {
                            if (!SHIFT) hu = __builtin_amdgcn_mfma_f32_16x16x4f32(bq[4 * kb + ks], ua[ks], hu, 0, 0, 0);
                            hb = __builtin_amdgcn_mfma_f32_16x16x4f32(bq[4 * kb + ks], ba[ks], hb, 0, 0, 0);
                        }
                }
                const bool tgt_ok = pb + u < n_pairs && 16 * (pb + u) + j < g.T;
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const float beta = bounded4(hb[r]);
                    const float v = fmaf(pst[u].x, x[u][r], pst[u].y);
                    float out, wl = 0.0f;
                    if (SHIFT) {
                        out = INV ? v - beta : v + beta;
                    } else {
                        const float u_ = bounded4(hu[r]);
                        wl = fmaf(u_, 0.5f, kAffC0);                    // affine.py:33-34, as tfk_glow.hip
                        const float alpha = __builtin_amdgcn_exp2f(wl * __int_as_float(0x3fb8aa3b)) + kAffMinScale;
                        out = INV ? (v - beta) * __builtin_amdgcn_rcpf(alpha) : alpha * v + beta;
                    }
                    if (tgt_ok && ok[r]) {
                        xr0[(long long)r * D + ph[u]] = out;
                        ldr[r] += INV ? -wl : wl;
                    }
                }
            }
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) {
#pragma unroll
            for (int o = 1; o < 16; o <<= 1) ldr[r] += __shfl_xor(ldr[r], o, kWave);
            if (j == 0) ldpart[wave * 16 + 4 * q + r] = ldr[r];
        }
        __syncthreads();
        if (!SHIFT && tid < nrows) {
            float s = 0.0f;
            for (int w = 0; w < 4; ++w) s += ldpart[w * 16 + tid];
            logdet[row_base + tid] += s;
        }
        __syncthreads();                                        // park, ldpart and the partial sums are free again
    }
}

// geometry of kinds 4 and 6 behind glow_geometry_base: the modifier writes into buffer A (34 x 34 with the halo)
void glow_resnet_geometry(GlowGeom &g)
{
    g.a0h = g.a0w = 34, g.a0y0 = g.a0x0 = -1;
    g.slot_floats = kRnSlot, g.fixed_floats = kRnFixed;
    g.h_stride = 0;
}

bool glow_resnet_plan(GlowGeom &g, int want_slots, int want_block, int *block_out)
{
    if ((want_block && want_block != kRnBlock) || want_slots < 0 || want_slots > kRnMaxSlots) return false;
    g.slots = want_slots ? want_slots : kRnMaxSlots;
    if (4 * (kRnFixed + g.slots * kRnSlot) > kGlowLdsBytes - 1024) return false;
    g.cg1 = g.cg2 = 4, g.tile_rows = kGlowMaxRows;
    *block_out = kRnBlock;
    return true;
}

int glow_resnet_launch(float *rows, float *logdet, int64_t N, const GlowGeom &g, int block, size_t lds,
                       const tfk_glow_layer *layer, int inverse, hipStream_t s, const char *fn)
{
    if (block != kRnBlock || g.slots < 1 || g.slots > kRnMaxSlots || g.tile_rows != kGlowMaxRows)
        return fail(TFK_EINVAL, "%s: a ResNet coupling runs in workgroups of %d threads with 1 .. %d slots", fn, kRnBlock,
                    kRnMaxSlots);
    if (!layer->bg1 || !aligned16(layer->bg1))
        return fail(TFK_EINVAL, "%s: bg1 (linear1 in tile order) needs 16-byte alignment", fn);
    const int64_t tiles = (N + kGlowMaxRows - 1) / kGlowMaxRows;
    const int wgs_per_cu = imax(1, (int)(kGlowLdsBytes / lds));
    int64_t grid = layer->grid > 0 ? layer->grid : (int64_t)cu_count() * wgs_per_cu;
    if (grid > tiles) grid = tiles;
    const float4 *w1t = reinterpret_cast<const float4 *>(layer->bg1);
    const float *bias1 = layer->bg1 + (size_t)kRnHidTiles * 32 * 64 * 4;
#define TFK_GLOW_RN(S_, I_)                                                                                          \
    do {                                                                                                             \
        auto kern = k_glow_resnet<S_, I_>;                                                                           \
        if (hipFuncSetAttribute(reinterpret_cast<const void *>(kern), hipFuncAttributeMaxDynamicSharedMemorySize,    \
                                kGlowLdsBytes) != hipSuccess)                                                        \
            return fail(TFK_ELAUNCH, "%s: cannot raise the dynamic LDS limit: %s", fn,                               \
                        hipGetErrorString(hipGetLastError()));                                                       \
        hipLaunchKernelGGL(kern, dim3((unsigned)grid), dim3(block), lds, s, rows, logdet, (long long)N, g,           \
                           layer->src_idx, reinterpret_cast<const float2 *>(layer->src_st), layer->tgt_idx,          \
                           reinterpret_cast<const float2 *>(layer->tgt_st), layer->weights, w1t, bias1,              \
                           reinterpret_cast<const float4 *>(layer->w_eff), layer->b_eff);                            \
    } while (0)
    const bool shift = (g.kind & 3) == 2;
    if (!shift && !inverse) TFK_GLOW_RN(false, false);
    else if (!shift) TFK_GLOW_RN(false, true);
    else if (!inverse) TFK_GLOW_RN(true, false);
    else TFK_GLOW_RN(true, true);
#undef TFK_GLOW_RN
    return check_launch(fn);
}

}  // namespace tfk
