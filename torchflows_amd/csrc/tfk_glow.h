// tfk_glow.h -- what the one-launch-per-coupling kernel (tfk_glow.hip) and the level kernel (tfk_glow_level.hip: several
// couplings per launch on rows held in the LDS) share: the geometry of a convolutional coupling, the packed weight
// layout, the conv3x3 -> ReLU -> MaxPool -> affine stage and the window arithmetic.
#pragma once

#include <cstdlib>

#include "tfk_common.h"

namespace tfk {

typedef float gf32x4 __attribute__((ext_vector_type(4)));
typedef float gf32x2 __attribute__((ext_vector_type(2)));

constexpr int kGlowMaxRows = 16;        // samples per tile = MFMA N
constexpr int kGlowMaxCh = 16;          // 1x1 convolution: target channels kept in registers
#ifndef TFK_GLOW_PB
#define TFK_GLOW_PB 2
#endif
constexpr int kGlowPB = TFK_GLOW_PB;     // target groups (of 16) per wave and step of the Linear / transform loop
constexpr int kGlowFrame = 32;          // ConvModifier's target height / width (classic.py:13-16)

struct GlowGeom {
    int c_in, hi, wi, oy, ox;           // source image; where the modifier's non-constant rectangle starts in the 32x32 frame
    int kh, kw, rh, rw, cm;             // modifier kernel (1 or 2 per axis); the rectangle's size (hi + kh - 1, wi + kw - 1); c_in kh kw
    int a0h, a0w, a0y0, a0x0;           // modifier output buffer (4 channels): dims, frame coordinates of its origin
    int p1h, p1w, p1y0, p1x0;           // pooled-1 window computed per sample (16x16 frame)
    int b1h, b1w, b1y0, b1x0;           // pooled-1 buffer (8 channels)
    int p2h, p2w, p2y0, p2x0;           // pooled-2 window (8x8 frame); its buffer is always 10x10 at (-1,-1)
    int off_p1, off_p2, off_p3, slot_floats;   // float offsets inside a slot
    int fixed_floats;                   // LDS floats in front of the slots
    int slots, tile_rows;               // G, NS
    int T, n_params, n_tiles, D;
    int kind, n_ch, hw;                 // 1x1 convolution: channels, pixels; deep sigmoidal: components C, hidden_dim K
    int cg1, cg2;                       // output channels per lane task in conv block 1 / 2
    int h_stride;                       // kind 1: floats per sample in the parameter buffer
    int skip;                           // timing ablations only (TFK_GLOW_SKIP): 1 no S0, 2 no conv blocks, 4 no Linear / transform
};

// offsets into the packed fp32 weights of a layer (see tfk.h: tfk_glow_layer.weights)
__host__ __device__ inline int gw_bm(int c_in) { return 4 * c_in; }
__host__ __device__ inline int gw_w1(int c_in) { return 4 * c_in + 4; }
__host__ __device__ inline int gw_b1(int c_in) { return gw_w1(c_in) + 4 * 8 * 9; }
__host__ __device__ inline int gw_w2(int c_in) { return gw_b1(c_in) + 24; }
__host__ __device__ inline int gw_b2(int c_in) { return gw_w2(c_in) + 8 * 8 * 9; }
__host__ __device__ inline int gw_w3(int c_in) { return gw_b2(c_in) + 24; }
__host__ __device__ inline int gw_b3(int c_in) { return gw_w3(c_in) + 8 * 4 * 9; }
__host__ __device__ inline int gw_m2(int c_in) { return gw_b3(c_in) + 4; }
__host__ __device__ inline int gw_total(int c_in) { return gw_m2(c_in) + 5; }

// conv3x3(pad 1) -> ReLU -> MaxPool2d(2) -> per-channel scale / shift for one window of pooled pixels, all resident
// slots at once.  Lane task = one pooled pixel x CG output channels; a wave's 64 tasks share the channel group, so its
// weights are wave-uniform: scalar loads, packed [ci][ky][kx][co] so that two neighbouring output channels are one SGPR
// pair and one v_pk_fma_f32 updates both (the patch value is broadcast by op_sel): 18 CG packed fmas per input channel
// (measured on MI355X, tools/micro/rates.hip: v_pk_fma_f32 55 TMAC/s against 31 for v_fmac_f32).  Input buffer: origin =
// (first conv row - 1, first conv column - 1), so the 4x4 patch of pooled pixel (ly, lx) of the window starts at buffer
// (2 ly, 2 lx); even row width: aligned float2 reads.
template <int CI, int CO, int CG, bool AFFINE>
__device__ __forceinline__ void conv_stage(float *slot0, int slot_floats, int in_off, int ih, int iw, int out_off,
                                           int oh, int ow, int oy0, int ox0, int ph, int pw, int G,
                                           const float *__restrict__ w, const float *__restrict__ bias,
                                           const float *__restrict__ sc, const float *__restrict__ sh)
{
    static_assert(CG % 2 == 0 && CO % CG == 0, "channel groups are whole SGPR pairs");
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nw = blockDim.x >> 6;
    const int per_slot = ph * pw, n = G * per_slot;
    const int chunks = (n + 63) >> 6;
    constexpr int NG = CO / CG, CP = CG / 2;
    const int plane_in = ih * iw, plane_out = oh * ow;
    for (int c = wave; c < chunks * NG; c += nw) {
        const int cgi = __builtin_amdgcn_readfirstlane(c / chunks);
        const int t = (c - cgi * chunks) * 64 + lane;
        const bool active = t < n;
        const int tt = active ? t : n - 1;
        const int slot = tt / per_slot, rem = tt - slot * per_slot;
        const int ly = rem / pw, lx = rem - ly * pw;
        const float *ip = slot0 + slot * slot_floats + in_off + (2 * ly) * iw + 2 * lx;
        gf32x2 acc[CP][4];
#pragma unroll
        for (int cp = 0; cp < CP; ++cp) acc[cp][0] = acc[cp][1] = acc[cp][2] = acc[cp][3] = gf32x2{0.0f, 0.0f};
        const float *wg = w + cgi * CG;
#pragma unroll 1
        for (int ci = 0; ci < CI; ++ci) {
            float p[4][4];
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const float2 a = *reinterpret_cast<const float2 *>(ip + r * iw);
                const float2 b = *reinterpret_cast<const float2 *>(ip + r * iw + 2);
                p[r][0] = a.x, p[r][1] = a.y, p[r][2] = b.x, p[r][3] = b.y;
            }
            const float *wc = wg + ci * (9 * CO);
#pragma unroll
            for (int ky = 0; ky < 3; ++ky)
#pragma unroll
                for (int kx = 0; kx < 3; ++kx)
#pragma unroll
                    for (int cp = 0; cp < CP; ++cp) {
                        const gf32x2 wv = *reinterpret_cast<const gf32x2 *>(wc + (ky * 3 + kx) * CO + 2 * cp);
                        acc[cp][0] = __builtin_elementwise_fma(wv, gf32x2{p[ky][kx], p[ky][kx]}, acc[cp][0]);
                        acc[cp][1] = __builtin_elementwise_fma(wv, gf32x2{p[ky][kx + 1], p[ky][kx + 1]}, acc[cp][1]);
                        acc[cp][2] = __builtin_elementwise_fma(wv, gf32x2{p[ky + 1][kx], p[ky + 1][kx]}, acc[cp][2]);
                        acc[cp][3] = __builtin_elementwise_fma(wv, gf32x2{p[ky + 1][kx + 1], p[ky + 1][kx + 1]}, acc[cp][3]);
                    }
            ip += plane_in;
        }
        if (active) {
            float *op = slot0 + slot * slot_floats + out_off + (cgi * CG) * plane_out + (oy0 + ly) * ow + ox0 + lx;
#pragma unroll
            for (int co = 0; co < CG; ++co) {
                const int ch = cgi * CG + co, cp = co >> 1, e = co & 1;
                float m = fmaxf(fmaxf(acc[cp][0][e], acc[cp][1][e]), fmaxf(acc[cp][2][e], acc[cp][3][e])) + bias[ch];
                m = fmaxf(m, 0.0f);                       // max of ReLUs = ReLU of the max (bias shared by the window)
                if (AFFINE) m = fmaf(sc[ch], m, sh[ch]);
                op[co * plane_out] = m;
            }
        }
    }
}

template <int CI, int CO, bool AFFINE>
__device__ __forceinline__ void conv_stage_cg(int cg, float *slot0, int slot_floats, int in_off, int ih, int iw,
                                              int out_off, int oh, int ow, int oy0, int ox0, int ph, int pw, int G,
                                              const float *__restrict__ w, const float *__restrict__ bias,
                                              const float *__restrict__ sc, const float *__restrict__ sh)
{
    if (cg == 8) conv_stage<CI, CO, 8, AFFINE>(slot0, slot_floats, in_off, ih, iw, out_off, oh, ow, oy0, ox0, ph, pw, G, w, bias, sc, sh);
    else if (cg == 4) conv_stage<CI, CO, 4, AFFINE>(slot0, slot_floats, in_off, ih, iw, out_off, oh, ow, oy0, ox0, ph, pw, G, w, bias, sc, sh);
    else conv_stage<CI, CO, 2, AFFINE>(slot0, slot_floats, in_off, ih, iw, out_off, oh, ow, oy0, ox0, ph, pw, G, w, bias, sc, sh);
}

// ---- the stages every coupling kernel starts with (tfk_glow.hip, tfk_glow_dsf.hip): from the rows to the 16 numbers per
// sample that feed the Linear layer ------------------------------------------------------------------------------

// S0: the source elements of G resident samples (gathered through the layer's table, pending maps applied)
// through the first ConvModifier into the modifier buffer's rectangle.  ONE: the 1x1 kernel (every BASELINE shape), taps and
// bounds tests compiled out (the general form costs the 1x1 case 5 %, same-box A/B).
template <bool ONE>
__device__ __forceinline__ void s0_modifier(const GlowGeom &g, const float *rows, long long N, long long row_first, int G,
                                            float *slot0, const int *__restrict__ src_idx,
                                            const float2 *__restrict__ src_st, const float *__restrict__ wts)
{
    const int npix = g.hi * g.wi, rpix = g.rh * g.rw;
    const float *bm = wts + gw_bm(g.cm);
    const int taps = ONE ? 1 : g.kh * g.kw;
    for (int t = threadIdx.x; t < G * rpix; t += blockDim.x) {
        const int slot = t / rpix, pix = t - slot * rpix;
        const int iy = pix / g.rw, ix = pix - iy * g.rw;
        long long row = row_first + slot;
        if (row > N - 1) row = N - 1;
        const float *xr = rows + row * g.D;
        float o0 = bm[0], o1 = bm[1], o2 = bm[2], o3 = bm[3];
        for (int tap = 0; tap < taps; ++tap) {
            bool inside = true;
            int spix = pix;
            if (!ONE) {
                const int ky = tap / g.kw, kx = tap - ky * g.kw;
                const int sy = iy - (g.kh - 1) + ky, sx = ix - (g.kw - 1) + kx;      // out[Y] = sum_k W[k] x[Y + k - pad]
                inside = sy >= 0 && sy < g.hi && sx >= 0 && sx < g.wi;
                spix = inside ? sy * g.wi + sx : 0;
            }
            for (int c0 = 0; c0 < g.c_in; c0 += 4) {             // four channels' loads in flight together
                int idx[4];
                float2 st[4];
                float raw[4];
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    const int c = c0 + u < g.c_in ? c0 + u : g.c_in - 1;
                    const int e = c * npix + spix;
                    idx[u] = src_idx[e];
                    st[u] = src_st[e];
                }
#pragma unroll
                for (int u = 0; u < 4; ++u) raw[u] = xr[idx[u]];
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    const int c = c0 + u;
                    const bool on = c < g.c_in;
                    const int w = (on ? c : 0) * taps + tap;
                    const float v = (on && inside) ? fmaf(st[u].x, raw[u], st[u].y) : 0.0f;
                    o0 = fmaf(wts[w], v, o0);
                    o1 = fmaf(wts[g.cm + w], v, o1);
                    o2 = fmaf(wts[2 * g.cm + w], v, o2);
                    o3 = fmaf(wts[3 * g.cm + w], v, o3);
                }
            }
        }
        float *a = slot0 + slot * g.slot_floats + (g.oy + iy - g.a0y0) * g.a0w + (g.ox + ix - g.a0x0);
        const int plane = g.a0h * g.a0w;
        a[0] = o0, a[plane] = o1, a[2 * plane] = o2, a[3 * plane] = o3;
    }
}

// Once per workgroup: everything of the slots' buffers that no sample changes (zero outside the frames, the first
// modifier's bias, bg1, bg2); ends with a barrier.
__device__ __forceinline__ void glow_background(const GlowGeom &g, float *slot0, const float *__restrict__ wts,
                                                const float *__restrict__ bg1, const float *__restrict__ bg2)
{
    const int tid = threadIdx.x, nthr = blockDim.x, G = g.slots;
    const float *bm = wts + gw_bm(g.cm);
    const int a0 = 4 * g.a0h * g.a0w, b1 = 8 * g.b1h * g.b1w;
    for (int i = tid; i < G * a0; i += nthr) {
        const int slot = i / a0, e = i - slot * a0;
        const int ch = e / (g.a0h * g.a0w), r = (e / g.a0w) % g.a0h, c = e % g.a0w;
        const int y = g.a0y0 + r, x = g.a0x0 + c;
        const bool in = y >= 0 && y < kGlowFrame && x >= 0 && x < kGlowFrame;
        slot0[slot * g.slot_floats + e] = in ? bm[ch] : 0.0f;
    }
    for (int i = tid; i < G * b1; i += nthr) {
        const int slot = i / b1, e = i - slot * b1;
        const int ch = e / (g.b1h * g.b1w), r = (e / g.b1w) % g.b1h, c = e % g.b1w;
        const int y = g.b1y0 + r, x = g.b1x0 + c;
        const bool in = y >= 0 && y < 16 && x >= 0 && x < 16;
        slot0[slot * g.slot_floats + g.off_p1 + e] = in ? bg1[(ch * 16 + y) * 16 + x] : 0.0f;
    }
    for (int i = tid; i < G * 800; i += nthr) {
        const int slot = i / 800, e = i - slot * 800;
        const int ch = e / 100, r = (e / 10) % 10, c = e % 10;
        const int y = r - 1, x = c - 1;
        const bool in = y >= 0 && y < 8 && x >= 0 && x < 8;
        slot0[slot * g.slot_floats + g.off_p2 + e] = in ? bg2[(ch * 8 + y) * 8 + x] : 0.0f;
    }
    __syncthreads();
}

// S0 .. S4 for the tile of g.tile_rows samples that starts at row_base, g.slots of them per round: V[sample][16] holds
// what the Linear layer reads (rows past N - 1 repeat the last one); ends with a barrier.
__device__ __forceinline__ void glow_conditioner16(const GlowGeom &g, const float *rows, long long N, long long row_base,
                                                   float *slot0, float *V, const int *__restrict__ src_idx,
                                                   const float2 *__restrict__ src_st, const float *__restrict__ wts)
{
    const int tid = threadIdx.x, nthr = blockDim.x, G = g.slots;
    for (int s0 = 0; s0 < g.tile_rows; s0 += G) {
        // ---- S0: pending map + ConvModifier (c_in -> 4 channels; kernel 1x1, or 2 wide along an axis whose padding is
        //      odd, classic.py:26-33) into the rectangle of the frame that is not the bias ----
        if (!(g.skip & 1)) {
            if (g.kh * g.kw == 1) s0_modifier<true>(g, rows, N, row_base + s0, G, slot0, src_idx, src_st, wts);
            else s0_modifier<false>(g, rows, N, row_base + s0, G, slot0, src_idx, src_st, wts);
        }
        __syncthreads();
        // ---- S1 .. S3: the three conv blocks on their windows ----
        const int ci = g.cm;
        if (!(g.skip & 2)) {
            conv_stage_cg<4, 8, true>(g.cg1, slot0, g.slot_floats, 0, g.a0h, g.a0w, g.off_p1, g.b1h, g.b1w,
                                      g.p1y0 - g.b1y0, g.p1x0 - g.b1x0, g.p1h, g.p1w, G, wts + gw_w1(ci),
                                      wts + gw_b1(ci), wts + gw_b1(ci) + 8, wts + gw_b1(ci) + 16);
            __syncthreads();
            conv_stage_cg<8, 8, true>(g.cg2, slot0, g.slot_floats, g.off_p1, g.b1h, g.b1w, g.off_p2, 10, 10,
                                      g.p2y0 + 1, g.p2x0 + 1, g.p2h, g.p2w, G, wts + gw_w2(ci), wts + gw_b2(ci),
                                      wts + gw_b2(ci) + 8, wts + gw_b2(ci) + 16);
            __syncthreads();
            conv_stage<8, 4, 2, false>(slot0, g.slot_floats, g.off_p2, 10, 10, g.off_p3, 4, 4, 0, 0, 4, 4, G,
                                       wts + gw_w3(ci), wts + gw_b3(ci), nullptr, nullptr);
            __syncthreads();
        }
        // ---- S4: BatchNorm 3 + second ConvModifier (4 -> 1 channel), folded on the host ----
        for (int t = tid; t < G * 16; t += nthr) {
            const int slot = t >> 4, p = t & 15;
            const float *p3 = slot0 + slot * g.slot_floats + g.off_p3 + p;
            const float *m2 = wts + gw_m2(ci);
            float v = m2[4];
            v = fmaf(m2[0], p3[0], v);
            v = fmaf(m2[1], p3[16], v);
            v = fmaf(m2[2], p3[32], v);
            v = fmaf(m2[3], p3[48], v);
            V[(s0 + slot) * 16 + p] = v;
        }
        // (the next round's S0 writes A0, last read before two barriers; P3 is rewritten after three more)
    }
    __syncthreads();
}

// lo + (hi - lo) * sigmoid(h) with (lo, hi) = (-2, 2); the caller hands in h * log2(e) (the rows of W_eff / b_eff arrive
// pre-multiplied), so the exponential is one v_exp_f32; s * 4 is exact, so the reference's multiply-then-add is one fma
__device__ __forceinline__ float bounded4(float h_log2e)
{
    return fmaf(__builtin_amdgcn_rcpf(1.0f + __builtin_amdgcn_exp2f(-h_log2e)), 4.0f, -2.0f);
}

// ---- host: windows and buffers --------------------------------------------------------------------------------
static inline int floor2(int v) { return v & ~1; }
static inline int ceil2(int v) { return (v + 1) & ~1; }
static inline int imax(int a, int b) { return a > b ? a : b; }
static inline int imin(int a, int b) { return a < b ? a : b; }

// windows and buffers from the image's rectangle (rows [oy, oy + hi), columns [ox, ox + wi) of the 32x32 frame)
[[maybe_unused]] static void glow_windows(GlowGeom &g)
{
    const int y0 = imax(g.oy - 1, 0), y1 = imin(g.oy + g.rh + 1, kGlowFrame);
    const int x0 = imax(g.ox - 1, 0), x1 = imin(g.ox + g.rw + 1, kGlowFrame);
    const int c1y0 = floor2(y0), c1y1 = ceil2(y1), c1x0 = floor2(x0), c1x1 = ceil2(x1);
    g.a0y0 = c1y0 - 1, g.a0x0 = c1x0 - 1, g.a0h = c1y1 - c1y0 + 2, g.a0w = c1x1 - c1x0 + 2;
    g.p1y0 = c1y0 / 2, g.p1x0 = c1x0 / 2, g.p1h = (c1y1 - c1y0) / 2, g.p1w = (c1x1 - c1x0) / 2;
    const int qy0 = imax(g.p1y0 - 1, 0), qy1 = imin(g.p1y0 + g.p1h + 1, 16);
    const int qx0 = imax(g.p1x0 - 1, 0), qx1 = imin(g.p1x0 + g.p1w + 1, 16);
    const int c2y0 = floor2(qy0), c2y1 = ceil2(qy1), c2x0 = floor2(qx0), c2x1 = ceil2(qx1);
    g.b1y0 = c2y0 - 1, g.b1x0 = c2x0 - 1, g.b1h = c2y1 - c2y0 + 2, g.b1w = c2x1 - c2x0 + 2;
    g.p2y0 = c2y0 / 2, g.p2x0 = c2x0 / 2, g.p2h = (c2y1 - c2y0) / 2, g.p2w = (c2x1 - c2x0) / 2;
    g.off_p1 = 4 * g.a0h * g.a0w;
    g.off_p2 = g.off_p1 + 8 * g.b1h * g.b1w;
    g.off_p3 = g.off_p2 + 800;
    g.slot_floats = g.off_p3 + 64;
}

constexpr int kGlowLdsBytes = 160 * 1024;

// validated geometry of one layer (no launch shape): shared by tfk_glow_plan / tfk_glow_coupling / the level packer
int glow_geometry_base(const tfk_glow_layer *L, int32_t D, GlowGeom &g, const char *fn);

// kind 3 (deep sigmoidal, tfk_glow_dsf.hip) behind tfk_glow_coupling: g, block and lds as tfk_glow_plan reports them
int glow_dsf_launch(float *rows, float *logdet, int64_t N, const GlowGeom &g, int block, size_t lds,
                    const tfk_glow_layer *layer, int inverse, hipStream_t s, const char *fn);

// kinds 4 and 6 (affine / shift behind the ResNet conditioner, tfk_glow_resnet.hip): the geometry behind
// glow_geometry_base, the launch shape and the launch behind tfk_glow_coupling
void glow_resnet_geometry(GlowGeom &g);
bool glow_resnet_plan(GlowGeom &g, int want_slots, int want_block, int *block_out);
int glow_resnet_launch(float *rows, float *logdet, int64_t N, const GlowGeom &g, int block, size_t lds,
                       const tfk_glow_layer *layer, int inverse, hipStream_t s, const char *fn);

}  // namespace tfk
