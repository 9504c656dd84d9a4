// SegNet-Basic training at float32 accuracy on the f16 matrix cores (train_segnet.py --split_planes): the eight pass
// forms of spa_segnet_train.hip -- forward (conv1's image, a 64-channel map, the decoder's unpooled map), dgrad (plain
// and the decoder's pooled-gradient gather) and wgrad (conv1, encoder, decoder) -- with every float32 operand carried
// as two half-precision planes and three products per float32 product (the split of spa_segnet_dev.h).
//
// Each operand TENSOR gets one scale (the inference kernels: one per image).  Forward and dgrad keep the cross terms in
// accumulators of their own, added to the h_a h_b accumulators after the K loop (sg_mma3); the epilogue multiplies by
// 2^-(k_a + k_b) before y, the BN partial sums, the dgrad gather or a wgrad chunk partial is formed.  The scales are
// computed on the device inside each call: per-workgroup maxima of |v|, then one workgroup per tensor reduces them --
// no atomics are used.  Inputs are the float32 values of the float32 kernels (the input forms of spa_segnet_dev.h; the
// scale of a decoder's input is that of its pooled map), dy, and the weights (split once per call into a packed f16
// plane pair in the context workspace).
//
// Tiling, K steps, conv1's tap packing, the transposed wgrad staging and every reduction are those of
// spa_segnet_train_bf16.hip; forward and dgrad run the split staging and K loop shared with spa_segnet_f16x3.hip
// (spa_segnet_split_main.inc).  This file owns the kernels' LDS and launches, the per-tensor maxima, the
// scale reduction, the split weight packing and the split wgrad kernel, which stages h and l as two images of the bf16
// layout.  The work split depends on the shape only, so the bits do not depend on the run or the device.
#include "spa_segnet_dev.h"

// ---------------------------------------------------------------------------------------------------- scales
// the workgroup's maximum of 256 per-thread values -> part[blockIdx.x]
__device__ __forceinline__ void sgh_max_store(unsigned m, unsigned *red, unsigned *part)
{
    const int t = threadIdx.x;
    red[t] = m;
    __syncthreads();
    for (int d = 128; d >= 1; d >>= 1) {
        if (t < d) red[t] = max(red[t], red[t + d]);
        __syncthreads();
    }
    if (t == 0) part[blockIdx.x] = red[0];
}

// part[blockIdx.x] = the bit pattern of max |a[i]| over this workgroup's share of a[0 .. 4 n4) (16-byte aligned)
__global__ __launch_bounds__(256) void k_sgh_amax(const float *__restrict__ a, long long n4, unsigned *__restrict__ part)
{
    __shared__ unsigned red[256];
    unsigned m = 0u;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n4; i += (long long)gridDim.x * 256) {
        const sg_f32x4 v = ((const sg_f32x4 *)a)[i];
        m = max(max(m, max(sg_absbits(v.x), sg_absbits(v.y))), max(sg_absbits(v.z), sg_absbits(v.w)));
    }
    sgh_max_store(m, red, part);
}

// the same for conv1's operand: the standardised, LRN-normalised image (B,3,H,W), as the kernels stage it
__global__ __launch_bounds__(256) void k_sgh_amax_conv1(const float *__restrict__ x, int B, int H, int W, SgStd st,
                                                        unsigned *__restrict__ part)
{
    __shared__ unsigned red[256];
    const long long plane = (long long)H * W, n = (long long)B * plane;
    unsigned m = 0u;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) {
        const long long b = i / plane, o = i - b * plane;
        const sg_f32x4 v = sg_conv1_val(x + b * 3 * plane, plane, (int)(o / W), (int)(o % W), H, W, st);
        m = max(m, max(max(sg_absbits(v.x), sg_absbits(v.y)), sg_absbits(v.z)));
    }
    sgh_max_store(m, red, part);
}

// ex[j] = k with 2^k max|v| in [2^14, 2^15) for operand j = blockIdx.x (per-workgroup maxima part[j * SG_NAMAX ..]);
// k = 0 for an all-zero operand.  The exponent is clamped to [-112, 127] so that 2^k is a normal float: a maximum
// below 2^-112 (subnormal inputs) lands lower, a NaN or infinite one at 2^-113.
__global__ __launch_bounds__(256) void k_sg_scale(const unsigned *__restrict__ part, int *__restrict__ ex)
{
    __shared__ unsigned red[256];
    const int t = threadIdx.x;
    unsigned m = 0u;
    for (int i = t; i < SG_NAMAX; i += 256) m = max(m, part[(long long)blockIdx.x * SG_NAMAX + i]);
    red[t] = m;
    __syncthreads();
    for (int d = 128; d >= 1; d >>= 1) {
        if (t < d) red[t] = max(red[t], red[t + d]);
        __syncthreads();
    }
    if (t == 0) {
        const unsigned bits = red[0];
        int e = (int)(bits >> 23) - 127;
        e = e < -112 ? -112 : (e > 127 ? 127 : e);
        ex[blockIdx.x] = bits == 0u ? 0 : 14 - e;
    }
}

SG_LOCAL void sg_launch_scale(hipStream_t s, int nop, const unsigned *part, int *ex)
{
    hipLaunchKernelGGL(k_sg_scale, dim3(nop), dim3(256), 0, s, part, ex);
}

// ---------------------------------------------------------------------------------------------------- forward, dgrad
// Y = conv7x7(input form MODE of X (, I); Wp) at output resolution (H, W).  Wp: the h plane, then the l plane, each
// (49,64,64) = (tap, n, c) for the 64-channel forms or (7,64,32) = (K step, n, k) for conv1 (k = 4 (tap - 8 step) + c,
// zero past tap 48).  ex[0] = the input's scale exponent, ex[1] = the weights'.  EPI, Io, part: as sg_train_epilogue.
template <int MODE, int EPI>
__global__ __launch_bounds__(SG_THREADS, 2) void k_sgh_conv(const float *__restrict__ X, const uint8_t *__restrict__ I,
                                                            const unsigned short *__restrict__ Wp,
                                                            const uint8_t *__restrict__ Io, float *__restrict__ Y,
                                                            float *__restrict__ part, const int *__restrict__ ex, int H,
                                                            int W, SgStd st)
{
    constexpr int IN = MODE;
    constexpr int NHALO = SG_HPIX * sg_ps_split(MODE) * 2;
    constexpr int NB = NHALO > 8192 ? NHALO : 8192;                      // bytes: the halo, or the BN reduction
    __shared__ __attribute__((aligned(16))) unsigned short xs[NB / 2];
    float *red = (float *)xs;

    const int tid = threadIdx.x, lane = tid & 63;
    const int w = tid >> 6;
    const int b = blockIdx.z;
    const int ty0 = blockIdx.y * SG_TH, tx0 = blockIdx.x * SG_TW;
    const int kin = ex[0], kw = ex[1];
    const float sc = sg_pow2(kin);
    const auto [fi, fq, frow, fcol] = sg_geom(lane, w);

    sg_f32x4 acc[4][4], accx[4][4];
#pragma unroll
    for (int m = 0; m < 4; ++m)
#pragma unroll
        for (int nt = 0; nt < 4; ++nt) acc[m][nt] = accx[m][nt] = (sg_f32x4){0.f, 0.f, 0.f, 0.f};

#include "spa_segnet_split_main.inc"

    // epilogue: sg_train_epilogue's on the unscaled sums (its comment says why this is a copy)
    const int unscale = -(kin + kw);
#pragma unroll
    for (int m = 0; m < 4; ++m)
#pragma unroll
        for (int nt = 0; nt < 4; ++nt)
#pragma unroll
            for (int r = 0; r < 4; ++r) acc[m][nt][r] = acc[m][nt][r] + accx[m][nt][r];
    const int oy = ty0 + 2 * w, ox = tx0 + 2 * fq;
    const bool row_in = oy < H;
    if (EPI == SG_FULL) {
        float s[4] = {0.f, 0.f, 0.f, 0.f}, q[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int m = 0; m < 4; ++m) {
            const int x = ox + 8 * m;
            if (x >= W || !row_in) continue;
#pragma unroll
            for (int nt = 0; nt < 4; ++nt) {
                const int n = 16 * nt + fi;
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const float v = ldexpf(acc[m][nt][r], unscale);
                    Y[(((long long)b * H + oy + (r >> 1)) * W + x + (r & 1)) * 64 + n] = v;
                    s[nt] += v;
                    q[nt] = fmaf(v, v, q[nt]);
                }
            }
        }
        if (part) {
            // fixed order: lanes' sums -> LDS [wave][fq][channel], then 128 threads add the 16 entries of a channel
            __syncthreads();                                           // xs is free once every wave left the K loop
#pragma unroll
            for (int nt = 0; nt < 4; ++nt) {
                const int n = 16 * nt + fi;
                red[((w * 4 + fq) * 64 + n) * 2] = s[nt];
                red[((w * 4 + fq) * 64 + n) * 2 + 1] = q[nt];
            }
            __syncthreads();
            if (tid < 128) {
                const int n = tid & 63, k = tid >> 6;
                float t = 0.f;
                for (int j = 0; j < 16; ++j) t += red[(j * 64 + n) * 2 + k];
                const long long blk = ((long long)b * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x;
                part[blk * 128 + k * 64 + n] = t;
            }
        }
    } else {
        const int Hh = H >> 1, Wh = W >> 1;
        const int py = oy >> 1;
#pragma unroll
        for (int m = 0; m < 4; ++m) {
            const int px = (ox >> 1) + 4 * m;
            if (px >= Wh || py >= Hh) continue;
            const long long o = (((long long)b * Hh + py) * Wh + px) * 64;
#pragma unroll
            for (int nt = 0; nt < 4; ++nt) {
                const int n = 16 * nt + fi;
                const int r = Io[o + n];
                const sg_f32x4 a = acc[m][nt];
                Y[o + n] = ldexpf(r == 0 ? a[0] : r == 1 ? a[1] : r == 2 ? a[2] : a[3], unscale);
            }
        }
    }
}

// the split planes of a 64-channel layer's weights with scale 2^kw[0]: Wp[0][t][o][i] = h, Wp[1][t][o][i] = l of
// Wt[t][o][i], or with rot (dgrad) of Wt[48 - t][i][o]
__global__ __launch_bounds__(256) void k_sg_split_wpack64(const float *__restrict__ Wt, int rot,
                                                          const int *__restrict__ kw,
                                                          unsigned short *__restrict__ Wp)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= SG_W64) return;
    const int t = i / 4096, o = (i >> 6) & 63, c = i & 63;
    sg_split(rot ? Wt[((48 - t) * 64 + c) * 64 + o] : Wt[i], sg_pow2(kw[0]), Wp[i], Wp[SG_W64 + i]);
}

SG_LOCAL void sg_launch_split_wpack64(hipStream_t s, const float *wt, int rot, const int *kw, unsigned short *wp)
{
    hipLaunchKernelGGL(k_sg_split_wpack64, dim3(SG_W64 / 256), dim3(256), 0, s, wt, rot, kw, wp);
}

// conv1's split weights in K steps of 8 taps: plane j, Wp[j][s][n][k] of Wt[8 s + k / 4][n][k % 4], zero past tap 48
__global__ __launch_bounds__(256) void k_sg_split_wpack1(const float *__restrict__ Wt,
                                                         const int *__restrict__ kw,
                                                         unsigned short *__restrict__ Wp)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= SG_W1) return;
    const int s = i >> 11, n = (i >> 5) & 63, k = i & 31, t = 8 * s + (k >> 2);
    sg_split(t < 49 ? Wt[(t * 64 + n) * 4 + (k & 3)] : 0.f, sg_pow2(kw[0]), Wp[i], Wp[SG_W1 + i]);
}

SG_LOCAL void sg_launch_split_wpack1(hipStream_t s, const float *wt, const int *kw, unsigned short *wp)
{
    hipLaunchKernelGGL(k_sg_split_wpack1, dim3(SG_W1 / 256), dim3(256), 0, s, wt, kw, wp);
}

// ---------------------------------------------------------------------------------------------------- wgrad
#define SGHW_GS 72                   // LDS f16 per staged 64-channel pixel of one plane (128 bytes + 16 of padding)

// part[(chunk * 49 + ky * 7 + kx) * 64 * CP + n * CP + c] = the chunk's sum of G[p][n] * X[p + (ky - 3, kx - 3)][c].
// G (B,H,W,64) channels-last; ex[0] the input form's scale exponent, ex[1] G's.  Grid (chunks, 7): blockIdx.y = ky.
// K step s of a tile = its row s, k = column.  MFMA A = G (rows n, lane 16-group fq holds pixels 8 fq .. 8 fq + 7),
// B = X shifted by the tap (columns c); each operand staged as an h and an l image.
// 64-channel forms: wave w owns channels c = 16 w .. 16 w + 15 of all seven taps of the row and all 64 n.
// conv1 (CP 4): the 16 MFMA columns are (kx, c) = (4 ct + (j >> 2), j & 3) for column tiles ct 0, 1 (kx 7 is
// discarded); wave w owns column tile w >> 1 and the row tiles nt = 2 (w & 1), 2 (w & 1) + 1.
template <int MODE>
__global__ __launch_bounds__(SG_THREADS) void k_sgh_wgrad(const float *__restrict__ G, const float *__restrict__ X,
                                                           const uint8_t *__restrict__ I, float *__restrict__ part,
                                                           const int *__restrict__ ex, int B, int H, int W, int nch,
                                                           SgStd st)
{
    constexpr int CP = MODE == SG_CONV1 ? 4 : 64;
    constexpr int XW = MODE == SG_CONV1 ? SGW_TW + 8 : SGW_TW + 6;     // staged input columns (conv1: kx 7 too)
    constexpr int XS = MODE == SG_CONV1 ? 4 : SGHW_GS;                    // LDS f16 per staged input pixel and plane
    constexpr int GPL = SGW_TR * SGW_TW * SGHW_GS, XPL = SGW_TR * XW * XS;  // f16 per plane
    __shared__ __attribute__((aligned(16))) unsigned short gs[2 * GPL];
    __shared__ __attribute__((aligned(16))) unsigned short xs[2 * XPL];

    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int fi = lane & 15, fq = lane >> 4;
    const int ky = blockIdx.y, chunk = blockIdx.x;
    const int txn = (W + SGW_TW - 1) / SGW_TW, tyn = H / SGW_TR;
    const long long tiles = (long long)B * tyn * txn;
    const long long t0 = tiles * chunk / nch, t1 = tiles * (chunk + 1) / nch;
    const long long plane = (long long)H * W;
    const int kin = ex[0], kg = ex[1];
    const float scx = sg_pow2(kin), scg = sg_pow2(kg);

    constexpr int NA = MODE == SG_CONV1 ? 1 : 7;
    constexpr int NT = MODE == SG_CONV1 ? 2 : 4;
    const int nt0 = MODE == SG_CONV1 ? 2 * (w & 1) : 0;
    sg_f32x4 acc[NA][NT];
#pragma unroll
    for (int a = 0; a < NA; ++a)
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) acc[a][nt] = (sg_f32x4){0.f, 0.f, 0.f, 0.f};

    // the lane's transposed-read addresses in the h images (pixel row (fi >> 2) of the 4-pixel block, column group
    // fi & 3); the l images are GPL / XPL further
    const int kp = 8 * fq + (fi >> 2);
    const unsigned short *ga = &gs[kp * SGHW_GS + 4 * (fi & 3)];
    const unsigned short *xa = MODE == SG_CONV1 ? &xs[(kp + 4 * (w >> 1) + (fi & 3)) * XS]
                                                 : &xs[kp * XS + 16 * w + 4 * (fi & 3)];

    for (long long t = t0; t < t1; ++t) {
        int b, y0, x0;
        sg_wgrad_tile(t, txn, tyn, b, y0, x0);
        if (t != t0) __syncthreads();
        // stage G (zero past the right edge: those pixels contribute nothing) and the input rows y0 + ky - 3 + r
        for (int e = tid; e < SGW_TR * SGW_TW * 8; e += SG_THREADS) {
            const int p = e >> 3, q = e & 7;
            const int gy = y0 + p / SGW_TW, gx = x0 + p % SGW_TW;
            uint4 h = make_uint4(0u, 0u, 0u, 0u), l = h;
            if (gx < W) {
                const float *g = G + (((long long)b * H + gy) * W + gx) * 64 + 8 * q;
                h = sg_split8(*(const sg_f32x4 *)g, *(const sg_f32x4 *)(g + 4), scg, l);
            }
            *(uint4 *)&gs[p * SGHW_GS + 8 * q] = h;
            *(uint4 *)&gs[GPL + p * SGHW_GS + 8 * q] = l;
        }
        if (MODE == SG_CONV1) {
            const float *xb = X + (long long)b * 3 * plane;
            for (int p = tid; p < SGW_TR * XW; p += SG_THREADS) {
                uint2 l;
                *(uint2 *)&xs[p * XS] = sg_split_conv1_px(xb, plane, y0 + ky - 3 + p / XW, x0 - 3 + p % XW, H, W, st, scx, l);
                *(uint2 *)&xs[XPL + p * XS] = l;
            }
        } else {
            for (int e = tid; e < SGW_TR * XW * 8; e += SG_THREADS) {
                const int p = e >> 3, q = e & 7;
                uint4 l;
                *(uint4 *)&xs[p * XS + 8 * q] =
                    sg_split_px8<MODE>(X, I, b, y0 + ky - 3 + p / XW, x0 - 3 + p % XW, 8 * q, H, W, scx, l);
                *(uint4 *)&xs[XPL + p * XS + 8 * q] = l;
            }
        }
        __syncthreads();

#pragma unroll
        for (int s = 0; s < SGW_TR; ++s) {
            sg_f16x8 ah[NT], al[NT];
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) {
                const unsigned short *p0 = ga + s * SGW_TW * SGHW_GS + 16 * (nt0 + nt);
                ah[nt] = sg_tr8<sg_f16x8>(p0, p0 + 4 * SGHW_GS);
                al[nt] = sg_tr8<sg_f16x8>(p0 + GPL, p0 + GPL + 4 * SGHW_GS);
            }
            constexpr int NK = MODE == SG_CONV1 ? 1 : 7;          // conv1: one column fragment covers the taps
#pragma unroll
            for (int kx = 0; kx < NK; ++kx) {
                const unsigned short *p0 = xa + (s * XW + kx) * XS;
                const sg_f16x8 bh = sg_tr8<sg_f16x8>(p0, p0 + 4 * XS);
                const sg_f16x8 bl = sg_tr8<sg_f16x8>(p0 + XPL, p0 + XPL + 4 * XS);
#pragma unroll
                for (int nt = 0; nt < NT; ++nt) {
                    acc[kx][nt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(ah[nt], bl, acc[kx][nt], 0, 0, 0);
                    acc[kx][nt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(al[nt], bh, acc[kx][nt], 0, 0, 0);
                    acc[kx][nt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(ah[nt], bh, acc[kx][nt], 0, 0, 0);
                }
            }
        }
    }

    // D layout: column (c or (kx, c)) = lane & 15, row n = 16 nt + 4 (lane >> 4) + r; stored unscaled
    const int unscale = -(kin + kg);
    float *pb = part + ((long long)chunk * 49 + ky * 7) * 64 * CP;
    if (MODE == SG_CONV1) {
        const int kx = 4 * (w >> 1) + (fi >> 2), c = fi & 3;
        if (kx < 7) {
#pragma unroll
            for (int nt = 0; nt < NT; ++nt)
#pragma unroll
                for (int r = 0; r < 4; ++r)
                    pb[((long long)kx * 64 + 16 * (nt0 + nt) + 4 * fq + r) * CP + c] = ldexpf(acc[0][nt][r], unscale);
        }
    } else {
        const int c = 16 * w + fi;
#pragma unroll
        for (int kx = 0; kx < 7; ++kx)
#pragma unroll
            for (int nt = 0; nt < 4; ++nt)
#pragma unroll
                for (int r = 0; r < 4; ++r)
                    pb[((long long)kx * 64 + 16 * nt + 4 * fq + r) * CP + c] = ldexpf(acc[kx][nt][r], unscale);
    }
}

// ---------------------------------------------------------------------------------------------------- C ABI
// the two operands' scale exponents -> ex[0], ex[1] (device words in the workspace), without a host synchronisation:
// operand 0 is a (n0 floats) or, with Cin == 3, conv1's operand of the image a; operand 1 is b (n1 floats)
static int sgh_scales(spa_ctx *ctx, hipStream_t s, const float *a, long long n0, int Cin, int B, int H, int W,
                      const SgStd &st, const float *b, long long n1, int **ex)
{
    unsigned *part = nullptr;
    int rc = spa_ws_reserve(ctx, WS_SEGNET_AMAX, 2 * SG_NAMAX * sizeof(unsigned) + 16, (void **)&part);
    if (rc != SPA_OK) return rc;
    if (Cin == 3)
        hipLaunchKernelGGL(k_sgh_amax_conv1, dim3(SG_NAMAX), dim3(256), 0, s, a, B, H, W, st, part);
    else
        hipLaunchKernelGGL(k_sgh_amax, dim3(SG_NAMAX), dim3(256), 0, s, a, n0 / 4, part);
    SPA_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_sgh_amax, dim3(SG_NAMAX), dim3(256), 0, s, b, n1 / 4, part + SG_NAMAX);
    SPA_LAUNCH_CHECK();
    *ex = (int *)(part + 2 * SG_NAMAX);
    sg_launch_scale(s, 2, part, *ex);
    SPA_LAUNCH_CHECK();
    return SPA_OK;
}

extern "C" int spa_segnet_train_forward_f16x3(spa_ctx *ctx, const float *x, const uint8_t *idx, int32_t x_layout,
                                              int32_t B, int32_t H, int32_t W, int32_t Cin, const float *wt,
                                              const float *mean_host, const float *std_host, float *y, double *stats,
                                              void *stream)
{
    SPA_ARG(ctx && x && wt && y);
    int rc = sg_check_shape("spa_segnet_train_forward_f16x3", B, H, W, Cin);
    if (rc != SPA_OK) return rc;
    SPA_ARG(sg_al16(x) && sg_al16(wt));
    SgStd st = {};
    rc = sg_input_form("spa_segnet_train_forward_f16x3", Cin, x_layout, mean_host, std_host, idx, &st);
    if (rc != SPA_OK) return rc;
    hipStream_t s = spa_stream(stream);
    const dim3 grid = sg_conv_grid(B, H, W);
    const long long nblk = (long long)grid.x * grid.y * grid.z;
    unsigned short *wp = nullptr;
    if ((rc = spa_ws_reserve(ctx, WS_SEGNET_WF16X3, 2 * SG_W64 * sizeof(unsigned short), (void **)&wp)) != SPA_OK)
        return rc;
    float *part = nullptr;
    if (stats) {
        if ((rc = spa_ws_reserve(ctx, WS_SEGNET_BNPART, (size_t)nblk * 128 * sizeof(float), (void **)&part)) != SPA_OK)
            return rc;
    }
    // the input's scale: the image's conv1 operand, the map, or a decoder's pooled map (its unpooled values are a
    // subset of it)
    const long long nx = Cin == 3 ? 0 : (long long)B * (idx ? (H / 2) * (W / 2) : H * W) * 64;
    int *ex = nullptr;
    if ((rc = sgh_scales(ctx, s, x, nx, Cin, B, H, W, st, wt, 49ll * 64 * (Cin == 3 ? 4 : 64), &ex)) != SPA_OK)
        return rc;
    if (Cin == 3)
        sg_launch_split_wpack1(s, wt, ex + 1, wp);
    else
        sg_launch_split_wpack64(s, wt, 0, ex + 1, wp);
    SPA_LAUNCH_CHECK();
    if (Cin == 3)
        hipLaunchKernelGGL((k_sgh_conv<SG_CONV1, SG_FULL>), grid, dim3(SG_THREADS), 0, s, x, nullptr, wp, nullptr, y,
                           part, ex, H, W, st);
    else if (!idx)
        hipLaunchKernelGGL((k_sgh_conv<SG_ENC, SG_FULL>), grid, dim3(SG_THREADS), 0, s, x, nullptr, wp, nullptr, y,
                           part, ex, H, W, st);
    else
        hipLaunchKernelGGL((k_sgh_conv<SG_DEC, SG_FULL>), grid, dim3(SG_THREADS), 0, s, x, idx, wp, nullptr, y, part,
                           ex, H, W, st);
    SPA_LAUNCH_CHECK();
    if (stats) {
        sg_launch_bnstat(s, part, nblk, stats);
        SPA_LAUNCH_CHECK();
    }
    return SPA_OK;
}

extern "C" int spa_segnet_train_dgrad_f16x3(spa_ctx *ctx, const float *dy, const float *wt, const uint8_t *idx,
                                            int32_t B, int32_t H, int32_t W, float *dx, void *stream)
{
    SPA_ARG(ctx && dy && wt && dx);
    int rc = sg_check_shape("spa_segnet_train_dgrad_f16x3", B, H, W, 64);
    if (rc != SPA_OK) return rc;
    SPA_ARG(sg_al16(dy) && sg_al16(wt) && ((uintptr_t)idx & 3) == 0);
    unsigned short *wp = nullptr;
    if ((rc = spa_ws_reserve(ctx, WS_SEGNET_WF16X3, 2 * SG_W64 * sizeof(unsigned short), (void **)&wp)) != SPA_OK)
        return rc;
    hipStream_t s = spa_stream(stream);
    int *ex = nullptr;
    if ((rc = sgh_scales(ctx, s, dy, (long long)B * H * W * 64, 64, B, H, W, SgStd{}, wt, SG_W64, &ex)) != SPA_OK)
        return rc;
    sg_launch_split_wpack64(s, wt, 1, ex + 1, wp);
    SPA_LAUNCH_CHECK();
    const dim3 grid = sg_conv_grid(B, H, W);
    if (idx)
        hipLaunchKernelGGL((k_sgh_conv<SG_ENC, SG_POOLED>), grid, dim3(SG_THREADS), 0, s, dy, nullptr, wp, idx, dx,
                           nullptr, ex, H, W, SgStd{});
    else
        hipLaunchKernelGGL((k_sgh_conv<SG_ENC, SG_FULL>), grid, dim3(SG_THREADS), 0, s, dy, nullptr, wp, nullptr, dx,
                           nullptr, ex, H, W, SgStd{});
    SPA_LAUNCH_CHECK();
    return SPA_OK;
}

extern "C" int spa_segnet_train_wgrad_f16x3(spa_ctx *ctx, const float *dy, const float *x, const uint8_t *idx,
                                            int32_t x_layout, int32_t B, int32_t H, int32_t W, int32_t Cin,
                                            const float *mean_host, const float *std_host, float *dw, void *stream)
{
    SPA_ARG(ctx && dy && x && dw);
    int rc = sg_check_shape("spa_segnet_train_wgrad_f16x3", B, H, W, Cin);
    if (rc != SPA_OK) return rc;
    SPA_ARG(sg_al16(dy) && sg_al16(x));
    SgStd st = {};
    rc = sg_input_form("spa_segnet_train_wgrad_f16x3", Cin, x_layout, mean_host, std_host, idx, &st);
    if (rc != SPA_OK) return rc;
    int nch, n;
    float *part = nullptr;
    if ((rc = sg_wgrad_plan(ctx, B, H, W, Cin, &nch, &n, &part)) != SPA_OK) return rc;
    hipStream_t s = spa_stream(stream);
    // ex[0] the input form's scale (as in the forward), ex[1] dy's
    const long long nx = Cin == 3 ? 0 : (long long)B * (idx ? (H / 2) * (W / 2) : H * W) * 64;
    int *ex = nullptr;
    if ((rc = sgh_scales(ctx, s, x, nx, Cin, B, H, W, st, dy, (long long)B * H * W * 64, &ex)) != SPA_OK) return rc;
    dim3 grid(nch, 7);
    if (Cin == 3)
        hipLaunchKernelGGL(k_sgh_wgrad<SG_CONV1>, grid, dim3(SG_THREADS), 0, s, dy, x, nullptr, part, ex, B, H, W, nch,
                           st);
    else if (!idx)
        hipLaunchKernelGGL(k_sgh_wgrad<SG_ENC>, grid, dim3(SG_THREADS), 0, s, dy, x, nullptr, part, ex, B, H, W, nch,
                           st);
    else
        hipLaunchKernelGGL(k_sgh_wgrad<SG_DEC>, grid, dim3(SG_THREADS), 0, s, dy, x, idx, part, ex, B, H, W, nch, st);
    SPA_LAUNCH_CHECK();
    sg_launch_wsum(s, part, nch, n, dw);
    SPA_LAUNCH_CHECK();
    return SPA_OK;
}
