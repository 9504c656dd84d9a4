// SegNet-Basic training (train_segnet.py --dtype bf16) on the bf16 matrix cores: the eight pass forms of
// spa_segnet_train.hip -- forward (conv1's image, a 64-channel map, the decoder's unpooled map), dgrad (plain and the
// decoder's pooled-gradient gather) and wgrad (conv1, encoder, decoder) -- with bf16 operands and float32 accumulation.
//
// Operands and outputs stay float32 in memory.  Every product operand is the round-to-nearest-even bf16 of the float32
// value the float32 kernels use at that point, rounded while it is staged (the input forms of spa_segnet_dev.h, dy),
// and of the weights (rounded once per call into a packed bf16 copy in the context workspace).  The products are
// v_mfma_f32_16x16x32_bf16 accumulating in float32; y, dx, the BN partial sums (float32 per workgroup, reduced in
// float64 in block order) and dW (split-K, the chunks summed in chunk order in float64) are float32 as before.  No
// atomics; the work split depends on the shape only, so the bits do not depend on the run or the device.  This file and
// spa_segnet_bf16.hip are compiled with -fno-slp-vectorize (Makefile): with conv1's LRN packed into v_pk_*_f32
// instructions the staged operand was not the same in every call at grids of several workgroups per CU.
//
// Forward and dgrad run the bf16 staging and K loop shared with spa_segnet_bf16.hip (sg_conv_main_bf16 of
// spa_segnet_dev.h).  This file owns the kernels' LDS and launches, the bf16 wgrad kernel and the bf16 weight packing.
//
// wgrad sums over pixels: K = 32 consecutive pixels of one row.  The gradient tile and the shifted input rows are
// staged channels-last in LDS and read with ds_read_b64_tr_b16, which turns 4 pixels x 16 channels into each lane's
// 4 pixels of one channel: two reads make a K step's fragment for either operand, at any pixel shift kx.
#include "spa_segnet_dev.h"

// Y = conv7x7(input form MODE of X (, I); Wb) at output resolution (H, W).  Wb bf16: (49,64,64) = (tap, n, c) for the
// 64-channel forms, (7,64,32) = (K step, n, k) for conv1 (k = 4 (tap - 8 step) + c, zero past tap 48).  EPI, Io, part:
// sg_train_epilogue.
template <int MODE, int EPI>
__global__ __launch_bounds__(SG_THREADS) void k_sgb_conv(const float *__restrict__ X, const uint8_t *__restrict__ I,
                                                         const unsigned short *__restrict__ Wb,
                                                         const uint8_t *__restrict__ Io, float *__restrict__ Y,
                                                         float *__restrict__ part, int H, int W, SgStd st)
{
    constexpr int NHALO = SG_HPIX * sg_ps_bf16(MODE) * 2;
    constexpr int NB = NHALO > 8192 ? NHALO : 8192;                      // bytes: the halo, or the BN reduction
    __shared__ __attribute__((aligned(16))) unsigned short xs[NB / 2];

    const int tid = threadIdx.x, lane = tid & 63;
    const int w = tid >> 6;
    const int b = blockIdx.z;
    const int ty0 = blockIdx.y * SG_TH, tx0 = blockIdx.x * SG_TW;
    const SgGeom g = sg_geom(lane, w);
    const int fi = g.fi, fq = g.fq;

    sg_f32x4 acc[4][4];
#pragma unroll
    for (int m = 0; m < 4; ++m)
#pragma unroll
        for (int nt = 0; nt < 4; ++nt) acc[m][nt] = (sg_f32x4){0.f, 0.f, 0.f, 0.f};

    sg_conv_main_bf16<MODE>(acc, xs, X, I, Wb, b, ty0, tx0, g, H, W, st);

    sg_train_epilogue<EPI>(acc, Io, Y, part, (float *)xs, b, ty0, tx0, w, fi, fq, H, W);
}

// the bf16 weights of a 64-channel layer: Wb[t][o][i] = bf16(Wt[t][o][i]), or with rot (dgrad) bf16(Wt[48 - t][i][o])
__global__ __launch_bounds__(256) void k_sg_bf16_wpack64(const float *__restrict__ Wt, int rot,
                                                         unsigned short *__restrict__ Wb)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= SG_W64) return;
    const int t = i / 4096, o = (i >> 6) & 63, c = i & 63;
    Wb[i] = (unsigned short)sg_bf16_bits(rot ? Wt[((48 - t) * 64 + c) * 64 + o] : Wt[i]);
}

SG_LOCAL void sg_launch_bf16_wpack64(hipStream_t s, const float *wt, int rot, unsigned short *wb)
{
    hipLaunchKernelGGL(k_sg_bf16_wpack64, dim3(SG_W64 / 256), dim3(256), 0, s, wt, rot, wb);
}

// conv1's bf16 weights in K steps of 8 taps: Wb[s][n][k] = bf16(Wt[8 s + k / 4][n][k % 4]), zero past tap 48
__global__ __launch_bounds__(256) void k_sg_bf16_wpack1(const float *__restrict__ Wt,
                                                        unsigned short *__restrict__ Wb)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= SG_W1) return;
    const int s = i >> 11, n = (i >> 5) & 63, k = i & 31, t = 8 * s + (k >> 2);
    Wb[i] = t < 49 ? (unsigned short)sg_bf16_bits(Wt[(t * 64 + n) * 4 + (k & 3)]) : (unsigned short)0;
}

SG_LOCAL void sg_launch_bf16_wpack1(hipStream_t s, const float *wt, unsigned short *wb)
{
    hipLaunchKernelGGL(k_sg_bf16_wpack1, dim3(SG_W1 / 256), dim3(256), 0, s, wt, wb);
}

// ---------------------------------------------------------------------------------------------------- wgrad
#define SGBW_GS 72                   // LDS bf16 per staged 64-channel pixel (128 bytes + 16 of padding)

// part[(chunk * 49 + ky * 7 + kx) * 64 * CP + n * CP + c] = the chunk's sum of G[p][n] * X[p + (ky - 3, kx - 3)][c].
// G (B,H,W,64) channels-last.  Grid (chunks, 7): blockIdx.y = ky.  K step s of a tile = its row s, k = column.
// MFMA A = G (rows n, lane 16-group fq holds pixels 8 fq .. 8 fq + 7), B = X shifted by the tap (columns c).
// 64-channel forms: wave w owns channels c = 16 w .. 16 w + 15 of all seven taps of the row and all 64 n.
// conv1 (CP 4): the 16 MFMA columns are (kx, c) = (4 ct + (j >> 2), j & 3) for column tiles ct 0, 1 (kx 7 is
// discarded); wave w owns column tile w >> 1 and the row tiles nt = 2 (w & 1), 2 (w & 1) + 1.
template <int MODE>
__global__ __launch_bounds__(SG_THREADS) void k_sgb_wgrad(const float *__restrict__ G, const float *__restrict__ X,
                                                           const uint8_t *__restrict__ I, float *__restrict__ part,
                                                           int B, int H, int W, int nch, SgStd st)
{
    constexpr int CP = MODE == SG_CONV1 ? 4 : 64;
    constexpr int XW = MODE == SG_CONV1 ? SGW_TW + 8 : SGW_TW + 6;     // staged input columns (conv1: kx 7 too)
    constexpr int XS = MODE == SG_CONV1 ? 4 : SGBW_GS;                    // LDS bf16 per staged input pixel
    __shared__ __attribute__((aligned(16))) unsigned short gs[SGW_TR * SGW_TW * SGBW_GS];
    __shared__ __attribute__((aligned(16))) unsigned short xs[SGW_TR * XW * XS];

    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int fi = lane & 15, fq = lane >> 4;
    const int ky = blockIdx.y, chunk = blockIdx.x;
    const int txn = (W + SGW_TW - 1) / SGW_TW, tyn = H / SGW_TR;
    const long long tiles = (long long)B * tyn * txn;
    const long long t0 = tiles * chunk / nch, t1 = tiles * (chunk + 1) / nch;
    const long long plane = (long long)H * W;

    constexpr int NA = MODE == SG_CONV1 ? 2 : 7;
    constexpr int NT = MODE == SG_CONV1 ? 2 : 4;
    const int nt0 = MODE == SG_CONV1 ? 2 * (w & 1) : 0;
    sg_f32x4 acc[NA][NT];
#pragma unroll
    for (int a = 0; a < NA; ++a)
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) acc[a][nt] = (sg_f32x4){0.f, 0.f, 0.f, 0.f};

    // the lane's transposed-read addresses (pixel row (fi >> 2) of the 4-pixel block, column group fi & 3)
    const int kp = 8 * fq + (fi >> 2);
    const unsigned short *ga = &gs[kp * SGBW_GS + 4 * (fi & 3)];
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
            uint4 v = make_uint4(0u, 0u, 0u, 0u);
            if (gx < W) {
                const float *g = G + (((long long)b * H + gy) * W + gx) * 64 + 8 * q;
                v = sg_bf16_pack8(*(const sg_f32x4 *)g, *(const sg_f32x4 *)(g + 4));
            }
            *(uint4 *)&gs[p * SGBW_GS + 8 * q] = v;
        }
        if (MODE == SG_CONV1) {
            const float *xb = X + (long long)b * 3 * plane;
            for (int p = tid; p < SGW_TR * XW; p += SG_THREADS)
                *(uint2 *)&xs[p * XS] = sg_bf16_conv1_px(xb, plane, y0 + ky - 3 + p / XW, x0 - 3 + p % XW, H, W, st);
        } else {
            for (int e = tid; e < SGW_TR * XW * 8; e += SG_THREADS) {
                const int p = e >> 3, q = e & 7;
                *(uint4 *)&xs[p * XS + 8 * q] =
                    sg_bf16_px8<MODE>(X, I, b, y0 + ky - 3 + p / XW, x0 - 3 + p % XW, 8 * q, H, W);
            }
        }
        __syncthreads();

#pragma unroll
        for (int s = 0; s < SGW_TR; ++s) {
            sg_bf16x8 a[NT];
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) {
                const unsigned short *p0 = ga + s * SGW_TW * SGBW_GS + 16 * (nt0 + nt);
                a[nt] = sg_tr8<sg_bf16x8>(p0, p0 + 4 * SGBW_GS);
            }
            if (MODE == SG_CONV1) {
                const unsigned short *p0 = xa + s * XW * XS;
                const sg_bf16x8 bx = sg_tr8<sg_bf16x8>(p0, p0 + 4 * XS);
#pragma unroll
                for (int nt = 0; nt < NT; ++nt)
                    acc[0][nt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[nt], bx, acc[0][nt], 0, 0, 0);
            } else {
#pragma unroll
                for (int kx = 0; kx < 7; ++kx) {
                    const unsigned short *p0 = xa + (s * XW + kx) * XS;
                    const sg_bf16x8 bx = sg_tr8<sg_bf16x8>(p0, p0 + 4 * XS);
#pragma unroll
                    for (int nt = 0; nt < NT; ++nt)
                        acc[kx][nt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[nt], bx, acc[kx][nt], 0, 0, 0);
                }
            }
        }
    }

    // D layout: column (c or (kx, c)) = lane & 15, row n = 16 nt + 4 (lane >> 4) + r
    float *pb = part + ((long long)chunk * 49 + ky * 7) * 64 * CP;
    if (MODE == SG_CONV1) {
        const int kx = 4 * (w >> 1) + (fi >> 2), c = fi & 3;
        if (kx < 7) {
#pragma unroll
            for (int nt = 0; nt < NT; ++nt)
#pragma unroll
                for (int r = 0; r < 4; ++r)
                    pb[((long long)kx * 64 + 16 * (nt0 + nt) + 4 * fq + r) * CP + c] = acc[0][nt][r];
        }
    } else {
        const int c = 16 * w + fi;
#pragma unroll
        for (int kx = 0; kx < 7; ++kx)
#pragma unroll
            for (int nt = 0; nt < 4; ++nt)
#pragma unroll
                for (int r = 0; r < 4; ++r) pb[((long long)kx * 64 + 16 * nt + 4 * fq + r) * CP + c] = acc[kx][nt][r];
    }
}

// ---------------------------------------------------------------------------------------------------- C ABI
extern "C" int spa_segnet_train_forward_bf16(spa_ctx *ctx, const float *x, const uint8_t *idx, int32_t x_layout,
                                             int32_t B, int32_t H, int32_t W, int32_t Cin, const float *wt,
                                             const float *mean_host, const float *std_host, float *y, double *stats,
                                             void *stream)
{
    SPA_ARG(ctx && x && wt && y);
    int rc = sg_check_shape("spa_segnet_train_forward_bf16", B, H, W, Cin);
    if (rc != SPA_OK) return rc;
    SPA_ARG(sg_al16(x) && sg_al16(wt));
    SgStd st = {};
    rc = sg_input_form("spa_segnet_train_forward_bf16", Cin, x_layout, mean_host, std_host, idx, &st);
    if (rc != SPA_OK) return rc;
    hipStream_t s = spa_stream(stream);
    const dim3 grid = sg_conv_grid(B, H, W);
    const long long nblk = (long long)grid.x * grid.y * grid.z;
    unsigned short *wb = nullptr;
    if ((rc = spa_ws_reserve(ctx, WS_SEGNET_WBF16, SG_W64 * sizeof(unsigned short), (void **)&wb)) != SPA_OK)
        return rc;
    float *part = nullptr;
    if (stats) {
        if ((rc = spa_ws_reserve(ctx, WS_SEGNET_BNPART, (size_t)nblk * 128 * sizeof(float), (void **)&part)) != SPA_OK)
            return rc;
    }
    if (Cin == 3)
        sg_launch_bf16_wpack1(s, wt, wb);
    else
        sg_launch_bf16_wpack64(s, wt, 0, wb);
    SPA_LAUNCH_CHECK();
    if (Cin == 3)
        hipLaunchKernelGGL((k_sgb_conv<SG_CONV1, SG_FULL>), grid, dim3(SG_THREADS), 0, s, x, nullptr, wb, nullptr, y,
                           part, H, W, st);
    else if (!idx)
        hipLaunchKernelGGL((k_sgb_conv<SG_ENC, SG_FULL>), grid, dim3(SG_THREADS), 0, s, x, nullptr, wb, nullptr, y,
                           part, H, W, st);
    else
        hipLaunchKernelGGL((k_sgb_conv<SG_DEC, SG_FULL>), grid, dim3(SG_THREADS), 0, s, x, idx, wb, nullptr, y, part,
                           H, W, st);
    SPA_LAUNCH_CHECK();
    if (stats) {
        sg_launch_bnstat(s, part, nblk, stats);
        SPA_LAUNCH_CHECK();
    }
    return SPA_OK;
}

extern "C" int spa_segnet_train_dgrad_bf16(spa_ctx *ctx, const float *dy, const float *wt, const uint8_t *idx,
                                           int32_t B, int32_t H, int32_t W, float *dx, void *stream)
{
    SPA_ARG(ctx && dy && wt && dx);
    int rc = sg_check_shape("spa_segnet_train_dgrad_bf16", B, H, W, 64);
    if (rc != SPA_OK) return rc;
    SPA_ARG(sg_al16(dy) && sg_al16(wt) && ((uintptr_t)idx & 3) == 0);
    unsigned short *wb = nullptr;
    if ((rc = spa_ws_reserve(ctx, WS_SEGNET_WBF16, SG_W64 * sizeof(unsigned short), (void **)&wb)) != SPA_OK)
        return rc;
    hipStream_t s = spa_stream(stream);
    sg_launch_bf16_wpack64(s, wt, 1, wb);
    SPA_LAUNCH_CHECK();
    const dim3 grid = sg_conv_grid(B, H, W);
    if (idx)
        hipLaunchKernelGGL((k_sgb_conv<SG_ENC, SG_POOLED>), grid, dim3(SG_THREADS), 0, s, dy, nullptr, wb, idx, dx,
                           nullptr, H, W, SgStd{});
    else
        hipLaunchKernelGGL((k_sgb_conv<SG_ENC, SG_FULL>), grid, dim3(SG_THREADS), 0, s, dy, nullptr, wb, nullptr, dx,
                           nullptr, H, W, SgStd{});
    SPA_LAUNCH_CHECK();
    return SPA_OK;
}

extern "C" int spa_segnet_train_wgrad_bf16(spa_ctx *ctx, const float *dy, const float *x, const uint8_t *idx,
                                           int32_t x_layout, int32_t B, int32_t H, int32_t W, int32_t Cin,
                                           const float *mean_host, const float *std_host, float *dw, void *stream)
{
    SPA_ARG(ctx && dy && x && dw);
    int rc = sg_check_shape("spa_segnet_train_wgrad_bf16", B, H, W, Cin);
    if (rc != SPA_OK) return rc;
    SPA_ARG(sg_al16(dy) && sg_al16(x));
    SgStd st = {};
    rc = sg_input_form("spa_segnet_train_wgrad_bf16", Cin, x_layout, mean_host, std_host, idx, &st);
    if (rc != SPA_OK) return rc;
    int nch, n;
    float *part = nullptr;
    if ((rc = sg_wgrad_plan(ctx, B, H, W, Cin, &nch, &n, &part)) != SPA_OK) return rc;
    hipStream_t s = spa_stream(stream);
    dim3 grid(nch, 7);
    if (Cin == 3)
        hipLaunchKernelGGL(k_sgb_wgrad<SG_CONV1>, grid, dim3(SG_THREADS), 0, s, dy, x, nullptr, part, B, H, W, nch, st);
    else if (!idx)
        hipLaunchKernelGGL(k_sgb_wgrad<SG_ENC>, grid, dim3(SG_THREADS), 0, s, dy, x, nullptr, part, B, H, W, nch, st);
    else
        hipLaunchKernelGGL(k_sgb_wgrad<SG_DEC>, grid, dim3(SG_THREADS), 0, s, dy, x, idx, part, B, H, W, nch, st);
    SPA_LAUNCH_CHECK();
    sg_launch_wsum(s, part, nch, n, dw);
    SPA_LAUNCH_CHECK();
    return SPA_OK;
}
