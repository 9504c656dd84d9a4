// SegNet-Basic training (train_segnet.py --model basic) on the float32 matrix cores: the forward convolutions in
// training form, their input gradients (dgrad) and their weight gradients (wgrad).  Every product is a float32
// v_mfma_f32_16x16x4_f32, as in spa_segnet.hip; BatchNorm, ReLU, pooling and the loss stay with the caller.
//
//   forward:  y = conv7x7(x; W)          no bias (Convolution2D(..., nobias=True)), full-resolution y stored, plus
//                                         per-workgroup per-channel partial sums of y and y^2 for the batch statistics
//   dgrad:    dx = conv7x7(dy; W')        W'[t][c][n] = W[48 - t][n][c] (rotated 180 degrees, in/out swapped)
//             decoder layers: dh[p] = dx[2p + idx(p)], the gradient at the pooled input, gathered in the epilogue
//   wgrad:    dW[t][n][c] = sum_{b,y,x} dy[b,y,x,n] * x[b, y + ky - 3, x + kx - 3, c]
//
// Tiling, the three input forms, the forward / dgrad K loop (shared with spa_segnet.hip) and the epilogues:
// spa_segnet_dev.h.  This file owns the kernels' LDS and launches, the float32 wgrad kernel and the two reductions
// every operand type ends with (k_sg_bnstat, k_sg_wsum).
//
// wgrad is split-K: K = B*H*W pixels in 2 x 32 tiles, chunk j of sg_wgrad_plan's (at most 96) owns a contiguous run of
// tiles, one workgroup per (chunk, ky).  Each writes its chunk's partial dW to the context workspace; a second kernel
// sums the chunks in chunk order (in double).  No atomics anywhere.
#include "spa_segnet_dev.h"

// Y = conv7x7(input form MODE of X (, I); Wt) at output resolution (H, W), Wt (49,64,CP) = (tap, n, c); EPI, Io, part:
// sg_train_epilogue.
template <int MODE, int EPI>
__global__ __launch_bounds__(SG_THREADS) void k_sgt_conv(const float *__restrict__ X, const uint8_t *__restrict__ I,
                                                         const float *__restrict__ Wt, const uint8_t *__restrict__ Io,
                                                         float *__restrict__ Y, float *__restrict__ part, int H, int W,
                                                         SgStd st)
{
    constexpr int NHALO = SG_HPIX * sg_ps_f32(MODE);
    constexpr int NLDS = NHALO > 2048 ? NHALO : 2048;                    // the halo, or the BN reduction
    __shared__ __attribute__((aligned(16))) float xs[NLDS];

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

    sg_conv_main_f32<MODE>(acc, xs, X, I, Wt, b, ty0, tx0, g, H, W, st);

    sg_train_epilogue<EPI>(acc, Io, Y, part, xs, b, ty0, tx0, w, fi, fq, H, W);
}

// Wr[t][c][n] = Wt[48 - t][n][c] (64 x 64 per tap)
__global__ __launch_bounds__(256) void k_sgt_wrot(const float *__restrict__ Wt, float *__restrict__ Wr)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= 49 * 64 * 64) return;
    const int t = i / 4096, c = (i >> 6) & 63, n = i & 63;
    Wr[i] = Wt[((48 - t) * 64 + n) * 64 + c];
}

// ---------------------------------------------------------------------------------------------------- wgrad
#define SGW_XW (SGW_TW + 6)          // staged input columns
#define SGW_GS 68                    // LDS floats per staged 64-channel pixel

// part[(chunk * 49 + ky * 7 + kx) * 64 * CP + n * CP + c] = the chunk's sum of G[p][n] * X[p + (ky - 3, kx - 3)][c].
// G (B,H,W,64) channels-last.  Grid (chunks, 7): blockIdx.y = ky.
// 64-channel forms: wave w owns channels c = 16 w .. 16 w + 15 of all seven taps of the row and all 64 n: MFMA A = G
// (rows n, K = 4 pixels), B = X shifted by the tap (columns c), 7 x 4 accumulator tiles.
// conv1 (CP 4): the 16 MFMA columns are (kx, c) = (4 ct + (j >> 2), j & 3) for column tiles ct 0, 1 (kx 7 is zero);
// the four waves take every fourth K step of a tile and their sums are added in wave order at the end.
template <int MODE>
__global__ __launch_bounds__(SG_THREADS) void k_sgt_wgrad(const float *__restrict__ G, const float *__restrict__ X,
                                                          const uint8_t *__restrict__ I, float *__restrict__ part,
                                                          int B, int H, int W, int nch, SgStd st)
{
    constexpr int CP = MODE == SG_CONV1 ? 4 : 64;
    constexpr int XS = MODE == SG_CONV1 ? 4 : SGW_GS;      // LDS floats per staged input pixel
    constexpr int NG = SGW_TR * SGW_TW * SGW_GS;
    constexpr int NX = SGW_TR * SGW_XW * XS;
    constexpr int NLDS = MODE == SG_CONV1 ? (NG + NX > 4 * 64 * 32 ? NG + NX : 4 * 64 * 32) : NG + NX;
    __shared__ __attribute__((aligned(16))) float lds[NLDS];
    float *gs = lds, *xs = lds + NG;

    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int fi = lane & 15, fq = lane >> 4;
    const int ky = blockIdx.y, chunk = blockIdx.x;
    const int txn = (W + SGW_TW - 1) / SGW_TW, tyn = H / SGW_TR;
    const long long tiles = (long long)B * tyn * txn;
    const long long t0 = tiles * chunk / nch, t1 = tiles * (chunk + 1) / nch;
    const long long plane = (long long)H * W;

    constexpr int NA = MODE == SG_CONV1 ? 2 : 7;
    sg_f32x4 acc[NA][4];
#pragma unroll
    for (int a = 0; a < NA; ++a)
#pragma unroll
        for (int nt = 0; nt < 4; ++nt) acc[a][nt] = (sg_f32x4){0.f, 0.f, 0.f, 0.f};

    for (long long t = t0; t < t1; ++t) {
        int b, y0, x0;
        sg_wgrad_tile(t, txn, tyn, b, y0, x0);
        if (t != t0) __syncthreads();
        // stage G (zero past the right edge: those pixels contribute nothing) and the input rows y0 + ky - 3 + r
        for (int e = tid; e < SGW_TR * SGW_TW * 16; e += SG_THREADS) {
            const int p = e >> 4, q = e & 15;
            const int gy = y0 + p / SGW_TW, gx = x0 + p % SGW_TW;
            sg_f32x4 v = {0.f, 0.f, 0.f, 0.f};
            if (gx < W) v = *(const sg_f32x4 *)(G + (((long long)b * H + gy) * W + gx) * 64 + 4 * q);
            *(sg_f32x4 *)&gs[p * SGW_GS + 4 * q] = v;
        }
        if (MODE == SG_CONV1) {
            const float *xb = X + (long long)b * 3 * plane;
            for (int p = tid; p < SGW_TR * SGW_XW; p += SG_THREADS)
                *(sg_f32x4 *)&xs[p * XS] =
                    sg_conv1_val4(xb, plane, y0 + ky - 3 + p / SGW_XW, x0 - 3 + p % SGW_XW, H, W, st);
        } else {
            for (int e = tid; e < SGW_TR * SGW_XW * 16; e += SG_THREADS) {
                const int p = e >> 4, q = e & 15;
                *(sg_f32x4 *)&xs[p * XS + 4 * q] =
                    sg_px4<MODE>(X, I, b, y0 + ky - 3 + p / SGW_XW, x0 - 3 + p % SGW_XW, 4 * q, H, W);
            }
        }
        __syncthreads();

        if (MODE == SG_CONV1) {
            const int kxo = fi >> 2, c = fi & 3;
            for (int s = w; s < SGW_TR * SGW_TW / 4; s += 4) {
                const int k = 4 * s + fq, pr = k / SGW_TW, pc = k % SGW_TW;
                float a[4], bx[2];
#pragma unroll
                for (int nt = 0; nt < 4; ++nt) a[nt] = gs[k * SGW_GS + 16 * nt + fi];
#pragma unroll
                for (int ct = 0; ct < 2; ++ct) {
                    const int kx = 4 * ct + kxo;
                    bx[ct] = kx < 7 ? xs[(pr * SGW_XW + pc + kx) * XS + c] : 0.f;
                }
#pragma unroll
                for (int ct = 0; ct < 2; ++ct)
#pragma unroll
                    for (int nt = 0; nt < 4; ++nt)
                        acc[ct][nt] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[nt], bx[ct], acc[ct][nt], 0, 0, 0);
            }
        } else {
            const int c = 16 * w + fi;
            for (int s = 0; s < SGW_TR * SGW_TW / 4; ++s) {
                const int k = 4 * s + fq, pr = k / SGW_TW, pc = k % SGW_TW;
                float a[4];
#pragma unroll
                for (int nt = 0; nt < 4; ++nt) a[nt] = gs[k * SGW_GS + 16 * nt + fi];
                const float *xr = &xs[(pr * SGW_XW + pc) * XS + c];
#pragma unroll
                for (int kx = 0; kx < 7; ++kx) {
                    const float bx = xr[kx * XS];
#pragma unroll
                    for (int nt = 0; nt < 4; ++nt)
                        acc[kx][nt] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[nt], bx, acc[kx][nt], 0, 0, 0);
                }
            }
        }
    }

    // D layout: column (c or (kx, c)) = lane & 15, row n = 16 nt + 4 (lane >> 4) + r
    float *pb = part + ((long long)chunk * 49 + ky * 7) * 64 * CP;
    if (MODE == SG_CONV1) {
        __syncthreads();
        float *red = lds;
#pragma unroll
        for (int ct = 0; ct < 2; ++ct)
#pragma unroll
            for (int nt = 0; nt < 4; ++nt)
#pragma unroll
                for (int r = 0; r < 4; ++r) red[((w * 2 + ct) * 16 + nt * 4 + r) * 64 + lane] = acc[ct][nt][r];
        __syncthreads();
        if (w == 0) {
#pragma unroll
            for (int ct = 0; ct < 2; ++ct) {
                const int kx = 4 * ct + (fi >> 2), c = fi & 3;
#pragma unroll
                for (int nt = 0; nt < 4; ++nt)
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const int j = (ct * 16 + nt * 4 + r) * 64 + lane;
                        const float v = ((red[j] + red[2 * 16 * 64 + j]) + red[4 * 16 * 64 + j]) + red[6 * 16 * 64 + j];
                        if (kx < 7) pb[((long long)kx * 64 + 16 * nt + 4 * fq + r) * CP + c] = v;
                    }
            }
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

// ---------------------------------------------------------------------------------------------------- reductions
// stats[k * 64 + n] = sum over the nblk partials of part[blk][k * 64 + n], in block order, in double (k 0: sum y,
// 1: sum y^2).  One workgroup per (k, n); thread t takes blocks t, t + 256, ...; then a fixed tree.
__global__ __launch_bounds__(256) void k_sg_bnstat(const float *__restrict__ part, long long nblk,
                                                   double *__restrict__ stats)
{
    __shared__ double red[256];
    const int j = blockIdx.x, t = threadIdx.x;
    double s = 0.0;
    for (long long i = t; i < nblk; i += 256) s += (double)part[i * 128 + j];
    red[t] = s;
    __syncthreads();
    for (int d = 128; d >= 1; d >>= 1) {
        if (t < d) red[t] += red[t + d];
        __syncthreads();
    }
    if (t == 0) stats[j] = red[0];
}

SG_LOCAL void sg_launch_bnstat(hipStream_t s, const float *part, long long nblk, double *stats)
{
    hipLaunchKernelGGL(k_sg_bnstat, dim3(128), dim3(256), 0, s, part, nblk, stats);
}

// dw[i] = sum over chunks j = 0 .. nch - 1 of part[j * n + i], in chunk order, in double, rounded once
__global__ __launch_bounds__(256) void k_sg_wsum(const float *__restrict__ part, int nch, int n,
                                                 float *__restrict__ dw)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    double s = 0.0;
    for (int j = 0; j < nch; ++j) s += (double)part[(long long)j * n + i];
    dw[i] = (float)s;
}

SG_LOCAL void sg_launch_wsum(hipStream_t s, const float *part, int nch, int n, float *dw)
{
    hipLaunchKernelGGL(k_sg_wsum, dim3((n + 255) / 256), dim3(256), 0, s, part, nch, n, dw);
}

// ---------------------------------------------------------------------------------------------------- C ABI
extern "C" int spa_segnet_train_forward(spa_ctx *ctx, const float *x, const uint8_t *idx, int32_t x_layout, int32_t B,
                                        int32_t H, int32_t W, int32_t Cin, const float *wt, const float *mean_host,
                                        const float *std_host, float *y, double *stats, void *stream)
{
    SPA_ARG(ctx && x && wt && y);
    int rc = sg_check_shape("spa_segnet_train_forward", B, H, W, Cin);
    if (rc != SPA_OK) return rc;
    SPA_ARG(sg_al16(x) && sg_al16(wt));
    SgStd st = {};
    rc = sg_input_form("spa_segnet_train_forward", Cin, x_layout, mean_host, std_host, idx, &st);
    if (rc != SPA_OK) return rc;
    hipStream_t s = spa_stream(stream);
    const dim3 grid = sg_conv_grid(B, H, W);
    const long long nblk = (long long)grid.x * grid.y * grid.z;
    float *part = nullptr;
    if (stats) {
        if ((rc = spa_ws_reserve(ctx, WS_SEGNET_BNPART, (size_t)nblk * 128 * sizeof(float), (void **)&part)) != SPA_OK)
            return rc;
    }
    if (Cin == 3)
        hipLaunchKernelGGL((k_sgt_conv<SG_CONV1, SG_FULL>), grid, dim3(SG_THREADS), 0, s, x, nullptr, wt, nullptr, y,
                           part, H, W, st);
    else if (!idx)
        hipLaunchKernelGGL((k_sgt_conv<SG_ENC, SG_FULL>), grid, dim3(SG_THREADS), 0, s, x, nullptr, wt, nullptr, y,
                           part, H, W, st);
    else
        hipLaunchKernelGGL((k_sgt_conv<SG_DEC, SG_FULL>), grid, dim3(SG_THREADS), 0, s, x, idx, wt, nullptr, y, part,
                           H, W, st);
    SPA_LAUNCH_CHECK();
    if (stats) {
        sg_launch_bnstat(s, part, nblk, stats);
        SPA_LAUNCH_CHECK();
    }
    return SPA_OK;
}

extern "C" int spa_segnet_train_dgrad(spa_ctx *ctx, const float *dy, const float *wt, const uint8_t *idx, int32_t B,
                                      int32_t H, int32_t W, float *dx, void *stream)
{
    SPA_ARG(ctx && dy && wt && dx);
    int rc = sg_check_shape("spa_segnet_train_dgrad", B, H, W, 64);
    if (rc != SPA_OK) return rc;
    SPA_ARG(sg_al16(dy) && sg_al16(wt) && ((uintptr_t)idx & 3) == 0);
    float *wr = nullptr;
    if ((rc = spa_ws_reserve(ctx, WS_SEGNET_WROT, 49 * 64 * 64 * sizeof(float), (void **)&wr)) != SPA_OK) return rc;
    hipStream_t s = spa_stream(stream);
    hipLaunchKernelGGL(k_sgt_wrot, dim3(49 * 64 * 64 / 256), dim3(256), 0, s, wt, wr);
    SPA_LAUNCH_CHECK();
    const dim3 grid = sg_conv_grid(B, H, W);
    if (idx)
        hipLaunchKernelGGL((k_sgt_conv<SG_ENC, SG_POOLED>), grid, dim3(SG_THREADS), 0, s, dy, nullptr, wr, idx, dx,
                           nullptr, H, W, SgStd{});
    else
        hipLaunchKernelGGL((k_sgt_conv<SG_ENC, SG_FULL>), grid, dim3(SG_THREADS), 0, s, dy, nullptr, wr, nullptr, dx,
                           nullptr, H, W, SgStd{});
    SPA_LAUNCH_CHECK();
    return SPA_OK;
}

extern "C" int spa_segnet_train_wgrad(spa_ctx *ctx, const float *dy, const float *x, const uint8_t *idx,
                                      int32_t x_layout, int32_t B, int32_t H, int32_t W, int32_t Cin,
                                      const float *mean_host, const float *std_host, float *dw, void *stream)
{
    SPA_ARG(ctx && dy && x && dw);
    int rc = sg_check_shape("spa_segnet_train_wgrad", B, H, W, Cin);
    if (rc != SPA_OK) return rc;
    SPA_ARG(sg_al16(dy) && sg_al16(x));
    SgStd st = {};
    rc = sg_input_form("spa_segnet_train_wgrad", Cin, x_layout, mean_host, std_host, idx, &st);
    if (rc != SPA_OK) return rc;
    int nch, n;
    float *part = nullptr;
    if ((rc = sg_wgrad_plan(ctx, B, H, W, Cin, &nch, &n, &part)) != SPA_OK) return rc;
    hipStream_t s = spa_stream(stream);
    dim3 grid(nch, 7);
    if (Cin == 3)
        hipLaunchKernelGGL(k_sgt_wgrad<SG_CONV1>, grid, dim3(SG_THREADS), 0, s, dy, x, nullptr, part, B, H, W, nch, st);
    else if (!idx)
        hipLaunchKernelGGL(k_sgt_wgrad<SG_ENC>, grid, dim3(SG_THREADS), 0, s, dy, x, nullptr, part, B, H, W, nch, st);
    else
        hipLaunchKernelGGL(k_sgt_wgrad<SG_DEC>, grid, dim3(SG_THREADS), 0, s, dy, x, idx, part, B, H, W, nch, st);
    SPA_LAUNCH_CHECK();
    sg_launch_wsum(s, part, nch, n, dw);
    SPA_LAUNCH_CHECK();
    return SPA_OK;
}
