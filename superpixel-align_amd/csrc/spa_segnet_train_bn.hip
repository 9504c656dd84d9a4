// SegNet-Basic training, what lies between the 7x7 convolutions (train_segnet.py --fused_bn): BatchNorm with ReLU and
// 2x2 max pooling (encoder) or alone (decoder), its backward (the two per-channel sums, then dy), and the 64 -> 2
// classifier with its backward.  All of it is streaming work on (B,H,W,64) float32 channels-last maps.
//
// Geometry of every kernel: 256 threads, lane cg = tid & 15 owns channels [4 cg, 4 cg + 4) -- one 16-byte load of a map,
// one dword of four index bytes -- and slot = tid >> 4 names one of the workgroup's 16 pixels, so a wave covers four
// whole pixels (1 KB) per load.  A workgroup walks the pixels slot + 16 (block + k grid); the grid is
// min(ceil(pixels / 16), SGB_MAXBLK), a function of the shape alone.  The per-channel parameters sit in registers.
// Encoder forms walk the POOLED pixels and touch the four full-resolution pixels of each 2x2 window.
//
// Reductions: a lane adds its terms in float32 for at most SGB_CHUNK pixels, then adds that run to a double; the four
// slots of a wave are combined by two shuffles, the four waves through LDS in wave order, one double partial per
// workgroup and output goes to the context workspace, and k_sgb_final adds the workgroups' partials in block order.  No
// atomics and no counters: the same call gives the same bits on every run and device.
#include "spa_segnet_dev.h"

#define SGB_THREADS 256
#define SGB_MAXBLK 2048               // workgroups of a streaming kernel at most (8 per CU of a 256-CU chip)
#define SGB_CHUNK 32                  // pixels a lane sums in float32 before the run goes into its double
#define SGB_NQ 192                    // doubles of one workgroup's partial: up to three quantities x 64 channels

// ---------------------------------------------------------------------------------------------------- device helpers
__device__ __forceinline__ sg_f32x4 sgb_ld4(const float *p) { return *(const sg_f32x4 *)p; }

// the full-resolution pixel index of the top-left pixel of pooled pixel pp: rows b * H + 2 py = 2 (b * Hh + py)
__device__ __forceinline__ long long sgb_window(long long pp, int Wh)
{
    // a 64-bit division costs a few hundred instructions; maps below 2^32 pooled pixels never take it
    const long long row = (pp >> 32) ? pp / Wh : (long long)((unsigned)pp / (unsigned)Wh);
    const int px = (int)(pp - row * Wh);
    return row * 4 * Wh + 2 * px;                 // (2 row) * W + 2 px, W = 2 Wh
}

// position r (ky * 2 + kx) of the window whose top-left pixel is w0
__device__ __forceinline__ long long sgb_at(long long w0, int r, int W) { return w0 + (long long)(r >> 1) * W + (r & 1); }

// this lane's Q x 4 doubles -> part[block][q * 64 + channel], slots then waves in a fixed order.  red: 4 * Q * 64 doubles
template <int Q>
__device__ __forceinline__ void sgb_block_sum(double (&d)[Q][4], double *red, double *part)
{
    const int tid = threadIdx.x, cg = tid & 15, wave = tid >> 6;
#pragma unroll
    for (int q = 0; q < Q; ++q)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            double v = d[q][j];
            v += __shfl_xor(v, 16);
            v += __shfl_xor(v, 32);
            if ((tid & 63) < 16) red[(wave * Q + q) * 64 + 4 * cg + j] = v;
        }
    __syncthreads();
    if (tid < Q * 64) {
        double t = 0.0;
#pragma unroll
        for (int w = 0; w < 4; ++w) t += red[w * Q * 64 + tid];
        part[(long long)blockIdx.x * SGB_NQ + tid] = t;
    }
}

// ---------------------------------------------------------------------------------------------------- BatchNorm forward
// o = (y - mean) * (rstd * gamma) + beta, each operation rounded on its own (the build has no contraction).
// ENC: O (B,H/2,W/2,64) = max over the window of relu(o), I its first maximum (ky * 2 + kx); n = pooled pixels.
// otherwise O (B,H,W,64) = o; n = pixels.
template <bool ENC>
__global__ __launch_bounds__(SGB_THREADS) void k_sgb_fwd(const float *__restrict__ Y, const float *__restrict__ mean,
                                                         const float *__restrict__ rstd,
                                                         const float *__restrict__ gamma,
                                                         const float *__restrict__ beta, float *__restrict__ O,
                                                         uint8_t *__restrict__ I, int W, long long n)
{
    const int cg = threadIdx.x & 15, c = 4 * cg;
    const sg_f32x4 mu = sgb_ld4(mean + c), sc = sgb_ld4(rstd + c) * sgb_ld4(gamma + c), be = sgb_ld4(beta + c);
    const long long step = (long long)gridDim.x * 16;
    for (long long p = (long long)blockIdx.x * 16 + (threadIdx.x >> 4); p < n; p += step) {
        if (ENC) {
            const long long w0 = sgb_window(p, W >> 1);
            sg_f32x4 v[4];
#pragma unroll
            for (int r = 0; r < 4; ++r) v[r] = sgb_ld4(Y + sgb_at(w0, r, W) * 64 + c);
            sg_f32x4 best;
            unsigned ix = 0u;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                float b = fmaxf((v[0][j] - mu[j]) * sc[j] + be[j], 0.f);
                unsigned k = 0u;
#pragma unroll
                for (int r = 1; r < 4; ++r) {
                    const float a = fmaxf((v[r][j] - mu[j]) * sc[j] + be[j], 0.f);
                    if (a > b) { b = a; k = (unsigned)r; }
                }
                best[j] = b;
                ix |= k << (8 * j);
            }
            *(sg_f32x4 *)(O + p * 64 + c) = best;
            *(unsigned *)(I + p * 64 + c) = ix;
        } else {
            const sg_f32x4 v = sgb_ld4(Y + p * 64 + c);
            *(sg_f32x4 *)(O + p * 64 + c) = (v - mu) * sc + be;
        }
    }
}

// ---------------------------------------------------------------------------------------------------- BatchNorm backward
// The full-resolution gradient g of the encoder form is never stored: at window position r of channel j it is the
// pooled gradient where the index byte is r and the saved pooled output is > 0 (the ReLU mask), zero elsewhere.
// An index byte is used & 3: a map that holds anything else cannot send a load outside the window.

// part[block] = this workgroup's (sum g, sum g xhat), xhat = (y - mean) * rstd.  ENC: G, P, I at the pooled size, n =
// pooled pixels, only the selected y is read; otherwise G, Y (B,H,W,64), n = pixels.
template <bool ENC>
__global__ __launch_bounds__(SGB_THREADS) void k_sgb_sums(const float *__restrict__ G, const uint8_t *__restrict__ I,
                                                          const float *__restrict__ P, const float *__restrict__ Y,
                                                          const float *__restrict__ mean,
                                                          const float *__restrict__ rstd, double *__restrict__ part,
                                                          int W, long long n)
{
    __shared__ double red[4 * 2 * 64];
    const int cg = threadIdx.x & 15, c = 4 * cg;
    const sg_f32x4 mu = sgb_ld4(mean + c), rs = sgb_ld4(rstd + c);
    const long long step = (long long)gridDim.x * 16;
    double d[2][4] = {};
    long long p = (long long)blockIdx.x * 16 + (threadIdx.x >> 4);
    while (p < n) {
        sg_f32x4 s0 = {0.f, 0.f, 0.f, 0.f}, s1 = {0.f, 0.f, 0.f, 0.f};
        for (int it = 0; it < SGB_CHUNK && p < n; ++it, p += step) {
            sg_f32x4 g = sgb_ld4(G + p * 64 + c), y;
            if (ENC) {
                const sg_f32x4 po = sgb_ld4(P + p * 64 + c);
                const unsigned ix = *(const unsigned *)(I + p * 64 + c);
                const long long w0 = sgb_window(p, W >> 1);
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    y[j] = Y[sgb_at(w0, (int)((ix >> (8 * j)) & 3u), W) * 64 + c + j];
                    g[j] = po[j] > 0.f ? g[j] : 0.f;
                }
            } else {
                y = sgb_ld4(Y + p * 64 + c);
            }
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                s0[j] += g[j];
                s1[j] = fmaf(g[j], (y[j] - mu[j]) * rs[j], s1[j]);
            }
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            d[0][j] += (double)s0[j];
            d[1][j] += (double)s1[j];
        }
    }
    sgb_block_sum<2>(d, red, part);
}

// out[j] = sum over the nblk partials of part[blk][j] in block order, in double: thread t takes blocks t, t + 256, ...,
// then a fixed tree.  One workgroup per output j.  o64 != NULL: stored as it is; otherwise rounded once to float32 into
// oa[j] (j < na) or ob[j - na].
__global__ __launch_bounds__(256) void k_sgb_final(const double *__restrict__ part, int nblk, double *__restrict__ o64,
                                                   float *__restrict__ oa, int na, float *__restrict__ ob)
{
    __shared__ double red[256];
    const int j = blockIdx.x, t = threadIdx.x;
    double s = 0.0;
    for (int i = t; i < nblk; i += 256) s += part[(long long)i * SGB_NQ + j];
    red[t] = s;
    __syncthreads();
    for (int k = 128; k >= 1; k >>= 1) {
        if (t < k) red[t] += red[t + k];
        __syncthreads();
    }
    if (t == 0) {
        if (o64) o64[j] = red[0];
        else if (j < na) oa[j] = (float)red[0];
        else ob[j - na] = (float)red[0];
    }
}

// DY (B,H,W,64) = k ((g - a) - xhat b), k = gamma rstd, a = S0 / m, b = S1 / m formed in double and rounded once:
// (gamma rstd / m) (m g - S0 - xhat S1) without the products by m, which only cost digits.  S (2,64) double.
template <bool ENC>
__global__ __launch_bounds__(SGB_THREADS) void k_sgb_dy(const float *__restrict__ G, const uint8_t *__restrict__ I,
                                                        const float *__restrict__ P, const float *__restrict__ Y,
                                                        const float *__restrict__ mean, const float *__restrict__ rstd,
                                                        const float *__restrict__ gamma, const double *__restrict__ S,
                                                        double m, float *__restrict__ DY, int W, long long n)
{
    const int cg = threadIdx.x & 15, c = 4 * cg;
    const sg_f32x4 mu = sgb_ld4(mean + c), rs = sgb_ld4(rstd + c), k = sgb_ld4(gamma + c) * rs;
    sg_f32x4 a, b;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        a[j] = (float)(S[c + j] / m);
        b[j] = (float)(S[64 + c + j] / m);
    }
    const long long step = (long long)gridDim.x * 16;
    for (long long p = (long long)blockIdx.x * 16 + (threadIdx.x >> 4); p < n; p += step) {
        const sg_f32x4 g = sgb_ld4(G + p * 64 + c);
        if (ENC) {
            const sg_f32x4 po = sgb_ld4(P + p * 64 + c);
            const unsigned ix = *(const unsigned *)(I + p * 64 + c);
            const long long w0 = sgb_window(p, W >> 1);
            sg_f32x4 y[4];
#pragma unroll
            for (int r = 0; r < 4; ++r) y[r] = sgb_ld4(Y + sgb_at(w0, r, W) * 64 + c);
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                sg_f32x4 o;
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const float gr = (((ix >> (8 * j)) & 3u) == (unsigned)r && po[j] > 0.f) ? g[j] : 0.f;
                    o[j] = k[j] * ((gr - a[j]) - (y[r][j] - mu[j]) * rs[j] * b[j]);
                }
                *(sg_f32x4 *)(DY + sgb_at(w0, r, W) * 64 + c) = o;
            }
        } else {
            const sg_f32x4 y = sgb_ld4(Y + p * 64 + c);
            *(sg_f32x4 *)(DY + p * 64 + c) = k * ((g - a) - (y - mu) * rs * b);
        }
    }
}

// ---------------------------------------------------------------------------------------------------- classifier
// S (pixels,2) = h Wc^T + bc: a lane's four products per class, then the 16 lanes of a pixel by four shuffles (a fixed
// tree); lane 0 of the pixel stores both scores.
__global__ __launch_bounds__(SGB_THREADS) void k_sgb_cls_fwd(const float *__restrict__ Hm, const float *__restrict__ Wc,
                                                             const float *__restrict__ bc, float *__restrict__ S,
                                                             long long n)
{
    const int cg = threadIdx.x & 15, c = 4 * cg;
    const sg_f32x4 w0 = sgb_ld4(Wc + c), w1 = sgb_ld4(Wc + 64 + c);
    const float b0 = bc[0], b1 = bc[1];
    const long long step = (long long)gridDim.x * 16;
    // every lane of a wave runs the same number of rounds (the shuffles need the pixel's 16 lanes): clamp, then guard
    const long long first = (long long)blockIdx.x * 16;
    for (long long q = first; q < n; q += step) {
        const long long p = q + (threadIdx.x >> 4);
        const bool in = p < n;
        const sg_f32x4 h = in ? sgb_ld4(Hm + p * 64 + c) : (sg_f32x4){0.f, 0.f, 0.f, 0.f};
        float s0 = fmaf(h[3], w0[3], fmaf(h[2], w0[2], fmaf(h[1], w0[1], h[0] * w0[0])));
        float s1 = fmaf(h[3], w1[3], fmaf(h[2], w1[2], fmaf(h[1], w1[1], h[0] * w1[0])));
#pragma unroll
        for (int k = 1; k < 16; k <<= 1) {
            s0 += __shfl_xor(s0, k);
            s1 += __shfl_xor(s1, k);
        }
        if (in && cg == 0) *(float2 *)(S + p * 2) = make_float2(s0 + b0, s1 + b1);
    }
}

// DH (pixels,64) = ds Wc; part[block] = this workgroup's (sum ds0 h, sum ds1 h, {sum ds0, sum ds1} in channels 0, 1)
__global__ __launch_bounds__(SGB_THREADS) void k_sgb_cls_bwd(const float *__restrict__ DS, const float *__restrict__ Hm,
                                                             const float *__restrict__ Wc, float *__restrict__ DH,
                                                             double *__restrict__ part, long long n)
{
    __shared__ double red[4 * 3 * 64];
    const int cg = threadIdx.x & 15, c = 4 * cg;
    const sg_f32x4 w0 = sgb_ld4(Wc + c), w1 = sgb_ld4(Wc + 64 + c);
    const long long step = (long long)gridDim.x * 16;
    double d[3][4] = {};
    long long p = (long long)blockIdx.x * 16 + (threadIdx.x >> 4);
    while (p < n) {
        sg_f32x4 a0 = {0.f, 0.f, 0.f, 0.f}, a1 = {0.f, 0.f, 0.f, 0.f};
        float t0 = 0.f, t1 = 0.f;
        for (int it = 0; it < SGB_CHUNK && p < n; ++it, p += step) {
            const float2 ds = *(const float2 *)(DS + p * 2);
            const sg_f32x4 h = sgb_ld4(Hm + p * 64 + c);
            *(sg_f32x4 *)(DH + p * 64 + c) = ds.x * w0 + ds.y * w1;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                a0[j] = fmaf(ds.x, h[j], a0[j]);
                a1[j] = fmaf(ds.y, h[j], a1[j]);
            }
            t0 += ds.x;
            t1 += ds.y;
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            d[0][j] += (double)a0[j];
            d[1][j] += (double)a1[j];
        }
        d[2][0] += (double)t0;             // every lane of a pixel holds the same two sums; lane cg 0's are kept
        d[2][1] += (double)t1;
    }
    sgb_block_sum<3>(d, red, part);
}

// ---------------------------------------------------------------------------------------------------- C ABI
// any B >= 1 and even H, W >= 2; every offset is 64-bit, so no size limit remains
static int sgb_check(const char *fn, const spa_ctx *ctx, int B, int H, int W)
{
    SG_ARG(ctx && B > 0 && H > 0 && W > 0 && H % 2 == 0 && W % 2 == 0);
    return SPA_OK;
}

static int sgb_grid(long long n) { return (int)((n + 15) / 16 < SGB_MAXBLK ? (n + 15) / 16 : SGB_MAXBLK); }

static int sgb_partials(spa_ctx *ctx, double **part)
{
    return spa_ws_reserve(ctx, WS_SEGNET_BNRED, (size_t)SGB_MAXBLK * SGB_NQ * sizeof(double), (void **)part);
}

extern "C" int spa_segnet_train_bn_forward(spa_ctx *ctx, const float *y, const float *mean, const float *rstd,
                                           const float *gamma, const float *beta, int32_t B, int32_t H, int32_t W,
                                           float *out, uint8_t *idx, void *stream)
{
    int rc = sgb_check("spa_segnet_train_bn_forward", ctx, B, H, W);
    if (rc != SPA_OK) return rc;
    SPA_ARG(y && mean && rstd && gamma && beta && out);
    SPA_ARG(sg_al16(y) && sg_al16(mean) && sg_al16(rstd) && sg_al16(gamma) && sg_al16(beta) && sg_al16(out) &&
            ((uintptr_t)idx & 3) == 0);
    hipStream_t s = spa_stream(stream);
    const long long n = (long long)B * H * W;
    if (idx)
        hipLaunchKernelGGL(k_sgb_fwd<true>, dim3(sgb_grid(n / 4)), dim3(SGB_THREADS), 0, s, y, mean, rstd, gamma, beta,
                           out, idx, W, n / 4);
    else
        hipLaunchKernelGGL(k_sgb_fwd<false>, dim3(sgb_grid(n)), dim3(SGB_THREADS), 0, s, y, mean, rstd, gamma, beta,
                           out, nullptr, W, n);
    SPA_LAUNCH_CHECK();
    return SPA_OK;
}

extern "C" int spa_segnet_train_bn_backward_sums(spa_ctx *ctx, const float *g, const uint8_t *idx, const float *p,
                                                 const float *y, const float *mean, const float *rstd, int32_t B,
                                                 int32_t H, int32_t W, double *sums, void *stream)
{
    int rc = sgb_check("spa_segnet_train_bn_backward_sums", ctx, B, H, W);
    if (rc != SPA_OK) return rc;
    SPA_ARG(g && y && mean && rstd && sums && (idx == nullptr) == (p == nullptr));
    SPA_ARG(sg_al16(g) && sg_al16(y) && sg_al16(mean) && sg_al16(rstd) && sg_al16(p) && ((uintptr_t)idx & 3) == 0 &&
            ((uintptr_t)sums & 7) == 0);
    double *part = nullptr;
    if ((rc = sgb_partials(ctx, &part)) != SPA_OK) return rc;
    hipStream_t s = spa_stream(stream);
    const long long n = idx ? (long long)B * H * W / 4 : (long long)B * H * W;
    const int nblk = sgb_grid(n);
    if (idx)
        hipLaunchKernelGGL(k_sgb_sums<true>, dim3(nblk), dim3(SGB_THREADS), 0, s, g, idx, p, y, mean, rstd, part, W, n);
    else
        hipLaunchKernelGGL(k_sgb_sums<false>, dim3(nblk), dim3(SGB_THREADS), 0, s, g, nullptr, nullptr, y, mean, rstd,
                           part, W, n);
    SPA_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_sgb_final, dim3(128), dim3(256), 0, s, part, nblk, sums, nullptr, 0, nullptr);
    SPA_LAUNCH_CHECK();
    return SPA_OK;
}

extern "C" int spa_segnet_train_bn_backward_dy(spa_ctx *ctx, const float *g, const uint8_t *idx, const float *p,
                                               const float *y, const float *mean, const float *rstd,
                                               const float *gamma, const double *sums, double m, int32_t B, int32_t H,
                                               int32_t W, float *dy, void *stream)
{
    int rc = sgb_check("spa_segnet_train_bn_backward_dy", ctx, B, H, W);
    if (rc != SPA_OK) return rc;
    SPA_ARG(g && y && mean && rstd && gamma && sums && dy && m >= 1.0 && (idx == nullptr) == (p == nullptr));
    SPA_ARG(sg_al16(g) && sg_al16(y) && sg_al16(mean) && sg_al16(rstd) && sg_al16(gamma) && sg_al16(p) &&
            sg_al16(dy) && ((uintptr_t)idx & 3) == 0 && ((uintptr_t)sums & 7) == 0);
    hipStream_t s = spa_stream(stream);
    const long long n = idx ? (long long)B * H * W / 4 : (long long)B * H * W;
    if (idx)
        hipLaunchKernelGGL(k_sgb_dy<true>, dim3(sgb_grid(n)), dim3(SGB_THREADS), 0, s, g, idx, p, y, mean, rstd, gamma,
                           sums, m, dy, W, n);
    else
        hipLaunchKernelGGL(k_sgb_dy<false>, dim3(sgb_grid(n)), dim3(SGB_THREADS), 0, s, g, nullptr, nullptr, y, mean,
                           rstd, gamma, sums, m, dy, W, n);
    SPA_LAUNCH_CHECK();
    return SPA_OK;
}

extern "C" int spa_segnet_train_classifier_forward(spa_ctx *ctx, const float *h, const float *wc, const float *bc,
                                                   int32_t B, int32_t H, int32_t W, float *score, void *stream)
{
    int rc = sgb_check("spa_segnet_train_classifier_forward", ctx, B, H, W);
    if (rc != SPA_OK) return rc;
    SPA_ARG(h && wc && bc && score);
    SPA_ARG(sg_al16(h) && sg_al16(wc) && ((uintptr_t)bc & 3) == 0 && ((uintptr_t)score & 7) == 0);
    const long long n = (long long)B * H * W;
    hipLaunchKernelGGL(k_sgb_cls_fwd, dim3(sgb_grid(n)), dim3(SGB_THREADS), 0, spa_stream(stream), h, wc, bc, score, n);
    SPA_LAUNCH_CHECK();
    return SPA_OK;
}

extern "C" int spa_segnet_train_classifier_backward(spa_ctx *ctx, const float *dscore, const float *h, const float *wc,
                                                    int32_t B, int32_t H, int32_t W, float *dh, float *dwc, float *db,
                                                    void *stream)
{
    int rc = sgb_check("spa_segnet_train_classifier_backward", ctx, B, H, W);
    if (rc != SPA_OK) return rc;
    SPA_ARG(dscore && h && wc && dh && dwc && db);
    SPA_ARG(sg_al16(h) && sg_al16(wc) && sg_al16(dh) && ((uintptr_t)dscore & 7) == 0 && ((uintptr_t)dwc & 3) == 0 &&
            ((uintptr_t)db & 3) == 0);
    double *part = nullptr;
    if ((rc = sgb_partials(ctx, &part)) != SPA_OK) return rc;
    hipStream_t s = spa_stream(stream);
    const long long n = (long long)B * H * W;
    const int nblk = sgb_grid(n);
    hipLaunchKernelGGL(k_sgb_cls_bwd, dim3(nblk), dim3(SGB_THREADS), 0, s, dscore, h, wc, dh, part, n);
    SPA_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_sgb_final, dim3(130), dim3(256), 0, s, part, nblk, (double *)nullptr, dwc, 128, db);
    SPA_LAUNCH_CHECK();
    return SPA_OK;
}
