// SegNet-Basic inference (models/segnet_basic.py, the network labels_from_segnet.py evaluates) on the float32 matrix
// cores: every 7x7 convolution is an implicit GEMM on v_mfma_f32_16x16x4_f32 (float32 in, float32 accumulate: an exact
// fmaf chain per output), M = output pixels, N = the 64 output channels, K = 49 taps x Cin.
//
//   encoder (conv1 .. conv4):  pooled, idx = maxpool2x2_argmax(relu(conv7x7(x) + bias))      (BatchNorm folded)
//   decoder (decode4 .. 2):    y = conv7x7(unpool(x, idx)) + bias
//   decode1:                   p = softmax(conv1x1(conv7x7(unpool(x, idx)) + bias; wc) + bc)
//   score:                     mask = argmax(Pillow BILINEAR resize of p to the evaluation shape)
//
// One workgroup = one 8 x 32 output tile x all 64 channels, 4 waves, wave w owns output rows 2w, 2w + 1.  A 16-row
// MFMA tile of a wave is FOUR 2x2 pooling blocks: row i of the tile is pixel (i & 3) of block i >> 2, so the C/D
// layout (row = 4 (lane >> 4) + reg) puts the four pixels of one 2x2 window in the four accumulator registers of one
// lane — the pooling and its argmax are register-only, and the full-resolution convolution output is never stored.
// The input halo (14 x 38 pixels) is staged in LDS 16 channels at a time (20-float pixel stride: the 16 pixels of a
// fragment read fall into distinct banks); the decoder builds the unpooled halo while staging (value where the stored
// index selects the position, zero elsewhere), so the 4x larger unpooled tensor never exists.  conv1 stages its three
// channels standardised (two float32 operations, as the dataset) and LRN-normalised (Chainer's formula), padded to 4:
// one tap = one K = 4 step.  No atomics anywhere: every output is one thread's fixed-order sum, the same bits for any
// batch size or position in the batch.
#include "spa_common.h"

typedef float f32x4 __attribute__((ext_vector_type(4)));

#define SG_TH 8                       // output tile rows
#define SG_TW 32                      // output tile columns
#define SG_HH (SG_TH + 6)             // halo rows
#define SG_HW (SG_TW + 6)             // halo columns
#define SG_HPIX (SG_HH * SG_HW)       // 532 halo pixels
#define SG_THREADS 256

enum { SG_CONV1 = 0, SG_ENC = 1, SG_DEC = 2, SG_DEC1 = 3 };

struct SgStd {
    float mean[3], std[3];
};

// Chainer's local_response_normalization, n = 5, k = 1, alpha = 1e-4 / 5, beta = 0.75 (alpha is NOT divided by n):
// with three channels every channel's window holds all three, summed in Chainer's order (own square, then the
// neighbours at distance 1, then 2).
__device__ __forceinline__ void sg_lrn3(float &a, float &b, float &c)
{
    const float a2 = a * a, b2 = b * b, c2 = c * c;
    const float s0 = (a2 + b2) + c2;          // c = 0: own, +1, +2
    const float s1 = (b2 + a2) + c2;          // c = 1: own, -1, +1
    const float s2 = (c2 + b2) + a2;          // c = 2: own, -1, -2
    const float alpha = 1e-4f / 5.f;
    a = a * powf(1.f + alpha * s0, -0.75f);
    b = b * powf(1.f + alpha * s1, -0.75f);
    c = c * powf(1.f + alpha * s2, -0.75f);
}

// MODE SG_CONV1: X (B,3,H,W) float32 planar 0..255, Wt (49,64,4).  SG_ENC: X (B,H,W,64), Wt (49,64,64).  Both write
// Y (B,H/2,W/2,64) pooled and Yi (B,H/2,W/2,64) uint8 argmax (ky * 2 + kx, first maximum).
// SG_DEC / SG_DEC1: X, I (B,H/2,W/2,64) = the pooled map and indices of the matching encoder; Y (B,H,W,64), or for
// SG_DEC1 (B,2,H,W) planar softmax probabilities (wc (2,64), bc (2) the classifier).
template <int MODE>
__global__ __launch_bounds__(SG_THREADS) void k_segnet_conv(const float *__restrict__ X, const uint8_t *__restrict__ I,
                                                            const float *__restrict__ Wt, const float *__restrict__ bias,
                                                            const float *__restrict__ wc, const float *__restrict__ bc,
                                                            float *__restrict__ Y, uint8_t *__restrict__ Yi, int H, int W,
                                                            SgStd st)
{
    constexpr int CP = MODE == SG_CONV1 ? 4 : 64;          // channels of a weight row (conv1: 3 padded to 4)
    constexpr int CH = MODE == SG_CONV1 ? 4 : 16;          // channels staged per chunk
    constexpr int PS = MODE == SG_CONV1 ? 4 : 20;          // LDS floats per halo pixel
    __shared__ __attribute__((aligned(16))) float xs[SG_HPIX * PS];

    const int tid = threadIdx.x, lane = tid & 63;
    const int w = tid >> 6;
    const int b = blockIdx.z;
    const int ty0 = blockIdx.y * SG_TH, tx0 = blockIdx.x * SG_TW;
    const int Hh = H >> 1, Wh = W >> 1;

    // this lane's fragment pixel: tile row i = lane & 15 is pixel (i & 3) of 2x2 block i >> 2
    const int fi = lane & 15, fq = lane >> 4;
    const int frow = 2 * w + ((fi & 3) >> 1), fcol = 2 * (fi >> 2) + (fi & 1);

    f32x4 acc[4][4];
#pragma unroll
    for (int m = 0; m < 4; ++m)
#pragma unroll
        for (int nt = 0; nt < 4; ++nt) acc[m][nt] = (f32x4){0.f, 0.f, 0.f, 0.f};

    for (int c0 = 0; c0 < CP; c0 += CH) {
        if (c0) __syncthreads();
        // ---- stage the halo of channels [c0, c0 + CH)
        if (MODE == SG_CONV1) {
            const long long plane = (long long)H * W;
            const float *xb = X + (long long)b * 3 * plane;
            for (int p = tid; p < SG_HPIX; p += SG_THREADS) {
                const int gy = ty0 - 3 + p / SG_HW, gx = tx0 - 3 + p % SG_HW;
                f32x4 v = {0.f, 0.f, 0.f, 0.f};
                if (gy >= 0 && gy < H && gx >= 0 && gx < W) {
                    const long long o = (long long)gy * W + gx;
                    float r = xb[o], g = xb[plane + o], bl = xb[2 * plane + o];
                    r = (r - st.mean[0]) / st.std[0];              // img -= mean; img /= std (two roundings)
                    g = (g - st.mean[1]) / st.std[1];
                    bl = (bl - st.mean[2]) / st.std[2];
                    sg_lrn3(r, g, bl);
                    v = (f32x4){r, g, bl, 0.f};
                }
                *(f32x4 *)&xs[p * PS] = v;
            }
        } else {
            for (int e = tid; e < SG_HPIX * 4; e += SG_THREADS) {
                const int p = e >> 2, q = e & 3;
                const int gy = ty0 - 3 + p / SG_HW, gx = tx0 - 3 + p % SG_HW;
                f32x4 v = {0.f, 0.f, 0.f, 0.f};
                if (gy >= 0 && gy < H && gx >= 0 && gx < W) {
                    if (MODE == SG_ENC) {
                        v = *(const f32x4 *)(X + (((long long)b * H + gy) * W + gx) * 64 + c0 + 4 * q);
                    } else {
                        const long long o = (((long long)b * Hh + (gy >> 1)) * Wh + (gx >> 1)) * 64 + c0 + 4 * q;
                        const f32x4 h = *(const f32x4 *)(X + o);
                        const unsigned ix = *(const unsigned *)(I + o);
                        const unsigned sel = (unsigned)(((gy & 1) << 1) | (gx & 1));
                        v.x = ((ix & 0xffu) == sel) ? h.x : 0.f;
                        v.y = (((ix >> 8) & 0xffu) == sel) ? h.y : 0.f;
                        v.z = (((ix >> 16) & 0xffu) == sel) ? h.z : 0.f;
                        v.w = ((ix >> 24) == sel) ? h.w : 0.f;
                    }
                }
                *(f32x4 *)&xs[p * PS + 4 * q] = v;
            }
        }
        __syncthreads();

        // ---- 49 taps x CH channels.  K order inside a chunk (64-channel forms): MFMA step s takes channel
        // c0 + 4 (lane >> 4) + s from both operands, so one 16-byte read per operand serves four steps.
        const float *wl = Wt + (long long)fi * CP + c0 + (MODE == SG_CONV1 ? fq : 4 * fq);
        for (int ky = 0; ky < 7; ++ky) {
            const float *xr = &xs[((frow + ky) * SG_HW + fcol) * PS + (MODE == SG_CONV1 ? fq : 4 * fq)];
#pragma unroll
            for (int kx = 0; kx < 7; ++kx) {
                const float *wt = wl + (long long)(ky * 7 + kx) * 64 * CP;
                if (MODE == SG_CONV1) {
                    float bw[4], a[4];
#pragma unroll
                    for (int nt = 0; nt < 4; ++nt) bw[nt] = wt[nt * 16 * CP];
#pragma unroll
                    for (int m = 0; m < 4; ++m) a[m] = xr[(kx + 8 * m) * PS];
#pragma unroll
                    for (int m = 0; m < 4; ++m)
#pragma unroll
                        for (int nt = 0; nt < 4; ++nt)
                            acc[m][nt] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[m], bw[nt], acc[m][nt], 0, 0, 0);
                } else {
                    f32x4 bw[4], a[4];
#pragma unroll
                    for (int nt = 0; nt < 4; ++nt) bw[nt] = *(const f32x4 *)(wt + nt * 16 * CP);
#pragma unroll
                    for (int m = 0; m < 4; ++m) a[m] = *(const f32x4 *)&xr[(kx + 8 * m) * PS];
#pragma unroll
                    for (int s = 0; s < 4; ++s)
#pragma unroll
                        for (int m = 0; m < 4; ++m)
#pragma unroll
                            for (int nt = 0; nt < 4; ++nt)
                                acc[m][nt] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[m][s], bw[nt][s], acc[m][nt], 0, 0, 0);
                }
            }
        }
    }

    // ---- epilogue.  Lane: channel n = 16 nt + (lane & 15); register r = pixel r (ky * 2 + kx) of block (lane >> 4)
    // of MFMA tile m, i.e. output rows ty0 + 2w + (r >> 1), columns tx0 + 8m + 2 (lane >> 4) + (r & 1).
    const int oy = ty0 + 2 * w, ox = tx0 + 2 * fq;
    if (MODE == SG_CONV1 || MODE == SG_ENC) {
        const int py = oy >> 1;
        if (py >= Hh) return;
#pragma unroll
        for (int m = 0; m < 4; ++m) {
            const int px = (ox >> 1) + 4 * m;
            if (px >= Wh) continue;
            const long long o = (((long long)b * Hh + py) * Wh + px) * 64;
#pragma unroll
            for (int nt = 0; nt < 4; ++nt) {
                const int n = 16 * nt + fi;
                const float bn = bias[n];
                float best = 0.f;
                int arg = 0;
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    float v = acc[m][nt][r] + bn;
                    v = v > 0.f ? v : 0.f;                            // relu
                    if (r == 0 || best < v) { best = v; arg = r; }     // first maximum in window order
                }
                Y[o + n] = best;
                Yi[o + n] = (uint8_t)arg;
            }
        }
    } else if (MODE == SG_DEC) {
        if (oy >= H) return;
#pragma unroll
        for (int m = 0; m < 4; ++m) {
            const int x = ox + 8 * m;
            if (x >= W) continue;
#pragma unroll
            for (int nt = 0; nt < 4; ++nt) {
                const int n = 16 * nt + fi;
                const float bn = bias[n];
#pragma unroll
                for (int r = 0; r < 4; ++r)
                    Y[(((long long)b * H + oy + (r >> 1)) * W + x + (r & 1)) * 64 + n] = acc[m][nt][r] + bn;
            }
        }
    } else {
        // decode1: classifier over the 64 channels = this lane's four channels, then a butterfly over the 16 lanes of
        // the block (commutative pairwise sums: every lane of the group ends with the same bits), then the softmax
        float w0[4], w1[4], bn[4];
#pragma unroll
        for (int nt = 0; nt < 4; ++nt) {
            bn[nt] = bias[16 * nt + fi];
            w0[nt] = wc[16 * nt + fi];
            w1[nt] = wc[64 + 16 * nt + fi];
        }
        const float b0 = bc[0], b1 = bc[1];
        const long long plane = (long long)H * W;
        for (int m = 0; m < 4; ++m) {
            float z0[4], z1[4];
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                float s0 = 0.f, s1 = 0.f;
#pragma unroll
                for (int nt = 0; nt < 4; ++nt) {
                    const float h = acc[m][nt][r] + bn[nt];
                    s0 = fmaf(h, w0[nt], s0);
                    s1 = fmaf(h, w1[nt], s1);
                }
#pragma unroll
                for (int d = 8; d >= 1; d >>= 1) {
                    s0 += __shfl_xor(s0, d, 64);
                    s1 += __shfl_xor(s1, d, 64);
                }
                z0[r] = s0 + b0;
                z1[r] = s1 + b1;
            }
            const int x = ox + 8 * m;
            if (oy >= H || x >= W || fi >= 4) continue;
            float za = z0[0], zb = z1[0];
#pragma unroll
            for (int r = 1; r < 4; ++r)
                if (fi == r) { za = z0[r]; zb = z1[r]; }
            const float mx = za > zb ? za : zb;
            const float e0 = expf(za - mx), e1 = expf(zb - mx);
            const float sum = e0 + e1;
            const long long o = (long long)b * 2 * plane + (long long)(oy + (fi >> 1)) * W + x + (fi & 1);
            Y[o] = e0 / sum;
            Y[o + plane] = e1 / sum;
        }
    }
}

// Pillow's Image.resize(BILINEAR) of a mode 'F' image (chainercv.transforms.resize of the float32 score, PIL backend),
// upscales: per axis the coefficients of Resample.c precompute_coeffs in double (support 1, window bounds rounded by
// truncation and clipped, weights normalised by their sum), a horizontal pass accumulated in double and stored as
// float32, then the vertical pass over those float32 rows.  Each thread recomputes the (at most 3) horizontal values it
// needs with the same operations in the same order, so the result is Pillow's, bit for bit.
__device__ __forceinline__ int sg_pil_coeffs(int o, int in_size, double scale, double *k)
{
    const double center = (o + 0.5) * scale;
    int lo = (int)(center - 1.0 + 0.5);
    if (lo < 0) lo = 0;
    int hi = (int)(center + 1.0 + 0.5);
    if (hi > in_size) hi = in_size;
    const int n = hi - lo;
    double ww = 0.0;
    for (int j = 0; j < 3; ++j) {
        double t = 0.0;
        if (j < n) {
            double x = ((double)(j + lo) - center + 0.5) * 1.0;
            if (x < 0.0) x = -x;
            t = x < 1.0 ? 1.0 - x : 0.0;
        }
        k[j] = t;
        ww += t;
    }
    for (int j = 0; j < 3; ++j)
        if (ww != 0.0) k[j] /= ww;
    return lo | (n << 24);
}

__global__ __launch_bounds__(256) void k_segnet_score(const float *__restrict__ P, int h, int w, int H, int W,
                                                      uint8_t *__restrict__ mask, float *__restrict__ S)
{
    const int x = blockIdx.x * 256 + threadIdx.x, y = blockIdx.y, b = blockIdx.z;
    if (x >= W) return;
    double kx[3], ky[3];
    const int bx = sg_pil_coeffs(x, w, (double)w / (double)W, kx);
    const int by = sg_pil_coeffs(y, h, (double)h / (double)H, ky);
    const int x0 = bx & 0xffffff, nx = bx >> 24, y0 = by & 0xffffff, ny = by >> 24;
    float out[2];
#pragma unroll
    for (int c = 0; c < 2; ++c) {
        const float *pc = P + ((long long)b * 2 + c) * h * w;
        double sv = 0.0;
        for (int j = 0; j < ny; ++j) {
            const float *row = pc + (long long)(y0 + j) * w + x0;
            double sh = 0.0;
            for (int i = 0; i < nx; ++i) sh += (double)row[i] * kx[i];
            sv += (double)(float)sh * ky[j];
        }
        out[c] = (float)sv;
    }
    const long long o = ((long long)b * H + y) * W + x;
    mask[o] = out[1] > out[0] ? 1 : 0;                // argmax, ties to class 0
    if (S) {
        S[((long long)b * 2) * H * W + (long long)y * W + x] = out[0];
        S[((long long)b * 2 + 1) * H * W + (long long)y * W + x] = out[1];
    }
}

static bool sg_al16(const void *p) { return ((uintptr_t)p & 15) == 0; }

extern "C" int spa_segnet_encode(spa_ctx *ctx, const float *x, int32_t x_layout, int32_t B, int32_t H, int32_t W,
                                 int32_t Cin, const float *wt, const float *bias, const float *mean_host,
                                 const float *std_host, float *pooled, uint8_t *idx, void *stream)
{
    SPA_ARG(ctx && x && wt && bias && pooled && idx && B > 0 && B < 65536 && H > 0 && W > 0);
    SPA_ARG(Cin == 3 || Cin == 64);
    // conv1 sees the network input: all four poolings must be even (H, W % 16); the deeper layers pool once more
    SPA_ARG(Cin == 3 ? (H % 16 == 0 && W % 16 == 0) : (H % 2 == 0 && W % 2 == 0));
    SPA_ARG((long long)H * W * 64 < (1ll << 31) && H / SG_TH < 65536);
    SPA_ARG(sg_al16(x) && sg_al16(wt));
    if (Cin == 3) {
        SPA_ARG(mean_host && std_host);
        if (x_layout != SPA_LAYOUT_NCHW) {
            spa_set_error("spa_segnet_encode: the conv1 input is the planar (B,3,H,W) image");
            return SPA_ERR_LAYOUT;
        }
    } else if (x_layout != SPA_LAYOUT_NHWC) {
        spa_set_error("spa_segnet_encode: 64-channel inputs must be channels-last (B,H,W,64)");
        return SPA_ERR_LAYOUT;
    }
    SgStd st = {};
    if (Cin == 3)
        for (int c = 0; c < 3; ++c) { st.mean[c] = mean_host[c]; st.std[c] = std_host[c]; }
    hipStream_t s = spa_stream(stream);
    dim3 grid((W + SG_TW - 1) / SG_TW, (H + SG_TH - 1) / SG_TH, B);
    if (Cin == 3)
        hipLaunchKernelGGL(k_segnet_conv<SG_CONV1>, grid, dim3(SG_THREADS), 0, s, x, nullptr, wt, bias, nullptr, nullptr,
                           pooled, idx, H, W, st);
    else
        hipLaunchKernelGGL(k_segnet_conv<SG_ENC>, grid, dim3(SG_THREADS), 0, s, x, nullptr, wt, bias, nullptr, nullptr,
                           pooled, idx, H, W, st);
    SPA_LAUNCH_CHECK();
    return SPA_OK;
}

extern "C" int spa_segnet_decode(spa_ctx *ctx, const float *x, const uint8_t *idx, int32_t x_layout, int32_t B,
                                 int32_t Hh, int32_t Wh, const float *wt, const float *bias, const float *wc,
                                 const float *bc, float *y, void *stream)
{
    SPA_ARG(ctx && x && idx && wt && bias && y && B > 0 && B < 65536 && Hh > 0 && Wh > 0);
    SPA_ARG((wc == nullptr) == (bc == nullptr));
    const int H = 2 * Hh, W = 2 * Wh;
    // decode1 writes the network's output: the input size, a multiple of 16
    SPA_ARG(!wc || (H % 16 == 0 && W % 16 == 0));
    SPA_ARG((long long)H * W * 64 < (1ll << 31) && H / SG_TH < 65536);
    SPA_ARG(sg_al16(x) && sg_al16(wt) && ((uintptr_t)idx & 3) == 0);
    if (x_layout != SPA_LAYOUT_NHWC) {
        spa_set_error("spa_segnet_decode: the pooled map and its indices must be channels-last (B,H/2,W/2,64)");
        return SPA_ERR_LAYOUT;
    }
    hipStream_t s = spa_stream(stream);
    dim3 grid((W + SG_TW - 1) / SG_TW, (H + SG_TH - 1) / SG_TH, B);
    if (wc)
        hipLaunchKernelGGL(k_segnet_conv<SG_DEC1>, grid, dim3(SG_THREADS), 0, s, x, idx, wt, bias, wc, bc, y, nullptr, H,
                           W, SgStd{});
    else
        hipLaunchKernelGGL(k_segnet_conv<SG_DEC>, grid, dim3(SG_THREADS), 0, s, x, idx, wt, bias, nullptr, nullptr, y,
                           nullptr, H, W, SgStd{});
    SPA_LAUNCH_CHECK();
    return SPA_OK;
}

extern "C" int spa_segnet_score(spa_ctx *ctx, const float *prob, int32_t B, int32_t h, int32_t w, int32_t H, int32_t W,
                                uint8_t *mask, float *scores, void *stream)
{
    SPA_ARG(ctx && prob && mask && B > 0 && B < 65536 && h > 0 && w > 0 && H > 0 && W > 0);
    SPA_ARG(H < 65536 && W < (1 << 24) && h < (1 << 24) && w < (1 << 24));
    if (H < h || W < w) {
        spa_set_error("spa_segnet_score: (%d, %d) -> (%d, %d) is a downscale; only upscales are supported", h, w, H, W);
        return SPA_ERR_ARG;
    }
    hipStream_t s = spa_stream(stream);
    hipLaunchKernelGGL(k_segnet_score, dim3((W + 255) / 256, H, B), dim3(256), 0, s, prob, h, w, H, W, mask, scores);
    SPA_LAUNCH_CHECK();
    return SPA_OK;
}
