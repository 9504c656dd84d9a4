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
// The forward and dgrad kernel is the inference kernel's tiling (one workgroup = 8 x 32 output pixels x 64 channels,
// wave w owns rows 2w, 2w + 1, a 16-row MFMA tile = four 2x2 blocks, so a lane's four accumulators are one 2x2 window)
// with the same three input forms: conv1's planar image standardised and LRN-normalised in the load, a channels-last
// 64-channel map, and the decoder's pooled map unpooled through its index map while staging.
//
// wgrad is split-K: K = B*H*W pixels in 2 x 32 tiles, chunk j of sgt_wgrad_chunks (at most 96) owns a contiguous run of tiles, one
// workgroup per (chunk, ky).  Each writes its chunk's partial dW to the context workspace; a second kernel sums the
// chunks in chunk order (in double).  The split depends on (B, H, W) only, so the bits do not depend on the device.
// No atomics anywhere.
#include "spa_common.h"

typedef float f32x4 __attribute__((ext_vector_type(4)));

#define SG_TH 8
#define SG_TW 32
#define SG_HH (SG_TH + 6)
#define SG_HW (SG_TW + 6)
#define SG_HPIX (SG_HH * SG_HW)
#define SG_THREADS 256

enum { SGT_CONV1 = 0, SGT_ENC = 1, SGT_DEC = 2 };
enum { SGT_FULL = 0, SGT_POOLED = 1 };

struct SgtStd {
    float mean[3], std[3];
};

// Chainer's local_response_normalization with three channels (see spa_segnet.hip)
__device__ __forceinline__ void sgt_lrn3(float &a, float &b, float &c)
{
    const float a2 = a * a, b2 = b * b, c2 = c * c;
    const float s0 = (a2 + b2) + c2;
    const float s1 = (b2 + a2) + c2;
    const float s2 = (c2 + b2) + a2;
    const float alpha = 1e-4f / 5.f;
    a = a * powf(1.f + alpha * s0, -0.75f);
    b = b * powf(1.f + alpha * s1, -0.75f);
    c = c * powf(1.f + alpha * s2, -0.75f);
}

// the standardised, LRN-normalised conv1 input at (gy, gx), channel 3 zero; zero outside the image
__device__ __forceinline__ f32x4 sgt_conv1_px(const float *xb, long long plane, int gy, int gx, int H, int W,
                                              const SgtStd &st)
{
    f32x4 v = {0.f, 0.f, 0.f, 0.f};
    if (gy >= 0 && gy < H && gx >= 0 && gx < W) {
        const long long o = (long long)gy * W + gx;
        float r = xb[o], g = xb[plane + o], bl = xb[2 * plane + o];
        r = (r - st.mean[0]) / st.std[0];
        g = (g - st.mean[1]) / st.std[1];
        bl = (bl - st.mean[2]) / st.std[2];
        sgt_lrn3(r, g, bl);
        v = (f32x4){r, g, bl, 0.f};
    }
    return v;
}

// four channels [c, c + 4) of the 64-channel input at full-resolution (gy, gx): ENC reads the map, DEC the pooled map
// at (gy/2, gx/2) where its index selects (gy & 1, gx & 1), zero elsewhere; zero outside the image
template <int MODE>
__device__ __forceinline__ f32x4 sgt_px4(const float *X, const uint8_t *I, int b, int gy, int gx, int c, int H, int W)
{
    f32x4 v = {0.f, 0.f, 0.f, 0.f};
    if (gy >= 0 && gy < H && gx >= 0 && gx < W) {
        if (MODE == SGT_ENC) {
            v = *(const f32x4 *)(X + (((long long)b * H + gy) * W + gx) * 64 + c);
        } else {
            const int Hh = H >> 1, Wh = W >> 1;
            const long long o = (((long long)b * Hh + (gy >> 1)) * Wh + (gx >> 1)) * 64 + c;
            const f32x4 h = *(const f32x4 *)(X + o);
            const unsigned ix = *(const unsigned *)(I + o);
            const unsigned sel = (unsigned)(((gy & 1) << 1) | (gx & 1));
            v.x = ((ix & 0xffu) == sel) ? h.x : 0.f;
            v.y = (((ix >> 8) & 0xffu) == sel) ? h.y : 0.f;
            v.z = (((ix >> 16) & 0xffu) == sel) ? h.z : 0.f;
            v.w = ((ix >> 24) == sel) ? h.w : 0.f;
        }
    }
    return v;
}

// Y = conv7x7(input form MODE of X (, I); Wt) at output resolution (H, W), Wt (49,64,CP) = (tap, n, c).
// EPI SGT_FULL: Y (B,H,W,64); with part != NULL also part[blk][0..63] = sum y, part[blk][64..127] = sum y^2 over the
// workgroup's in-image pixels (blk = (b * gridDim.y + tile row) * gridDim.x + tile column).
// EPI SGT_POOLED: Y (B,H/2,W/2,64) = the value at the position Io (B,H/2,W/2,64) selects in each 2x2 block.
template <int MODE, int EPI>
__global__ __launch_bounds__(SG_THREADS) void k_sgt_conv(const float *__restrict__ X, const uint8_t *__restrict__ I,
                                                         const float *__restrict__ Wt, const uint8_t *__restrict__ Io,
                                                         float *__restrict__ Y, float *__restrict__ part, int H, int W,
                                                         SgtStd st)
{
    constexpr int CP = MODE == SGT_CONV1 ? 4 : 64;
    constexpr int CH = MODE == SGT_CONV1 ? 4 : 16;
    constexpr int PS = MODE == SGT_CONV1 ? 4 : 20;
    constexpr int NLDS = SG_HPIX * PS > 2048 ? SG_HPIX * PS : 2048;
    __shared__ __attribute__((aligned(16))) float xs[NLDS];

    const int tid = threadIdx.x, lane = tid & 63;
    const int w = tid >> 6;
    const int b = blockIdx.z;
    const int ty0 = blockIdx.y * SG_TH, tx0 = blockIdx.x * SG_TW;

    const int fi = lane & 15, fq = lane >> 4;
    const int frow = 2 * w + ((fi & 3) >> 1), fcol = 2 * (fi >> 2) + (fi & 1);

    f32x4 acc[4][4];
#pragma unroll
    for (int m = 0; m < 4; ++m)
#pragma unroll
        for (int nt = 0; nt < 4; ++nt) acc[m][nt] = (f32x4){0.f, 0.f, 0.f, 0.f};

    for (int c0 = 0; c0 < CP; c0 += CH) {
        if (c0) __syncthreads();
        if (MODE == SGT_CONV1) {
            const long long plane = (long long)H * W;
            const float *xb = X + (long long)b * 3 * plane;
            for (int p = tid; p < SG_HPIX; p += SG_THREADS)
                *(f32x4 *)&xs[p * PS] = sgt_conv1_px(xb, plane, ty0 - 3 + p / SG_HW, tx0 - 3 + p % SG_HW, H, W, st);
        } else {
            for (int e = tid; e < SG_HPIX * 4; e += SG_THREADS) {
                const int p = e >> 2, q = e & 3;
                *(f32x4 *)&xs[p * PS + 4 * q] =
                    sgt_px4<MODE>(X, I, b, ty0 - 3 + p / SG_HW, tx0 - 3 + p % SG_HW, c0 + 4 * q, H, W);
            }
        }
        __syncthreads();

        const float *wl = Wt + (long long)fi * CP + c0 + (MODE == SGT_CONV1 ? fq : 4 * fq);
        for (int ky = 0; ky < 7; ++ky) {
            const float *xr = &xs[((frow + ky) * SG_HW + fcol) * PS + (MODE == SGT_CONV1 ? fq : 4 * fq)];
#pragma unroll
            for (int kx = 0; kx < 7; ++kx) {
                const float *wt = wl + (long long)(ky * 7 + kx) * 64 * CP;
                if (MODE == SGT_CONV1) {
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

    // epilogue: lane holds channel n = 16 nt + fi, register r = pixel (r >> 1, r & 1) of the 2x2 block at output
    // rows oy, oy + 1 and columns x, x + 1 with x = ox + 8 m.  H and W are even: a block is wholly in or out.
    const int oy = ty0 + 2 * w, ox = tx0 + 2 * fq;
    const bool row_in = oy < H;
    if (EPI == SGT_FULL) {
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
                    const float v = acc[m][nt][r];
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
                xs[((w * 4 + fq) * 64 + n) * 2] = s[nt];
                xs[((w * 4 + fq) * 64 + n) * 2 + 1] = q[nt];
            }
            __syncthreads();
            if (tid < 128) {
                const int n = tid & 63, k = tid >> 6;
                float t = 0.f;
                for (int j = 0; j < 16; ++j) t += xs[(j * 64 + n) * 2 + k];
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
                const f32x4 a = acc[m][nt];
                Y[o + n] = r == 0 ? a[0] : r == 1 ? a[1] : r == 2 ? a[2] : a[3];
            }
        }
    }
}

// stats[k * 64 + n] = sum over the nblk partials of part[blk][k * 64 + n], in block order, in double (k 0: sum y,
// 1: sum y^2).  One workgroup per (k, n); thread t takes blocks t, t + 256, ...; then a fixed tree.
__global__ __launch_bounds__(256) void k_sgt_bnstat(const float *__restrict__ part, long long nblk,
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

// Wr[t][c][n] = Wt[48 - t][n][c] (64 x 64 per tap)
__global__ __launch_bounds__(256) void k_sgt_wrot(const float *__restrict__ Wt, float *__restrict__ Wr)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= 49 * 64 * 64) return;
    const int t = i / 4096, c = (i >> 6) & 63, n = i & 63;
    Wr[i] = Wt[((48 - t) * 64 + n) * 64 + c];
}

// ---------------------------------------------------------------------------------------------------- wgrad
#define SGW_TR 2                     // tile rows
#define SGW_TW 32                    // tile columns
#define SGW_XW (SGW_TW + 6)          // staged input columns
#define SGW_GS 68                    // LDS floats per staged 64-channel pixel
#define SGW_MAXCH 96                 // chunks of K at most

static inline int sgt_wgrad_chunks(long long tiles) { return (int)(tiles < SGW_MAXCH ? tiles : SGW_MAXCH); }

// part[(chunk * 49 + ky * 7 + kx) * 64 * CP + n * CP + c] = the chunk's sum of G[p][n] * X[p + (ky - 3, kx - 3)][c].
// G (B,H,W,64) channels-last.  Grid (chunks, 7): blockIdx.y = ky.
// 64-channel forms: wave w owns channels c = 16 w .. 16 w + 15 of all seven taps of the row and all 64 n: MFMA A = G
// (rows n, K = 4 pixels), B = X shifted by the tap (columns c), 7 x 4 accumulator tiles.
// conv1 (CP 4): the 16 MFMA columns are (kx, c) = (4 ct + (j >> 2), j & 3) for column tiles ct 0, 1 (kx 7 is zero);
// the four waves take every fourth K step of a tile and their sums are added in wave order at the end.
template <int MODE>
__global__ __launch_bounds__(SG_THREADS) void k_sgt_wgrad(const float *__restrict__ G, const float *__restrict__ X,
                                                          const uint8_t *__restrict__ I, float *__restrict__ part,
                                                          int B, int H, int W, int nch, SgtStd st)
{
    constexpr int CP = MODE == SGT_CONV1 ? 4 : 64;
    constexpr int XS = MODE == SGT_CONV1 ? 4 : SGW_GS;      // LDS floats per staged input pixel
    constexpr int NG = SGW_TR * SGW_TW * SGW_GS;
    constexpr int NX = SGW_TR * SGW_XW * XS;
    constexpr int NLDS = MODE == SGT_CONV1 ? (NG + NX > 4 * 64 * 32 ? NG + NX : 4 * 64 * 32) : NG + NX;
    __shared__ __attribute__((aligned(16))) float lds[NLDS];
    float *gs = lds, *xs = lds + NG;

    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int fi = lane & 15, fq = lane >> 4;
    const int ky = blockIdx.y, chunk = blockIdx.x;
    const int txn = (W + SGW_TW - 1) / SGW_TW, tyn = H / SGW_TR;
    const long long tiles = (long long)B * tyn * txn;
    const long long t0 = tiles * chunk / nch, t1 = tiles * (chunk + 1) / nch;
    const long long plane = (long long)H * W;

    constexpr int NA = MODE == SGT_CONV1 ? 2 : 7;
    f32x4 acc[NA][4];
#pragma unroll
    for (int a = 0; a < NA; ++a)
#pragma unroll
        for (int nt = 0; nt < 4; ++nt) acc[a][nt] = (f32x4){0.f, 0.f, 0.f, 0.f};

    for (long long t = t0; t < t1; ++t) {
        const int tx = (int)(t % txn);
        const long long r2 = t / txn;
        const int ty = (int)(r2 % tyn), b = (int)(r2 / tyn);
        const int y0 = ty * SGW_TR, x0 = tx * SGW_TW;
        if (t != t0) __syncthreads();
        // stage G (zero past the right edge: those pixels contribute nothing) and the input rows y0 + ky - 3 + r
        for (int e = tid; e < SGW_TR * SGW_TW * 16; e += SG_THREADS) {
            const int p = e >> 4, q = e & 15;
            const int gy = y0 + p / SGW_TW, gx = x0 + p % SGW_TW;
            f32x4 v = {0.f, 0.f, 0.f, 0.f};
            if (gx < W) v = *(const f32x4 *)(G + (((long long)b * H + gy) * W + gx) * 64 + 4 * q);
            *(f32x4 *)&gs[p * SGW_GS + 4 * q] = v;
        }
        if (MODE == SGT_CONV1) {
            const float *xb = X + (long long)b * 3 * plane;
            for (int p = tid; p < SGW_TR * SGW_XW; p += SG_THREADS)
                *(f32x4 *)&xs[p * XS] =
                    sgt_conv1_px(xb, plane, y0 + ky - 3 + p / SGW_XW, x0 - 3 + p % SGW_XW, H, W, st);
        } else {
            for (int e = tid; e < SGW_TR * SGW_XW * 16; e += SG_THREADS) {
                const int p = e >> 4, q = e & 15;
                *(f32x4 *)&xs[p * XS + 4 * q] =
                    sgt_px4<MODE>(X, I, b, y0 + ky - 3 + p / SGW_XW, x0 - 3 + p % SGW_XW, 4 * q, H, W);
            }
        }
        __syncthreads();

        if (MODE == SGT_CONV1) {
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
    if (MODE == SGT_CONV1) {
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

// dw[i] = sum over chunks j = 0 .. nch - 1 of part[j * n + i], in chunk order, in double, rounded once
__global__ __launch_bounds__(256) void k_sgt_wsum(const float *__restrict__ part, int nch, int n, float *__restrict__ dw)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    double s = 0.0;
    for (int j = 0; j < nch; ++j) s += (double)part[(long long)j * n + i];
    dw[i] = (float)s;
}

// ---------------------------------------------------------------------------------------------------- C ABI
static bool sgt_al16(const void *p) { return ((uintptr_t)p & 15) == 0; }

// the shape checks shared by the three entry points: (H, W) the convolution's resolution.  conv1 sees the network
// input (four poolings: H, W % 16); the deeper layers run at 1/2 .. 1/8 of it (H, W even)
static int sgt_check_shape(int B, int H, int W, int Cin)
{
    SPA_ARG(B > 0 && B < 65536 && H > 0 && W > 0);
    SPA_ARG(Cin == 3 ? (H % 16 == 0 && W % 16 == 0) : (H % 2 == 0 && W % 2 == 0));
    SPA_ARG((long long)H * W * 64 < (1ll << 31) && H / SG_TH < 65536);
    return SPA_OK;
}

static int sgt_input_form(const char *fn, int32_t Cin, int32_t x_layout, const float *mean_host, const float *std_host,
                          const uint8_t *idx, SgtStd *st)
{
    SPA_ARG(Cin == 3 || Cin == 64);
    if (Cin == 3) {
        SPA_ARG(mean_host && std_host && !idx);
        if (x_layout != SPA_LAYOUT_NCHW) {
            spa_set_error("%s: the conv1 input is the planar (B,3,H,W) image", fn);
            return SPA_ERR_LAYOUT;
        }
        for (int c = 0; c < 3; ++c) { st->mean[c] = mean_host[c]; st->std[c] = std_host[c]; }
    } else {
        SPA_ARG(((uintptr_t)idx & 3) == 0);
        if (x_layout != SPA_LAYOUT_NHWC) {
            spa_set_error("%s: 64-channel inputs (and index maps) must be channels-last", fn);
            return SPA_ERR_LAYOUT;
        }
    }
    return SPA_OK;
}

extern "C" int spa_segnet_train_forward(spa_ctx *ctx, const float *x, const uint8_t *idx, int32_t x_layout, int32_t B,
                                        int32_t H, int32_t W, int32_t Cin, const float *wt, const float *mean_host,
                                        const float *std_host, float *y, double *stats, void *stream)
{
    SPA_ARG(ctx && x && wt && y);
    int rc = sgt_check_shape(B, H, W, Cin);
    if (rc != SPA_OK) return rc;
    SPA_ARG(sgt_al16(x) && sgt_al16(wt));
    SgtStd st = {};
    rc = sgt_input_form("spa_segnet_train_forward", Cin, x_layout, mean_host, std_host, idx, &st);
    if (rc != SPA_OK) return rc;
    hipStream_t s = spa_stream(stream);
    dim3 grid((W + SG_TW - 1) / SG_TW, (H + SG_TH - 1) / SG_TH, B);
    const long long nblk = (long long)grid.x * grid.y * grid.z;
    float *part = nullptr;
    if (stats) {
        if ((rc = spa_ws_reserve(ctx, WS_SEGNET_BNPART, (size_t)nblk * 128 * sizeof(float), (void **)&part)) != SPA_OK)
            return rc;
    }
    if (Cin == 3)
        hipLaunchKernelGGL((k_sgt_conv<SGT_CONV1, SGT_FULL>), grid, dim3(SG_THREADS), 0, s, x, nullptr, wt, nullptr, y,
                           part, H, W, st);
    else if (!idx)
        hipLaunchKernelGGL((k_sgt_conv<SGT_ENC, SGT_FULL>), grid, dim3(SG_THREADS), 0, s, x, nullptr, wt, nullptr, y,
                           part, H, W, st);
    else
        hipLaunchKernelGGL((k_sgt_conv<SGT_DEC, SGT_FULL>), grid, dim3(SG_THREADS), 0, s, x, idx, wt, nullptr, y, part,
                           H, W, st);
    SPA_LAUNCH_CHECK();
    if (stats) {
        hipLaunchKernelGGL(k_sgt_bnstat, dim3(128), dim3(256), 0, s, part, nblk, stats);
        SPA_LAUNCH_CHECK();
    }
    return SPA_OK;
}

extern "C" int spa_segnet_train_dgrad(spa_ctx *ctx, const float *dy, const float *wt, const uint8_t *idx, int32_t B,
                                      int32_t H, int32_t W, float *dx, void *stream)
{
    SPA_ARG(ctx && dy && wt && dx);
    int rc = sgt_check_shape(B, H, W, 64);
    if (rc != SPA_OK) return rc;
    SPA_ARG(sgt_al16(dy) && sgt_al16(wt) && ((uintptr_t)idx & 3) == 0);
    float *wr = nullptr;
    if ((rc = spa_ws_reserve(ctx, WS_SEGNET_WROT, 49 * 64 * 64 * sizeof(float), (void **)&wr)) != SPA_OK) return rc;
    hipStream_t s = spa_stream(stream);
    hipLaunchKernelGGL(k_sgt_wrot, dim3(49 * 64 * 64 / 256), dim3(256), 0, s, wt, wr);
    SPA_LAUNCH_CHECK();
    dim3 grid((W + SG_TW - 1) / SG_TW, (H + SG_TH - 1) / SG_TH, B);
    if (idx)
        hipLaunchKernelGGL((k_sgt_conv<SGT_ENC, SGT_POOLED>), grid, dim3(SG_THREADS), 0, s, dy, nullptr, wr, idx, dx,
                           nullptr, H, W, SgtStd{});
    else
        hipLaunchKernelGGL((k_sgt_conv<SGT_ENC, SGT_FULL>), grid, dim3(SG_THREADS), 0, s, dy, nullptr, wr, nullptr, dx,
                           nullptr, H, W, SgtStd{});
    SPA_LAUNCH_CHECK();
    return SPA_OK;
}

extern "C" int spa_segnet_train_wgrad(spa_ctx *ctx, const float *dy, const float *x, const uint8_t *idx,
                                      int32_t x_layout, int32_t B, int32_t H, int32_t W, int32_t Cin,
                                      const float *mean_host, const float *std_host, float *dw, void *stream)
{
    SPA_ARG(ctx && dy && x && dw);
    int rc = sgt_check_shape(B, H, W, Cin);
    if (rc != SPA_OK) return rc;
    SPA_ARG(sgt_al16(dy) && sgt_al16(x));
    SgtStd st = {};
    rc = sgt_input_form("spa_segnet_train_wgrad", Cin, x_layout, mean_host, std_host, idx, &st);
    if (rc != SPA_OK) return rc;
    const int CP = Cin == 3 ? 4 : 64;
    const long long tiles = (long long)B * (H / SGW_TR) * ((W + SGW_TW - 1) / SGW_TW);
    const int nch = sgt_wgrad_chunks(tiles);
    const int n = 49 * 64 * CP;
    float *part = nullptr;
    if ((rc = spa_ws_reserve(ctx, WS_SEGNET_WGRAD, (size_t)nch * n * sizeof(float), (void **)&part)) != SPA_OK)
        return rc;
    hipStream_t s = spa_stream(stream);
    dim3 grid(nch, 7);
    if (Cin == 3)
        hipLaunchKernelGGL(k_sgt_wgrad<SGT_CONV1>, grid, dim3(SG_THREADS), 0, s, dy, x, nullptr, part, B, H, W, nch, st);
    else if (!idx)
        hipLaunchKernelGGL(k_sgt_wgrad<SGT_ENC>, grid, dim3(SG_THREADS), 0, s, dy, x, nullptr, part, B, H, W, nch, st);
    else
        hipLaunchKernelGGL(k_sgt_wgrad<SGT_DEC>, grid, dim3(SG_THREADS), 0, s, dy, x, idx, part, B, H, W, nch, st);
    SPA_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_sgt_wsum, dim3((n + 255) / 256), dim3(256), 0, s, part, nch, n, dw);
    SPA_LAUNCH_CHECK();
    return SPA_OK;
}
