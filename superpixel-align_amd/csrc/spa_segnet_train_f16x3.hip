// SegNet-Basic training at float32 accuracy on the f16 matrix cores (train_segnet.py --split_planes): the eight pass
// forms of spa_segnet_train.hip -- forward (conv1's image, a 64-channel map, the decoder's unpooled map), dgrad (plain
// and the decoder's pooled-gradient gather) and wgrad (conv1, encoder, decoder) -- with every float32 operand carried
// as two half-precision planes and three products per float32 product.
//
// Operand split.  Each operand tensor gets one power-of-two scale t = 2^k that brings its largest magnitude into
// [2^14, 2^15) (k = 0 for an all-zero tensor); a value v becomes h = f16_rn(t v), l = f16_rn(t v - h), 22 significand
// bits between them.  A product a b is h_a h_b + h_a l_b + l_a h_b: three v_mfma_f32_16x16x32_f16 accumulating in
// float32, the two small cross terms issued first (l_a l_b, 2^-22 of the product, is dropped).  Forward and dgrad keep
// the cross terms in accumulators of their own, added to the h_a h_b accumulators in the epilogue (sgh_mma3).  The epilogue multiplies by 2^-(k_a + k_b) (v_ldexp, exact)
// before y, the BN partial sums, the dgrad gather or a wgrad chunk partial is formed.  The scales are computed on the
// device inside each call: per-workgroup maxima of |v| (bit patterns: non-negative floats order as unsigned integers),
// then one workgroup per tensor reduces them -- a max is exact in any order and no atomics are used.  Inputs are the
// float32 values of the float32 kernels: the standardised, LRN-normalised conv1 input (computed in float32 exactly as
// sgt_conv1_px computes it), the map or the unpooled value (the scale of a decoder's input is that of its pooled map),
// dy, and the weights (split once per call into a packed f16 plane pair in the context workspace).
//
// Tiling, K steps, conv1's tap packing, the transposed wgrad staging and every reduction are those of
// spa_segnet_train_bf16.hip: one forward / dgrad workgroup = 8 x 32 output pixels x 64 channels, the BN partial sums
// float32 per workgroup and float64 across them in block order, split-K wgrad with the chunks summed in float64 in chunk
// order.  The forward halo holds a pixel's 32-channel chunk as [32 h | 32 l] (144 bytes with padding: 74.8 KiB, two
// workgroups per CU, conflict-free ds_read_b128); wgrad stages h and l as two images of the bf16 layout.  The work
// split depends on the shape only, so the bits do not depend on the run or the device.
#include "spa_common.h"

typedef float sgh_f32x4 __attribute__((ext_vector_type(4)));
typedef _Float16 sgh_f16x8 __attribute__((ext_vector_type(8)));
typedef short sgh_s16x4 __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(3))) sgh_s16x4 sgh_lds_s16x4;

#define SGH_TH 8
#define SGH_TW 32
#define SGH_HH (SGH_TH + 6)
#define SGH_HW (SGH_TW + 6)
#define SGH_HPIX (SGH_HH * SGH_HW)
#define SGH_THREADS 256
#define SGH_PS 72                    // LDS f16 per staged pixel of a 32-channel chunk: 32 h, 32 l, 16 bytes of padding
#define SGH_NAMAX 256                // workgroups of a max reduction
#define SGH_W64 (49 * 64 * 64)       // f16 per plane of a 64-channel layer's weights
#define SGH_W1 (7 * 64 * 32)         // f16 per plane of conv1's weights

enum { SGH_CONV1 = 0, SGH_ENC = 1, SGH_DEC = 2 };
enum { SGH_FULL = 0, SGH_POOLED = 1 };

struct SghStd {
    float mean[3], std[3];
};

// 2^k as a float (k in [-113, 126], as sgh_scale produces)
__device__ __forceinline__ float sgh_pow2(int k) { return __uint_as_float((unsigned)(127 + k) << 23); }

// h = f16_rn(v sc), l = f16_rn(v sc - h) as bit patterns (sc a power of two: v sc and the difference are exact)
__device__ __forceinline__ void sgh_split(float v, float sc, unsigned short &h, unsigned short &l)
{
    const float s = v * sc;
    const _Float16 hh = (_Float16)s;
    const _Float16 ll = (_Float16)(s - (float)hh);
    h = __builtin_bit_cast(unsigned short, hh);
    l = __builtin_bit_cast(unsigned short, ll);
}

// eight float32 values -> their h plane (returned) and l plane (through l), packed in channel order
__device__ __forceinline__ uint4 sgh_split8(sgh_f32x4 lo, sgh_f32x4 hi, float sc, uint4 &l)
{
    uint4 h;
    h.x = spa_split16_pair(lo.x, lo.y, sc, l.x);
    h.y = spa_split16_pair(lo.z, lo.w, sc, l.y);
    h.z = spa_split16_pair(hi.x, hi.y, sc, l.z);
    h.w = spa_split16_pair(hi.z, hi.w, sc, l.w);
    return h;
}

// Chainer's local_response_normalization with three channels: the float32 operations of sgt_lrn3
__device__ __forceinline__ void sgh_lrn3(float &a, float &b, float &c)
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

// the standardised, LRN-normalised conv1 input at (gy, gx) as sgt_conv1_px computes it; zero outside the image
__device__ __forceinline__ sgh_f32x4 sgh_conv1_val(const float *xb, long long plane, int gy, int gx, int H, int W,
                                                   const SghStd &st)
{
    float r = 0.f, g = 0.f, bl = 0.f;
    if (gy >= 0 && gy < H && gx >= 0 && gx < W) {
        const long long o = (long long)gy * W + gx;
        r = xb[o];
        g = xb[plane + o];
        bl = xb[2 * plane + o];
        r = (r - st.mean[0]) / st.std[0];
        g = (g - st.mean[1]) / st.std[1];
        bl = (bl - st.mean[2]) / st.std[2];
        sgh_lrn3(r, g, bl);
    }
    return (sgh_f32x4){r, g, bl, 0.f};
}

// that value split: the h plane's 4 values (channel 3 zero) returned, the l plane's through l
__device__ __forceinline__ uint2 sgh_conv1_px(const float *xb, long long plane, int gy, int gx, int H, int W,
                                              const SghStd &st, float sc, uint2 &l)
{
    const sgh_f32x4 v = sgh_conv1_val(xb, plane, gy, gx, H, W, st);
    uint2 h;
    h.x = spa_split16_pair(v.x, v.y, sc, l.x);
    h.y = spa_split16_pair(v.z, 0.f, sc, l.y);
    return h;
}

// channels [c, c + 8) of the 64-channel input at full-resolution (gy, gx), split: ENC reads the map, DEC the pooled
// map at (gy/2, gx/2) where its index selects (gy & 1, gx & 1), zero elsewhere; zero outside the image
template <int MODE>
__device__ __forceinline__ uint4 sgh_px8(const float *X, const uint8_t *I, int b, int gy, int gx, int c, int H, int W,
                                         float sc, uint4 &l)
{
    uint4 h = make_uint4(0u, 0u, 0u, 0u);
    l = h;
    if (gy >= 0 && gy < H && gx >= 0 && gx < W) {
        if (MODE == SGH_ENC) {
            const float *p = X + (((long long)b * H + gy) * W + gx) * 64 + c;
            h = sgh_split8(*(const sgh_f32x4 *)p, *(const sgh_f32x4 *)(p + 4), sc, l);
        } else {
            const int Hh = H >> 1, Wh = W >> 1;
            const long long o = (((long long)b * Hh + (gy >> 1)) * Wh + (gx >> 1)) * 64 + c;
            sgh_f32x4 lo = *(const sgh_f32x4 *)(X + o), hi = *(const sgh_f32x4 *)(X + o + 4);
            const unsigned i0 = *(const unsigned *)(I + o), i1 = *(const unsigned *)(I + o + 4);
            const unsigned sel = (unsigned)(((gy & 1) << 1) | (gx & 1));
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                if (((i0 >> (8 * j)) & 0xffu) != sel) lo[j] = 0.f;
                if (((i1 >> (8 * j)) & 0xffu) != sel) hi[j] = 0.f;
            }
            h = sgh_split8(lo, hi, sc, l);
        }
    }
    return h;
}

__device__ __forceinline__ sgh_f16x8 sgh_frag(uint4 v) { return __builtin_bit_cast(sgh_f16x8, v); }

// one K step's products a b = h_a h_b + h_a l_b + l_a h_b, small terms first: the two cross terms (2^-11 of h_a h_b)
// into their own accumulator x, h_a h_b into acc; the epilogue adds the two.  Chained into one accumulator instead,
// each pass still met the float32 bounds element by element, but its errors summed over a layer's pixels did not
// cancel as the float32 passes' do: in a whole step, updates that are cancellation residuals (conv1_bn/beta) missed
// float64 by 9.7e-3 against 4.3e-6 in float32.  With the separate accumulators they land at 4.2e-6.
__device__ __forceinline__ void sgh_mma3(sgh_f32x4 &acc, sgh_f32x4 &x, sgh_f16x8 ah, sgh_f16x8 al, sgh_f16x8 bh,
                                         sgh_f16x8 bl)
{
    x = __builtin_amdgcn_mfma_f32_16x16x32_f16(ah, bl, x, 0, 0, 0);
    x = __builtin_amdgcn_mfma_f32_16x16x32_f16(al, bh, x, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(ah, bh, acc, 0, 0, 0);
}

// ---------------------------------------------------------------------------------------------------- scales
__device__ __forceinline__ unsigned sgh_absbits(float v) { return __float_as_uint(v) & 0x7fffffffu; }

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
        const sgh_f32x4 v = ((const sgh_f32x4 *)a)[i];
        m = max(max(m, max(sgh_absbits(v.x), sgh_absbits(v.y))), max(sgh_absbits(v.z), sgh_absbits(v.w)));
    }
    sgh_max_store(m, red, part);
}

// the same for conv1's operand: the standardised, LRN-normalised image (B,3,H,W), as the kernels stage it
__global__ __launch_bounds__(256) void k_sgh_amax_conv1(const float *__restrict__ x, int B, int H, int W, SghStd st,
                                                        unsigned *__restrict__ part)
{
    __shared__ unsigned red[256];
    const long long plane = (long long)H * W, n = (long long)B * plane;
    unsigned m = 0u;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) {
        const long long b = i / plane, o = i - b * plane;
        const sgh_f32x4 v = sgh_conv1_val(x + b * 3 * plane, plane, (int)(o / W), (int)(o % W), H, W, st);
        m = max(m, max(max(sgh_absbits(v.x), sgh_absbits(v.y)), sgh_absbits(v.z)));
    }
    sgh_max_store(m, red, part);
}

// ex[j] = k with 2^k max|v| in [2^14, 2^15) for tensor j = blockIdx.x (maxima part[j * SGH_NAMAX ..]); k = 0 for an
// all-zero tensor.  The exponent is clamped to [-112, 127] so that 2^k is a normal float: a maximum below 2^-112
// (subnormal inputs) lands lower, a NaN or infinite one at 2^-113.
__global__ __launch_bounds__(256) void k_sgh_scale(const unsigned *__restrict__ part, int *__restrict__ ex)
{
    __shared__ unsigned red[256];
    const int t = threadIdx.x;
    unsigned m = 0u;
    for (int i = t; i < SGH_NAMAX; i += 256) m = max(m, part[blockIdx.x * SGH_NAMAX + i]);
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

// ---------------------------------------------------------------------------------------------------- forward, dgrad
// Y = conv7x7(input form MODE of X (, I); Wp) at output resolution (H, W).  Wp: the h plane, then the l plane, each
// (49,64,64) = (tap, n, c) for the 64-channel forms or (7,64,32) = (K step, n, k) for conv1 (k = 4 (tap - 8 step) + c,
// zero past tap 48).  ex[0] = the input's scale exponent, ex[1] = the weights'.
// EPI SGH_FULL: Y (B,H,W,64); with part != NULL also part[blk][0..63] = sum y, part[blk][64..127] = sum y^2 over the
// workgroup's in-image pixels (blk = (b * gridDim.y + tile row) * gridDim.x + tile column).
// EPI SGH_POOLED: Y (B,H/2,W/2,64) = the value at the position Io (B,H/2,W/2,64) selects in each 2x2 block.
template <int MODE, int EPI>
__global__ __launch_bounds__(SGH_THREADS, 2) void k_sgh_conv(const float *__restrict__ X, const uint8_t *__restrict__ I,
                                                          const unsigned short *__restrict__ Wp,
                                                          const uint8_t *__restrict__ Io, float *__restrict__ Y,
                                                          float *__restrict__ part, const int *__restrict__ ex, int H,
                                                          int W, SghStd st)
{
    constexpr int PS = MODE == SGH_CONV1 ? 8 : SGH_PS;                   // conv1: [4 h | 4 l] per pixel
    constexpr int NCH = MODE == SGH_CONV1 ? 1 : 2;                       // 32-channel chunks
    constexpr int NB = SGH_HPIX * PS * 2 > 8192 ? SGH_HPIX * PS * 2 : 8192;  // the halo, or the BN reduction
    constexpr int WPL = MODE == SGH_CONV1 ? SGH_W1 : SGH_W64;            // f16 per weight plane
    __shared__ __attribute__((aligned(16))) unsigned short xs[NB / 2];
    float *red = (float *)xs;

    const int tid = threadIdx.x, lane = tid & 63;
    const int w = tid >> 6;
    const int b = blockIdx.z;
    const int ty0 = blockIdx.y * SGH_TH, tx0 = blockIdx.x * SGH_TW;
    const int kin = ex[0], kw = ex[1];
    const float sc = sgh_pow2(kin);

    const int fi = lane & 15, fq = lane >> 4;
    const int frow = 2 * w + ((fi & 3) >> 1), fcol = 2 * (fi >> 2) + (fi & 1);

    sgh_f32x4 acc[4][4], accx[4][4];
#pragma unroll
    for (int m = 0; m < 4; ++m)
#pragma unroll
        for (int nt = 0; nt < 4; ++nt) acc[m][nt] = accx[m][nt] = (sgh_f32x4){0.f, 0.f, 0.f, 0.f};

    for (int ch = 0; ch < NCH; ++ch) {
        if (ch) __syncthreads();
        if (MODE == SGH_CONV1) {
            const long long plane = (long long)H * W;
            const float *xb = X + (long long)b * 3 * plane;
            for (int p = tid; p < SGH_HPIX; p += SGH_THREADS) {
                uint2 l;
                const uint2 h = sgh_conv1_px(xb, plane, ty0 - 3 + p / SGH_HW, tx0 - 3 + p % SGH_HW, H, W, st, sc, l);
                *(uint4 *)&xs[p * PS] = make_uint4(h.x, h.y, l.x, l.y);
            }
        } else {
            for (int e = tid; e < SGH_HPIX * 4; e += SGH_THREADS) {
                const int p = e >> 2, q = e & 3;
                uint4 l;
                const uint4 h =
                    sgh_px8<MODE>(X, I, b, ty0 - 3 + p / SGH_HW, tx0 - 3 + p % SGH_HW, 32 * ch + 8 * q, H, W, sc, l);
                *(uint4 *)&xs[p * PS + 8 * q] = h;
                *(uint4 *)&xs[p * PS + 32 + 8 * q] = l;
            }
        }
        __syncthreads();

        if (MODE == SGH_CONV1) {
            // lane quarter fq holds taps t0 = 8 s + 2 fq and t0 + 1 of K step s, 4 channels each
            const unsigned short *xr = &xs[(frow * SGH_HW + fcol) * PS];
#pragma unroll
            for (int s = 0; s < 7; ++s) {
                const int t0 = 8 * s + 2 * fq, t1 = t0 + 1;
                const int o0 = ((t0 / 7) * SGH_HW + t0 % 7) * PS, o1 = ((t1 / 7) * SGH_HW + t1 % 7) * PS;
                sgh_f16x8 bh[4], bl[4], ah[4], al[4];
#pragma unroll
                for (int nt = 0; nt < 4; ++nt) {
                    const unsigned short *wq = Wp + ((long long)s * 64 + 16 * nt + fi) * 32 + 8 * fq;
                    bh[nt] = *(const sgh_f16x8 *)wq;
                    bl[nt] = *(const sgh_f16x8 *)(wq + WPL);
                }
#pragma unroll
                for (int m = 0; m < 4; ++m) {
                    const uint4 lo = t0 < 49 ? *(const uint4 *)&xr[o0 + 8 * m * PS] : make_uint4(0u, 0u, 0u, 0u);
                    const uint4 hi = t1 < 49 ? *(const uint4 *)&xr[o1 + 8 * m * PS] : make_uint4(0u, 0u, 0u, 0u);
                    ah[m] = sgh_frag(make_uint4(lo.x, lo.y, hi.x, hi.y));
                    al[m] = sgh_frag(make_uint4(lo.z, lo.w, hi.z, hi.w));
                }
#pragma unroll
                for (int m = 0; m < 4; ++m)
#pragma unroll
                    for (int nt = 0; nt < 4; ++nt) {
                        sgh_mma3(acc[m][nt], accx[m][nt], ah[m], al[m], bh[nt], bl[nt]);
                    }
            }
        } else {
            const unsigned short *wl = Wp + (long long)fi * 64 + 32 * ch + 8 * fq;
            for (int ky = 0; ky < 7; ++ky) {
                const unsigned short *xr = &xs[((frow + ky) * SGH_HW + fcol) * PS + 8 * fq];
#pragma unroll
                for (int kx = 0; kx < 7; ++kx) {
                    const unsigned short *wt = wl + (long long)(ky * 7 + kx) * 64 * 64;
                    sgh_f16x8 bh[4], bl[4], ah[4], al[4];
#pragma unroll
                    for (int nt = 0; nt < 4; ++nt) {
                        bh[nt] = *(const sgh_f16x8 *)(wt + nt * 16 * 64);
                        bl[nt] = *(const sgh_f16x8 *)(wt + WPL + nt * 16 * 64);
                    }
#pragma unroll
                    for (int m = 0; m < 4; ++m) {
                        ah[m] = *(const sgh_f16x8 *)&xr[(kx + 8 * m) * PS];
                        al[m] = *(const sgh_f16x8 *)&xr[(kx + 8 * m) * PS + 32];
                    }
#pragma unroll
                    for (int m = 0; m < 4; ++m)
#pragma unroll
                        for (int nt = 0; nt < 4; ++nt) {
                            sgh_mma3(acc[m][nt], accx[m][nt], ah[m], al[m], bh[nt], bl[nt]);
                        }
                }
            }
        }
    }

    // epilogue (the float32 kernel's, on the unscaled sums): lane holds channel n = 16 nt + fi, register r = pixel
    // (r >> 1, r & 1) of the 2x2 block at output rows oy, oy + 1 and columns x, x + 1 with x = ox + 8 m.  H, W even.
    const int unscale = -(kin + kw);
#pragma unroll
    for (int m = 0; m < 4; ++m)
#pragma unroll
        for (int nt = 0; nt < 4; ++nt)
#pragma unroll
            for (int r = 0; r < 4; ++r) acc[m][nt][r] = acc[m][nt][r] + accx[m][nt][r];
    const int oy = ty0 + 2 * w, ox = tx0 + 2 * fq;
    const bool row_in = oy < H;
    if (EPI == SGH_FULL) {
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
                const sgh_f32x4 a = acc[m][nt];
                Y[o + n] = ldexpf(r == 0 ? a[0] : r == 1 ? a[1] : r == 2 ? a[2] : a[3], unscale);
            }
        }
    }
}

// stats[k * 64 + n] = sum over the nblk partials of part[blk][k * 64 + n], in block order, in double: the reduction
// of k_sgt_bnstat (one workgroup per (k, n); thread t takes blocks t, t + 256, ...; then a fixed tree)
__global__ __launch_bounds__(256) void k_sgh_bnstat(const float *__restrict__ part, long long nblk,
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

// the split planes of a 64-channel layer's weights with scale 2^ex[1]: Wp[0][t][o][i] = h, Wp[1][t][o][i] = l of
// Wt[t][o][i], or with rot (dgrad) of Wt[48 - t][i][o]
__global__ __launch_bounds__(256) void k_sgh_wpack64(const float *__restrict__ Wt, int rot, const int *__restrict__ ex,
                                                     unsigned short *__restrict__ Wp)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= SGH_W64) return;
    const int t = i / 4096, o = (i >> 6) & 63, c = i & 63;
    sgh_split(rot ? Wt[((48 - t) * 64 + c) * 64 + o] : Wt[i], sgh_pow2(ex[1]), Wp[i], Wp[SGH_W64 + i]);
}

// conv1's split weights in K steps of 8 taps: plane j, Wp[j][s][n][k] of Wt[8 s + k / 4][n][k % 4], zero past tap 48
__global__ __launch_bounds__(256) void k_sgh_wpack1(const float *__restrict__ Wt, const int *__restrict__ ex,
                                                    unsigned short *__restrict__ Wp)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= SGH_W1) return;
    const int s = i >> 11, n = (i >> 5) & 63, k = i & 31, t = 8 * s + (k >> 2);
    sgh_split(t < 49 ? Wt[(t * 64 + n) * 4 + (k & 3)] : 0.f, sgh_pow2(ex[1]), Wp[i], Wp[SGH_W1 + i]);
}

// ---------------------------------------------------------------------------------------------------- wgrad
#define SGHW_TR 2                    // tile rows: one K step each
#define SGHW_TW 32                   // tile columns = the K step's 32 pixels
#define SGHW_GS 72                   // LDS f16 per staged 64-channel pixel of one plane (128 bytes + 16 of padding)
#define SGHW_MAXCH 96                // chunks of K at most

static inline int sgh_wgrad_chunks(long long tiles) { return (int)(tiles < SGHW_MAXCH ? tiles : SGHW_MAXCH); }

// one K step's f16 operand fragment from two transposed LDS reads: p0 the lane's address for pixels k .. k + 3, p1
// for k + 4 .. k + 7 (ds_read_b64_tr_b16: lane 4q + p of each 16-lane group names row q, columns 4p .. 4p + 3 of a
// 4 x 16 block; lane i receives column i of the 4 rows).  Every lane of the wave must take part.
__device__ __forceinline__ sgh_f16x8 sgh_tr8(const unsigned short *p0, const unsigned short *p1)
{
    const sgh_s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((sgh_lds_s16x4 *)p0);
    const sgh_s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((sgh_lds_s16x4 *)p1);
    return __builtin_bit_cast(sgh_f16x8, __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7));
}

// part[(chunk * 49 + ky * 7 + kx) * 64 * CP + n * CP + c] = the chunk's sum of G[p][n] * X[p + (ky - 3, kx - 3)][c].
// G (B,H,W,64) channels-last; ex[0] the input form's scale exponent, ex[1] G's.  Grid (chunks, 7): blockIdx.y = ky.
// K step s of a tile = its row s, k = column.  MFMA A = G (rows n, lane 16-group fq holds pixels 8 fq .. 8 fq + 7),
// B = X shifted by the tap (columns c); each operand staged as an h and an l image.
// 64-channel forms: wave w owns channels c = 16 w .. 16 w + 15 of all seven taps of the row and all 64 n.
// conv1 (CP 4): the 16 MFMA columns are (kx, c) = (4 ct + (j >> 2), j & 3) for column tiles ct 0, 1 (kx 7 is
// discarded); wave w owns column tile w >> 1 and the row tiles nt = 2 (w & 1), 2 (w & 1) + 1.
template <int MODE>
__global__ __launch_bounds__(SGH_THREADS) void k_sgh_wgrad(const float *__restrict__ G, const float *__restrict__ X,
                                                           const uint8_t *__restrict__ I, float *__restrict__ part,
                                                           const int *__restrict__ ex, int B, int H, int W, int nch,
                                                           SghStd st)
{
    constexpr int CP = MODE == SGH_CONV1 ? 4 : 64;
    constexpr int XW = MODE == SGH_CONV1 ? SGHW_TW + 8 : SGHW_TW + 6;     // staged input columns (conv1: kx 7 too)
    constexpr int XS = MODE == SGH_CONV1 ? 4 : SGHW_GS;                    // LDS f16 per staged input pixel and plane
    constexpr int GPL = SGHW_TR * SGHW_TW * SGHW_GS, XPL = SGHW_TR * XW * XS;  // f16 per plane
    __shared__ __attribute__((aligned(16))) unsigned short gs[2 * GPL];
    __shared__ __attribute__((aligned(16))) unsigned short xs[2 * XPL];

    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int fi = lane & 15, fq = lane >> 4;
    const int ky = blockIdx.y, chunk = blockIdx.x;
    const int txn = (W + SGHW_TW - 1) / SGHW_TW, tyn = H / SGHW_TR;
    const long long tiles = (long long)B * tyn * txn;
    const long long t0 = tiles * chunk / nch, t1 = tiles * (chunk + 1) / nch;
    const long long plane = (long long)H * W;
    const int kin = ex[0], kg = ex[1];
    const float scx = sgh_pow2(kin), scg = sgh_pow2(kg);

    constexpr int NA = MODE == SGH_CONV1 ? 1 : 7;
    constexpr int NT = MODE == SGH_CONV1 ? 2 : 4;
    const int nt0 = MODE == SGH_CONV1 ? 2 * (w & 1) : 0;
    sgh_f32x4 acc[NA][NT];
#pragma unroll
    for (int a = 0; a < NA; ++a)
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) acc[a][nt] = (sgh_f32x4){0.f, 0.f, 0.f, 0.f};

    // the lane's transposed-read addresses in the h images (pixel row (fi >> 2) of the 4-pixel block, column group
    // fi & 3); the l images are GPL / XPL further
    const int kp = 8 * fq + (fi >> 2);
    const unsigned short *ga = &gs[kp * SGHW_GS + 4 * (fi & 3)];
    const unsigned short *xa = MODE == SGH_CONV1 ? &xs[(kp + 4 * (w >> 1) + (fi & 3)) * XS]
                                                 : &xs[kp * XS + 16 * w + 4 * (fi & 3)];

    for (long long t = t0; t < t1; ++t) {
        const int tx = (int)(t % txn);
        const long long r2 = t / txn;
        const int ty = (int)(r2 % tyn), b = (int)(r2 / tyn);
        const int y0 = ty * SGHW_TR, x0 = tx * SGHW_TW;
        if (t != t0) __syncthreads();
        // stage G (zero past the right edge: those pixels contribute nothing) and the input rows y0 + ky - 3 + r
        for (int e = tid; e < SGHW_TR * SGHW_TW * 8; e += SGH_THREADS) {
            const int p = e >> 3, q = e & 7;
            const int gy = y0 + p / SGHW_TW, gx = x0 + p % SGHW_TW;
            uint4 h = make_uint4(0u, 0u, 0u, 0u), l = h;
            if (gx < W) {
                const float *g = G + (((long long)b * H + gy) * W + gx) * 64 + 8 * q;
                h = sgh_split8(*(const sgh_f32x4 *)g, *(const sgh_f32x4 *)(g + 4), scg, l);
            }
            *(uint4 *)&gs[p * SGHW_GS + 8 * q] = h;
            *(uint4 *)&gs[GPL + p * SGHW_GS + 8 * q] = l;
        }
        if (MODE == SGH_CONV1) {
            const float *xb = X + (long long)b * 3 * plane;
            for (int p = tid; p < SGHW_TR * XW; p += SGH_THREADS) {
                uint2 l;
                *(uint2 *)&xs[p * XS] = sgh_conv1_px(xb, plane, y0 + ky - 3 + p / XW, x0 - 3 + p % XW, H, W, st, scx, l);
                *(uint2 *)&xs[XPL + p * XS] = l;
            }
        } else {
            for (int e = tid; e < SGHW_TR * XW * 8; e += SGH_THREADS) {
                const int p = e >> 3, q = e & 7;
                uint4 l;
                *(uint4 *)&xs[p * XS + 8 * q] =
                    sgh_px8<MODE>(X, I, b, y0 + ky - 3 + p / XW, x0 - 3 + p % XW, 8 * q, H, W, scx, l);
                *(uint4 *)&xs[XPL + p * XS + 8 * q] = l;
            }
        }
        __syncthreads();

#pragma unroll
        for (int s = 0; s < SGHW_TR; ++s) {
            sgh_f16x8 ah[NT], al[NT];
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) {
                const unsigned short *p0 = ga + s * SGHW_TW * SGHW_GS + 16 * (nt0 + nt);
                ah[nt] = sgh_tr8(p0, p0 + 4 * SGHW_GS);
                al[nt] = sgh_tr8(p0 + GPL, p0 + GPL + 4 * SGHW_GS);
            }
            constexpr int NK = MODE == SGH_CONV1 ? 1 : 7;          // conv1: one column fragment covers the taps
#pragma unroll
            for (int kx = 0; kx < NK; ++kx) {
                const unsigned short *p0 = xa + (s * XW + kx) * XS;
                const sgh_f16x8 bh = sgh_tr8(p0, p0 + 4 * XS);
                const sgh_f16x8 bl = sgh_tr8(p0 + XPL, p0 + XPL + 4 * XS);
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
    if (MODE == SGH_CONV1) {
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

// dw[i] = sum over chunks j = 0 .. nch - 1 of part[j * n + i], in chunk order, in double, rounded once (k_sgt_wsum)
__global__ __launch_bounds__(256) void k_sgh_wsum(const float *__restrict__ part, int nch, int n, float *__restrict__ dw)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    double s = 0.0;
    for (int j = 0; j < nch; ++j) s += (double)part[(long long)j * n + i];
    dw[i] = (float)s;
}

// ---------------------------------------------------------------------------------------------------- C ABI
// The argument checks are the float32 entry points' (spa_segnet_train.hip): the same shapes, layouts and alignments
// are taken and refused, and a refused call launches nothing.
static bool sgh_al16(const void *p) { return ((uintptr_t)p & 15) == 0; }

static int sgh_check_shape(int B, int H, int W, int Cin)
{
    SPA_ARG(B > 0 && B < 65536 && H > 0 && W > 0);
    SPA_ARG(Cin == 3 ? (H % 16 == 0 && W % 16 == 0) : (H % 2 == 0 && W % 2 == 0));
    SPA_ARG((long long)H * W * 64 < (1ll << 31) && H / SGH_TH < 65536);
    return SPA_OK;
}

static int sgh_input_form(const char *fn, int32_t Cin, int32_t x_layout, const float *mean_host, const float *std_host,
                          const uint8_t *idx, SghStd *st)
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

// the two operands' scale exponents -> ex[0], ex[1] (device words in the workspace), without a host synchronisation:
// operand 0 is a (n0 floats) or, with Cin == 3, conv1's operand of the image a; operand 1 is b (n1 floats)
static int sgh_scales(spa_ctx *ctx, hipStream_t s, const float *a, long long n0, int Cin, int B, int H, int W,
                      const SghStd &st, const float *b, long long n1, int **ex)
{
    unsigned *part = nullptr;
    int rc = spa_ws_reserve(ctx, WS_SEGNET_AMAX, 2 * SGH_NAMAX * sizeof(unsigned) + 16, (void **)&part);
    if (rc != SPA_OK) return rc;
    if (Cin == 3)
        hipLaunchKernelGGL(k_sgh_amax_conv1, dim3(SGH_NAMAX), dim3(256), 0, s, a, B, H, W, st, part);
    else
        hipLaunchKernelGGL(k_sgh_amax, dim3(SGH_NAMAX), dim3(256), 0, s, a, n0 / 4, part);
    SPA_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_sgh_amax, dim3(SGH_NAMAX), dim3(256), 0, s, b, n1 / 4, part + SGH_NAMAX);
    SPA_LAUNCH_CHECK();
    *ex = (int *)(part + 2 * SGH_NAMAX);
    hipLaunchKernelGGL(k_sgh_scale, dim3(2), dim3(256), 0, s, part, *ex);
    SPA_LAUNCH_CHECK();
    return SPA_OK;
}

extern "C" int spa_segnet_train_forward_f16x3(spa_ctx *ctx, const float *x, const uint8_t *idx, int32_t x_layout,
                                              int32_t B, int32_t H, int32_t W, int32_t Cin, const float *wt,
                                              const float *mean_host, const float *std_host, float *y, double *stats,
                                              void *stream)
{
    SPA_ARG(ctx && x && wt && y);
    int rc = sgh_check_shape(B, H, W, Cin);
    if (rc != SPA_OK) return rc;
    SPA_ARG(sgh_al16(x) && sgh_al16(wt));
    SghStd st = {};
    rc = sgh_input_form("spa_segnet_train_forward_f16x3", Cin, x_layout, mean_host, std_host, idx, &st);
    if (rc != SPA_OK) return rc;
    hipStream_t s = spa_stream(stream);
    dim3 grid((W + SGH_TW - 1) / SGH_TW, (H + SGH_TH - 1) / SGH_TH, B);
    const long long nblk = (long long)grid.x * grid.y * grid.z;
    unsigned short *wp = nullptr;
    if ((rc = spa_ws_reserve(ctx, WS_SEGNET_WF16X3, 2 * SGH_W64 * sizeof(unsigned short), (void **)&wp)) != SPA_OK)
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
        hipLaunchKernelGGL(k_sgh_wpack1, dim3(SGH_W1 / 256), dim3(256), 0, s, wt, ex, wp);
    else
        hipLaunchKernelGGL(k_sgh_wpack64, dim3(SGH_W64 / 256), dim3(256), 0, s, wt, 0, ex, wp);
    SPA_LAUNCH_CHECK();
    if (Cin == 3)
        hipLaunchKernelGGL((k_sgh_conv<SGH_CONV1, SGH_FULL>), grid, dim3(SGH_THREADS), 0, s, x, nullptr, wp, nullptr,
                           y, part, ex, H, W, st);
    else if (!idx)
        hipLaunchKernelGGL((k_sgh_conv<SGH_ENC, SGH_FULL>), grid, dim3(SGH_THREADS), 0, s, x, nullptr, wp, nullptr, y,
                           part, ex, H, W, st);
    else
        hipLaunchKernelGGL((k_sgh_conv<SGH_DEC, SGH_FULL>), grid, dim3(SGH_THREADS), 0, s, x, idx, wp, nullptr, y,
                           part, ex, H, W, st);
    SPA_LAUNCH_CHECK();
    if (stats) {
        hipLaunchKernelGGL(k_sgh_bnstat, dim3(128), dim3(256), 0, s, part, nblk, stats);
        SPA_LAUNCH_CHECK();
    }
    return SPA_OK;
}

extern "C" int spa_segnet_train_dgrad_f16x3(spa_ctx *ctx, const float *dy, const float *wt, const uint8_t *idx,
                                            int32_t B, int32_t H, int32_t W, float *dx, void *stream)
{
    SPA_ARG(ctx && dy && wt && dx);
    int rc = sgh_check_shape(B, H, W, 64);
    if (rc != SPA_OK) return rc;
    SPA_ARG(sgh_al16(dy) && sgh_al16(wt) && ((uintptr_t)idx & 3) == 0);
    unsigned short *wp = nullptr;
    if ((rc = spa_ws_reserve(ctx, WS_SEGNET_WF16X3, 2 * SGH_W64 * sizeof(unsigned short), (void **)&wp)) != SPA_OK)
        return rc;
    hipStream_t s = spa_stream(stream);
    int *ex = nullptr;
    if ((rc = sgh_scales(ctx, s, dy, (long long)B * H * W * 64, 64, B, H, W, SghStd{}, wt, SGH_W64, &ex)) != SPA_OK)
        return rc;
    hipLaunchKernelGGL(k_sgh_wpack64, dim3(SGH_W64 / 256), dim3(256), 0, s, wt, 1, ex, wp);
    SPA_LAUNCH_CHECK();
    dim3 grid((W + SGH_TW - 1) / SGH_TW, (H + SGH_TH - 1) / SGH_TH, B);
    if (idx)
        hipLaunchKernelGGL((k_sgh_conv<SGH_ENC, SGH_POOLED>), grid, dim3(SGH_THREADS), 0, s, dy, nullptr, wp, idx, dx,
                           nullptr, ex, H, W, SghStd{});
    else
        hipLaunchKernelGGL((k_sgh_conv<SGH_ENC, SGH_FULL>), grid, dim3(SGH_THREADS), 0, s, dy, nullptr, wp, nullptr,
                           dx, nullptr, ex, H, W, SghStd{});
    SPA_LAUNCH_CHECK();
    return SPA_OK;
}

extern "C" int spa_segnet_train_wgrad_f16x3(spa_ctx *ctx, const float *dy, const float *x, const uint8_t *idx,
                                            int32_t x_layout, int32_t B, int32_t H, int32_t W, int32_t Cin,
                                            const float *mean_host, const float *std_host, float *dw, void *stream)
{
    SPA_ARG(ctx && dy && x && dw);
    int rc = sgh_check_shape(B, H, W, Cin);
    if (rc != SPA_OK) return rc;
    SPA_ARG(sgh_al16(dy) && sgh_al16(x));
    SghStd st = {};
    rc = sgh_input_form("spa_segnet_train_wgrad_f16x3", Cin, x_layout, mean_host, std_host, idx, &st);
    if (rc != SPA_OK) return rc;
    const int CP = Cin == 3 ? 4 : 64;
    const long long tiles = (long long)B * (H / SGHW_TR) * ((W + SGHW_TW - 1) / SGHW_TW);
    const int nch = sgh_wgrad_chunks(tiles);
    const int n = 49 * 64 * CP;
    float *part = nullptr;
    if ((rc = spa_ws_reserve(ctx, WS_SEGNET_WGRAD, (size_t)nch * n * sizeof(float), (void **)&part)) != SPA_OK)
        return rc;
    hipStream_t s = spa_stream(stream);
    // ex[0] the input form's scale (as in the forward), ex[1] dy's
    const long long nx = Cin == 3 ? 0 : (long long)B * (idx ? (H / 2) * (W / 2) : H * W) * 64;
    int *ex = nullptr;
    if ((rc = sgh_scales(ctx, s, x, nx, Cin, B, H, W, st, dy, (long long)B * H * W * 64, &ex)) != SPA_OK) return rc;
    dim3 grid(nch, 7);
    if (Cin == 3)
        hipLaunchKernelGGL(k_sgh_wgrad<SGH_CONV1>, grid, dim3(SGH_THREADS), 0, s, dy, x, nullptr, part, ex, B, H, W,
                           nch, st);
    else if (!idx)
        hipLaunchKernelGGL(k_sgh_wgrad<SGH_ENC>, grid, dim3(SGH_THREADS), 0, s, dy, x, nullptr, part, ex, B, H, W, nch,
                           st);
    else
        hipLaunchKernelGGL(k_sgh_wgrad<SGH_DEC>, grid, dim3(SGH_THREADS), 0, s, dy, x, idx, part, ex, B, H, W, nch,
                           st);
    SPA_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_sgh_wsum, dim3((n + 255) / 256), dim3(256), 0, s, part, nch, n, dw);
    SPA_LAUNCH_CHECK();
    return SPA_OK;
}
