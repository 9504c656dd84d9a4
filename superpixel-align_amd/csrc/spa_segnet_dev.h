// The one copy of what the six SegNet-Basic kernel files (spa_segnet*.hip: inference | training x float32 | bf16 |
// split f16 planes) have in common: the tile geometry, the input forms (conv1's standardised, LRN-normalised image;
// a 64-channel map; a decoder's pooled map unpooled through its index map), the 16-bit operand packers, the float32
// epilogues, the small reduction / weight-packing kernels and the host-side argument checks.  The numeric contract of
// the family lives here: a 16-bit file multiplies the rounding (bf16) or the split (two f16 planes) of exactly the
// float32 value the float32 kernel multiplies, because all of them get that value from the same function, and every
// epilogue after the float32 accumulators is the same function.
//
// Tiling (all conv kernels): one workgroup = one 8 x 32 output tile x all 64 channels, 4 waves, wave w owns output
// rows 2w, 2w + 1.  A 16-row MFMA tile of a wave is FOUR 2x2 pooling blocks: row i of the tile is pixel (i & 3) of
// block i >> 2, so the C/D layout (row = 4 (lane >> 4) + reg, the same for the 16x16x4 float32 and the 16x16x32 16-bit
// instructions) puts the four pixels of one 2x2 window in the four accumulator registers of one lane -- pooling, its
// argmax and the pooled-gradient gather are register-only.  No atomics anywhere: every output is one thread's
// fixed-order sum, the same bits for any batch size or position in the batch.
//
// Every device function is __forceinline__ and takes the accumulators by reference (a call would put them in scratch).
// The small kernels every file of an operand type launches are defined once, in the training file of that type, behind
// the host functions declared at the end.
#pragma once
#include "spa_common.h"

typedef float sg_f32x4 __attribute__((ext_vector_type(4)));
typedef __bf16 sg_bf16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 sg_f16x8 __attribute__((ext_vector_type(8)));
typedef short sg_s16x4 __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(3))) sg_s16x4 sg_lds_s16x4;

#define SG_TH 8                       // output tile rows
#define SG_TW 32                      // output tile columns
#define SG_HH (SG_TH + 6)             // halo rows
#define SG_HW (SG_TW + 6)             // halo columns
#define SG_HPIX (SG_HH * SG_HW)       // 532 halo pixels
#define SG_THREADS 256
#define SG_NAMAX 256                  // workgroups of one operand's max reduction (split planes)
#define SG_W64 (49 * 64 * 64)         // elements of a 64-channel layer's weights (per plane)
#define SG_W1 (7 * 64 * 32)           // elements of conv1's 16-bit weights (per plane): 7 K steps of 8 taps x 4 channels
#define SGW_TR 2                      // wgrad tile rows
#define SGW_TW 32                     // wgrad tile columns
#define SGW_MAXCH 96                  // wgrad: chunks of K at most

enum { SG_CONV1 = 0, SG_ENC = 1, SG_DEC = 2, SG_DEC1 = 3, SG_DEC1L = 4 };   // input / layer forms (training: the first three)
// the input form of a layer form: decode1, with the softmax (SG_DEC1) or with the raw classifier sums (SG_DEC1L), reads a
// decoder's input
constexpr int sg_input_form_of(int mode) { return mode == SG_DEC1 || mode == SG_DEC1L ? SG_DEC : mode; }
enum { SG_FULL = 0, SG_POOLED = 1 };                             // training epilogues

struct SgStd {
    float mean[3], std[3];
};

// this lane's fragment pixel: tile row fi = lane & 15 is pixel (fi & 3) of 2x2 block fi >> 2 -> halo row frow, column
// fcol (+ 8 m for MFMA tile m); fq = lane >> 4 is the lane quarter (K slice of an operand, 2x2 block of the C/D tile)
struct SgGeom {
    int fi, fq, frow, fcol;
};

__device__ __forceinline__ SgGeom sg_geom(int lane, int w)
{
    const int fi = lane & 15;
    return {fi, lane >> 4, 2 * w + ((fi & 3) >> 1), 2 * (fi >> 2) + (fi & 1)};
}

// ---------------------------------------------------------------------------------------------------- input forms
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

// the standardised (two float32 operations, as the dataset), LRN-normalised conv1 input at offset o of the planar image
// xb (plane = H * W)
__device__ __forceinline__ void sg_conv1_at(const float *xb, long long plane, long long o, const SgStd &st, float &r,
                                            float &g, float &bl)
{
    r = xb[o];
    g = xb[plane + o];
    bl = xb[2 * plane + o];
    r = (r - st.mean[0]) / st.std[0];          // img -= mean; img /= std (two roundings)
    g = (g - st.mean[1]) / st.std[1];
    bl = (bl - st.mean[2]) / st.std[2];
    sg_lrn3(r, g, bl);
}

// that value at (gy, gx), channel 3 zero; zero outside the image.  Two spellings of the zero: sg_conv1_val4 for the
// float32 kernels (which stage the vector), sg_conv1_val for the 16-bit ones (which convert the scalars).  The compiler
// packs the LRN arithmetic differently for them (v_pk_mul_f32 / v_pk_add_f32 against single operations), and each
// kernel keeps the instructions it was verified with (profiles/segnet_refactor_isa.md).
__device__ __forceinline__ sg_f32x4 sg_conv1_val4(const float *xb, long long plane, int gy, int gx, int H, int W,
                                                  const SgStd &st)
{
    sg_f32x4 v = {0.f, 0.f, 0.f, 0.f};
    if (gy >= 0 && gy < H && gx >= 0 && gx < W) {
        float r, g, bl;
        sg_conv1_at(xb, plane, (long long)gy * W + gx, st, r, g, bl);
        v = (sg_f32x4){r, g, bl, 0.f};
    }
    return v;
}

__device__ __forceinline__ sg_f32x4 sg_conv1_val(const float *xb, long long plane, int gy, int gx, int H, int W,
                                                 const SgStd &st)
{
    float r = 0.f, g = 0.f, bl = 0.f;
    if (gy >= 0 && gy < H && gx >= 0 && gx < W) sg_conv1_at(xb, plane, (long long)gy * W + gx, st, r, g, bl);
    return (sg_f32x4){r, g, bl, 0.f};
}

// four channels [c, c + 4) of the 64-channel input at full-resolution (gy, gx): SG_ENC reads the map X (B,H,W,64),
// SG_DEC the pooled map X (B,H/2,W/2,64) at (gy/2, gx/2) where its index I selects (gy & 1, gx & 1), zero elsewhere
// (so the 4x larger unpooled tensor never exists); zero outside the image
template <int MODE>
__device__ __forceinline__ sg_f32x4 sg_px4(const float *X, const uint8_t *I, int b, int gy, int gx, int c, int H, int W)
{
    sg_f32x4 v = {0.f, 0.f, 0.f, 0.f};
    if (gy >= 0 && gy < H && gx >= 0 && gx < W) {
        if (MODE == SG_ENC) {
            v = *(const sg_f32x4 *)(X + (((long long)b * H + gy) * W + gx) * 64 + c);
        } else {
            const int Hh = H >> 1, Wh = W >> 1;
            const long long o = (((long long)b * Hh + (gy >> 1)) * Wh + (gx >> 1)) * 64 + c;
            const sg_f32x4 h = *(const sg_f32x4 *)(X + o);
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

// eight channels [c, c + 8) of the same input forms into lo, hi; false (lo, hi untouched) outside the image, where the
// caller stages zeros without converting any
template <int MODE>
__device__ __forceinline__ bool sg_px8(const float *X, const uint8_t *I, int b, int gy, int gx, int c, int H, int W,
                                       sg_f32x4 &lo, sg_f32x4 &hi)
{
    if (!(gy >= 0 && gy < H && gx >= 0 && gx < W)) return false;
    if (MODE == SG_ENC) {
        const float *p = X + (((long long)b * H + gy) * W + gx) * 64 + c;
        lo = *(const sg_f32x4 *)p;
        hi = *(const sg_f32x4 *)(p + 4);
    } else {
        const int Hh = H >> 1, Wh = W >> 1;
        const long long o = (((long long)b * Hh + (gy >> 1)) * Wh + (gx >> 1)) * 64 + c;
        lo = *(const sg_f32x4 *)(X + o);
        hi = *(const sg_f32x4 *)(X + o + 4);
        const unsigned i0 = *(const unsigned *)(I + o), i1 = *(const unsigned *)(I + o + 4);
        const unsigned sel = (unsigned)(((gy & 1) << 1) | (gx & 1));
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            if (((i0 >> (8 * j)) & 0xffu) != sel) lo[j] = 0.f;
            if (((i1 >> (8 * j)) & 0xffu) != sel) hi[j] = 0.f;
        }
    }
    return true;
}

// ---------------------------------------------------------------------------------------------------- bf16 operands
__device__ __forceinline__ unsigned sg_bf16_bits(float f)
{
    const __bf16 h = (__bf16)f;                    // round to nearest even; subnormals kept, NaN stays NaN
    return (unsigned)__builtin_bit_cast(unsigned short, h);
}

__device__ __forceinline__ unsigned sg_bf16_pack2(float a, float b) { return sg_bf16_bits(a) | (sg_bf16_bits(b) << 16); }

__device__ __forceinline__ uint4 sg_bf16_pack8(sg_f32x4 lo, sg_f32x4 hi)
{
    return make_uint4(sg_bf16_pack2(lo.x, lo.y), sg_bf16_pack2(lo.z, lo.w), sg_bf16_pack2(hi.x, hi.y),
                      sg_bf16_pack2(hi.z, hi.w));
}

// sg_conv1_val rounded to bf16 (4 values, channel 3 zero)
__device__ __forceinline__ uint2 sg_bf16_conv1_px(const float *xb, long long plane, int gy, int gx, int H, int W,
                                                  const SgStd &st)
{
    const sg_f32x4 v = sg_conv1_val(xb, plane, gy, gx, H, W, st);
    return make_uint2(sg_bf16_pack2(v.x, v.y), sg_bf16_pack2(v.z, 0.f));
}

// channels [c, c + 8) of input form MODE (sg_px8) rounded to bf16
template <int MODE>
__device__ __forceinline__ uint4 sg_bf16_px8(const float *X, const uint8_t *I, int b, int gy, int gx, int c, int H,
                                             int W)
{
    sg_f32x4 lo, hi;
    return sg_px8<MODE>(X, I, b, gy, gx, c, H, W, lo, hi) ? sg_bf16_pack8(lo, hi) : make_uint4(0u, 0u, 0u, 0u);
}

// one K step's 16-bit operand fragment V (sg_bf16x8 / sg_f16x8) from two transposed LDS reads: p0 the lane's address
// for pixels k .. k + 3, p1 for k + 4 .. k + 7 (ds_read_b64_tr_b16: lane 4q + p of each 16-lane group names row q,
// columns 4p .. 4p + 3 of a 4 x 16 block; lane i receives column i of the 4 rows).  Every lane of the wave must take
// part.
template <typename V>
__device__ __forceinline__ V sg_tr8(const unsigned short *p0, const unsigned short *p1)
{
    const sg_s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((sg_lds_s16x4 *)p0);
    const sg_s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((sg_lds_s16x4 *)p1);
    return __builtin_bit_cast(V, __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7));
}

// ---------------------------------------------------------------------------------------------------- split f16 planes
// Each operand gets one power of two t = 2^k that brings its largest magnitude into [2^14, 2^15) (k = 0 for an
// all-zero operand).  A value v becomes h = f16_rn(t v), l = f16_rn(t v - h), 22 significand bits between them; a
// product a b is h_a h_b + h_a l_b + l_a h_b (l_a l_b, 2^-22 of the product, is dropped) and the float32 sum is
// multiplied by 2^-(k_a + k_b) (v_ldexp, exact) before anything else is done with it.

// 2^k as a float (k in [-113, 126], as k_sg_scale produces)
__device__ __forceinline__ float sg_pow2(int k) { return __uint_as_float((unsigned)(127 + k) << 23); }

// h = f16_rn(v sc), l = f16_rn(v sc - h) as bit patterns (sc a power of two: v sc and the difference are exact)
__device__ __forceinline__ void sg_split(float v, float sc, unsigned short &h, unsigned short &l)
{
    const float s = v * sc;
    const _Float16 hh = (_Float16)s;
    const _Float16 ll = (_Float16)(s - (float)hh);
    h = __builtin_bit_cast(unsigned short, hh);
    l = __builtin_bit_cast(unsigned short, ll);
}

// eight float32 values -> their h plane (returned) and l plane (through l), packed in channel order
__device__ __forceinline__ uint4 sg_split8(sg_f32x4 lo, sg_f32x4 hi, float sc, uint4 &l)
{
    uint4 h;
    h.x = spa_split16_pair(lo.x, lo.y, sc, l.x);
    h.y = spa_split16_pair(lo.z, lo.w, sc, l.y);
    h.z = spa_split16_pair(hi.x, hi.y, sc, l.z);
    h.w = spa_split16_pair(hi.z, hi.w, sc, l.w);
    return h;
}

// sg_conv1_val split: the h plane's 4 values (channel 3 zero) returned, the l plane's through l
__device__ __forceinline__ uint2 sg_split_conv1_px(const float *xb, long long plane, int gy, int gx, int H, int W,
                                                   const SgStd &st, float sc, uint2 &l)
{
    const sg_f32x4 v = sg_conv1_val(xb, plane, gy, gx, H, W, st);
    uint2 h;
    h.x = spa_split16_pair(v.x, v.y, sc, l.x);
    h.y = spa_split16_pair(v.z, 0.f, sc, l.y);
    return h;
}

// channels [c, c + 8) of input form MODE (sg_px8), split
template <int MODE>
__device__ __forceinline__ uint4 sg_split_px8(const float *X, const uint8_t *I, int b, int gy, int gx, int c, int H,
                                              int W, float sc, uint4 &l)
{
    sg_f32x4 lo, hi;
    if (sg_px8<MODE>(X, I, b, gy, gx, c, H, W, lo, hi)) return sg_split8(lo, hi, sc, l);
    return l = make_uint4(0u, 0u, 0u, 0u);
}

__device__ __forceinline__ sg_f16x8 sg_f16_frag(uint4 v) { return __builtin_bit_cast(sg_f16x8, v); }

// one K step's products a b = h_a h_b + h_a l_b + l_a h_b, small terms first: the two cross terms (2^-11 of h_a h_b)
// into their own accumulator x, h_a h_b into acc; the epilogue adds the two.  Chained into one accumulator instead,
// each pass still met the float32 bounds element by element, but its errors summed over a layer's pixels did not
// cancel as the float32 passes' do: in a whole step, updates that are cancellation residuals (conv1_bn/beta) missed
// float64 by 9.7e-3 against 4.3e-6 in float32.  With the separate accumulators they land at 4.2e-6.
__device__ __forceinline__ void sg_mma3(sg_f32x4 &acc, sg_f32x4 &x, sg_f16x8 ah, sg_f16x8 al, sg_f16x8 bh, sg_f16x8 bl)
{
    x = __builtin_amdgcn_mfma_f32_16x16x32_f16(ah, bl, x, 0, 0, 0);
    x = __builtin_amdgcn_mfma_f32_16x16x32_f16(al, bh, x, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(ah, bh, acc, 0, 0, 0);
}

// the bit pattern of |v|: non-negative floats order as unsigned integers, so a max of these is exact in any order
__device__ __forceinline__ unsigned sg_absbits(float v) { return __float_as_uint(v) & 0x7fffffffu; }

// ---------------------------------------------------------------------------------------------------- K loops
// The staging and K loop of a forward / dgrad convolution, one per operand type, shared by that type's inference and
// training kernel (the split-plane one is spa_segnet_split_main.inc): acc += conv7x7(input form MODE (SG_CONV1, SG_ENC
// or SG_DEC) of X (, I)) for this workgroup's tile, through the LDS halo xs (SG_HPIX pixels of sg_ps_*(MODE) elements).
// g = sg_geom(lane, wave).

constexpr int sg_ps_f32(int mode) { return mode == SG_CONV1 ? 4 : 20; }            // LDS floats per halo pixel
constexpr int sg_ps_bf16(int mode) { return mode == SG_CONV1 ? 4 : 40; }           // bf16: 32 channels + 16 bytes of padding
constexpr int sg_ps_split(int mode) { return mode == SG_CONV1 ? 8 : 72; }          // f16: 32 h, 32 l, padding; conv1 [4 h | 4 l]

// float32 (v_mfma_f32_16x16x4_f32): Wt (49,64,CP) = (tap, n, c).  The halo is staged 16 channels at a time (20-float
// pixel stride: the 16 pixels of a fragment read fall into distinct banks); conv1's three channels are padded to 4: one
// tap = one K = 4 step.
template <int MODE>
__device__ __forceinline__ void sg_conv_main_f32(sg_f32x4 (&acc)[4][4], float *xs, const float *X, const uint8_t *I,
                                                 const float *Wt, int b, int ty0, int tx0, const SgGeom &g, int H,
                                                 int W, const SgStd &st)
{
    constexpr int CP = MODE == SG_CONV1 ? 4 : 64;          // channels of a weight row (conv1: 3 padded to 4)
    constexpr int CH = MODE == SG_CONV1 ? 4 : 16;          // channels staged per chunk
    constexpr int PS = sg_ps_f32(MODE);
    const int tid = threadIdx.x;
    const auto [fi, fq, frow, fcol] = g;
    for (int c0 = 0; c0 < CP; c0 += CH) {
        if (c0) __syncthreads();
        // ---- stage the halo of channels [c0, c0 + CH)
        if (MODE == SG_CONV1) {
            const long long plane = (long long)H * W;
            const float *xb = X + (long long)b * 3 * plane;
            for (int p = tid; p < SG_HPIX; p += SG_THREADS)
                *(sg_f32x4 *)&xs[p * PS] = sg_conv1_val4(xb, plane, ty0 - 3 + p / SG_HW, tx0 - 3 + p % SG_HW, H, W, st);
        } else {
            for (int e = tid; e < SG_HPIX * 4; e += SG_THREADS) {
                const int p = e >> 2, q = e & 3;
                *(sg_f32x4 *)&xs[p * PS + 4 * q] =
                    sg_px4<MODE>(X, I, b, ty0 - 3 + p / SG_HW, tx0 - 3 + p % SG_HW, c0 + 4 * q, H, W);
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
                    sg_f32x4 bw[4], a[4];
#pragma unroll
                    for (int nt = 0; nt < 4; ++nt) bw[nt] = *(const sg_f32x4 *)(wt + nt * 16 * CP);
#pragma unroll
                    for (int m = 0; m < 4; ++m) a[m] = *(const sg_f32x4 *)&xr[(kx + 8 * m) * PS];
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
}

// bf16 (v_mfma_f32_16x16x32_bf16): Wb (49,64,64) = (tap, n, c), or conv1's (7,64,32) = (K step, n, k).  The A operand
// is 16 pixels x 32 input channels: a lane reads 8 consecutive channels of one pixel (16 bytes) from a channels-last
// bf16 halo (14 x 38 pixels x 40 bf16 = 42 560 bytes), staged in two 32-channel chunks.  conv1's K is (tap, channel)
// with the 3 channels padded to 4: a 32-wide K step packs 8 taps, the 49 taps fill 7 steps with the last 7 zero.
template <int MODE>
__device__ __forceinline__ void sg_conv_main_bf16(sg_f32x4 (&acc)[4][4], unsigned short *xs, const float *X,
                                                  const uint8_t *I, const unsigned short *Wb, int b, int ty0, int tx0,
                                                  const SgGeom &g, int H, int W, const SgStd &st)
{
    constexpr int PS = sg_ps_bf16(MODE);
    constexpr int NCH = MODE == SG_CONV1 ? 1 : 2;                        // 32-channel chunks
    const int tid = threadIdx.x;
    const auto [fi, fq, frow, fcol] = g;
    for (int ch = 0; ch < NCH; ++ch) {
        if (ch) __syncthreads();
        // ---- stage the bf16 halo of channels [32 ch, 32 ch + 32) (conv1: its 3 channels and a zero)
        if (MODE == SG_CONV1) {
            const long long plane = (long long)H * W;
            const float *xb = X + (long long)b * 3 * plane;
            for (int p = tid; p < SG_HPIX; p += SG_THREADS)
                *(uint2 *)&xs[p * PS] = sg_bf16_conv1_px(xb, plane, ty0 - 3 + p / SG_HW, tx0 - 3 + p % SG_HW, H, W, st);
        } else {
            for (int e = tid; e < SG_HPIX * 4; e += SG_THREADS) {
                const int p = e >> 2, q = e & 3;
                *(uint4 *)&xs[p * PS + 8 * q] =
                    sg_bf16_px8<MODE>(X, I, b, ty0 - 3 + p / SG_HW, tx0 - 3 + p % SG_HW, 32 * ch + 8 * q, H, W);
            }
        }
        __syncthreads();

        if (MODE == SG_CONV1) {
            // lane quarter fq holds taps t0 = 8 s + 2 fq and t0 + 1 of K step s, 4 channels each
            const unsigned short *xr = &xs[(frow * SG_HW + fcol) * PS];
#pragma unroll
            for (int s = 0; s < 7; ++s) {
                const int t0 = 8 * s + 2 * fq, t1 = t0 + 1;
                const int o0 = ((t0 / 7) * SG_HW + t0 % 7) * PS, o1 = ((t1 / 7) * SG_HW + t1 % 7) * PS;
                sg_bf16x8 bw[4], a[4];
#pragma unroll
                for (int nt = 0; nt < 4; ++nt)
                    bw[nt] = *(const sg_bf16x8 *)(Wb + ((long long)s * 64 + 16 * nt + fi) * 32 + 8 * fq);
#pragma unroll
                for (int m = 0; m < 4; ++m) {
                    const uint2 lo = t0 < 49 ? *(const uint2 *)&xr[o0 + 8 * m * PS] : make_uint2(0u, 0u);
                    const uint2 hi = t1 < 49 ? *(const uint2 *)&xr[o1 + 8 * m * PS] : make_uint2(0u, 0u);
                    a[m] = __builtin_bit_cast(sg_bf16x8, make_uint4(lo.x, lo.y, hi.x, hi.y));
                }
#pragma unroll
                for (int m = 0; m < 4; ++m)
#pragma unroll
                    for (int nt = 0; nt < 4; ++nt)
                        acc[m][nt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[m], bw[nt], acc[m][nt], 0, 0, 0);
            }
        } else {
            // K order inside a chunk: lane quarter fq holds channels 32 ch + 8 fq .. + 7 of both operands
            const unsigned short *wl = Wb + (long long)fi * 64 + 32 * ch + 8 * fq;
            for (int ky = 0; ky < 7; ++ky) {
                const unsigned short *xr = &xs[((frow + ky) * SG_HW + fcol) * PS + 8 * fq];
#pragma unroll
                for (int kx = 0; kx < 7; ++kx) {
                    const unsigned short *wt = wl + (long long)(ky * 7 + kx) * 64 * 64;
                    sg_bf16x8 bw[4], a[4];
#pragma unroll
                    for (int nt = 0; nt < 4; ++nt) bw[nt] = *(const sg_bf16x8 *)(wt + nt * 16 * 64);
#pragma unroll
                    for (int m = 0; m < 4; ++m) a[m] = *(const sg_bf16x8 *)&xr[(kx + 8 * m) * PS];
#pragma unroll
                    for (int m = 0; m < 4; ++m)
#pragma unroll
                        for (int nt = 0; nt < 4; ++nt)
                            acc[m][nt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[m], bw[nt], acc[m][nt], 0, 0, 0);
                }
            }
        }
    }
}

// ---------------------------------------------------------------------------------------------------- epilogues
// In all of them a lane holds channel n = 16 nt + fi; register r of acc[m][nt] is pixel r (ky * 2 + kx) of 2x2 block
// fq of MFMA tile m, i.e. output rows ty0 + 2w + (r >> 1), columns tx0 + 8m + 2 fq + (r & 1).  H and W are even: a
// block is wholly inside the image or outside.

// Inference, on the float32 sums acc.  SG_CONV1 / SG_ENC: Y (B,H/2,W/2,64) = maxpool2x2(relu(acc + bias)) and Yi its
// uint8 argmax (ky * 2 + kx, first maximum).  SG_DEC: Y (B,H,W,64) = acc + bias.  SG_DEC1: Y (B,2,H,W) planar =
// softmax(conv1x1(acc + bias; wc (2,64)) + bc (2)).  SG_DEC1L: the same two sums, stored before the softmax.
template <int MODE>
__device__ __forceinline__ void sg_infer_epilogue(sg_f32x4 (&acc)[4][4], const float *bias, const float *wc,
                                                  const float *bc, float *Y, uint8_t *Yi, int b, int ty0, int tx0,
                                                  int w, int fi, int fq, int H, int W)
{
#include "spa_segnet_infer_epilogue.inc"
}

// Training forward and dgrad of the float32 and bf16 kernels, on the float32 sums acc.  (k_sgh_conv keeps a copy of its
// own that unscales what it stores: as a call of this function with an exponent argument the compiler packed its
// partial sums into v_pk_add_f32 / v_pk_fma_f32, slow beside matrix instructions, where the inline text does not.)
// SG_FULL: Y (B,H,W,64) = the sums; with part != NULL also part[blk][0..63] = sum y, part[blk][64..127] = sum y^2 over
// the workgroup's in-image pixels (blk = (b * gridDim.y + tile row) * gridDim.x + tile column), through red (2048
// floats of LDS, free once every wave left the K loop).
// SG_POOLED: Y (B,H/2,W/2,64) = the sum at the position Io (B,H/2,W/2,64) selects in each 2x2 block.
template <int EPI>
__device__ __forceinline__ void sg_train_epilogue(sg_f32x4 (&acc)[4][4], const uint8_t *Io, float *Y, float *part,
                                                  float *red, int b, int ty0, int tx0, int w, int fi, int fq, int H,
                                                  int W)
{
    const int tid = threadIdx.x;
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
                    const float v = acc[m][nt][r];
                    Y[(((long long)b * H + oy + (r >> 1)) * W + x + (r & 1)) * 64 + n] = v;
                    s[nt] += v;
                    q[nt] = fmaf(v, v, q[nt]);
                }
            }
        }
        if (part) {
            // fixed order: lanes' sums -> LDS [wave][fq][channel], then 128 threads add the 16 entries of a channel
            __syncthreads();
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
                Y[o + n] = r == 0 ? a[0] : r == 1 ? a[1] : r == 2 ? a[2] : a[3];
            }
        }
    }
}

// wgrad: tile t of the (B, tyn = H / SGW_TR, txn) tiles of K -> image b, first row y0, first column x0
__device__ __forceinline__ void sg_wgrad_tile(long long t, int txn, int tyn, int &b, int &y0, int &x0)
{
    const int tx = (int)(t % txn);
    const long long r2 = t / txn;
    const int ty = (int)(r2 % tyn);
    b = (int)(r2 / tyn);
    y0 = ty * SGW_TR;
    x0 = tx * SGW_TW;
}

// ---------------------------------------------------------------------------------------------------- host side
// The small kernels, each launched on stream s through one host function (the caller follows with SPA_LAUNCH_CHECK).
// Library-internal: not exported from libspalign.so.
#define SG_LOCAL __attribute__((visibility("hidden")))
// spa_segnet_train.hip: stats (2,64) float64 = the nblk workgroups' BN partial sums added in block order; dw (n) = the
// nch wgrad chunk partials added in chunk order, in double, rounded once.
SG_LOCAL void sg_launch_bnstat(hipStream_t s, const float *part, long long nblk, double *stats);
SG_LOCAL void sg_launch_wsum(hipStream_t s, const float *part, int nch, int n, float *dw);
// spa_segnet_train_bf16.hip: the weights rounded to bf16, Wb (49,64,64) = (tap, n, c) (rot: dgrad's 180-degree
// rotation with in / out swapped) or conv1's (7,64,32) = (K step, n, k), k = 4 (tap - 8 step) + c, zero past tap 48.
SG_LOCAL void sg_launch_bf16_wpack64(hipStream_t s, const float *wt, int rot, unsigned short *wb);
SG_LOCAL void sg_launch_bf16_wpack1(hipStream_t s, const float *wt, unsigned short *wb);
// spa_segnet_train_f16x3.hip: ex[j] = the scale exponent of operand j < nop from its SG_NAMAX maxima part[j][..]; the
// weights in the bf16 layouts as an h plane then an l plane, split with scale 2^kw[0] (kw on the device).
SG_LOCAL void sg_launch_scale(hipStream_t s, int nop, const unsigned *part, int *ex);
SG_LOCAL void sg_launch_split_wpack64(hipStream_t s, const float *wt, int rot, const int *kw, unsigned short *wp);
SG_LOCAL void sg_launch_split_wpack1(hipStream_t s, const float *wt, const int *kw, unsigned short *wp);

// The argument checks of the entry points, once: the three operand types take and refuse the same shapes, layouts and
// alignments with the same codes, and a refused call launches nothing.  fn: the entry point's name for the error text.
// SPA_ARG for the shared checks: the same text, with the entry point fn in place of this header's name
#define SG_ARG(cond)                                                                    \
    do {                                                                                \
        if (!(cond)) {                                                                  \
            spa_set_error("invalid argument: %s (%s, %s:%d)", #cond, fn, __FILE__, __LINE__); \
            return SPA_ERR_ARG;                                                         \
        }                                                                               \
    } while (0)

static inline bool sg_al16(const void *p) { return ((uintptr_t)p & 15) == 0; }

static inline dim3 sg_conv_grid(int B, int H, int W) { return dim3((W + SG_TW - 1) / SG_TW, (H + SG_TH - 1) / SG_TH, B); }

// spa_segnet_encode*: fills st for conv1
static int sg_check_encode(const char *fn, const spa_ctx *ctx, const float *x, int32_t x_layout, int32_t B, int32_t H,
                           int32_t W, int32_t Cin, const float *wt, const float *bias, const float *mean_host,
                           const float *std_host, const float *pooled, const uint8_t *idx, SgStd *st)
{
    SG_ARG(ctx && x && wt && bias && pooled && idx && B > 0 && B < 65536 && H > 0 && W > 0);
    SG_ARG(Cin == 3 || Cin == 64);
    // conv1 sees the network input: all four poolings must be even (H, W % 16); the deeper layers pool once more
    SG_ARG(Cin == 3 ? (H % 16 == 0 && W % 16 == 0) : (H % 2 == 0 && W % 2 == 0));
    SG_ARG((long long)H * W * 64 < (1ll << 31) && H / SG_TH < 65536);
    SG_ARG(sg_al16(x) && sg_al16(wt));
    if (Cin == 3) {
        SG_ARG(mean_host && std_host);
        if (x_layout != SPA_LAYOUT_NCHW) {
            spa_set_error("%s: the conv1 input is the planar (B,3,H,W) image", fn);
            return SPA_ERR_LAYOUT;
        }
        for (int c = 0; c < 3; ++c) { st->mean[c] = mean_host[c]; st->std[c] = std_host[c]; }
    } else if (x_layout != SPA_LAYOUT_NHWC) {
        spa_set_error("%s: 64-channel inputs must be channels-last (B,H,W,64)", fn);
        return SPA_ERR_LAYOUT;
    }
    return SPA_OK;
}

// spa_segnet_decode*: (Hh, Wh) the pooled map's size
// logits (spa_segnet_decode_logits*): the classifier is required, and the raw sums are defined at every decoder size
static int sg_check_decode(const char *fn, const spa_ctx *ctx, const float *x, const uint8_t *idx, int32_t x_layout,
                           int32_t B, int32_t Hh, int32_t Wh, const float *wt, const float *bias, const float *wc,
                           const float *bc, const float *y, bool logits = false)
{
    SG_ARG(ctx && x && idx && wt && bias && y && B > 0 && B < 65536 && Hh > 0 && Wh > 0);
    SG_ARG((wc == nullptr) == (bc == nullptr));
    SG_ARG(!logits || wc);
    const int H = 2 * Hh, W = 2 * Wh;
    // decode1 writes the network's output: the input size, a multiple of 16
    SG_ARG(logits || !wc || (H % 16 == 0 && W % 16 == 0));
    SG_ARG((long long)H * W * 64 < (1ll << 31) && H / SG_TH < 65536);
    SG_ARG(sg_al16(x) && sg_al16(wt) && ((uintptr_t)idx & 3) == 0);
    if (x_layout != SPA_LAYOUT_NHWC) {
        spa_set_error("%s: the pooled map and its indices must be channels-last (B,H/2,W/2,64)", fn);
        return SPA_ERR_LAYOUT;
    }
    return SPA_OK;
}

// the shape checks shared by the training entry points: (H, W) the convolution's resolution.  conv1 sees the network
// input (four poolings: H, W % 16); the deeper layers run at 1/2 .. 1/8 of it (H, W even)
static int sg_check_shape(const char *fn, int B, int H, int W, int Cin)
{
    SG_ARG(B > 0 && B < 65536 && H > 0 && W > 0);
    SG_ARG(Cin == 3 ? (H % 16 == 0 && W % 16 == 0) : (H % 2 == 0 && W % 2 == 0));
    SG_ARG((long long)H * W * 64 < (1ll << 31) && H / SG_TH < 65536);
    return SPA_OK;
}

// the input form of a training forward / wgrad: fills st for conv1
static int sg_input_form(const char *fn, int32_t Cin, int32_t x_layout, const float *mean_host, const float *std_host,
                         const uint8_t *idx, SgStd *st)
{
    SG_ARG(Cin == 3 || Cin == 64);
    if (Cin == 3) {
        SG_ARG(mean_host && std_host && !idx);
        if (x_layout != SPA_LAYOUT_NCHW) {
            spa_set_error("%s: the conv1 input is the planar (B,3,H,W) image", fn);
            return SPA_ERR_LAYOUT;
        }
        for (int c = 0; c < 3; ++c) { st->mean[c] = mean_host[c]; st->std[c] = std_host[c]; }
    } else {
        SG_ARG(((uintptr_t)idx & 3) == 0);
        if (x_layout != SPA_LAYOUT_NHWC) {
            spa_set_error("%s: 64-channel inputs (and index maps) must be channels-last", fn);
            return SPA_ERR_LAYOUT;
        }
    }
    return SPA_OK;
}

// wgrad's split of K = B*H*W pixels: 2 x 32 tiles, chunk j of nch owns a contiguous run of tiles.  The split depends on
// (B, H, W) only, so the bits do not depend on the device.  Reserves the chunks' partial dW (nch, 49, 64, CP).
static int sg_wgrad_plan(spa_ctx *ctx, int B, int H, int W, int Cin, int *nch, int *n, float **part)
{
    const long long tiles = (long long)B * (H / SGW_TR) * ((W + SGW_TW - 1) / SGW_TW);
    *nch = (int)(tiles < SGW_MAXCH ? tiles : SGW_MAXCH);
    *n = 49 * 64 * (Cin == 3 ? 4 : 64);
    return spa_ws_reserve(ctx, WS_SEGNET_WGRAD, (size_t)*nch * *n * sizeof(float), (void **)part);
}
