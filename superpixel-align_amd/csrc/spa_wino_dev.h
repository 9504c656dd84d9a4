// Device helpers of the Winograd kernels (spa_wino.hip).
#pragma once
#include "spa_common.h"

struct WinoGeom { int B, H, W, d, th, tw; long long T; int interleaved; };
typedef float wino_v4 __attribute__((ext_vector_type(4)));
__device__ __forceinline__ float4 wino_nt_load(const float4 *p) { const wino_v4 v = __builtin_nontemporal_load((const wino_v4 *)p); return make_float4(v[0], v[1], v[2], v[3]); }

// tile id -> (image, sub-grid, tile row, tile column).  Sub-grid-major (the numbering before round 8): consecutive ids walk
// one sub-grid of the dilation, so the workgroups running at one moment read and write pixel vectors d pixels apart.
// Interleaved (g.interleaved): the tiles of the d sub-grids of a pixel row are interleaved the way their pixels are,
//   t = ((b * d + sy) * th + ty) * tw * d + gx,   gx = tx * d + sx,
// so that consecutive ids start at consecutive pixels; the sub-grid ROWS stay apart (interleaving them too,
// t = (b * th * d + ty * d + sy) * tw * d + gx, was measured: a third of the gain at d = 4).  Both forms
// enumerate the same (b, sy, sx, ty, tx) set on [0, T); for d = 1 they coincide.
__host__ __device__ __forceinline__ void wino_tile(const WinoGeom &g, long long t, int &b, int &sy, int &sx, int &ty, int &tx)
{
    if (g.interleaved) {
        const int rw = g.tw * g.d;
        const int gx = (int)(t % rw); t /= rw;
        sx = gx % g.d; tx = gx / g.d;
        ty = (int)(t % g.th); t /= g.th;
        sy = (int)(t % g.d);
        b = (int)(t / g.d);
        return;
    }
    tx = (int)(t % g.tw); t /= g.tw;
    ty = (int)(t % g.th); t /= g.th;
    sx = (int)(t % g.d); t /= g.d;
    sy = (int)(t % g.d);
    b = (int)(t / g.d);
}

__device__ __forceinline__ unsigned wino_absmax_bits(float4 v) { return max(max(__float_as_uint(v.x) & 0x7fffffffu, __float_as_uint(v.y) & 0x7fffffffu), max(__float_as_uint(v.z) & 0x7fffffffu, __float_as_uint(v.w) & 0x7fffffffu)); }
__device__ __forceinline__ float4 operator+(float4 a, float4 b) { return make_float4(a.x + b.x, a.y + b.y, a.z + b.z, a.w + b.w); }
__device__ __forceinline__ float4 operator-(float4 a, float4 b) { return make_float4(a.x - b.x, a.y - b.y, a.z - b.z, a.w - b.w); }
__device__ __forceinline__ float4 operator*(float s, float4 a) { return make_float4(s * a.x, s * a.y, s * a.z, s * a.w); }
template <typename V> __device__ __forceinline__ V wino_zero();
template <> __device__ __forceinline__ float4 wino_zero<float4>() { return make_float4(0.f, 0.f, 0.f, 0.f); }
__device__ __forceinline__ float4 wino_relu(float4 v) { return make_float4(fmaxf(v.x, 0.f), fmaxf(v.y, 0.f), fmaxf(v.z, 0.f), fmaxf(v.w, 0.f)); }

// y = B^T x for a 6-vector
template <typename V>
__device__ __forceinline__ void wino4_bt(const V (&x)[6], V (&y)[6])
{
    y[0] = 2.0f * (x[0] + x[4]) + 3.0f * (x[3] - x[1]) - 4.0f * x[2];
    y[1] = 2.0f * (x[4] - x[1]) + x[2] + 5.0f * x[3];
    y[2] = 5.0f * x[2] - 2.0f * (x[1] + x[4]) - x[3];
    y[3] = 2.0f * (x[1] - x[3]) + x[2] - x[4];
    y[4] = (x[1] - x[3]) + 2.0f * (x[4] - x[2]);
    y[5] = 2.0f * (x[1] + x[5]) + 3.0f * (x[4] - x[2]) - 4.0f * x[3];
}

// y = A^T x: 4 outputs from 6
template <typename V>
__device__ __forceinline__ void wino4_at(const V (&x)[6], V (&y)[4])
{
    y[0] = ((x[0] + x[1]) + x[2]) + (x[3] + x[4]);
    y[1] = (x[1] - x[2]) + (0.5f * x[3] - 2.0f * x[4]);
    y[2] = (x[1] + x[2]) + (0.25f * x[3] + 4.0f * x[4]);
    y[3] = ((x[1] - x[2]) + (0.125f * x[3] - 8.0f * x[4])) + x[5];
}

struct WinoScale { float c[36]; };

__device__ __forceinline__ int wino_amax_exp(unsigned bits)
{
    int e = (int)(bits >> 23) - 127;
    e = e < -100 ? -100 : (e > 100 ? 100 : e);
    return bits == 0u ? 0 : e;
}
__device__ __forceinline__ float wino_pow2(int k) { return __uint_as_float((unsigned)(127 + k) << 23); }

// The two half-precision planes of a scaled float32 pair (spa_gemm16.hip): h = rn16(x * sc), l = rn16(x * sc - h), each ONE
// mixed-precision fma per element (sc a power of two: product and difference are exact in float32, the conversion is the
// only rounding).  Element 0 in the low half of the word.  sc must be wave-uniform.
__device__ __forceinline__ unsigned wino_split_h(float x0, float x1, float sc)
{
    unsigned h;
    asm volatile("v_fma_mixlo_f16 %0, %1, %3, 0 op_sel_hi:[0,0,0]\n\t"
                 "v_fma_mixhi_f16 %0, %2, %3, 0 op_sel_hi:[0,0,0]"
                 : "=&v"(h) : "v"(x0), "v"(x1), "s"(sc));
    return h;
}
__device__ __forceinline__ unsigned wino_split_l(float x0, float x1, float sc, unsigned h)
{
    unsigned l;
    asm volatile("v_fma_mixlo_f16 %0, %1, %3, -%4 op_sel_hi:[0,0,1]\n\t"
                 "v_fma_mixhi_f16 %0, %2, %3, -%4 op_sel:[0,0,1] op_sel_hi:[0,0,1]"
                 : "=&v"(l) : "v"(x0), "v"(x1), "s"(sc), "v"(h));
    return l;
}
// the value of the neighbouring lane (lane ^ 1)
__device__ __forceinline__ unsigned wino_lane_swap(unsigned v)
{
    return (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0xB1 /* quad_perm [1, 0, 3, 2] */, 0xF, 0xF, false);
}
// exponent sum p_i + p_j of Winograd position z = 6 i + j (p = 4 4 4 3 3 4, spa_wino.hip)
__host__ __device__ __forceinline__ int wino4_psum(int z)
{
    const int zi = z / 6, zj = z - zi * 6;
    return ((0x433444 >> (4 * zi)) & 15) + ((0x433444 >> (4 * zj)) & 15);
}

// The numbering of a layer of dilation d: interleaved from dilation 4 on.  Measured per 30 images of a 128 x 256 map
// (profiles/r8_wino_operands_ab.txt): at d = 4 the input transform of a 512-channel layer 1.53 -> 1.34 ms and the output
// transform 1.78 -> 1.72; at d = 2 nothing beyond the spread at 256 channels and the input transform 0.04 ms SLOWER at 512 —
// there the spacing costs little, and interleaving moves the two halo columns that horizontally adjacent tiles of a sub-grid
// share from one workgroup (L1) to workgroups d tiles apart (L2).
static inline int wino_interleave(int d) { return d > 2; }

// F(4x4,3x3) tiling of the sub-grids of a dilation (host)
static inline void wino4_geom(int B, int H, int W, int d, WinoGeom *g)
{
    g->B = B; g->H = H; g->W = W; g->d = d; g->interleaved = wino_interleave(d);
    const int hs = (H + d - 1) / d, ws = (W + d - 1) / d;
    g->th = (hs + 3) / 4; g->tw = (ws + 3) / 4;
    g->T = (long long)B * d * d * g->th * g->tw;
}
