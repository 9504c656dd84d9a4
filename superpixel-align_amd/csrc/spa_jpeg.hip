// The demo movie's JPEG frames, entropy-coded where the blended frame is (MjpegAviWriter's Pillow encode of
// utils/create_movie.py's frames).  The format is fixed in include/spalign.h (spa_jpeg_encode_rgb8) and restated on the
// host in jpeg.py (encode_host): baseline sequential, YCbCr 4:2:0, the quality-75 tables, restart intervals of Ri MCUs.
// An interval starts from zero predictors and ends on a byte, so it is a unit of work that shares nothing:
//
//   k_jpeg_transform  one wave per MCU: colour, chroma averaging, the integer DCT, quantisation -> zigzag int16
//   k_jpeg_count      one lane per interval: the interval's stuffed byte count, its marker included
//   k_jpeg_scan       one workgroup per image: exclusive prefix sum of the byte counts, nbytes
//   k_jpeg_emit       one lane per interval: the same walk again, into the bytes
//
// Both walks go through jpg_walk_interval and JpgSink::byte, so the counted bytes are the emitted bytes by
// construction.  Every byte has one writer: no atomics, nothing is zeroed, and no byte at or past nbytes is touched.
#include "spa_common.h"

#define JPG_SCAN_THREADS 256
#define JPG_MCU_COEFS 384            // 6 blocks of 64
#define JPG_TAB_STRIDE 272           // per component class: 256 AC entries, then 16 DC entries

// ---- tables ------------------------------------------------------------------------------------------------------
// zigzag position of natural index 8 * v + u
__constant__ uint8_t JPG_ZZ_POS[64] = {
    0, 1, 5, 6, 14, 15, 27, 28, 2, 4, 7, 13, 16, 26, 29, 42, 3, 8, 12, 17, 25, 30, 41, 43, 9, 11, 18, 24, 31, 40, 44, 53,
    10, 19, 23, 32, 39, 45, 52, 54, 20, 22, 33, 38, 46, 51, 55, 60, 21, 34, 37, 47, 50, 56, 59, 61, 35, 36, 48, 49, 57,
    58, 62, 63};
// quantisation at quality 75, zigzag order: luminance, chrominance
__constant__ uint8_t JPG_Q[2][64] = {
    {8, 6, 6, 7, 6, 5, 8, 7, 7, 7, 9, 9, 8, 10, 12, 20, 13, 12, 11, 11, 12, 25, 18, 19, 15, 20, 29, 26, 31, 30, 29, 26,
     28, 28, 32, 36, 46, 39, 32, 34, 44, 35, 28, 28, 40, 55, 41, 44, 48, 49, 52, 52, 52, 31, 39, 57, 61, 56, 50, 60, 46,
     51, 52, 50},
    {9, 9, 9, 12, 11, 12, 24, 13, 13, 24, 50, 33, 28, 33, 50, 50, 50, 50, 50, 50, 50, 50, 50, 50, 50, 50, 50, 50, 50,
     50, 50, 50, 50, 50, 50, 50, 50, 50, 50, 50, 50, 50, 50, 50, 50, 50, 50, 50, 50, 50, 50, 50, 50, 50, 50, 50, 50, 50,
     50, 50, 50, 50, 50, 50}};
// the standard Huffman tables: codes per length 1..16, then the symbols in code order.  DC luminance, AC luminance,
// DC chrominance, AC chrominance
__constant__ uint8_t JPG_BITS[4][16] = {
    {0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0},
    {0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7d},
    {0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0},
    {0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77}};
__constant__ uint8_t JPG_DC_VALS[12] = {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11};
__constant__ uint8_t JPG_AC_VALS[2][162] = {
    {0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71, 0x14,
     0x32, 0x81, 0x91, 0xa1, 0x08, 0x23, 0x42, 0xb1, 0xc1, 0x15, 0x52, 0xd1, 0xf0, 0x24, 0x33, 0x62, 0x72, 0x82, 0x09,
     0x0a, 0x16, 0x17, 0x18, 0x19, 0x1a, 0x25, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x34, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a,
     0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65,
     0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88,
     0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9,
     0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca,
     0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe1, 0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea,
     0xf1, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa},
    {0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22, 0x32,
     0x81, 0x08, 0x14, 0x42, 0x91, 0xa1, 0xb1, 0xc1, 0x09, 0x23, 0x33, 0x52, 0xf0, 0x15, 0x62, 0x72, 0xd1, 0x0a, 0x16,
     0x24, 0x34, 0xe1, 0x25, 0xf1, 0x17, 0x18, 0x19, 0x1a, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x35, 0x36, 0x37, 0x38, 0x39,
     0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64,
     0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x82, 0x83, 0x84, 0x85, 0x86,
     0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7,
     0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8,
     0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9,
     0xea, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa}};

// ---- the transform -----------------------------------------------------------------------------------------------
// out[u] = sum_x T[u][x] * s[x] with SPA_JPEG_DCT's rows.  Row u is even (odd) about its middle for even (odd) u, so
// the sums run over s[x] + s[7-x] (s[x] - s[7-x]): the same integers, exactly, in half the products.
__device__ __forceinline__ void jpg_dct8(const int (&s)[8], int (&o)[8])
{
    const int e0 = s[0] + s[7], e1 = s[1] + s[6], e2 = s[2] + s[5], e3 = s[3] + s[4];
    const int d0 = s[0] - s[7], d1 = s[1] - s[6], d2 = s[2] - s[5], d3 = s[3] - s[4];
    o[0] = 2896 * (e0 + e1 + e2 + e3);
    o[4] = 2896 * (e0 - e1 - e2 + e3);
    o[2] = 3784 * (e0 - e3) + 1567 * (e1 - e2);
    o[6] = 1567 * (e0 - e3) - 3784 * (e1 - e2);
    o[1] = 4017 * d0 + 3406 * d1 + 2276 * d2 + 799 * d3;
    o[3] = 3406 * d0 - 799 * d1 - 4017 * d2 - 2276 * d3;
    o[5] = 2276 * d0 - 4017 * d1 + 799 * d2 + 3406 * d3;
    o[7] = 799 * d0 - 2276 * d1 + 3406 * d2 - 4017 * d3;
}

__device__ __forceinline__ void jpg_unpack8(const uint4 v, int (&s)[8])
{
    s[0] = (int)(short)(v.x & 0xffffu); s[1] = (int)v.x >> 16;
    s[2] = (int)(short)(v.y & 0xffffu); s[3] = (int)v.y >> 16;
    s[4] = (int)(short)(v.z & 0xffffu); s[5] = (int)v.z >> 16;
    s[6] = (int)(short)(v.w & 0xffffu); s[7] = (int)v.w >> 16;
}

// One wave per MCU, four MCUs per workgroup; a wave's 768 bytes of LDS are its own.  Lane l holds 4 pixels of row l/4
// of the 16x16 tile.  The level-shifted samples go to LDS as int16 [block][y][x]; 48 lanes take one block row each
// (one 16-byte read) and write the row pass transposed, [block][u][y], so that the column pass reads 16 bytes too;
// its 48 lanes quantise and scatter into zigzag order, and the wave stores the MCU's 768 bytes as 3 dwords per lane.
template <bool ALIGNED>
__global__ __launch_bounds__(256) void k_jpeg_transform(const uint8_t *__restrict__ rgb, int H, int W, long long total,
                                                        int16_t *__restrict__ coef)
{
    __shared__ __attribute__((aligned(16))) int16_t lds[4][JPG_MCU_COEFS];
    const int wave = threadIdx.x >> 6, l = threadIdx.x & 63;
    const long long m_raw = (long long)blockIdx.x * 4 + wave;
    const bool live = m_raw < total;
    const long long m = live ? m_raw : total - 1;        // an idle wave repeats the last MCU and stores nothing
    const int mx = W >> 4, n_mcu = mx * (H >> 4);
    const int b = (int)(m / n_mcu), k = (int)(m - (long long)b * n_mcu);
    const int y0 = (k / mx) << 4, x0 = (k % mx) << 4;
    int16_t *t = lds[wave];

    // colour and chroma
    const int r = l >> 2, cg = l & 3;
    const uint8_t *p = rgb + (((long long)b * H + y0 + r) * W + x0 + 4 * cg) * 3;
    uint32_t w[3];
    if (ALIGNED) {
        w[0] = ((const uint32_t *)p)[0]; w[1] = ((const uint32_t *)p)[1]; w[2] = ((const uint32_t *)p)[2];
    } else {
        w[0] = w[1] = w[2] = 0u;
#pragma unroll
        for (int i = 0; i < 12; ++i) w[i >> 2] |= (uint32_t)p[i] << (8 * (i & 3));
    }
    int yv[4], cb[4], cr[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int R = (int)((w[(3 * i) >> 2] >> (8 * ((3 * i) & 3))) & 255u);
        const int G = (int)((w[(3 * i + 1) >> 2] >> (8 * ((3 * i + 1) & 3))) & 255u);
        const int B = (int)((w[(3 * i + 2) >> 2] >> (8 * ((3 * i + 2) & 3))) & 255u);
        yv[i] = (19595 * R + 38470 * G + 7471 * B + 32768) >> 16;
        cb[i] = (-11059 * R - 21709 * G + 32768 * B + 8421375) >> 16;
        cr[i] = (32768 * R - 27439 * G - 5329 * B + 8421375) >> 16;
    }
    {
        const int blk = ((r >> 3) << 1) | (cg >> 1);
        uint2 v;
        v.x = (uint32_t)((yv[0] - 128) & 0xffff) | ((uint32_t)(yv[1] - 128) << 16);
        v.y = (uint32_t)((yv[2] - 128) & 0xffff) | ((uint32_t)(yv[3] - 128) << 16);
        *(uint2 *)(t + blk * 64 + (r & 7) * 8 + (cg & 1) * 4) = v;
    }
    {
        // the row below (above) is 4 lanes on
        int h[4] = {cb[0] + cb[1], cb[2] + cb[3], cr[0] + cr[1], cr[2] + cr[3]};
#pragma unroll
        for (int i = 0; i < 4; ++i) h[i] = ((h[i] + __shfl_xor(h[i], 4) + 2) >> 2) - 128;
        if (!(r & 1)) {
            const int at = (r >> 1) * 8 + 2 * cg;
            *(uint32_t *)(t + 4 * 64 + at) = (uint32_t)(h[0] & 0xffff) | ((uint32_t)h[1] << 16);
            *(uint32_t *)(t + 5 * 64 + at) = (uint32_t)(h[2] & 0xffff) | ((uint32_t)h[3] << 16);
        }
    }
    __syncthreads();

    // row pass
    const int blk = l >> 3, j = l & 7;                   // lanes 0..47: a block and one of its rows, then columns
    int s[8], o[8];
    if (l < 48) {
        jpg_unpack8(*(const uint4 *)(t + blk * 64 + j * 8), s);
        jpg_dct8(s, o);
    }
    __syncthreads();
    if (l < 48) {
#pragma unroll
        for (int u = 0; u < 8; ++u) t[blk * 64 + u * 8 + j] = (int16_t)((o[u] + 1024) >> 11);
    }
    __syncthreads();

    // column pass and quantisation: q = sign(b) * ((|b| + d/2) div d) with d = Q << 15, d/2 = Q << 14; a floor
    // division by Q * 2^15 is the floor division by Q of the floor division by 2^15, so no 64-bit division
    if (l < 48) {
        jpg_unpack8(*(const uint4 *)(t + blk * 64 + j * 8), s);
        jpg_dct8(s, o);
    }
    __syncthreads();
    if (l < 48) {
        const int cls = blk < 4 ? 0 : 1;
#pragma unroll
        for (int v = 0; v < 8; ++v) {
            const unsigned pos = JPG_ZZ_POS[v * 8 + j];
            const unsigned Q = JPG_Q[cls][pos];
            const unsigned a = (unsigned)(o[v] < 0 ? -o[v] : o[v]);
            const int q = (int)(((a + (Q << 14)) >> 15) / Q);
            t[blk * 64 + pos] = (int16_t)(o[v] < 0 ? -q : q);
        }
    }
    __syncthreads();
    if (live) {
        uint32_t *dst = (uint32_t *)(coef + m * JPG_MCU_COEFS);
        const uint32_t *src = (const uint32_t *)t;
        dst[l] = src[l]; dst[l + 64] = src[l + 64]; dst[l + 128] = src[l + 128];
    }
}

// ---- entropy coding ----------------------------------------------------------------------------------------------
// tab[class][symbol] = code << 5 | length; AC symbols at 0..255, DC categories at 256..267
__device__ __forceinline__ void jpg_build_tables(uint32_t (*tab)[JPG_TAB_STRIDE])
{
    for (int i = threadIdx.x; i < 2 * JPG_TAB_STRIDE; i += blockDim.x) (&tab[0][0])[i] = 0u;
    __syncthreads();
    for (int tb = 0; tb < 4; ++tb) {
        const int n = (tb & 1) ? 162 : 12;
        for (int k = threadIdx.x; k < n; k += blockDim.x) {
            unsigned code = 0, first = 0, len = 1;
            for (; len <= 16u; ++len) {
                const unsigned cnt = JPG_BITS[tb][len - 1];
                if ((unsigned)k < first + cnt) { code += (unsigned)k - first; break; }
                code = (code + cnt) << 1;
                first += cnt;
            }
            const unsigned sym = (tb & 1) ? JPG_AC_VALS[tb >> 1][k] : 256u + JPG_DC_VALS[k];
            tab[tb >> 1][sym] = (code << 5) | len;
        }
    }
    __syncthreads();
}

// The bytes of one interval.  Bits enter most-significant first; a 0x00 follows every 0xFF that the bits make.  EMIT:
// bytes collect in a dword that is stored whole once it is full and 4-byte aligned (all four bytes are this
// interval's), byte by byte at the interval's ragged ends; nothing at or past lim is stored.  Otherwise they are
// counted.  pos: the bytes so far.
template <bool EMIT> struct JpgSink {
    uint8_t *base;                       // EMIT: the aligned address that holds byte 0 of w
    long long room;                      // EMIT: bytes from base to the end of the image's stride
    unsigned long long acc;              // bits not yet in a byte: the low nb (< 8) bits of acc
    uint32_t nb;
    uint32_t w, on, lead;                // EMIT: the collected bytes; how many; how many of them are not ours
    uint32_t pos;

    __device__ __forceinline__ void open(uint8_t *at, long long room_)
    {
        acc = 0ull; nb = 0u; pos = 0u; w = 0u; on = 0u; lead = 0u;
        if (EMIT) {
            lead = (uint32_t)((uintptr_t)at & 3);
            base = at - lead; room = room_ + lead; on = lead;
        }
    }
    __device__ __forceinline__ void flush(uint32_t upto)
    {
        if (lead == 0u && upto == 4u) {
            if (room >= 4) *(uint32_t *)base = w;
        } else {
            for (uint32_t i = lead; i < upto; ++i)
                if ((long long)i < room) base[i] = (uint8_t)(w >> (8u * i));
        }
        base += 4; room -= 4; w = 0u; on = 0u; lead = 0u;
    }
    __device__ __forceinline__ void byte(uint32_t b)
    {
        ++pos;
        if (EMIT) {
            w |= b << (8u * on);
            if (++on == 4u) flush(4u);
        }
    }
    // at most 32 bits: a code and the value bits behind it go in together
    __device__ __forceinline__ void put(uint32_t code, uint32_t len)
    {
        acc = (acc << len) | code;
        nb += len;
        while (nb >= 8u) {
            nb -= 8u;
            const uint32_t b = (uint32_t)(acc >> nb) & 255u;
            byte(b);
            if (b == 255u) byte(0u);
        }
    }
    __device__ __forceinline__ void close()
    {
        if (EMIT && on > lead) flush(on);
    }
};

template <class Sink>
__device__ __forceinline__ void jpg_ac(Sink &s, const uint32_t *__restrict__ tab, int v, uint32_t &run)
{
    if (v == 0) { ++run; return; }
    while (run > 15u) { const uint32_t z = tab[0xF0]; s.put(z >> 5, z & 31u); run -= 16u; }
    const uint32_t cat = 32u - (uint32_t)__clz(v < 0 ? -v : v);
    const uint32_t e = tab[(run << 4) | cat];
    s.put(((e >> 5) << cat) | ((uint32_t)(v < 0 ? v - 1 : v) & ((1u << cat) - 1u)), (e & 31u) + cat);
    run = 0u;
}

// one block: 64 zigzag coefficients at c (16-byte aligned) -> the DC difference from pred, the AC run-lengths, EOB
template <class Sink>
__device__ __forceinline__ void jpg_walk_block(Sink &s, const uint32_t *__restrict__ tab, const uint4 *__restrict__ c,
                                               int &pred)
{
    uint32_t run = 0u;
    for (int q = 0; q < 8; ++q) {
        const uint4 v = c[q];
        const uint32_t d[4] = {v.x, v.y, v.z, v.w};
        if (q == 0) {
            const int dc = (int)(short)(d[0] & 0xffffu), diff = dc - pred;
            pred = dc;
            const uint32_t cat = 32u - (uint32_t)__clz(diff < 0 ? -diff : diff);
            const uint32_t e = tab[256u + cat];
            s.put(((e >> 5) << cat) | ((uint32_t)(diff < 0 ? diff - 1 : diff) & ((1u << cat) - 1u)), (e & 31u) + cat);
        } else if ((d[0] | d[1] | d[2] | d[3]) == 0u) {
            run += 8u;
            continue;
        }
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            if (i == 0 && q == 0) continue;
            jpg_ac(s, tab, (i & 1) ? (int)d[i >> 1] >> 16 : (int)(short)(d[i >> 1] & 0xffffu), run);
        }
    }
    if (run) { const uint32_t e = tab[0]; s.put(e >> 5, e & 31u); }
}

struct JpgScan {
    int n_mcu, n_int, Ri;                // per image
    long long intervals;                 // B * n_int
};

// interval g of the call: the MCUs [k Ri, min((k+1) Ri, n_mcu)) of its image, padded with 1-bits, then FF D0+(k mod 8)
// unless it is the image's last
template <class Sink>
__device__ __forceinline__ void jpg_walk_interval(Sink &s, const JpgScan &g, int k, const int16_t *__restrict__ coef,
                                                  const uint32_t (*tab)[JPG_TAB_STRIDE])
{
    const int lo = k * g.Ri, hi = lo + g.Ri < g.n_mcu ? lo + g.Ri : g.n_mcu;
    int pY = 0, pB = 0, pR = 0;
    for (int m = lo; m < hi; ++m) {
        const uint4 *c = (const uint4 *)(coef + (long long)m * JPG_MCU_COEFS);
        for (int j = 0; j < 4; ++j) jpg_walk_block(s, tab[0], c + 8 * j, pY);
        jpg_walk_block(s, tab[1], c + 32, pB);
        jpg_walk_block(s, tab[1], c + 40, pR);
    }
    if (s.nb) s.put((1u << (8u - s.nb)) - 1u, 8u - s.nb);
    if (k + 1 < g.n_int) { s.byte(0xFFu); s.byte(0xD0u + ((uint32_t)k & 7u)); }
    s.close();
}

__global__ __launch_bounds__(64) void k_jpeg_count(JpgScan g, const int16_t *__restrict__ coef,
                                                   uint32_t *__restrict__ lens)
{
    __shared__ uint32_t tab[2][JPG_TAB_STRIDE];
    jpg_build_tables(tab);
    const long long i = (long long)blockIdx.x * 64 + threadIdx.x;
    if (i >= g.intervals) return;
    const int b = (int)(i / g.n_int), k = (int)(i - (long long)b * g.n_int);
    JpgSink<false> s;
    s.open(nullptr, 0);
    jpg_walk_interval(s, g, k, coef + (long long)b * g.n_mcu * JPG_MCU_COEFS, tab);
    lens[i] = s.pos;
}

// One workgroup per image: thread t sums the intervals [t*chunk, (t+1)*chunk), thread 0 scans the 256 partial sums,
// and every thread turns its intervals' lengths into offsets, in place.
__global__ __launch_bounds__(JPG_SCAN_THREADS) void k_jpeg_scan(int n_int, uint32_t *__restrict__ lens,
                                                                int32_t *__restrict__ nbytes)
{
    __shared__ uint32_t part[JPG_SCAN_THREADS];
    const int b = blockIdx.x, t = threadIdx.x;
    uint32_t *mine = lens + (long long)b * n_int;
    const int chunk = (n_int + JPG_SCAN_THREADS - 1) / JPG_SCAN_THREADS;
    const int lo = t * chunk < n_int ? t * chunk : n_int, hi = lo + chunk < n_int ? lo + chunk : n_int;
    uint32_t sum = 0u;
    for (int i = lo; i < hi; ++i) sum += mine[i];
    part[t] = sum;
    __syncthreads();
    if (t == 0) {
        uint32_t run = 0u;
        for (int i = 0; i < JPG_SCAN_THREADS; ++i) { const uint32_t v = part[i]; part[i] = run; run += v; }
        nbytes[b] = (int32_t)run;
    }
    __syncthreads();
    uint32_t off = part[t];
    for (int i = lo; i < hi; ++i) { const uint32_t v = mine[i]; mine[i] = off; off += v; }
}

__global__ __launch_bounds__(64) void k_jpeg_emit(JpgScan g, const int16_t *__restrict__ coef,
                                                  const uint32_t *__restrict__ offs, uint8_t *__restrict__ out,
                                                  long long out_stride)
{
    __shared__ uint32_t tab[2][JPG_TAB_STRIDE];
    jpg_build_tables(tab);
    const long long i = (long long)blockIdx.x * 64 + threadIdx.x;
    if (i >= g.intervals) return;
    const int b = (int)(i / g.n_int), k = (int)(i - (long long)b * g.n_int);
    const uint32_t at = offs[i];
    JpgSink<true> s;
    s.open(out + (long long)b * out_stride + at, out_stride - (long long)at);
    jpg_walk_interval(s, g, k, coef + (long long)b * g.n_mcu * JPG_MCU_COEFS, tab);
}

extern "C" int64_t spa_jpeg_scan_bound(int32_t H, int32_t W, int32_t Ri)
{
    if (H <= 0 || W <= 0 || (H & 15) || (W & 15) || Ri < 1) return 0;
    const int64_t n_mcu = (int64_t)(H >> 4) * (W >> 4);
    const int64_t n_int = (n_mcu + Ri - 1) / Ri;
    return 2 * (int64_t)SPA_JPEG_MCU_BYTES_MAX * n_mcu + 2 * (n_int - 1);
}

extern "C" int spa_jpeg_encode_rgb8(spa_ctx *ctx, const uint8_t *rgb, int32_t B, int32_t H, int32_t W, int32_t Ri,
                                    int16_t *coef_ws, uint8_t *out, int64_t out_stride, int32_t *nbytes, void *stream)
{
    SPA_ARG(ctx && rgb && coef_ws && out && nbytes);
    SPA_ARG(B > 0 && H > 0 && W > 0 && (H & 15) == 0 && (W & 15) == 0 && Ri >= 1);
    SPA_ARG(((uintptr_t)coef_ws & 15) == 0);
    const int64_t bound = spa_jpeg_scan_bound(H, W, Ri);
    if (bound > 0x7fffffffLL) {
        spa_set_error("spa_jpeg_encode_rgb8: the scan of a %d x %d frame may need %lld bytes, more than nbytes holds", H,
                      W, (long long)bound);
        return SPA_ERR_ARG;
    }
    if (out_stride < bound) {
        spa_set_error("spa_jpeg_encode_rgb8: out_stride %lld is below spa_jpeg_scan_bound(%d, %d, %d) = %lld",
                      (long long)out_stride, H, W, Ri, (long long)bound);
        return SPA_ERR_ARG;
    }
    JpgScan g;
    g.n_mcu = (H >> 4) * (W >> 4);                       // < 2^23: the bound fits 31 bits
    g.Ri = Ri < g.n_mcu ? Ri : g.n_mcu;
    g.n_int = (g.n_mcu + g.Ri - 1) / g.Ri;
    g.intervals = (long long)B * g.n_int;
    const long long total = (long long)B * g.n_mcu;
    SPA_ARG(total <= 0x7fffffffLL * 4);
    uint32_t *lens;
    int rc = spa_ws_reserve(ctx, WS_JPEG_INTERVALS, (size_t)g.intervals * 4, (void **)&lens);
    if (rc != SPA_OK) return rc;
    hipStream_t s = spa_stream(stream);
    const unsigned gt = (unsigned)((total + 3) / 4), gi = (unsigned)((g.intervals + 63) / 64);
    if (((uintptr_t)rgb & 3) == 0) hipLaunchKernelGGL(k_jpeg_transform<true>, dim3(gt), dim3(256), 0, s, rgb, H, W, total, coef_ws);
    else hipLaunchKernelGGL(k_jpeg_transform<false>, dim3(gt), dim3(256), 0, s, rgb, H, W, total, coef_ws);
    hipLaunchKernelGGL(k_jpeg_count, dim3(gi), dim3(64), 0, s, g, (const int16_t *)coef_ws, lens);
    hipLaunchKernelGGL(k_jpeg_scan, dim3(B), dim3(JPG_SCAN_THREADS), 0, s, g.n_int, lens, nbytes);
    hipLaunchKernelGGL(k_jpeg_emit, dim3(gi), dim3(64), 0, s, g, (const int16_t *)coef_ws, (const uint32_t *)lens, out,
                       (long long)out_stride);
    SPA_LAUNCH_CHECK();
    return SPA_OK;
}
