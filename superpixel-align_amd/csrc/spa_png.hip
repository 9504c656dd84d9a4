// The label PNG's compressed payload, made where the mask is (cv.imwrite(save_fn, mask) of
// utils/apply_spalign_kmeans.py:145 and utils/create_demovideo.py:64).  The format is fixed in include/spalign.h
// (spa_png_deflate_u8) and restated on the host in png.py (deflate_rle_host): PNG's Up filter, then ONE fixed-Huffman
// deflate block whose tokens are the runs of equal bytes of every scanline, matched at distance 1.  A scanline's tokens
// depend on that scanline and the one above it only, so a row is a unit of work:
//
//   k_png_count  one lane per row: the row's bit count and its Adler-32 partial sums
//   k_png_scan   one workgroup per image: exclusive prefix sum of the bit counts, nbytes, adler
//   k_png_emit   one lane per row: the same walk again, into a 64-bit bit accumulator
//
// Rows meet inside bytes.  Every scanline opens with the literal 2 (the filter byte), eight bits that the row before it
// knows, so the row that ENDS inside a byte completes it with the first bits of that literal and the next row skips
// them: every byte has one writer, nothing is zeroed, no atomics, and no byte at or past nbytes is touched.
// Both walks go through png_walk_row and png_run_tokens, so the counted bits are the emitted bits by construction.
#include "spa_common.h"

#define PNG_ADLER_MOD 65521u
#define PNG_ROW_OPEN 0x4Cu          // literal 2 under the fixed code: 0x30 + 2 = 00110010, most-significant bit first
#define PNG_SCAN_THREADS 256

// ---- tokens ------------------------------------------------------------------------------------------------------
// literal v -> (bits, least-significant first; length)
__device__ __forceinline__ unsigned png_lit(unsigned v, unsigned &len)
{
    if (v < 144u) { len = 8; return __brev(0x30u + v) >> 24; }
    len = 9;
    return __brev(0x190u + (v - 144u)) >> 23;
}

// match of length L (3..258) at distance 1: the length symbol, its extra bits, the 5-bit distance code 0
__device__ __forceinline__ unsigned png_match(unsigned L, unsigned &len)
{
    unsigned sym, e = 0, extra = 0;
    if (L <= 10u) sym = 254u + L;
    else if (L == 258u) sym = 285u;
    else {
        const unsigned m = L - 3u;                       // 8..254
        e = 29u - (unsigned)__clz(m);                    // floor(log2 m) - 2: 1..5
        sym = 261u + 4u * e + ((m >> e) & 3u);
        extra = m & ((1u << e) - 1u);
    }
    unsigned hl, code;
    if (sym < 280u) { hl = 7; code = __brev(sym - 256u) >> 25; }
    else { hl = 8; code = __brev(0xC0u + (sym - 280u)) >> 24; }
    len = hl + e + 5u;
    return code | (extra << hl);
}

// a run of n bytes of value v: the literal, matches of at most 258 while 3 or more bytes remain, then literals
template <class Sink> __device__ __forceinline__ void png_run_tokens(Sink &s, unsigned v, unsigned n)
{
    unsigned len, bits = png_lit(v, len);
    s.put(bits, len);
    unsigned r = n - 1u;
    while (r >= 3u) {
        const unsigned L = r < 258u ? r : 258u;
        unsigned ml, mb = png_match(L, ml);
        s.put(mb, ml);
        r -= L;
    }
    while (r) { s.put(bits, len); --r; }
}

// ---- the two sinks -----------------------------------------------------------------------------------------------
struct PngCount {
    unsigned long long bits, a, b;       // a, b: Adler-32 sums of this row alone (from 0, 0), reduced lazily
    __device__ __forceinline__ void put(unsigned, unsigned len) { bits += len; }
    __device__ __forceinline__ void run(unsigned v, unsigned n)
    {
        // n bytes v after sums (a, b):  b += n*a + v*n(n+1)/2,  a += n*v
        const unsigned nm = n % PNG_ADLER_MOD;
        const unsigned tri = n < 65536u ? (n * (n + 1u) / 2u) % PNG_ADLER_MOD
                                        : (unsigned)(((unsigned long long)n * (n + 1ull) / 2ull) % PNG_ADLER_MOD);
        b += (unsigned long long)nm * a + (unsigned long long)v * tri;     // a < 2^41, nm < 2^16
        a += (unsigned long long)v * nm;
        if (a >> 40) a %= PNG_ADLER_MOD;
        if (b >> 62) b %= PNG_ADLER_MOD;
        png_run_tokens(*this, v, n);
    }
};

struct PngEmit {
    uint8_t *out;                        // the image's stream
    long long pos, lim;                  // next byte to write; nothing is stored at or past lim
    unsigned long long acc;
    unsigned nb, skip;                   // bits held; bits of the first token that the row before has written
    __device__ __forceinline__ void byte_out()
    {
        if (pos < lim) out[pos] = (uint8_t)acc;
        ++pos; acc >>= 8; nb -= 8u;
    }
    __device__ __forceinline__ void put(unsigned code, unsigned len)
    {
        acc |= (unsigned long long)code << nb;
        nb += len;
        if (skip) { acc >>= skip; nb -= skip; skip = 0; }
        while (nb >= 32u) {
            if ((((uintptr_t)(out + pos)) & 3) == 0) {
                if (pos + 4 <= lim) *(uint32_t *)(out + pos) = (uint32_t)acc;
                pos += 4; acc >>= 32; nb -= 32u;
            } else byte_out();
        }
    }
    __device__ __forceinline__ void run(unsigned v, unsigned n) { png_run_tokens(*this, v, n); }
};

// ---- the row walk ------------------------------------------------------------------------------------------------
// per-byte a - b mod 256 on four packed bytes
__device__ __forceinline__ uint32_t png_sub4(uint32_t a, uint32_t b)
{
    return ((a | 0x80808080u) - (b & 0x7f7f7f7fu)) ^ ((a ^ ~b) & 0x80808080u);
}

// The maximal runs of the scanline {2, cur[x] - prev[x] mod 256} go to s.run in order.  cur / prev: the source rows
// (prev NULL: the row above the image, zeros); VEC: the columns are the identity and both rows are 16-byte aligned;
// otherwise byte loads at col[x] (col NULL: x).
template <bool VEC, class Sink>
__device__ __forceinline__ void png_walk_row(const uint8_t *__restrict__ cur, const uint8_t *__restrict__ prev,
                                             const int32_t *__restrict__ col, int Wo, Sink &s)
{
    unsigned v = 2u, n = 1u;
    for (int x0 = 0; x0 < Wo; x0 += 16) {
        const int cnt = Wo - x0 < 16 ? Wo - x0 : 16;
        uint32_t w[4];
        if (VEC && cnt == 16) {
            const uint4 c = *(const uint4 *)(cur + x0);
            uint4 p = make_uint4(0u, 0u, 0u, 0u);
            if (prev) p = *(const uint4 *)(prev + x0);
            w[0] = png_sub4(c.x, p.x); w[1] = png_sub4(c.y, p.y); w[2] = png_sub4(c.z, p.z); w[3] = png_sub4(c.w, p.w);
        } else {
            w[0] = w[1] = w[2] = w[3] = 0u;
#pragma unroll
            for (int j = 0; j < 16; ++j) {
                const int x = x0 + j < Wo ? x0 + j : Wo - 1;            // past the row: a valid column, never used
                const int sx = col ? col[x] : x;
                const unsigned d = ((unsigned)cur[sx] - (prev ? (unsigned)prev[sx] : 0u)) & 255u;
                w[j >> 2] |= d << (8 * (j & 3));
            }
        }
        const uint32_t vv = v * 0x01010101u;
        if (cnt == 16 && w[0] == vv && w[1] == vv && w[2] == vv && w[3] == vv) { n += 16u; continue; }
        for (int j = 0; j < cnt; ++j) {
            const unsigned d = w[0] & 255u;
            w[0] = (w[0] >> 8) | (w[1] << 24); w[1] = (w[1] >> 8) | (w[2] << 24);
            w[2] = (w[2] >> 8) | (w[3] << 24); w[3] >>= 8;
            if (d == v) ++n;
            else { s.run(v, n); v = d; n = 1u; }
        }
    }
    s.run(v, n);
}

struct PngRows {
    const uint8_t *src; const int32_t *row_idx, *col_idx;
    int Hs, Ws, Ho, Wo;
    long long rows;                      // B * Ho
};

// row r of the call -> its image, and the source rows of scanline y and of the one above it
__device__ __forceinline__ void png_row_ptrs(const PngRows &g, long long r, int &b, int &y, const uint8_t *&cur,
                                             const uint8_t *&prev)
{
    b = (int)(r / g.Ho);
    y = (int)(r - (long long)b * g.Ho);
    const uint8_t *img = g.src + (long long)b * g.Hs * g.Ws;
    cur = img + (long long)(g.row_idx ? g.row_idx[y] : y) * g.Ws;
    prev = y ? img + (long long)(g.row_idx ? g.row_idx[y - 1] : y - 1) * g.Ws : nullptr;
}

// row r of the call, counted: its bits, and its Adler sums mod 65521
template <bool VEC>
__device__ __forceinline__ void png_count_row(const PngRows &g, long long r, unsigned long long *__restrict__ bits,
                                              uint32_t *__restrict__ s1, uint32_t *__restrict__ s2)
{
    int b, y;
    const uint8_t *cur, *prev;
    png_row_ptrs(g, r, b, y, cur, prev);
    PngCount c;
    c.bits = 0; c.a = 0; c.b = 0;
    png_walk_row<VEC>(cur, prev, g.col_idx, g.Wo, c);
    bits[r] = c.bits;
    s1[r] = (uint32_t)(c.a % PNG_ADLER_MOD);
    s2[r] = (uint32_t)(c.b % PNG_ADLER_MOD);
}

// row r of the call, written from its first bit bitoff[r] on (see the head of this file for who writes a shared byte)
template <bool VEC>
__device__ __forceinline__ void png_emit_row(const PngRows &g, long long r,
                                             const unsigned long long *__restrict__ bitoff, uint8_t *__restrict__ out,
                                             long long out_stride, long long lim)
{
    int b, y;
    const uint8_t *cur, *prev;
    png_row_ptrs(g, r, b, y, cur, prev);
    PngEmit e;
    e.out = out + (long long)b * out_stride;
    e.lim = lim;
    if (y == 0) {                        // BFINAL = 1, BTYPE = 01
        e.pos = 0; e.acc = 3ull; e.nb = 3u; e.skip = 0u;
    } else {
        const unsigned long long s = bitoff[r];
        const unsigned k = (unsigned)(s & 7ull);
        e.pos = (long long)(s >> 3) + (k ? 1 : 0);
        e.acc = 0ull; e.nb = 0u; e.skip = k ? 8u - k : 0u;
    }
    png_walk_row<VEC>(cur, prev, g.col_idx, g.Wo, e);
    if (y == g.Ho - 1) e.put(0u, 7u);    // symbol 256; the zero padding is the accumulator's
    while (e.nb >= 8u) e.byte_out();
    if (e.nb) {
        if (y != g.Ho - 1) e.acc |= (unsigned long long)PNG_ROW_OPEN << e.nb;      // the next row's opening bits
        e.nb = 8u;
        e.byte_out();
    }
}

// ---- kernels -----------------------------------------------------------------------------------------------------
template <bool VEC>
__global__ __launch_bounds__(64) void k_png_count(PngRows g, unsigned long long *__restrict__ bits,
                                                  uint32_t *__restrict__ s1, uint32_t *__restrict__ s2)
{
    const long long r = (long long)blockIdx.x * 64 + threadIdx.x;
    if (r < g.rows) png_count_row<VEC>(g, r, bits, s1, s2);
}

// One workgroup per image.  Thread t owns the rows [t*chunk, (t+1)*chunk): it sums their bit counts and composes their
// Adler sums (segment X then Y of lengths Lx, Ly:  s1 = s1x + s1y,  s2 = s2x + Ly*s1x + s2y, all mod 65521: exact, so
// the grouping does not change the value), thread 0 scans the 256 partials, and every thread turns its rows' counts
// into offsets.  bits[] holds each row's first bit afterwards; the stream's 3 header bits come first, the 7 bits of
// symbol 256 last.
__global__ __launch_bounds__(PNG_SCAN_THREADS) void k_png_scan(int Ho, int Wo, unsigned long long *__restrict__ bits,
                                                               const uint32_t *__restrict__ s1,
                                                               const uint32_t *__restrict__ s2,
                                                               int32_t *__restrict__ nbytes,
                                                               uint32_t *__restrict__ adler)
{
    __shared__ unsigned long long sh_bits[PNG_SCAN_THREADS];
    __shared__ uint32_t sh_s1[PNG_SCAN_THREADS], sh_s2[PNG_SCAN_THREADS], sh_len[PNG_SCAN_THREADS];
    const int b = blockIdx.x, t = threadIdx.x;
    const long long base = (long long)b * Ho;
    const int chunk = (Ho + PNG_SCAN_THREADS - 1) / PNG_SCAN_THREADS;
    const long long lo = (long long)t * chunk;
    const long long hi = lo + chunk < Ho ? lo + chunk : Ho;
    const unsigned rowlen = (unsigned)(((long long)Wo + 1) % PNG_ADLER_MOD);
    unsigned long long sum = 0;
    unsigned long long a = 0, bb = 0, len = 0;
    for (long long y = lo; y < hi; ++y) {
        sum += bits[base + y];
        bb = (bb + (unsigned long long)rowlen * a + s2[base + y]) % PNG_ADLER_MOD;
        a = (a + s1[base + y]) % PNG_ADLER_MOD;
        len = (len + rowlen) % PNG_ADLER_MOD;
    }
    sh_bits[t] = sum; sh_s1[t] = (uint32_t)a; sh_s2[t] = (uint32_t)bb; sh_len[t] = (uint32_t)len;
    __syncthreads();
    if (t == 0) {
        unsigned long long run = 3, A = 0, Bs = 0, L = 0;
        for (int i = 0; i < PNG_SCAN_THREADS; ++i) {
            const unsigned long long v = sh_bits[i];
            sh_bits[i] = run;
            run += v;
            Bs = (Bs + (unsigned long long)sh_len[i] * A + sh_s2[i]) % PNG_ADLER_MOD;
            A = (A + sh_s1[i]) % PNG_ADLER_MOD;
            L = (L + sh_len[i]) % PNG_ADLER_MOD;
        }
        nbytes[b] = (int32_t)((run + 7ull + 7ull) >> 3);
        // Adler-32 starts from a = 1, b = 0: a = 1 + sum d, b = N + sum (N - i) d
        adler[b] = (uint32_t)(((Bs + L) % PNG_ADLER_MOD) << 16) | (uint32_t)((A + 1ull) % PNG_ADLER_MOD);
    }
    __syncthreads();
    unsigned long long off = sh_bits[t];
    for (long long y = lo; y < hi; ++y) {
        const unsigned long long v = bits[base + y];
        bits[base + y] = off;
        off += v;
    }
}

template <bool VEC>
__global__ __launch_bounds__(64) void k_png_emit(PngRows g, const unsigned long long *__restrict__ bitoff,
                                                 uint8_t *__restrict__ out, long long out_stride, long long lim)
{
    const long long r = (long long)blockIdx.x * 64 + threadIdx.x;
    if (r < g.rows) png_emit_row<VEC>(g, r, bitoff, out, out_stride, lim);
}

extern "C" int64_t spa_png_deflate_bound(int32_t Ho, int32_t Wo)
{
    if (Ho <= 0 || Wo <= 0) return 0;
    const int64_t n = ((int64_t)Wo + 1) * (int64_t)Ho;
    if (n > (INT64_MAX - 17) / 9) return INT64_MAX;
    return (3 + 9 * n + 7 + 7) / 8;
}

extern "C" int spa_png_deflate_u8(spa_ctx *ctx, const uint8_t *src, int32_t B, int32_t Hs, int32_t Ws,
                                  const int32_t *row_idx, const int32_t *col_idx, int32_t Ho, int32_t Wo, uint8_t *out,
                                  int64_t out_stride, int32_t *nbytes, uint32_t *adler, void *stream)
{
    SPA_ARG(ctx && src && out && nbytes && adler);
    SPA_ARG(B > 0 && Hs > 0 && Ws > 0 && Ho > 0 && Wo > 0);
    SPA_ARG(row_idx || Ho == Hs);
    SPA_ARG(col_idx || Wo == Ws);
    const int64_t bound = spa_png_deflate_bound(Ho, Wo);
    if (bound > 0x7fffffffLL) {
        spa_set_error("spa_png_deflate_u8: a %d x %d image may need %lld bytes, more than an IDAT chunk's length field "
                      "holds", Ho, Wo, (long long)bound);
        return SPA_ERR_ARG;
    }
    if (out_stride < bound) {
        spa_set_error("spa_png_deflate_u8: out_stride %lld is below spa_png_deflate_bound(%d, %d) = %lld",
                      (long long)out_stride, Ho, Wo, (long long)bound);
        return SPA_ERR_CAPACITY;
    }
    const long long rows = (long long)B * Ho;
    SPA_ARG(rows <= 0x7fffffffLL * 64);
    unsigned long long *bits;
    int rc = spa_ws_reserve(ctx, WS_PNG_ROWS, (size_t)rows * 16, (void **)&bits);
    if (rc != SPA_OK) return rc;
    uint32_t *s1 = (uint32_t *)(bits + rows), *s2 = s1 + rows;
    PngRows g;
    g.src = src; g.row_idx = row_idx; g.col_idx = col_idx;
    g.Hs = Hs; g.Ws = Ws; g.Ho = Ho; g.Wo = Wo; g.rows = rows;
    const bool vec = !col_idx && Ws % 16 == 0 && ((uintptr_t)src & 15) == 0;
    const unsigned gx = (unsigned)((rows + 63) / 64);
    hipStream_t s = spa_stream(stream);
    if (vec) hipLaunchKernelGGL(k_png_count<true>, dim3(gx), dim3(64), 0, s, g, bits, s1, s2);
    else hipLaunchKernelGGL(k_png_count<false>, dim3(gx), dim3(64), 0, s, g, bits, s1, s2);
    hipLaunchKernelGGL(k_png_scan, dim3(B), dim3(PNG_SCAN_THREADS), 0, s, Ho, Wo, bits, (const uint32_t *)s1,
                       (const uint32_t *)s2, nbytes, adler);
    if (vec) hipLaunchKernelGGL(k_png_emit<true>, dim3(gx), dim3(64), 0, s, g, (const unsigned long long *)bits, out,
                                (long long)out_stride, (long long)bound);
    else hipLaunchKernelGGL(k_png_emit<false>, dim3(gx), dim3(64), 0, s, g, (const unsigned long long *)bits, out,
                            (long long)out_stride, (long long)bound);
    SPA_LAUNCH_CHECK();
    return SPA_OK;
}
