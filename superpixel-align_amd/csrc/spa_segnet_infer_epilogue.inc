// The inference epilogue on the float32 sums acc, as TEXT: the body of sg_infer_epilogue (spa_segnet_dev.h, where the
// float32 and bf16 kernels call it) and, included directly, the end of k_segnet_conv_f16x3 -- at the 256-VGPR limit
// that kernel's decode1 form spilled 9 registers instead of 5 around a call; as text it compiles as verified
// (profiles/segnet_refactor_isa.md).  It returns early: it must be the LAST statement of the enclosing function.
// Expects in scope: MODE, acc, bias, wc, bc, Y, Yi, b, ty0, tx0, w, fi, fq, H, W (sg_infer_epilogue's parameters).
{
    const int oy = ty0 + 2 * w, ox = tx0 + 2 * fq;
    if (MODE == SG_CONV1 || MODE == SG_ENC) {
        const int Hh = H >> 1, Wh = W >> 1;
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
        // (SG_DEC1) or the two sums as they are (SG_DEC1L)
        float w0[4], w1[4], bn[4];
#pragma unroll
        for (int nt = 0; nt < 4; ++nt) {
            bn[nt] = bias[16 * nt + fi];
            w0[nt] = wc[16 * nt + fi];
            w1[nt] = wc[64 + 16 * nt + fi];
        }
        const float b0 = bc[0], b1 = bc[1];
        const long long plane = (long long)H * W;
#pragma unroll
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
            const long long o = (long long)b * 2 * plane + (long long)(oy + (fi >> 1)) * W + x + (fi & 1);
            if (MODE == SG_DEC1L) {
                Y[o] = za;
                Y[o + plane] = zb;
            } else {
                const float mx = za > zb ? za : zb;
                const float e0 = expf(za - mx), e1 = expf(zb - mx);
                const float sum = e0 + e1;
                Y[o] = e0 / sum;
                Y[o + plane] = e1 / sum;
            }
        }
    }
}
