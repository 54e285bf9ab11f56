// mulut_ft_interval.h -- per-pass set-up of LUT-aware fine-tuning at the sampling intervals 5 and 6.
//
// The float twin of simplex4_iv(): the reference's differentiable module (MuLUT.InterpTorchBatch, sr/model.py:78-121, 191-282)
// with q = 2^IV, L = 2^(8-IV) + 1.  Four key values (floats, 0..255, not necessarily integers) -> the five table rows of the
// pass, their weights (q - f1, f1 - f2, f2 - f3, f3 - f4, f4) and the key that holds each rank.  Inference's simplex4_iv() may
// order TIES differently (there only zero-weight vertices move); gradients depend on the order, so the backward uses this one:
// the reference's 24-branch strict-'>' cascade = "f descending, on equal f the key with the higher index first"
// (tests/test_ft_order_cpu.py proves the equivalence for every tie pattern; the proof does not depend on q).
// Compiled by hipcc into mulut_ft_interval.hip and by g++ into tests/host_emul/emul_ft_interval.cpp (a CPU unit test of this
// header, not a product path).
#ifndef MULUT_FT_INTERVAL_H_
#define MULUT_FT_INTERVAL_H_

#if !defined(__HIPCC__)
#include <math.h>
#endif

#include "mulut_interval.h"

namespace mulut {

MULUT_HD int ft_iv_bits(float f) { return __builtin_bit_cast(int, f); }
MULUT_HD float ft_iv_float(int i) { return __builtin_bit_cast(float, i); }

// rank of key i = #{ j > i : f_j >= f_i } + #{ j < i : f_j > f_i }; f >= 0, so the int32 patterns order like the floats and
// [f_j < f_i] is the sign bit of their difference (as ft_order_code of mulut_ft.hip).  Returns the keys by rank, two bits each:
// key of rank j in bits 2j, 2j + 1.
MULUT_HD int ft_iv_order_code(float fa, float fb, float fc, float fd) {
    const int a = ft_iv_bits(fa), b = ft_iv_bits(fb), c = ft_iv_bits(fc), d = ft_iv_bits(fd);
#define MULUT_FT_IV_LT(x, y) ((int)((unsigned)((x) - (y)) >> 31))      // [x < y] for 0 <= x, y < 2^31
    const int s10 = MULUT_FT_IV_LT(b, a), s20 = MULUT_FT_IV_LT(c, a), s30 = MULUT_FT_IV_LT(d, a);
    const int s21 = MULUT_FT_IV_LT(c, b), s31 = MULUT_FT_IV_LT(d, b), s32 = MULUT_FT_IV_LT(d, c);
#undef MULUT_FT_IV_LT
    const int r1 = s10 + 2 - s21 - s31, r2 = s20 + s21 + 1 - s32, r3 = s30 + s31 + s32;
    return (1 << (2 * r1)) | (2 << (2 * r2)) | (3 << (2 * r3));
}

struct FtIvPass {
    int idx[5];      // table rows of the five vertices along the path 0000 -> 1111
    float wt[5];     // q - f1, f1 - f2, f2 - f3, f3 - f4, f4
    int ord;         // key (0 = a ... 3 = d) of rank j in bits 2j, 2j + 1
    int corner;      // parities of the anchor cell's four MSBs (key a in bit 3 ... key d in bit 0): vertex j of the pass sits at the
                     // corner whose code is this one with bit (3 - key) flipped for every key of rank < j -- the 16 corners of a
                     // cell have 16 different codes
};

template <int IV>
MULUT_HD void ft_iv_pass(const float (&v)[4], FtIvPass &p) {
    using G = IvGeom<IV>;
    int h[4];
    float f[4];
    for (int k = 0; k < 4; ++k) {
        const float hf = floorf(v[k] / (float)G::q);      // torch.floor_divide(img, q)
        f[k] = v[k] - (float)G::q * hf;                   // img % q
        h[k] = imin(imax((int)hf, 0), G::L - 2);          // (a value outside 0..255 must not leave the table)
    }
    const int ord = ft_iv_order_code(f[0], f[1], f[2], f[3]);
    p.ord = ord;
    // the LSBs by rank: only the VALUES are needed, and a min / max network sorts values whatever the ties
    float fs[4];
    {
        const int i0 = ft_iv_bits(f[0]), i1 = ft_iv_bits(f[1]), i2 = ft_iv_bits(f[2]), i3 = ft_iv_bits(f[3]);
        const int a = imax(i0, i1), b = imin(i0, i1), c = imax(i2, i3), d = imin(i2, i3);
        const int t1 = imin(a, c), t2 = imax(b, d);
        fs[0] = ft_iv_float(imax(a, c)); fs[1] = ft_iv_float(imax(t1, t2)); fs[2] = ft_iv_float(imin(t1, t2)); fs[3] = ft_iv_float(imin(b, d));
    }
    // stride of the key of rank j: a shift of a packed constant by that key's id
    constexpr unsigned long long kStrides = (unsigned long long)G::sA | ((unsigned long long)G::sB << 16) | ((unsigned long long)G::sC << 32) |
                                            ((unsigned long long)G::sD << 48);
    static_assert(G::sA < 65536, "packed stride constant");
    p.idx[0] = h[0] * G::sA + h[1] * G::sB + h[2] * G::sC + h[3];
    for (int j = 0; j < 4; ++j) {
        const int key = (ord >> (2 * j)) & 3;
        p.idx[j + 1] = imin(p.idx[j] + (int)((unsigned)(kStrides >> (16 * key)) & 0xFFFFu), G::rows - 1);
    }
    p.corner = ((h[0] & 1) << 3) | ((h[1] & 1) << 2) | ((h[2] & 1) << 1) | (h[3] & 1);
    p.wt[0] = (float)G::q - fs[0];
    p.wt[1] = fs[0] - fs[1];
    p.wt[2] = fs[1] - fs[2];
    p.wt[3] = fs[2] - fs[3];
    p.wt[4] = fs[3];
}

// corner code of vertex j (0..4) of a pass
MULUT_HD int ft_iv_corner(const FtIvPass &p, int j) {
    int c = p.corner;
    for (int i = 0; i < j; ++i) c ^= 8 >> ((p.ord >> (2 * i)) & 3);
    return c;
}

}  // namespace mulut
#endif  // MULUT_FT_INTERVAL_H_
