// mulut_ft_interval.h -- per-pass set-up of LUT-aware fine-tuning at the sampling intervals 5 and 6.
//
// The float twin of simplex4<IV>(): the reference's differentiable module (MuLUT.InterpTorchBatch, sr/model.py:78-121, 191-282)
// with q = 2^IV, L = 2^(8-IV) + 1.  Four key values (floats, 0..255, not necessarily integers) -> the five table rows of the
// pass, their weights (q - f1, f1 - f2, f2 - f3, f3 - f4, f4) and the key that holds each rank (the order code, the LSB sort and
// the weights are mulut_ft.h's, shared with interval 4).
// Compiled by hipcc into mulut_ft_interval.hip and by g++ into tests/host_emul/emul_ft_interval.cpp (a CPU unit test of this
// header, not a product path).
#ifndef MULUT_FT_INTERVAL_H_
#define MULUT_FT_INTERVAL_H_

#include "mulut_ft.h"

namespace mulut {

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
    const int ord = ft_order_code(f[0], f[1], f[2], f[3]);
    p.ord = ord;
    float fs[4];
    ft_sort_lsb(f, fs);
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
    ft_weights((float)G::q, fs, p.wt);
}

// corner code of vertex j (0..4) of a pass
MULUT_HD int ft_iv_corner(const FtIvPass &p, int j) {
    int c = p.corner;
    for (int i = 0; i < j; ++i) c ^= 8 >> ((p.ord >> (2 * i)) & 3);
    return c;
}

}  // namespace mulut
#endif  // MULUT_FT_INTERVAL_H_
