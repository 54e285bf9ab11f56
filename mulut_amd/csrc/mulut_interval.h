// mulut_interval.h -- per-site arithmetic of the coarser sampling intervals 5 and 6 (--interval, common/option.py:23).
//
// The interval-4 math of mulut_core.h is fixed at q = 16, L = 17; these templates take the interval IV as a parameter
// (sr/4_test_lut.py:14-16: q = 2^IV, L = 2^(8-IV) + 1).  Pure integer math, compiled by hipcc into mulut_interval.hip and by
// g++ into tests/host_emul/emul_interval.cpp (a CPU unit test of this header, not a product path).
//
// Sums are 32-bit: one pass is worth up to q * 127 (4064 at IV 5, 8128 at IV 6) and a stage numerator up to 4 M q 127
// (130,048 at IV 5 with 8 modes), beyond the 16-bit fields the interval-4 kernels pack their sums into.
#ifndef MULUT_INTERVAL_H_
#define MULUT_INTERVAL_H_

#include "mulut_core.h"

namespace mulut {

template <int IV>
struct IvGeom {
    static_assert(IV == 5 || IV == 6, "intervals 5 and 6 (interval 4 is mulut_core.h)");
    static constexpr int q = 1 << IV;                   // 32, 64
    static constexpr int L = (1 << (8 - IV)) + 1;       // 9, 5
    static constexpr int sA = L * L * L, sB = L * L, sC = L, sD = 1;   // key a (the anchor) slowest (:61)
    static constexpr int rows = L * L * L * L;          // 6561, 625
    static constexpr int all = sA + sB + sC + sD;       // p1111 - p0000
};

// Bytes of one table row on the device at intervals 5 / 6: the plain int8 values (no +128 bias, no band images), 1-byte rows
// packed, u*u-byte rows padded to whole dwords (one vector load per row)
MULUT_HD constexpr int iv_row_bytes(int u) { return u == 1 ? 1 : ((u * u + 3) / 4) * 4; }
// Bytes of one device table, padded to 16 (the LDS copy moves 16-byte chunks)
MULUT_HD constexpr int iv_table_bytes(int rows, int u) { return (rows * iv_row_bytes(u) + 15) & ~15; }

// One site: four key values (0..255) -> five table row indices along the monotone vertex path 0000 -> ... -> 1111 and their
// integer weights (q - f1, f1 - f2, f2 - f3, f3 - f4, f4), sum q.  h = v >> IV, f = v & (q - 1); the fractional parts are sorted
// descending by the 5-comparator network of simplex4() (ties only reorder zero-weight vertices: any order is the 24-case cascade).
template <int IV>
MULUT_HD void simplex4_iv(int va, int vb, int vc, int vd, int (&idx)[5], int (&w)[5]) {
    using G = IvGeom<IV>;
    constexpr int mask = G::q - 1;
    const int base = (va >> IV) * G::sA + (vb >> IV) * G::sB + (vc >> IV) * G::sC + (vd >> IV);
    uint32_t k0 = ((uint32_t)(va & mask) << 16) | (uint32_t)G::sA;
    uint32_t k1 = ((uint32_t)(vb & mask) << 16) | (uint32_t)G::sB;
    uint32_t k2 = ((uint32_t)(vc & mask) << 16) | (uint32_t)G::sC;
    uint32_t k3 = ((uint32_t)(vd & mask) << 16) | (uint32_t)G::sD;
    cmpx_desc(k0, k1);
    cmpx_desc(k2, k3);
    cmpx_desc(k0, k2);
    cmpx_desc(k1, k3);
    cmpx_desc(k1, k2);
    const int f1 = (int)(k0 >> 16), f2 = (int)(k1 >> 16), f3 = (int)(k2 >> 16), f4 = (int)(k3 >> 16);
    idx[0] = base;
    idx[1] = idx[0] + (int)(k0 & 0xFFFFu);
    idx[2] = idx[1] + (int)(k1 & 0xFFFFu);
    idx[3] = idx[2] + (int)(k2 & 0xFFFFu);
    idx[4] = base + G::all;
    w[0] = G::q - f1;
    w[1] = f1 - f2;
    w[2] = f2 - f3;
    w[3] = f3 - f4;
    w[4] = f4;
}

// Stage epilogue with q = 2^IV: K = q * pred summed over modes x 4 rotations,
//   non-final stage: out = clip(rhe((K + 127 q 4M) / (q 4M)))
//   final stage    : out = clip(rhe( K             / (q M)))
// The divisor q d (d = M or 4M) is taken as 2^(IV-1) * iv_div_modes(): floor(n / (q d)) = floor(floor(n / 2^(IV-1)) / (2 d)), so the
// shift leaves a quotient below 2^17 for a DivMagic of 2 d in 2..64 (make_div_magic needs a divisor >= 2 to fit its magic in 32 bits).
MULUT_HD int iv_div_modes(int n_modes, bool is_last) { return 2 * (is_last ? n_modes : 4 * n_modes); }
template <int IV>
MULUT_HD int iv_bias_num(int n_modes, bool is_last) { return is_last ? 0 : 127 * (1 << IV) * 4 * n_modes; }

// clip(round_half_even(n / (2^(IV-1) * dm.d)), 0, 255) for an integer numerator n (may be negative)
template <int IV>
MULUT_HD uint32_t rhe_clip_u8_iv(int n, DivMagic dm) {
    const uint32_t nn = (uint32_t)imax(n, 0);      // negative quotients round to <= 0 and clip to 0
    const uint32_t qq = (uint32_t)(((uint64_t)(nn >> (IV - 1)) * dm.magic) >> 32);
    const uint32_t d = dm.d << (IV - 1);
    const uint32_t r = nn - qq * d;
    const uint32_t up = (2u * r + (qq & 1u)) > d ? 1u : 0u;
    const uint32_t v = qq + up;
    return v > 255u ? 255u : v;
}

}  // namespace mulut
#endif  // MULUT_INTERVAL_H_
