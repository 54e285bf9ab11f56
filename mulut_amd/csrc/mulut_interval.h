// mulut_interval.h -- per-site arithmetic of the coarser sampling intervals 5 and 6 (--interval, common/option.py:23).
//
// The geometry IvGeom<IV> and the simplex walk simplex4<IV>() are mulut_core.h's, with the interval IV as a parameter
// (sr/4_test_lut.py:14-16: q = 2^IV, L = 2^(8-IV) + 1); here is what only these intervals have: their table row format and their
// epilogue division.  Pure integer math, compiled by hipcc into mulut_interval.hip and by g++ into
// tests/host_emul/emul_interval.cpp (a CPU unit test of this header, not a product path).
//
// Sums are 32-bit: one pass is worth up to q * 127 (4064 at IV 5, 8128 at IV 6) and a stage numerator up to 4 M q 127
// (130,048 at IV 5 with 8 modes), beyond the 16-bit fields the interval-4 kernels pack their sums into.
#ifndef MULUT_INTERVAL_H_
#define MULUT_INTERVAL_H_

#include "mulut_core.h"

namespace mulut {

// Bytes of one table row on the device at intervals 5 / 6: the plain int8 values (no +128 bias, no band images), 1-byte rows
// packed, u*u-byte rows padded to whole dwords (one vector load per row)
MULUT_HD constexpr int iv_row_bytes(int u) { return u == 1 ? 1 : ((u * u + 3) / 4) * 4; }
// Bytes of one device table, padded to 16 (the LDS copy moves 16-byte chunks)
MULUT_HD constexpr int iv_table_bytes(int rows, int u) { return (rows * iv_row_bytes(u) + 15) & ~15; }

// simplex4<IV>() and stage_bias_num<IV>() of mulut_core.h under the names the interval code and its host harness call them by
template <int IV>
MULUT_HD void simplex4_iv(int va, int vb, int vc, int vd, int (&idx)[5], int (&w)[5]) { simplex4<IV>(va, vb, vc, vd, idx, w); }
template <int IV>
MULUT_HD int iv_bias_num(int n_modes, bool is_last) { return stage_bias_num<IV>(n_modes, is_last); }

// Stage epilogue with q = 2^IV: K = q * pred summed over modes x 4 rotations,
//   non-final stage: out = clip(rhe((K + 127 q 4M) / (q 4M)))
//   final stage    : out = clip(rhe( K             / (q M)))
// The divisor q d (d = M or 4M) is taken as 2^(IV-1) * iv_div_modes(): floor(n / (q d)) = floor(floor(n / 2^(IV-1)) / (2 d)), so the
// shift leaves a quotient below 2^17 for a DivMagic of 2 d in 2..64 (make_div_magic needs a divisor >= 2 to fit its magic in 32 bits).
MULUT_HD int iv_div_modes(int n_modes, bool is_last) { return 2 * (is_last ? n_modes : 4 * n_modes); }

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
