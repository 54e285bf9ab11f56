// mulut_ft_exact.h -- the arithmetic of the bit-reproducible (fixed-point) backward of a fine-tune stage, defined once.
//
// Pure MULUT_HD functions, compiled by hipcc into the kernels of mulut_ft_exact.hip and by g++ into tests/host_emul/ft_exact_host.cpp
// (the host model the GPU tests ask equality of; a CPU test program, not a product path).  Both compile it without FMA contraction
// (`#pragma clang fp contract(off)` / -ffp-contract=off), as mulut_ft.h is compiled.
//
// The gradient of a stage (sr/model.py:69-312, autograd's backward of it) is a sum of CONTRIBUTIONS, each a float32 value given by
// one fixed expression -- those of ft_stage_bwd (mulut_ft.hip):
//   g[eo]            = inside bit eo of the site ? grad_out / avg : 0                                   fx_site_g()
//   table (idx[j], e) of mode m, rotation r:  v = (wt[j] / q) * g[eo],  e = row_elem(r, eo)              fx_table_term()
//   dsum[j]          = sum over eo ASCENDING of g[eo] * row_j[row_elem(r, eo)], in float32
//   df[j]            = (dsum[j + 1] - dsum[j]) / q;  key k of the pass gets the df of its rank            fx_key_grads()
// with the pass set-up (rows, weights, rank order, clamps) of ft_pass_setup() (interval 4) and ft_iv_pass<IV>() (5, 6) used as
// they are: fx_pass<IV>().  Every v and every dk is ONE contribution; nothing is summed in float across sites, passes or lanes.
// A contribution c becomes the integer llrint(c * 2^S) (fx_quant(), round half to even); integers are added -- in any order, the sum
// is the same -- and each sum becomes one float32, float((double)sum * 2^-S) (fx_result()), which is added to the destination.
//
// RESOLUTION.  S comes from gmax = max |grad_out| of the call (as the maximum of the float bit patterns with the sign cleared: an
// integer maximum has no order either) and from the call's shape, never from anything else in the data.  With gmax in
// [2^(E-1), 2^E) one unit of a table sum is 2^-S_w = 2^(E + ceil(log2(4 B C H W)) - 61) <= gmax * 2^(ceil(log2(4 B C H W)) - 60):
// at 256 x 48 x 48 sites gmax * 2^-38.  One unit of an input-gradient sum is 2^-S_x <= gmax * 2^(kx + ceil(log2 N_x) - 60), kx and
// N_x below: at u = 4 and three modes of reach 2 gmax * 2^-43.  A contribution below half a unit counts as 0.
#ifndef MULUT_FT_EXACT_H_
#define MULUT_FT_EXACT_H_

#include "mulut_ft_interval.h"

namespace mulut {

constexpr int kFxAccBits = 62;      // no accumulator leaves +-2^62, whatever the inputs (tables within +-127, grad_out finite)

MULUT_HD int fx_ceil_log2(unsigned long long n) {      // smallest k with 2^k >= n (n <= 2^62)
    int k = 0;
    while (k < 62 && (1ull << k) < n) ++k;
    return k;
}
// E with gmax < 2^E, from the bit pattern of gmax (sign cleared): the biased exponent - 126.  A denormal gmax gives -126, an
// infinity or a NaN 129: a defined scale for a call whose results are unspecified.
MULUT_HD int fx_gmax_exp(uint32_t gmax_bits) { return (int)((gmax_bits & 0x7fffffffu) >> 23) - 126; }

// 2^s as a double, s in [-1022, 1023] (every scale below lies in [-300, 300])
MULUT_HD double fx_pow2(int s) { return __builtin_bit_cast(double, (unsigned long long)(1023 + imin(imax(s, -1022), 1023)) << 52); }

// Scale of the table sums.  |v| = (wt / q) |g| <= |g| <= gmax < 2^E: a weight is at most q, and avg (M or 4 M) is at least 1.  One
// element (row, e) of one mode is reached by at most N_w = 4 B C H W contributions: four rotations times the sites -- the five
// vertices of a pass are five different rows, and under one rotation one block position eo lands on e.  A contribution's integer is
// at most |v| 2^S + 1/2, so with S_w = 61 - E - ceil(log2 N_w) a sum stays within N_w (2^(61 - ceil(log2 N_w)) + 1/2) <= 2^61 + 2^61.
MULUT_HD int fx_scale_w(uint32_t gmax_bits, long long nsite) {
    return (kFxAccBits - 1) - fx_gmax_exp(gmax_bits) - fx_ceil_log2(4ull * (unsigned long long)nsite);
}
// Scale of the input-gradient sums.  |dsum| <= u*u * 127 gmax (1 + 2^-24)^(u*u) (tables within +-127), so
// |dk| <= 2 u*u 127 / q gmax (1 + 2^-20) < 16 u*u gmax at q >= 16 (2 * 127 / 16 = 15.875): |dk| < 2^(E + kx), kx = 4 + ceil(log2 u*u).
// One pixel is the target of at most N_x = 16 M min((R + 1)^2, H W) contributions: M modes x 4 rotations x 4 keys, and for one
// (mode, rotation, key) -- one offset o with |o_y|, |o_x| <= R, the reach of the list -- the sites s with clamp(s + o) = p are one for
// an inner pixel and at most (R + 1) per direction for a corner pixel (replicate padding folds the R positions beyond the border
// onto it), never more than the plane has sites.  S_x = 61 - E - kx - ceil(log2 N_x) keeps a sum within 2^62 as above.
MULUT_HD int fx_scale_x(uint32_t gmax_bits, int u, int M, int reach, int H, int W) {
    const long long fold = (long long)(reach + 1) * (reach + 1), plane = (long long)H * W;
    const unsigned long long nx = 16ull * (unsigned long long)M * (unsigned long long)(fold < plane ? fold : plane);
    return (kFxAccBits - 1) - fx_gmax_exp(gmax_bits) - (4 + fx_ceil_log2((unsigned long long)(u * u))) - fx_ceil_log2(nx);
}

// The conversions.  float -> double and the product with a power of two are exact (a float's 24 bits and an exponent within
// +-300), so the ONE rounding is llrint's, half to even, on host and device alike -- a float path (c * 2^S in float32) would
// overflow or flush where the double cannot.  |c 2^S| <= 2^61 for every contribution the bounds above cover.
MULUT_HD long long fx_quant(float c, int S) { return llrint((double)c * fx_pow2(S)); }
// (int64 -> double rounds to nearest even where the sum has more than 53 bits, the product is exact, double -> float rounds again:
// the same two roundings on host and device)
MULUT_HD float fx_result(long long sum, int S) { return (float)((double)sum * fx_pow2(-S)); }

// Reach of a mode list as the scale of the input gradient takes it: the largest key offset, at least 2 (ft_halo() of the filled
// arguments gives the same number on the device side)
MULUT_HD int fx_list_reach(const char *modes, int M) {
    int r = 2;
    for (int m = 0; m < M; ++m) r = imax(r, pattern_reach(modes[m]));
    return r;
}

// One pass of any interval in one shape: the five table rows, the five weights, the key of every rank
struct FxPass {
    int idx[5];
    float wt[5];
    int ord;
    int slot[5];      // interval 4: tube-band slots of the rows when the pass lies in the tube, else -1 (where a kernel keeps the sums: no arithmetic)
};
template <int IV>
MULUT_HD void fx_pass(const float *plane, int H, int W, int y, int x, int r, const int (&di)[3], const int (&dj)[3], FxPass &p) {
    if constexpr (IV == 4) {
        FtPass t;
        ft_pass_setup(plane, H, W, y, x, r, di, dj, t);
        for (int j = 0; j < 5; ++j) p.idx[j] = t.idx[j], p.wt[j] = t.wt[j], p.slot[j] = t.in_tube ? t.tslot[j] : -1;
        p.ord = t.ord;
    } else {
        float v[4];
        v[0] = plane[y * W + x];
        for (int k = 0; k < 3; ++k) {
            int dy, dx;
            sample_offset(r, di[k], dj[k], dy, dx);
            v[k + 1] = plane[imin(imax(y + dy, 0), H - 1) * W + imin(imax(x + dx, 0), W - 1)];
        }
        FtIvPass t;
        ft_iv_pass<IV>(v, t);
        for (int j = 0; j < 5; ++j) p.idx[j] = t.idx[j], p.wt[j] = t.wt[j], p.slot[j] = -1;
        p.ord = t.ord;
    }
}

// g = dL/d pred of one site.  pg: grad_out of the site's plane [H*U][W*U]; inside: the site's mask word (0 for no site)
template <int U>
MULUT_HD void fx_site_g(const float *pg, int W, int y, int x, uint32_t inside, float avg, float (&g)[U * U]) {
    for (int eo = 0; eo < U * U; ++eo) {
        const float go = pg[(long long)(y * U + eo / U) * (W * U) + (x * U + eo % U)];
        g[eo] = ((inside >> eo) & 1u) ? go / avg : 0.0f;
    }
}

// contribution of block position eo of a site to element row_elem(r, eo) of the table row of vertex j
MULUT_HD float fx_table_term(float wt, float q, float g) { return (wt / q) * g; }

// the four input-gradient contributions of a pass, by key (0 = the site's own pixel, k = 1..3 the pixel at pattern offset k - 1)
template <int IV, int U>
MULUT_HD void fx_key_grads(const float *tab, const FxPass &p, int r, const float (&g)[U * U], float (&dk)[4]) {
    constexpr int EL = U * U;
    float dsum[5];
    for (int j = 0; j < 5; ++j) {
        const float *row = tab + (long long)p.idx[j] * EL;
        float acc = 0.0f;
        for (int eo = 0; eo < EL; ++eo) acc += g[eo] * row[row_elem(r, eo / U, eo % U, U)];
        dsum[j] = acc;
    }
    float df[4];
    for (int j = 0; j < 4; ++j) df[j] = (dsum[j + 1] - dsum[j]) / (float)IvGeom<IV>::q;
    const int o0 = p.ord & 3, o1 = (p.ord >> 2) & 3, o2 = (p.ord >> 4) & 3;
    for (int k = 0; k < 4; ++k) dk[k] = o0 == k ? df[0] : o1 == k ? df[1] : o2 == k ? df[2] : df[3];
}

// The workspace, in 64-bit words: [0] gmax's bit pattern (low half), [1 ..) the table sums [M][rows][u*u], then the input sums
// [B][C][H][W]
MULUT_HD long long fx_ws_words(int M, int rows, int u, long long nsite) { return 1 + (long long)M * rows * (u * u) + nsite; }

}  // namespace mulut
#endif  // MULUT_FT_EXACT_H_
