// mulut_ft.h -- what the fine-tuning kernels of every sampling interval share (mulut_ft.hip: interval 4, mulut_ft_interval.hip: 5 and 6).
//
// First part, pure arithmetic compiled by hipcc into both files and by g++ into tests/host_emul/emul_ft_interval.cpp and emul_ft_clamp.cpp (CPU unit
// tests, not a product path): the order of the four keys of a pass, their sorted LSBs and the five weights (the reference's
// differentiable module, MuLUT.InterpTorchBatch, sr/model.py:78-121, 191-282).  The MSB / row-index part of the set-up stays per
// family: ft_pass_setup() below (interval 4) also derives tube slots, ft_iv_pass<IV>() of mulut_ft_interval.h (5 and 6) corner codes;
// both clamp the MSB of every key into 0 .. L - 2, so no key value -- out of 0..255, infinite or NaN -- takes a pass out of its table.
// Both files include it under `#pragma clang fp contract(off)` (the reference's float expressions are not contracted); g++ gets
// -ffp-contract=off from the test.
// Second part (hipcc only): the kernel argument struct with its argument checks, and the LDS float add and DPP row helpers of the
// backward kernels.
#ifndef MULUT_FT_H_
#define MULUT_FT_H_

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>

#include <cstring>

#include "../../include/mulut.h"
#else
#include <math.h>
#endif

#include "mulut_core.h"

namespace mulut {

MULUT_HD int ft_bits(float f) { return __builtin_bit_cast(int, f); }
MULUT_HD float ft_float(int i) { return __builtin_bit_cast(float, i); }
MULUT_HD int ft_lt(int x, int y) { return (int)((unsigned)(x - y) >> 31); }      // [x < y] for 0 <= x, y < 2^31

// The reference orders the four keys by a 24-branch cascade of strict '>' comparisons (sr/model.py:191-282).  Inference's simplex4()
// may order TIES differently (there only zero-weight vertices move); gradients depend on the order, so the backward uses this one.
// For EVERY tie pattern that cascade equals the stable order "f descending, on equal f the key with the higher index first"
// (exhaustive check over all orderings and ties, against this very function compiled by g++: tests/test_ft_order_cpu.py; the proof
// does not depend on q), so the rank of key i is the number of keys that come before it:
//   rank_i = #{ j > i : f_j >= f_i } + #{ j < i : f_j > f_i }.
// f lies in [0, q): the int32 patterns of non-negative floats order like the floats, and [f_j < f_i] is the sign bit of their
// difference -- the ranks are adds and shifts, no compare + select (a v_cndmask_b32 costs six full-rate instructions on this chip and
// the cascade was ~20 of them per pass, the selects by rank another ~36).
// Returns the keys by rank, two bits each: key of rank j in bits 2j, 2j + 1.
MULUT_HD int ft_order_code(float fa, float fb, float fc, float fd) {
    const int a = ft_bits(fa), b = ft_bits(fb), c = ft_bits(fc), d = ft_bits(fd);
    const int s10 = ft_lt(b, a), s20 = ft_lt(c, a), s30 = ft_lt(d, a), s21 = ft_lt(c, b), s31 = ft_lt(d, b), s32 = ft_lt(d, c);
    const int r1 = s10 + 2 - s21 - s31, r2 = s20 + s21 + 1 - s32, r3 = s30 + s31 + s32;      // (rank of key a: 3 - s10 - s20 - s30, contributes 0)
    return (1 << (2 * r1)) | (2 << (2 * r2)) | (3 << (2 * r3));
}

// The LSBs by rank.  Only the VALUES are needed, and a min / max network sorts values whatever the ties (on the int32 patterns,
// as the ranks: integer min / max need no NaN canonicalisation of their operands).
MULUT_HD void ft_sort_lsb(const float (&f)[4], float (&fs)[4]) {
    const int i0 = ft_bits(f[0]), i1 = ft_bits(f[1]), i2 = ft_bits(f[2]), i3 = ft_bits(f[3]);
    const int a = imax(i0, i1), b = imin(i0, i1), c = imax(i2, i3), d = imin(i2, i3);
    const int t1 = imin(a, c), t2 = imax(b, d);
    fs[0] = ft_float(imax(a, c)); fs[1] = ft_float(imax(t1, t2)); fs[2] = ft_float(imin(t1, t2)); fs[3] = ft_float(imin(b, d));
}
// The five weights of a pass from its sorted LSBs
MULUT_HD void ft_weights(float q, const float (&fs)[4], float (&wt)[5]) {
    wt[0] = q - fs[0];
    wt[1] = fs[0] - fs[1];
    wt[2] = fs[1] - fs[2];
    wt[3] = fs[2] - fs[3];
    wt[4] = fs[3];
}

// One pass at interval 4 (q = 16, L = 17): the four keys of site (y, x) of `plane` under rotation r, their table rows, weights, tube
// slots and rank order.  For x in 0..255 this is the reference's set-up.  For ANY float it stays inside the table and the tube band:
//   - the MSB of every key is clamped into 0 .. L - 2 = 15 (255 has MSB 15), in float before the conversion, so a value the int
//     cannot hold, an infinity or a NaN converts defined and alike on host and device (NaN -> 0, +inf -> 15);
//   - the keys are ranked on |LSB|.  The LSB, v - q floor(v / q) (the reference's img % q), is >= +0 for every v in range; out of range
//     it can carry a sign bit (a NaN of either sign, a negative denormal whose quotient underflows to -0), and ft_order_code() orders
//     int32 patterns, which is a total order on non-negative patterns only -- with a sign bit its six comparisons can form a cycle and
//     the code is no permutation: one key's stride added twice, a row past 83520 or a slot past 1040.  On non-negative patterns the
//     code is always a permutation, so row 4 = row 0 + 5220 <= 83520 and slot 4 = slot 0 + 65 <= 1040.
// Such a pixel gets a defined, meaningless weight (NaN for a NaN or an infinity), never an address.
struct FtPass {
    int idx[5];      // table rows of the five vertices
    float wt[5];     // q-f1, f1-f2, f2-f3, f3-f4, f4
    int tslot[5];    // tube-band slots of the five vertices (mulut_core.h), valid when in_tube
    bool in_tube;    // the four MSBs span at most one step: every vertex lies in the 1041-slot tube band
    int ord;         // key (0 = a ... 3 = d) of rank j in bits 2j, 2j + 1
};

MULUT_HD void ft_pass_setup(const float *plane, int H, int W, int y, int x, int r, const int (&di)[3], const int (&dj)[3], FtPass &p) {
    int pix[4];
    float v[4];
    pix[0] = y * W + x;
    for (int k = 0; k < 3; ++k) {
        int dy, dx;
        sample_offset(r, di[k], dj[k], dy, dx);
        pix[k + 1] = imin(imax(y + dy, 0), H - 1) * W + imin(imax(x + dx, 0), W - 1);
    }
    int h[4];
    float f[4];
    for (int k = 0; k < 4; ++k) {
        v[k] = plane[pix[k]];
        const float hf = floorf(v[k] / (float)kQ);       // torch.floor_divide(img, q)
        f[k] = v[k] - (float)kQ * hf;                    // img % q
        h[k] = (int)fminf(fmaxf(hf, 0.0f), (float)(kL - 2));      // (a value outside 0..255 must not leave the table; fmaxf drops a NaN)
    }
    const int ord = ft_order_code(fabsf(f[0]), fabsf(f[1]), fabsf(f[2]), fabsf(f[3]));      // (a permutation for any four floats: see above)
    p.ord = ord;
    float fs[4];
    ft_sort_lsb(f, fs);
    // strides of the key of rank j: a shift of a packed constant by that key's id
    constexpr unsigned long long kRowStrides = (unsigned long long)kStrideA | ((unsigned long long)kStrideB << 16) | ((unsigned long long)kStrideC << 32) |
                                               ((unsigned long long)kStrideD << 48);
    constexpr uint32_t kTubeStrides = (uint32_t)kTubeSA | ((uint32_t)kTubeSB << 8) | ((uint32_t)kTubeSC << 16) | ((uint32_t)kTubeSD << 24);
    static_assert(kStrideA < 65536 && kTubeSA < 256 && kStrideD == 1, "packed stride constants");
    int ss[4], ts[4];
    for (int j = 0; j < 4; ++j) {
        const int d = (ord >> (2 * j)) & 3;
        ss[j] = (int)((uint32_t)(kRowStrides >> (16 * d)) & 0xFFFFu);
        ts[j] = (int)((kTubeStrides >> (8 * d)) & 0xFFu);
    }
    {
        p.tslot[0] = tube_slot(h[0], h[1], h[2], h[3]);
        p.tslot[1] = p.tslot[0] + ts[0];
        p.tslot[2] = p.tslot[1] + ts[1];
        p.tslot[3] = p.tslot[2] + ts[2];
        p.tslot[4] = p.tslot[3] + ts[3];
        const int hx = imax(imax(h[0], h[1]), imax(h[2], h[3])), hn = imin(imin(h[0], h[1]), imin(h[2], h[3]));
        p.in_tube = hx - hn <= 1;
    }
    p.idx[0] = h[0] * kStrideA + h[1] * kStrideB + h[2] * kStrideC + h[3];
    p.idx[1] = p.idx[0] + ss[0];
    p.idx[2] = p.idx[1] + ss[1];
    p.idx[3] = p.idx[2] + ss[2];
    p.idx[4] = p.idx[3] + ss[3];
    ft_weights((float)kQ, fs, p.wt);
}

#if defined(__HIPCC__)
// ---------------------------------------------------------------------------------------------------------------- hipcc only
constexpr int kMaxFtModes = MULUT_MAX_MODES;

struct FtArgs {
    const float *w[kMaxFtModes];
    float *gw[kMaxFtModes];
    const float *x;     // [B][C][H][W], values 0..255
    const float *gout;  // [B][C][H*u][W*u]
    float *out;         // [B][C][H*u][W*u]
    float *gx;          // [B][C][H][W]
    uint16_t *inside;   // [B][C][H][W]: bit eo of a site = the stage's clamp lets gradient through at block position eo
                        // (0 <= pred / avg + bias <= 255); the forward writes it, a backward that gets it skips the forward recomputation
                        // (optional at interval 4)
    int B, C, H, W, u, M, is_last;
    int di[kMaxFtModes][3], dj[kMaxFtModes][3];
};

// FtArgs with tiles_per_wg, and where it is: the arguments of the interval-5 / 6 kernels (mulut_ft_interval.hip).  Not FtArgs with the
// field appended: behind di / dj the backward kernels fetch it with a scalar load of its own (next to is_last the two come as one),
// and in the middle of FtArgs it would move the argument offsets of the interval-4 kernels.  `inside` is mandatory here.
struct FtIvArgs {
    const float *w[kMaxFtModes];
    float *gw[kMaxFtModes];
    const float *x, *gout;
    float *out, *gx;
    uint16_t *inside;
    int B, C, H, W, u, M, is_last;
    int tiles_per_wg;     // backward: consecutive tiles of sites a workgroup walks
    int di[kMaxFtModes][3], dj[kMaxFtModes][3];
};

// float add into LDS as ds_add_f32: an atomicAdd on a pointer the compiler cannot prove to be LDS (here: one of two targets chosen
// at run time) becomes flat_atomic_add_f32, which reaches the LDS through the texture path
__device__ __forceinline__ void lds_add_f32(float *p, float v) {
    // (as an instruction of its own: written as an atomic on an address_space(3) pointer it is still merged with the global
    // atomic of the other branch into one flat atomic on a selected pointer.)  The compiler does not count this LDS operation:
    // LDS returns in order, so its own waits can only get stricter, and lds_adds_done() drains before a barrier publishes the sums.
    asm volatile("ds_add_f32 %0, %1" : : "v"((uint32_t)(uintptr_t)p), "v"(v) : "memory");
}
__device__ __forceinline__ void lds_adds_done() { asm volatile("s_waitcnt lgkmcnt(0)" : : : "memory"); }

__device__ __forceinline__ float ft_sum16(float v) {      // sum over the 16 lanes of a DPP row; every lane gets it
    v += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x128, 0xF, 0xF, true));      // row_ror:8
    v += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x124, 0xF, 0xF, true));      // row_ror:4
    v += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x122, 0xF, 0xF, true));      // row_ror:2
    v += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x121, 0xF, 0xF, true));      // row_ror:1
    return v;
}
// lane K of every 16-lane row to all lanes of its row (v_mov_b32_dpp row_newbcast:K)
template <int K> __device__ __forceinline__ int ft_bcast(int v) { return __builtin_amdgcn_update_dpp(0, v, 0x150 + K, 0xF, 0xF, true); }
template <int K> __device__ __forceinline__ float ft_bcast(float v) { return __int_as_float(ft_bcast<K>(__float_as_int(v))); }

template <int U>
__device__ __forceinline__ int eo_of_elem(int r, int e) {      // block position whose table element is e under rotation r (inverse of row_elem)
    return r == 0 ? e : r == 1 ? U * (e % U) + (U - 1 - e / U) : r == 2 ? U * U - 1 - e : U * (U - 1 - e % U) + e / U;
}

// Argument checks of every fine-tuning entry point, decided before the device is touched; their order -- and so which MULUT_E* code a
// bad call gets -- is part of the ABI (include/mulut.h).  need_mask: the entry point cannot do without `inside`; interval_ok: the
// caller's own verdict on its interval argument (entry points without one pass true); max_reach: the largest pattern reach the entry
// point accepts, i.e. the largest HALO its backward kernels are instantiated for (2: s, d, y; 3: e, h, o as well).
// Args: FtArgs or FtIvArgs.
template <class Args>
static inline int ft_fill(Args &a, bool interval_ok, const float *const *weights, float *const *grad_wq, const char *modes, int is_last, int u,
                   const float *x, const uint16_t *inside, bool need_mask, int max_reach, int B, int C, int H, int W) {
    if (!weights || !modes || !x || (need_mask && !inside) || B <= 0 || C <= 0 || H <= 0 || W <= 0) return MULUT_EINVAL;
    if (!interval_ok) return MULUT_EUNSUPPORTED;
    const size_t M = strlen(modes);
    if (M < 1 || M > (size_t)kMaxFtModes || u < 1 || u > 4) return MULUT_EUNSUPPORTED;
    memset(&a, 0, sizeof(a));
    for (size_t m = 0; m < M; ++m) {
        int di[3], dj[3];
        // the input-gradient tiles of the backward kernels stage a halo of HALO pixels: a pattern must not reach beyond the one launched
        if (!pattern_offsets(modes[m], di, dj) || pattern_reach(modes[m]) > max_reach) return MULUT_EMODE;
        if (!weights[m] || (grad_wq && !grad_wq[m])) return MULUT_EINVAL;
        a.w[m] = weights[m];
        a.gw[m] = grad_wq ? grad_wq[m] : nullptr;
        for (int k = 0; k < 3; ++k) {
            a.di[m][k] = di[k];
            a.dj[m][k] = dj[k];
        }
    }
    a.x = x;
    a.inside = const_cast<uint16_t *>(inside);
    a.B = B; a.C = C; a.H = H; a.W = W; a.u = u; a.M = (int)M; a.is_last = is_last ? 1 : 0;
    return MULUT_OK;
}

// The halo a filled argument struct needs: the largest key offset of its modes, at least 2 (the s, d, y instances)
template <class Args>
static inline int ft_halo(const Args &a) {
    int r = 2;
    for (int m = 0; m < a.M; ++m)
        for (int k = 0; k < 3; ++k) r = imax(r, imax(a.di[m][k], a.dj[m][k]));
    return r;
}

// One stage, forward or backward, of a filled argument struct: the one launcher each kernel file exports.  halo: ft_halo() of the
// arguments for a backward, 2 for a forward (the forward kernels have no halo).  The entry points and the one function that checks,
// fills and launches for all of them are in mulut_ft.hip.
hipError_t launch_ft_stage(const FtArgs &a, bool backward, int halo, hipStream_t st);                                              // mulut_ft.hip: interval 4
hipError_t launch_ft_interval_stage(const FtIvArgs &a, int interval, bool backward, int halo, int num_cus, hipStream_t st);        // mulut_ft_interval.hip: 5 and 6
#endif  // __HIPCC__

}  // namespace mulut
#endif  // MULUT_FT_H_
