// mulut_wide.hip -- stages of mode lists that hold a 4 x 4 sampling pattern (e, h, o: keys up to 3 px from the anchor, so a
// stage reaches 3 LR rows / columns beyond its outputs instead of 2).  Every stage of such a list runs here, whatever mix of
// the six patterns it holds; the s / d / y kernels of the other translation units are not involved (their tiles stage a
// 2-px halo, and their tube bands, work lists and tile marks assume the s / d / y offsets).
//   stage_wide1_kernel    1-byte rows (non-final stages; a final stage at scale 1): one mode's whole 83.5 KB table in LDS next
//                         to the image tile with a 3-px halo, swapped per mode, the next table prefetched through registers
//                         (the stage_u1w_kernel scheme of mulut_k1.hip); one template instance of the pass body per pattern
//   stage_wide_up_kernel  u*u-byte rows (final stage, u in {2,3,4}): the five rows of a pass gathered from the full table in
//                         global memory, one vector load per row (the stage_up_kernel scheme), generic output layout
#include <hip/hip_runtime.h>

#include "mulut_dev.h"

namespace mulut {

// ------------------------------------------------------------------------------------------
// 1-byte rows.  Tile 64 x 64, 1024 threads, a thread owns four horizontally adjacent pixels of a row.  LDS:
//   [ table: kU1TableBytes = 83,536 ][ image: C x 70 rows x 72 bytes (64 + 2 x 3 columns, padded to whole dwords) = 15,120 for C = 3 ]
// = 98,656 B: one workgroup per CU, as stage_u1w_kernel (which holds 97,408).  64 x 64 keeps the halo overhead at 1.23x the tile's
// pixels (a 32 x 32 tile would pay 1.52x) and fills 1024 threads with four pixels each; the LDS left over could not hold a second
// table or a second workgroup (2 x 98.7 KB > 160 KB) anyway.
// Per channel and mode a thread reads its 7 x 12-byte window of pixels once (21 ds_read_b32: rows ty-3 .. ty+3, columns x-3 .. x+8
// of its first pixel x); every key of every pixel and rotation is then one v_perm_b32 of two window registers.  Rotations r and r + 2
// run in packed 16-bit halves (simplex4_full_pair1) and their five table bytes each are combined by one v_dot2_i32_i16.
// ------------------------------------------------------------------------------------------
constexpr int kWide1LdsMax = kU1TableBytes + 3 * K3_PH * K3_PW;      // 98,656 (the tile of mulut_dev.h, K3_*)

// byte (Q1, J1) | byte (Q2, J2) << 16 of the 7 x 12-byte window
template <int Q1, int J1, int Q2, int J2>
__device__ __forceinline__ uint32_t wwin_pair(const uint32_t (&win)[7][3]) {
    static_assert(Q1 >= 0 && Q1 < 7 && Q2 >= 0 && Q2 < 7 && J1 >= 0 && J1 < 12 && J2 >= 0 && J2 < 12, "window is 7 rows x 12 bytes");
    constexpr uint32_t sel = 0x0C000C00u | ((uint32_t)(4 + (J2 & 3)) << 16) | (uint32_t)(J1 & 3);
    return __builtin_amdgcn_perm(win[Q2][J2 >> 2], win[Q1][J1 >> 2], sel);
}

// rotations R and R + 2 of pixel I (window column I + 3) for pattern PAT; returns sum + q * (both passes)
template <int PAT, int R, int I>
__device__ __forceinline__ int wide1_pair(const int8_t *s_lut, const uint32_t (&win)[7][3], uint32_t k0, uint32_t ta, int sum) {
    constexpr int H = kHalo3;
    constexpr int yb = rot_dy(R, kPatDi[PAT][0], kPatDj[PAT][0]), xb = rot_dx(R, kPatDi[PAT][0], kPatDj[PAT][0]);
    constexpr int yc = rot_dy(R, kPatDi[PAT][1], kPatDj[PAT][1]), xc = rot_dx(R, kPatDi[PAT][1], kPatDj[PAT][1]);
    constexpr int yd = rot_dy(R, kPatDi[PAT][2], kPatDj[PAT][2]), xd = rot_dx(R, kPatDi[PAT][2], kPatDj[PAT][2]);
    FullPair1 fp;      // rotation R + 2 displaces by the negated offsets
    simplex4_full_pair1(k0, wwin_pair<H + yb, I + H + xb, H - yb, I + H - xb>(win), wwin_pair<H + yc, I + H + xc, H - yc, I + H - xc>(win),
                        wwin_pair<H + yd, I + H + xd, H - yd, I + H - xd>(win), fp);
    uint32_t ra[4], rb[4];
    ra[0] = add_word<0>(ta, fp.base);
    rb[0] = add_word<1>(ta, fp.base);
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        ra[j + 1] = add_word<0>(ra[0], fp.cum[j]);
        rb[j + 1] = add_word<1>(rb[0], fp.cum[j]);
    }
    int va[5], vb[5];
#pragma unroll
    for (int j = 0; j < 5; ++j) {
        va[j] = (int)s_lut[ra[j < 4 ? j : 0] + (uint32_t)(j < 4 ? 0 : kAllStrides)];
        vb[j] = (int)s_lut[rb[j < 4 ? j : 0] + (uint32_t)(j < 4 ? 0 : kAllStrides)];
    }
#pragma unroll
    for (int j = 0; j < 5; ++j) {
        typedef short s16x2 __attribute__((ext_vector_type(2)));
        const uint32_t t = __builtin_amdgcn_perm((uint32_t)vb[j], (uint32_t)va[j], 0x05040100u);      // value of pass A | value of pass B
        sum = __builtin_amdgcn_sdot2(__builtin_bit_cast(s16x2, t), __builtin_bit_cast(s16x2, fp.w[j]), sum, false);
    }
    return sum;
}

// one mode (pattern PAT) over the thread's C x 4 sites; acc[4 c + i] = pixel i of channel c
template <int PAT>
__device__ __forceinline__ void wide1_mode(const int8_t *s_lut, const uint8_t *s_img, int ty, int x4, int C, int (&acc)[12]) {
    static_for<0, 3>([&](auto CC) {
        constexpr int c = CC;
        if (c < C) {          // workgroup-uniform
            const uint32_t *row = (const uint32_t *)(s_img + c * (K3_PH * K3_PW) + ty * K3_PW + x4);
            uint32_t win[7][3];
#pragma unroll
            for (int q = 0; q < 7; ++q)
#pragma unroll
                for (int k = 0; k < 3; ++k) win[q][k] = row[q * (K3_PW / 4) + k];
            static_for<0, 4>([&](auto II) {
                constexpr int i = II;
                constexpr int J = i + kHalo3;      // the pixel's window column
                const uint32_t va = (win[kHalo3][J >> 2] >> (8 * (J & 3))) & 0xFFu;
                uint32_t k0 = full1_anchor_key(va);
                const uint32_t ta = (va >> 4) * (uint32_t)kStrideA;
                int sum = wide1_pair<PAT, 0, i>(s_lut, win, k0, ta, acc[4 * c + i]);
                asm volatile("" : "+v"(sum), "+v"(k0));      // one pair at a time (register budget)
                acc[4 * c + i] = wide1_pair<PAT, 1, i>(s_lut, win, k0, ta, sum);
            });
        }
    });
}

__global__ void __launch_bounds__(K3_NT) stage_wide1_kernel(StageArgs a, PatternArgs wa) {
    constexpr int TW = K3_TW, TH = K3_TH, NT = K3_NT, PW = K3_PW, PH = K3_PH, HALO = kHalo3;
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    const int8_t *s_lut = (const int8_t *)smem;
    uint8_t *s_img = smem + kU1TableBytes;
    int n, y0, x0;
    decode_tile(a, xcd_remap(blockIdx.x, gridDim.x), n, y0, x0, TW, TH);

    // the table of the NEXT mode travels through registers: fetched (6 x 16 B per thread) while the current mode is being
    // computed, written to LDS between the two barriers of the swap
    static_assert((kU1TableBytes / 16 + NT - 1) / NT == 6, "six 16-byte chunks of the table per thread");
    constexpr int kVecs = kU1TableBytes / 16;
    const int c0 = (int)threadIdx.x, c5 = c0 + 5 * NT < kVecs ? c0 + 5 * NT : 0;   // chunk 5 exists for the first threads only
    uint4 n0, n1, n2, n3, n4, n5;
#define MULUT_W1_FETCH(LUT)                                                                                         \
    do {                                                                                                            \
        const uint4 *src_ = (const uint4 *)(LUT);                                                                   \
        n0 = src_[c0]; n1 = src_[c0 + NT]; n2 = src_[c0 + 2 * NT]; n3 = src_[c0 + 3 * NT]; n4 = src_[c0 + 4 * NT];  \
        n5 = src_[c5];                                                                                              \
    } while (0)
    MULUT_W1_FETCH(a.lut[0]);
    {   // image tile with a 3-px halo, edge-replicated at the true image borders only; rows clamped to the band the caller holds
        // ([oy0 - 3, oy1 + 3) is an identity for every row a valid site reads).  Every byte load in flight before the first store.
        constexpr int PER = (3 * PH * PW + NT - 1) / NT;
        const int total = a.C * PH * PW;
        const int ylo = imax(a.oy0 - HALO, 0), yhi = imin(a.oy1 + HALO, a.H) - 1;
        uint8_t v[PER];
#pragma unroll
        for (int k = 0; k < PER; ++k) {
            const int i = (int)threadIdx.x + k * NT;
            const int px = i % PW, py = (i / PW) % PH, c = imin(i / (PW * PH), a.C - 1);   // past the end: a valid address, never stored
            const int gy = imin(imax(y0 + py - HALO, ylo), yhi);
            const int gx = imin(imax(x0 + px - HALO, 0), a.W - 1);
            v[k] = *view_addr(a.in, n, c, gy, gx);
        }
#pragma unroll
        for (int k = 0; k < PER; ++k) {
            const int i = (int)threadIdx.x + k * NT;
            if (i < total) s_img[i] = v[k];
        }
    }
    const int x4 = (int)(threadIdx.x % (TW / 4)) * 4, ty = (int)(threadIdx.x / (TW / 4));
    int acc[12];   // [channel][pixel]
#pragma unroll
    for (int k = 0; k < 12; ++k) acc[k] = 0;

    for (int mv = 0; mv < a.M; ++mv) {
        const int m = __builtin_amdgcn_readfirstlane(mv);
        __syncthreads();  // everyone done with the previous table
        {
            uint4 *dst = (uint4 *)smem;
            dst[c0] = n0; dst[c0 + NT] = n1; dst[c0 + 2 * NT] = n2; dst[c0 + 3 * NT] = n3; dst[c0 + 4 * NT] = n4;
            if (c0 + 5 * NT < kVecs) dst[c0 + 5 * NT] = n5;
        }
        if (mv + 1 < a.M) MULUT_W1_FETCH(a.lut[__builtin_amdgcn_readfirstlane(mv + 1)]);
        __syncthreads();  // table and (m == 0) tile in place
        switch (wa.pat[m]) {      // scalar: the pattern id of the mode's letter
            case 0: wide1_mode<0>(s_lut, s_img, ty, x4, a.C, acc); break;
            case 1: wide1_mode<1>(s_lut, s_img, ty, x4, a.C, acc); break;
            case 2: wide1_mode<2>(s_lut, s_img, ty, x4, a.C, acc); break;
            case 3: wide1_mode<3>(s_lut, s_img, ty, x4, a.C, acc); break;
            case 4: wide1_mode<4>(s_lut, s_img, ty, x4, a.C, acc); break;
            default: wide1_mode<5>(s_lut, s_img, ty, x4, a.C, acc); break;
        }
    }
#undef MULUT_W1_FETCH
    const int y = y0 + ty;
    if (y < a.oy1) {
#pragma unroll
        for (int c = 0; c < 3; ++c)
            if (c < a.C) {
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const int x = x0 + x4 + i;
                    if (x < a.W) *const_cast<uint8_t *>(view_addr(a.out, n, c, y, x)) = (uint8_t)rhe_clip_u8(acc[c * 4 + i] + a.bias_num, a.div);
                }
            }
    }
}

// ------------------------------------------------------------------------------------------
// u*u-byte rows.  One thread = one LR pixel (32 x 8 tile, 256 threads), channels in sequence; the tile with a 3-px halo in LDS
// (3 x 14 x 38 B).  Per mode the pattern offsets are wave-uniform scalars from the kernel arguments; per rotation the 5 rows
// are accumulated as 16-bit fields (RotAcc); u == 4 merges rotation pairs for up to 4 modes and keeps one accumulator set per
// rotation beyond that (a merged field would overflow: 4 M 16 255 < 65536 only for M <= 4).
// ------------------------------------------------------------------------------------------
constexpr int KWU_TW = 32, KWU_TH = 8;

template <int U, bool MERGED>
__global__ void __launch_bounds__(KWU_TW * KWU_TH, 4) stage_wide_up_kernel(StageArgs a) {
    constexpr int TW = KWU_TW, TH = KWU_TH, NT = TW * TH, HALO = kHalo3;
    constexpr int PW = TW + 2 * HALO, PH = TH + 2 * HALO;
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    uint8_t *s_img = smem;
    int n, y0, x0;
    decode_tile(a, xcd_remap(blockIdx.x, gridDim.x), n, y0, x0, TW, TH);
    const int lt = threadIdx.x;
    {
        const int total = a.C * PH * PW;
        const int ylo = imax(a.oy0 - HALO, 0), yhi = imin(a.oy1 + HALO, a.H) - 1;
        for (int i = lt; i < total; i += NT) {
            const int px = i % PW, py = (i / PW) % PH, c = i / (PW * PH);
            const int gy = imin(imax(y0 + py - HALO, ylo), yhi);
            const int gx = imin(imax(x0 + px - HALO, 0), a.W - 1);
            s_img[i] = *view_addr(a.in, n, c, gy, gx);
        }
    }
    __syncthreads();
    const int tx = lt % TW, ty = lt / TW;
    const int y = y0 + ty, x = x0 + tx;
    if (y >= a.oy1 || x >= a.W) return;      // (no barrier below)
    for (int c = 0; c < a.C; ++c) {
        const uint8_t *ctr = s_img + c * (PH * PW) + (ty + HALO) * PW + (tx + HALO);
        const int va = ctr[0];
        RotAcc<U, MERGED> acc;
        acc.clear();
        for (int mv = 0; mv < a.M; ++mv) {
            const int m = __builtin_amdgcn_readfirstlane(mv);      // scalar loads of the mode's table pointer and offsets
            const void *lut = a.lut[m];
            const int di0 = a.di[m][0], di1 = a.di[m][1], di2 = a.di[m][2];
            const int dj0 = a.dj[m][0], dj1 = a.dj[m][1], dj2 = a.dj[m][2];
            static_for<0, 4>([&](auto R) {
                constexpr int r = R;
                int dy, dx, v0, v1, v2;
                sample_offset(r, di0, dj0, dy, dx); v0 = ctr[dy * PW + dx];
                sample_offset(r, di1, dj1, dy, dx); v1 = ctr[dy * PW + dx];
                sample_offset(r, di2, dj2, dy, dx); v2 = ctr[dy * PW + dx];
                pass_global<U, r>(lut, va, v0, v1, v2, a, acc);
            });
        }
        uint32_t o[U];
        finish_channel<U, kOutGeneric>(a, acc, n, c, y, x, o);
    }
}

void stage_wide_tile(int u, int &tw, int &th) {
    if (u == 1) { tw = K3_TW; th = K3_TH; }
    else { tw = KWU_TW; th = KWU_TH; }
}

const char *stage_wide_name(int u) {
    switch (u) {
        case 1: return "stage_wide1_kernel";
        case 2: return "stage_wide_up_kernel<2>";
        case 3: return "stage_wide_up_kernel<3>";
        default: return "stage_wide_up_kernel<4>";
    }
}

hipError_t launch_stage_wide1(const StageArgs &a, const PatternArgs &w, hipStream_t st) {
    if (a.C < 1 || a.C > 3 || a.M < 1 || a.M > kMaxModes) return hipErrorInvalidValue;
    for (int m = 0; m < a.M; ++m)
        if (w.pat[m] < 0 || w.pat[m] > 5) return hipErrorInvalidValue;
    const void *kern = (const void *)stage_wide1_kernel;
    {
        const hipError_t e = raise_lds_limit(kern, kWide1LdsMax);
        if (e != hipSuccess) return e;
    }
    const long long nb = (long long)a.N * a.tiles_x * a.tiles_y;
    if (nb <= 0 || nb > 0x7fffffffLL) return hipErrorInvalidValue;
    const size_t lds = (size_t)kU1TableBytes + (size_t)a.C * K3_PH * K3_PW;
    hipLaunchKernelGGL(stage_wide1_kernel, dim3((unsigned)nb), dim3(K3_NT), lds, st, a, w);
    return hipGetLastError();
}

template <int U, bool MERGED>
static hipError_t launch_wide_up_t(const StageArgs &a, hipStream_t st) {
    constexpr int tile_bytes = ((3 * (KWU_TH + 2 * kHalo3) * (KWU_TW + 2 * kHalo3) + 15) / 16) * 16;
    auto kern = stage_wide_up_kernel<U, MERGED>;
    {
        const hipError_t e = raise_lds_limit((const void *)kern, tile_bytes);
        if (e != hipSuccess) return e;
    }
    const long long nb = (long long)a.N * a.tiles_x * a.tiles_y;
    if (nb <= 0 || nb > 0x7fffffffLL) return hipErrorInvalidValue;
    hipLaunchKernelGGL(kern, dim3((unsigned)nb), dim3(KWU_TW * KWU_TH), (size_t)tile_bytes, st, a);
    return hipGetLastError();
}

hipError_t launch_stage_wide_up(const StageArgs &a, int u, hipStream_t st) {
    if (a.C < 1 || a.C > 3 || a.M < 1 || a.M > kMaxModes) return hipErrorInvalidValue;
    switch (u) {
        case 2: return launch_wide_up_t<2, false>(a, st);
        case 3: return launch_wide_up_t<3, false>(a, st);
        case 4: return a.M <= 4 ? launch_wide_up_t<4, true>(a, st) : launch_wide_up_t<4, false>(a, st);
        default: return hipErrorInvalidValue;
    }
}

}  // namespace mulut
