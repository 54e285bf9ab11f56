// mulut_interval.hip -- stages and passes of contexts configured at the sampling intervals 5 and 6 (q = 32 / 64, tables of
// L^4 = 9^4 / 5^4 rows).  Every stage of such a context runs here, whatever its mode list (any mix of the six patterns) and
// upscale; the interval-4 kernels of the other translation units are not involved (their tube bands, slabs and 16-bit sums are
// built for q = 16 and 17^4-row tables).  Tables are plain int8 rows (mulut_interval.h iv_row_bytes); sums are 32-bit.
//   stage_interval_kernel<IV, U, LDS>  64 x 64 tiles with a 3-px halo in LDS (one family serves all six patterns), 1024 threads,
//                                      four horizontally adjacent pixels per thread.  LDS = true: the whole stage's tables
//                                      (M * iv_table_bytes <= kIvLdsBudget) are staged into LDS once per persistent workgroup
//                                      next to the tile; LDS = false: the five rows of a pass are gathered from the tables in
//                                      global memory (26-105 KB per mode: L2-resident), one vector load per row
// One template instance of the pass body per pattern, chosen by the mode letter (scalar switch), as stage_u1w_kernel of mulut_k1.hip does from the offsets.
// mulut_pass at these intervals is pass_kernel<IV> of mulut_kernels.hip.
#include <hip/hip_runtime.h>

#include "mulut_dev.h"
#include "mulut_interval.h"

namespace mulut {

constexpr int kIvImgBytes = 3 * K3_PH * K3_PW;      // the tile of mulut_dev.h (K3_*: 64 x 64, 3-px halo), 15,120 for C = 3
static_assert(kIvLdsBudget + kIvImgBytes <= 160 * 1024, "tables and tile fit one CU's LDS");

// one table row of U*U int8 values (U > 1): dwords of iv_row_bytes(U), from LDS or global memory
template <int U>
__device__ __forceinline__ void iv_row(const uint8_t *tab, int idx, uint32_t (&row)[row_dwords(U)]) {
    if constexpr (U == 4) {
        const uint4 v = *(const uint4 *)(tab + ((uint32_t)idx << 4));
        row[0] = v.x; row[1] = v.y; row[2] = v.z; row[3] = v.w;
    } else {
        const uint32_t *p = (const uint32_t *)(tab + (uint32_t)idx * (uint32_t)iv_row_bytes(U));
#pragma unroll
        for (int k = 0; k < row_dwords(U); ++k) row[k] = p[k];
    }
}

template <int E, int RW>
__device__ __forceinline__ int iv_elem(const uint32_t (&row)[RW]) {
    return (int)(int8_t)(uint8_t)(row[E >> 2] >> (8 * (E & 3)));
}

// pass (pattern PAT, rotation R) of the site whose anchor sits at ctr in the LDS tile: acc[block position] += q * pred
template <int IV, int U, int PAT, int R>
__device__ __forceinline__ void iv_pass(const uint8_t *tab, const uint8_t *ctr, int (&acc)[U * U]) {
    constexpr int yb = rot_dy(R, kPatDi[PAT][0], kPatDj[PAT][0]), xb = rot_dx(R, kPatDi[PAT][0], kPatDj[PAT][0]);
    constexpr int yc = rot_dy(R, kPatDi[PAT][1], kPatDj[PAT][1]), xc = rot_dx(R, kPatDi[PAT][1], kPatDj[PAT][1]);
    constexpr int yd = rot_dy(R, kPatDi[PAT][2], kPatDj[PAT][2]), xd = rot_dx(R, kPatDi[PAT][2], kPatDj[PAT][2]);
    int idx[5], w[5];
    simplex4_iv<IV>(ctr[0], ctr[yb * K3_PW + xb], ctr[yc * K3_PW + xc], ctr[yd * K3_PW + xd], idx, w);
    if constexpr (U == 1) {
#pragma unroll
        for (int j = 0; j < 5; ++j) acc[0] += w[j] * (int)(int8_t)tab[idx[j]];
    } else {
        constexpr int RW = row_dwords(U);
        uint32_t row[5][RW];
#pragma unroll
        for (int j = 0; j < 5; ++j) iv_row<U>(tab, idx[j], row[j]);
        static_for<0, U * U>([&](auto P) {
            constexpr int p = P;
            constexpr int e = row_elem(R, p / U, p % U, U);      // the row element that lands on block position p
            int s = acc[p];
#pragma unroll
            for (int j = 0; j < 5; ++j) s += w[j] * iv_elem<e, RW>(row[j]);
            acc[p] = s;
        });
    }
}

// the four rotations one after the other: the scheduler may not hoist a later pass's row loads over an earlier pass's MACs (with
// u*u-byte rows that would hold 5 rows per pass in flight, beyond the 128 VGPRs of a 1024-thread workgroup)
template <int IV, int U, int PAT>
__device__ __forceinline__ void iv_mode(const uint8_t *tab, const uint8_t *ctr, int (&acc)[U * U]) {
    static_for<0, 4>([&](auto R) {
        iv_pass<IV, U, PAT, R>(tab, ctr, acc);
        if constexpr (U > 2) __builtin_amdgcn_sched_barrier(0);
    });
}

template <int IV, int U, bool LDS>
__global__ void __launch_bounds__(K3_NT) stage_interval_kernel(StageArgs a, IvArgs v) {
    constexpr int TW = K3_TW, TH = K3_TH, NT = K3_NT, PW = K3_PW, PH = K3_PH, HALO = kHalo3;
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    uint8_t *s_img = smem + (LDS ? a.M * v.table_bytes : 0);
    if constexpr (LDS) {      // every table of the stage, once per workgroup (the first barrier of the tile loop publishes them)
        const int chunks = v.table_bytes / 16;
        for (int m = 0; m < a.M; ++m) {
            const uint4 *src = (const uint4 *)a.lut[m];
            uint4 *dst = (uint4 *)(smem + m * v.table_bytes);
            for (int i = (int)threadIdx.x; i < chunks; i += NT) dst[i] = src[i];
        }
    }
    const int ntiles = a.N * a.tiles_x * a.tiles_y;
    const int ty = (int)threadIdx.x / (TW / 4), x4 = ((int)threadIdx.x % (TW / 4)) * 4;
    // rows are clamped to the band the caller holds ([oy0 - reach, oy1 + reach) is an identity for every row a valid site reads)
    const int ylo = imax(a.oy0 - v.reach, 0), yhi = imin(a.oy1 + v.reach, a.H) - 1;
    for (int t = (int)blockIdx.x; t < ntiles; t += (int)gridDim.x) {
        int n, y0, x0;
        decode_tile(a, (int)gridDim.x == ntiles ? xcd_remap(t, ntiles) : t, n, y0, x0, TW, TH);
        __syncthreads();      // everyone done with the previous tile
        {   // image tile with a 3-px halo, edge-replicated at the true image borders; every byte load in flight before the first store
            constexpr int PER = (3 * PH * PW + NT - 1) / NT;
            const int total = a.C * PH * PW;
            int tid = (int)threadIdx.x;
            asm volatile("" : "+v"(tid));      // recomputed per tile: hoisted out of the loop, the PER index triples would pin 45 VGPRs
            uint8_t b[PER];
#pragma unroll
            for (int k = 0; k < PER; ++k) {
                const int i = tid + k * NT;
                const int px = i % PW, py = (i / PW) % PH, c = imin(i / (PW * PH), a.C - 1);   // past the end: a valid address, never stored
                const int gy = imin(imax(y0 + py - HALO, ylo), yhi);
                const int gx = imin(imax(x0 + px - HALO, 0), a.W - 1);
                b[k] = *view_addr(a.in, n, c, gy, gx);
            }
#pragma unroll
            for (int k = 0; k < PER; ++k) {
                const int i = tid + k * NT;
                if (i < total) s_img[i] = b[k];
            }
        }
        __syncthreads();      // tile (and, on the first tile, the tables) in place
        const int y = y0 + ty;
        if (y >= a.oy1) continue;      // (no barrier before the next iteration's first one)
        #pragma unroll 1
        for (int i = 0; i < 4; ++i) {
            const int x = x0 + x4 + i;
            if (x >= a.W) break;
            #pragma unroll 1
            for (int c = 0; c < a.C; ++c) {
                const uint8_t *ctr = s_img + c * (PH * PW) + (ty + HALO) * PW + (x4 + i + HALO);
                int acc[U * U];
#pragma unroll
                for (int p = 0; p < U * U; ++p) acc[p] = 0;
                #pragma unroll 1
                for (int mv = 0; mv < a.M; ++mv) {
                    const int m = __builtin_amdgcn_readfirstlane(mv);
                    const uint8_t *tab = LDS ? smem + m * v.table_bytes : (const uint8_t *)a.lut[m];
                    switch (v.pat[m]) {      // scalar: the pattern id of the mode's letter
                        case 0: iv_mode<IV, U, 0>(tab, ctr, acc); break;
                        case 1: iv_mode<IV, U, 1>(tab, ctr, acc); break;
                        case 2: iv_mode<IV, U, 2>(tab, ctr, acc); break;
                        case 3: iv_mode<IV, U, 3>(tab, ctr, acc); break;
                        case 4: iv_mode<IV, U, 4>(tab, ctr, acc); break;
                        default: iv_mode<IV, U, 5>(tab, ctr, acc); break;
                    }
                }
                static_for<0, U>([&](auto SY) {
                    constexpr int sy = SY;
                    uint8_t *dst = const_cast<uint8_t *>(view_addr(a.out, n, c, y * U + sy, x * U));
                    uint32_t o[U];
#pragma unroll
                    for (int sx = 0; sx < U; ++sx) o[sx] = rhe_clip_u8_iv<IV>(acc[sy * U + sx] + v.bias_num, v.dm);
                    if (U == 4 && a.out.sX == 1 && ((uintptr_t)dst & 3) == 0) {      // planar output: one dword per block row
                        *(uint32_t *)dst = o[0] | (o[U > 1 ? 1 : 0] << 8) | (o[U > 2 ? 2 : 0] << 16) | (o[U > 3 ? 3 : 0] << 24);
                    } else {
#pragma unroll
                        for (int sx = 0; sx < U; ++sx) dst[(long long)sx * a.out.sX] = (uint8_t)o[sx];
                    }
                });
            }
        }
    }
}

void stage_interval_tile(int &tw, int &th) {
    tw = K3_TW;
    th = K3_TH;
}

const char *stage_interval_name(int interval, int u, bool lds) {
    static const char *const names[2][4][2] = {
        {{"stage_interval_kernel<5,1,global>", "stage_interval_kernel<5,1,lds>"}, {"stage_interval_kernel<5,2,global>", "stage_interval_kernel<5,2,lds>"},
         {"stage_interval_kernel<5,3,global>", "stage_interval_kernel<5,3,lds>"}, {"stage_interval_kernel<5,4,global>", "stage_interval_kernel<5,4,lds>"}},
        {{"stage_interval_kernel<6,1,global>", "stage_interval_kernel<6,1,lds>"}, {"stage_interval_kernel<6,2,global>", "stage_interval_kernel<6,2,lds>"},
         {"stage_interval_kernel<6,3,global>", "stage_interval_kernel<6,3,lds>"}, {"stage_interval_kernel<6,4,global>", "stage_interval_kernel<6,4,lds>"}}};
    if ((interval != 5 && interval != 6) || u < 1 || u > 4) return "";
    return names[interval - 5][u - 1][lds ? 1 : 0];
}

template <int IV, int U, bool LDS>
static hipError_t launch_interval_t(const StageArgs &a, const IvArgs &v, int num_cus, hipStream_t st) {
    const void *kern = (const void *)stage_interval_kernel<IV, U, LDS>;
    const size_t tables = LDS ? (size_t)a.M * v.table_bytes : 0;
    if (tables > (size_t)kIvLdsBudget) return hipErrorInvalidValue;
    {
        const hipError_t e = raise_lds_limit(kern, (LDS ? kIvLdsBudget : 0) + kIvImgBytes);
        if (e != hipSuccess) return e;
    }
    const long long nt = (long long)a.N * a.tiles_x * a.tiles_y;
    if (nt <= 0 || nt > 0x7fffffffLL) return hipErrorInvalidValue;
    // LDS: persistent workgroups (the tables are staged once per workgroup), two per CU while both fit its LDS
    long long nb = nt;
    if (LDS) {
        const long long per_cu = tables + kIvImgBytes <= 80 * 1024 ? 2 : 1;
        nb = nt < per_cu * num_cus ? nt : per_cu * num_cus;
    }
    hipLaunchKernelGGL((stage_interval_kernel<IV, U, LDS>), dim3((unsigned)nb), dim3(K3_NT), tables + (size_t)a.C * K3_PH * K3_PW, st, a, v);
    return hipGetLastError();
}

template <int IV>
static hipError_t launch_interval_iv(const StageArgs &a, const IvArgs &v, int u, bool lds, int num_cus, hipStream_t st) {
    switch (u * 2 + (lds ? 1 : 0)) {
        case 2: return launch_interval_t<IV, 1, false>(a, v, num_cus, st);
        case 3: return launch_interval_t<IV, 1, true>(a, v, num_cus, st);
        case 4: return launch_interval_t<IV, 2, false>(a, v, num_cus, st);
        case 5: return launch_interval_t<IV, 2, true>(a, v, num_cus, st);
        case 6: return launch_interval_t<IV, 3, false>(a, v, num_cus, st);
        case 7: return launch_interval_t<IV, 3, true>(a, v, num_cus, st);
        case 8: return launch_interval_t<IV, 4, false>(a, v, num_cus, st);
        case 9: return launch_interval_t<IV, 4, true>(a, v, num_cus, st);
        default: return hipErrorInvalidValue;
    }
}

hipError_t launch_stage_interval(const StageArgs &a, const IvArgs &v, int interval, int u, bool lds, int num_cus, hipStream_t st) {
    if (a.C < 1 || a.C > 3 || a.M < 1 || a.M > kMaxModes || v.reach < 2 || v.reach > kHalo3 || num_cus < 1) return hipErrorInvalidValue;
    for (int m = 0; m < a.M; ++m)
        if (v.pat[m] < 0 || v.pat[m] > 5) return hipErrorInvalidValue;
    if (interval == 5) return launch_interval_iv<5>(a, v, u, lds, num_cus, st);
    if (interval == 6) return launch_interval_iv<6>(a, v, u, lds, num_cus, st);
    return hipErrorInvalidValue;
}

}  // namespace mulut
