// mulut_ft_interval.hip -- LUT-aware fine-tuning at the sampling intervals 5 and 6 (q = 32 / 64, tables of 9^4 / 5^4 rows).
//
// Reference: MuLUT.InterpTorchBatch + MuLUT.forward with interval = 5 / 6, sr/model.py:42-44, 69-312 (driver
// sr/3_finetune_lut.py:82,166).  The arithmetic is that of mulut_ft.hip with q = 2^IV: per pass the float32 expression
//   ((((q-f1)*p0 + (f1-f2)*p1) + (f2-f3)*p2) + (f3-f4)*p3) + f4*p4, /q   (no FMA contraction),
// pred = round(pred + pass) after EVERY pass (:308), stage output round(clamp(pred/avg + bias, 0, 255)) (:309), rounding a BPDA
// identity in the backward, the clamp passing gradient on [0, 255] inclusive.  The per-pass set-up is mulut_ft_interval.h.
//
// What is different from interval 4 is the size of the tables: 625 rows (interval 6) or 6,561 rows (interval 5) instead of
// 83,521.  The interval-4 kernels keep a 1041-slot band of the table gradient in LDS; here the WHOLE gradient table of a mode
// is an LDS image wherever rows * u*u floats fit kFtIvLdsBudget -- all of interval 6, interval 5 at u = 1 and 2 -- and the
// forward stages the stage's tables themselves into LDS under the same rule.
//   ft_interval_stage_fwd<IV, U, LDS>   one site per thread, persistent workgroups when the tables are staged (LDS)
//   ft_interval_stage_bwd<IV, U, RES, HALO>
//                                       one site per thread (u = 1, 2, 3).  Modes are walked one at a time, so one image serves
//                                       any number of modes.  Per vertex the lanes of a 16-lane row that share the row leader's
//                                       table row are summed by DPP and added once, row-wide (lane l adds element l); the
//                                       others add on their own.  RES: into the image, flushed once per workgroup and mode as
//                                       contiguous memory-side atomics; else (interval 5, u = 3) straight to memory.
//   ft_interval_stage_bwd4<IV, RES, HALO>
//                                       u = 4: the design of ft_stage_bwd4 -- 16 lanes (= row elements) own a 4 x 4 block of
//                                       sites and a private 16-entry cache of gradient rows, read + add + write, no atomic -- with
//                                       the cache keyed by the CORNER of the MSB cell (ft_iv_corner): cells are 32 / 64 grey
//                                       levels wide, so a block of smooth content stays in one cell and its 16 corners never
//                                       evict one another.  An evicted entry goes into the image (RES, interval 6: ds_add_f32).
//                                       Interval 5 (420 KB per table) keeps a BAND instead: the 121 rows whose MSBs span at most
//                                       one step (7.6 KB) -- the rows natural crops touch -- flushed like an image; an entry
//                                       outside the band goes to memory as a row-wide atomic (16 lanes, one 64-byte segment).
//                                       (Measured without the band, every eviction a memory-side atomic: 2.28 ms per launch on
//                                       config 4's batch against 1.24 ms at interval 6 -- the hot rows serialise.)
// Both backward kernels run persistent workgroups over several tiles of sites: the image is zeroed and flushed once per
// workgroup and mode, not once per 256 sites.  HALO (2 or 3) is the halo of their input-gradient tiles, as in mulut_ft.hip: 2 for
// lists of s, d, y, 3 with one of e, h, o in the list; the HALO = 2 instances are the kernels as they were before the 4 x 4 patterns.
#include <hip/hip_runtime.h>

#include <cstring>

#include "mulut_kernels.h"

#pragma clang fp contract(off)

#include "mulut_ft_interval.h"

namespace mulut {

// The one LDS rule of this file: the stage's float tables (forward: all M of them) or one mode's gradient image (backward) live
// in LDS when they take at most this many bytes; the rest of a CU's 160 KB is for what the kernel keeps beside them (at most
// 24 KB + the u = 4 backward's 77 KB, which only ever meets the 40 KB image of interval 6).
constexpr int kFtIvLdsBudget = 120 * 1024;

// (the argument struct, FtIvArgs: mulut_ft.h)
template <int IV>
__device__ __forceinline__ void ftiv_pass_setup(const float *plane, int H, int W, int y, int x, int r, const int (&di)[3], const int (&dj)[3],
                                                FtIvPass &p) {
    float v[4];
    v[0] = plane[y * W + x];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        int dy, dx;
        sample_offset(r, di[k], dj[k], dy, dx);
        v[k + 1] = plane[imin(imax(y + dy, 0), H - 1) * W + imin(imax(x + dx, 0), W - 1)];
    }
    ft_iv_pass<IV>(v, p);
}

// ---------------------------------------------------------------------------------------------------------------- forward
constexpr int kFtIvFwdNT = 512;

template <int IV, int U, bool LDS>
__global__ void __launch_bounds__(kFtIvFwdNT) ft_interval_stage_fwd(FtIvArgs a) {
    using G = IvGeom<IV>;
    constexpr int EL = U * U, NT = kFtIvFwdNT, TAB = G::rows * EL;
    extern __shared__ __attribute__((aligned(16))) float ftiv_tab[];
    if constexpr (LDS) {      // every table of the stage, once per workgroup
        for (int m = 0; m < a.M; ++m) {
            const float *src = a.w[m];
            for (int i = (int)threadIdx.x; i < TAB; i += NT) ftiv_tab[m * TAB + i] = src[i];
        }
        __syncthreads();
    }
    const long long nsite = (long long)a.B * a.C * a.H * a.W;
    const long long ntile = (nsite + NT - 1) / NT;
    const float avg = a.is_last ? (float)a.M : (float)(4 * a.M), bias = a.is_last ? 0.0f : 127.0f;
    for (long long t = blockIdx.x; t < ntile; t += gridDim.x) {
        const long long s = t * NT + threadIdx.x;
        if (s >= nsite) continue;
        const int x = (int)(s % a.W), y = (int)((s / a.W) % a.H);
        const long long bc = s / ((long long)a.W * a.H);
        const float *plane = a.x + bc * a.H * a.W;
        float pred[EL];
#pragma unroll
        for (int e = 0; e < EL; ++e) pred[e] = 0.0f;
        for (int m = 0; m < a.M; ++m) {
            const int di[3] = {a.di[m][0], a.di[m][1], a.di[m][2]}, dj[3] = {a.dj[m][0], a.dj[m][1], a.dj[m][2]};
            static_for<0, 4>([&](auto R) {
                constexpr int r = R;
                FtIvPass p;
                ftiv_pass_setup<IV>(plane, a.H, a.W, y, x, r, di, dj, p);
                auto row = [&](int j, int e) -> float {
                    if constexpr (LDS) return ftiv_tab[m * TAB + p.idx[j] * EL + e];
                    else return a.w[m][p.idx[j] * EL + e];
                };
                static_for<0, EL>([&](auto E) {
                    constexpr int eo = E;                                   // block position sy*U+sx
                    constexpr int e = row_elem(r, eo / U, eo % U, U);       // table element landing there
                    const float val = ((((p.wt[0] * row(0, e) + p.wt[1] * row(1, e)) + p.wt[2] * row(2, e)) + p.wt[3] * row(3, e)) +
                                       p.wt[4] * row(4, e)) / (float)G::q;
                    pred[eo] = rintf(pred[eo] + val);                       // pred += ...; pred = round_func(pred)
                });
            });
        }
        float *po = a.out + bc * (long long)(a.H * U) * (a.W * U);
        uint32_t inside = 0;
        static_for<0, EL>([&](auto E) {
            constexpr int eo = E;
            const float t0 = pred[eo] / avg + bias;
            inside |= (t0 >= 0.0f && t0 <= 255.0f) ? 1u << eo : 0u;
            po[(long long)(y * U + eo / U) * (a.W * U) + (x * U + eo % U)] = rintf(fminf(fmaxf(t0, 0.0f), 255.0f));
        });
        a.inside[s] = (uint16_t)inside;
    }
}

// --------------------------------------------------------------------------------------------------------------- backward
// (the LDS float add and the DPP row helpers: mulut_ft.h)
// g = dL/d pred of one site: the clamp's mask saved by the forward, then d(pred / avg).  (The mask branch of mulut_ft.hip's
// ft_site_g, which stays in place there: called as a helper it moved the code of three timed backward kernels.)
template <int U, class F>
__device__ __forceinline__ void ftiv_site_g(const FtIvArgs &a, long long bc, int y, int x, bool valid, F &&put) {
    const float avg = a.is_last ? (float)a.M : (float)(4 * a.M);
    const float *pg = a.gout + bc * (long long)(a.H * U) * (a.W * U);
    const uint32_t inside = valid ? a.inside[(bc * a.H + y) * a.W + x] : 0u;
    static_for<0, U * U>([&](auto E) {
        constexpr int eo = E;
        const float go = pg[(long long)(y * U + eo / U) * (a.W * U) + (x * U + eo % U)];
        put(eo, ((inside >> eo) & 1u) ? go / avg : 0.0f);
    });
}

constexpr int kFtIvNT = 256;           // threads = sites of a tile (ft_interval_stage_bwd)
constexpr int kFtIvGxTile = 1024;      // floats of a wave's input-gradient tile
template <int U> constexpr int ftiv_bwd_lds(int image_floats) { return (image_floats + (kFtIvNT / 64) * kFtIvGxTile + kFtIvNT * (U * U + 1)) * 4; }

// One site per thread.  The input gradient uses the wave-private padded tile of ft_stage_bwd (the key offsets of a pattern are the
// same <= HALO pixels at every interval): a pass gives d/d f of each key to that key's pixel; the site's own pixel is summed in a
// register, keys b, c, d hit 64 different positions of the wave's tile -- a plain LDS read + add + write, folded onto the image
// (replicate padding) at the end of the tile; crops too wide for the tile add to memory.
template <int IV, int U, bool RES, int HALO>
__global__ void __launch_bounds__(kFtIvNT) ft_interval_stage_bwd(FtIvArgs a) {
    static_assert(HALO == 2 || HALO == 3, "halo of the input-gradient tile");
    using G = IvGeom<IV>;
    constexpr int EL = U * U, NT = kFtIvNT, IMG = RES ? G::rows * EL : 0;
    extern __shared__ __attribute__((aligned(16))) float ftiv_smem[];
    float *s_img = ftiv_smem;                                          // [rows][EL], RES only
    float *s_gxt = ftiv_smem + IMG;                                    // [NT / 64][kFtIvGxTile]
    float (*s_g)[EL + 1] = (float (*)[EL + 1])(s_gxt + (NT / 64) * kFtIvGxTile);
    const long long nsite = (long long)a.B * a.C * a.H * a.W;
    const long long ntile = (nsite + NT - 1) / NT;
    const long long t0 = (long long)blockIdx.x * a.tiles_per_wg, t1 = t0 + a.tiles_per_wg < ntile ? t0 + a.tiles_per_wg : ntile;
    const int lane = (int)threadIdx.x & 63, l16 = (int)threadIdx.x & 15;
    float *tile = s_gxt + (threadIdx.x >> 6) * kFtIvGxTile;
    const int PWd = a.W + 2 * HALO, PHt = a.H + 2 * HALO;
    auto padded_row = [&](long long R) { return R + 2 * HALO * (R / a.H) + HALO; };      // stacked image row (plane * H + y) -> row of the padded stack
    for (int m = 0; m < a.M; ++m) {
        const float *tab = a.w[m];
        float *gtab = a.gw[m];
        const int di[3] = {a.di[m][0], a.di[m][1], a.di[m][2]}, dj[3] = {a.dj[m][0], a.dj[m][1], a.dj[m][2]};
        if constexpr (RES) {
            for (int i = threadIdx.x; i < IMG; i += NT) s_img[i] = 0.0f;
            __syncthreads();      // the image is zero before any wave adds into it
        }
        for (long long t = t0; t < t1; ++t) {
            const long long s = t * NT + threadIdx.x;
            const bool valid = s < nsite;
            const long long sc = valid ? s : nsite - 1;      // surplus threads shadow the last site and contribute nothing
            const int x = (int)(sc % a.W), y = (int)((sc / a.W) % a.H);
            const long long bc = sc / ((long long)a.W * a.H);
            const float *plane = a.x + bc * a.H * a.W;
            float *gplane = a.gx + bc * a.H * a.W;
            const long long w0 = t * NT + (threadIdx.x & ~63u);
            const long long R0 = (w0 < nsite ? w0 : nsite - 1) / a.W, R1 = (w0 + 63 < nsite ? w0 + 63 : nsite - 1) / a.W;
            const long long pr0 = padded_row(R0) - HALO;
            const long long t_rows = padded_row(R1) + HALO - pr0 + 1;
            const int t_n = t_rows * PWd <= kFtIvGxTile ? (int)(t_rows * PWd) : 0;      // 0: does not fit
            for (int i = lane; i < t_n; i += 64) tile[i] = 0.0f;                        // (wave-private, and LDS serves a wave in order: no barrier)
            const int t_own = (int)(padded_row(bc * a.H + y) - pr0) * PWd + x + HALO;
            // (own row of s_g only: written and read by this thread)
            ftiv_site_g<U>(a, bc, y, x, valid, [&](int eo, float v) { s_g[threadIdx.x][eo] = v; });
            float own = 0.0f;
#pragma unroll 1
            for (int r = 0; r < 4; ++r) {
                FtIvPass p;
                ftiv_pass_setup<IV>(plane, a.H, a.W, y, x, r, di, dj, p);
                float gr[EL];      // g by TABLE element under this rotation
#pragma unroll
                for (int e = 0; e < EL; ++e) gr[e] = s_g[threadIdx.x][eo_of_elem<U>(r, e)];
                float dsum[5];     // sum_e g * p_j[e]
#pragma unroll
                for (int j = 0; j < 5; ++j) {
                    const float *row = tab + p.idx[j] * EL;
                    float acc = 0.0f;
#pragma unroll
                    for (int e = 0; e < EL; ++e) acc += gr[e] * row[e];
                    dsum[j] = acc;
                    // table gradient of the vertex: w_j / q * g.  Neighbouring sites of smooth content hit the SAME row: the lanes of a
                    // 16-lane row that share the row leader's table row are summed by DPP (every lane gets every sum; lane l keeps
                    // element l) and added once, row-wide; the others add on their own.  (All 256 threads are here: the broadcast and
                    // the row sums read every lane.)
                    const float wq = valid ? p.wt[j] / (float)G::q : 0.0f;
                    const int lead = ft_bcast<0>(p.idx[j]);
                    const bool with_lead = p.idx[j] == lead;
                    float mine = 0.0f;
#pragma unroll
                    for (int e = 0; e < EL; ++e) {
                        const float sum = ft_sum16(with_lead ? wq * gr[e] : 0.0f);
                        if (EL == 1 || l16 == e) mine = sum;
                    }
                    if (l16 < EL && mine != 0.0f) {
                        if constexpr (RES) lds_add_f32(&s_img[lead * EL + l16], mine);
                        else atomicAdd(&gtab[lead * EL + l16], mine);
                    }
                    if (!with_lead) {
#pragma unroll
                        for (int e = 0; e < EL; ++e) {
                            const float v = wq * gr[e];
                            if (v != 0.0f) {
                                if constexpr (RES) lds_add_f32(&s_img[p.idx[j] * EL + e], v);
                                else atomicAdd(&gtab[p.idx[j] * EL + e], v);
                            }
                        }
                    }
                }
                // d/d f of rank j = (p_{j+1} - p_j) . g / q belongs to the key of that rank
                float df[4];
#pragma unroll
                for (int j = 0; j < 4; ++j) df[j] = (dsum[j + 1] - dsum[j]) / (float)G::q;
                const int o0 = p.ord & 3, o1 = (p.ord >> 2) & 3, o2 = (p.ord >> 4) & 3;
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const float dk = o0 == k ? df[0] : o1 == k ? df[1] : o2 == k ? df[2] : df[3];
                    if (k == 0) own += dk;
                    else {
                        int dy, dx;
                        sample_offset(r, di[k - 1], dj[k - 1], dy, dx);
                        if (t_n) {
                            if (valid) {      // (a surplus thread shadows the last site: its read + add + write would race with that site's)
                                float *tp = tile + t_own + dy * PWd + dx;
                                *tp = *tp + dk;
                            }
                        } else if (valid && dk != 0.0f) atomicAdd(&gplane[imin(imax(y + dy, 0), a.H - 1) * a.W + imin(imax(x + dx, 0), a.W - 1)], dk);
                    }
                }
            }
            // the wave's tile onto the image: padded row / column -> plane and pixel, clamped into the plane (replicate padding)
            if (t_n) {
                if (valid) tile[t_own] += own;
                for (int i = lane; i < t_n; i += 64) {
                    const float v = tile[i];
                    if (v == 0.0f) continue;
                    const long long pr = pr0 + i / PWd;
                    const int cx = i % PWd - HALO, yy = (int)(pr % PHt) - HALO;
                    const long long pl = pr / PHt;
                    if (pl < (long long)a.B * a.C) atomicAdd(&a.gx[(pl * a.H + imin(imax(yy, 0), a.H - 1)) * a.W + imin(imax(cx, 0), a.W - 1)], v);
                }
            } else if (valid && own != 0.0f) atomicAdd(&gplane[y * a.W + x], own);
        }
        if constexpr (RES) {
            // the workgroup's image into the table gradient: contiguous floats, a wave adds 256 bytes at a time
            lds_adds_done();
            __syncthreads();
            for (int i = threadIdx.x; i < IMG; i += NT) {
                const float v = s_img[i];
                if (v != 0.0f) atomicAdd(&gtab[i], v);
            }
            __syncthreads();
        }
    }
}

// u = 4: 16 lanes per table row.  LDS: [ image rows x 16 f32 (RES) or band 121 x 16 f32 ][ g of the sites, 17 floats each ][ caches: 16 x 16 f32 per group ]
//        [ tags: 16 per group ][ input-gradient tiles: (4 + 2 HALO)^2 f32 per group ]
constexpr int kFtIvB4Sites = 512, kFtIvB4Groups = kFtIvB4Sites / 16;
constexpr int ftiv_b4_tile(int halo) { return (4 + 2 * halo) * (4 + 2 * halo); }      // floats of a group's input-gradient tile
constexpr int ftiv_bwd4_lds(int image_floats, int halo) {
    return image_floats * 4 + kFtIvB4Sites * 17 * 4 + kFtIvB4Groups * 16 * 16 * 4 + kFtIvB4Groups * 16 * 4 + kFtIvB4Groups * ftiv_b4_tile(halo) * 4;
}
static_assert(ftiv_bwd4_lds(IvGeom<6>::rows * 16, 2) <= 160 * 1024 && kFtIvLdsBudget + ftiv_bwd_lds<2>(0) <= 160 * 1024, "LDS");
static_assert(ftiv_bwd4_lds(IvGeom<6>::rows * 16, 3) == ftiv_bwd4_lds(IvGeom<6>::rows * 16, 2) + 32 * 144 &&
              ftiv_bwd4_lds(IvGeom<6>::rows * 16, 3) <= 160 * 1024, "LDS, HALO = 3");

// The band of a table that does not fit: the rows whose four MSBs span at most one step -- (L - 1) * 15 + 1 of them, 121 at
// interval 5, the rows a batch of natural crops touches (smooth content lives next to the diagonal of the grid).  Slot of a row:
// 15 * (smallest MSB) + (which of the four MSBs are one step above it, key a in bit 3), -1 outside the band.
template <int IV> constexpr int kFtIvBandRows = (IvGeom<IV>::L - 1) * 15 + 1;
template <int IV>
__device__ __forceinline__ int ftiv_band_slot(int row) {
    using G = IvGeom<IV>;
    const int A = row / G::sA, B = row / G::sB % G::L, C = row / G::sC % G::L, D = row % G::L;
    const int mn = imin(imin(A, B), imin(C, D)), mx = imax(imax(A, B), imax(C, D));
    if (mx - mn > 1) return -1;
    return mn * 15 + (mx == mn ? 0 : ((A - mn) << 3) | ((B - mn) << 2) | ((C - mn) << 1) | (D - mn));
}
template <int IV>
__device__ __forceinline__ int ftiv_band_row(int slot) {
    using G = IvGeom<IV>;
    const int n = slot / 15, mask = slot % 15;
    return n * G::all + ((mask >> 3) & 1) * G::sA + ((mask >> 2) & 1) * G::sB + ((mask >> 1) & 1) * G::sC + (mask & 1);
}

template <int IV, bool RES, int HALO>
__global__ void __launch_bounds__(kFtIvB4Sites) ft_interval_stage_bwd4(FtIvArgs a) {
    static_assert(HALO == 2 || HALO == 3, "halo of the input-gradient tile");
    using G = IvGeom<IV>;
    constexpr int U = 4, EL = 16, NT = kFtIvB4Sites, NG = kFtIvB4Groups, IMG = (RES ? G::rows : kFtIvBandRows<IV>) * EL;
    constexpr int TW = 4 + 2 * HALO, TN = ftiv_b4_tile(HALO);
    extern __shared__ __attribute__((aligned(16))) float ftiv_smem[];
    float *s_img = ftiv_smem;
    float (*s_g)[17] = (float (*)[17])(ftiv_smem + IMG);
    float *s_cache = ftiv_smem + IMG + NT * 17;
    int *s_tag = (int *)(s_cache + NG * 256);             // [NG][16]
    float *s_gxt = (float *)(s_tag + NG * 16);            // [NG][TW][TW]
    // a group's 16 sites are a 4x4 block of one plane (lane = 4 * row + column); lanes beyond the plane shadow its last site
    const int e = (int)threadIdx.x & 15, grp = (int)threadIdx.x >> 4, first = grp * 16;
    const int bw = (a.W + 3) / 4, bh = (a.H + 3) / 4;
    const long long nblock = (long long)a.B * a.C * bh * bw;
    const long long ntile = (nblock + NG - 1) / NG;
    const long long t0 = (long long)blockIdx.x * a.tiles_per_wg, t1 = t0 + a.tiles_per_wg < ntile ? t0 + a.tiles_per_wg : ntile;
    float *gxt = s_gxt + grp * TN;
    float *gxt_own = gxt + (HALO + (e >> 2)) * TW + HALO + (e & 3);
    float *cache = s_cache + grp * 256;      // [16 corners][16 elements]
    int *tags = s_tag + grp * 16;            // (row << 4 | corner) held by the entry of that corner, -1: none
    // an entry's sum leaves the cache: into the image; without one into the band, or, a row outside it, to memory as one 64-byte segment
    auto retire = [&](float *gtab, int tag, float v) {
        if constexpr (RES) lds_add_f32(&s_img[(tag >> 4) * EL + e], v);
        else {
            const int slot = ftiv_band_slot<IV>(tag >> 4);      // (uniform in the group)
            if (slot >= 0) lds_add_f32(&s_img[slot * EL + e], v);
            else if (v != 0.0f) atomicAdd(&gtab[(tag >> 4) * EL + e], v);
        }
    };
    for (int m = 0; m < a.M; ++m) {
        const float *tab = a.w[m];
        float *gtab = a.gw[m];
        const int di[3] = {a.di[m][0], a.di[m][1], a.di[m][2]}, dj[3] = {a.dj[m][0], a.dj[m][1], a.dj[m][2]};
        for (int i = threadIdx.x; i < IMG; i += NT) s_img[i] = 0.0f;
        tags[e] = -1;
        __syncthreads();      // image zeroed before any group adds into it
        for (long long t = t0; t < t1; ++t) {
            const long long block = t * NG + grp;
            const long long blk = block < nblock ? block : nblock - 1;
            const long long bc = blk / ((long long)bh * bw);
            const int brem = (int)(blk % ((long long)bh * bw));
            const int y0 = (brem / bw) * 4 + (e >> 2), x0 = (brem % bw) * 4 + (e & 3);
            const bool valid = block < nblock && y0 < a.H && x0 < a.W;
            const int y = imin(y0, a.H - 1), x = imin(x0, a.W - 1);
            const float *plane = a.x + bc * a.H * a.W;
            float *gplane = a.gx + bc * a.H * a.W;
#pragma unroll
            for (int i = 0; i < (TN + 15) / 16; ++i)
                if (TN % 16 == 0 || e + 16 * i < TN) gxt[e + 16 * i] = 0.0f;      // (only this group touches its tile and its rows of s_g, and LDS serves a wave in order)
            ftiv_site_g<U>(a, bc, y, x, valid, [&](int eo, float v) { s_g[threadIdx.x][eo] = v; });
            float own = 0.0f;
#pragma unroll 1
            for (int r = 0; r < 4; ++r) {
                // this lane's site, per vertex: table row and corner code as row << 4 | corner (-1: no site) and weight / q
                int tagv[5], ord;
                float wq[5];
                {
                    FtIvPass p;
                    ftiv_pass_setup<IV>(plane, a.H, a.W, y, x, r, di, dj, p);
                    int c = p.corner;
#pragma unroll
                    for (int j = 0; j < 5; ++j) {
                        tagv[j] = valid ? (p.idx[j] << 4) | c : -1;
                        wq[j] = valid ? p.wt[j] / (float)G::q : 0.0f;
                        if (j < 4) c ^= 8 >> ((p.ord >> (2 * j)) & 3);
                    }
                    ord = p.ord;
                }
                const int eo = eo_of_elem<U>(r, e);
                float rowv[16][5];
                static_for<0, 16>([&](auto K) {
#pragma unroll
                    for (int j = 0; j < 5; ++j) rowv[K][j] = tab[(imax(ft_bcast<K>(tagv[j]), 0) >> 4) * EL + e];
                });
                float dm[5] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f};      // g . row of this lane's site, per vertex
                static_for<0, 16>([&](auto K) {
                    asm volatile("" : : : "memory");      // one site at a time (registers)
                    const float gv = s_g[first + K][eo];
                    int tg[5];
                    float v[5], d[5];
#pragma unroll
                    for (int j = 0; j < 5; ++j) {
                        tg[j] = ft_bcast<K>(tagv[j]);
                        v[j] = ft_bcast<K>(wq[j]) * gv;
                        d[j] = ft_sum16(gv * rowv[K][j]);
                    }
                    if (e == K) {
#pragma unroll
                        for (int j = 0; j < 5; ++j) dm[j] = d[j];
                    }
                    if (tg[0] >= 0) {      // the lane K has a site (uniform in the group); its five vertices are five different corners
                        int have[5];
                        float old[5];
#pragma unroll
                        for (int j = 0; j < 5; ++j) {
                            have[j] = tags[tg[j] & 15];
                            old[j] = cache[(tg[j] & 15) * 16 + e];
                        }
#pragma unroll
                        for (int j = 0; j < 5; ++j) {
                            // hit: old + v; miss: v, and the entry's sum leaves the cache
                            const bool hit = have[j] == tg[j];
                            cache[(tg[j] & 15) * 16 + e] = hit ? old[j] + v[j] : v[j];
                            if (!hit) {
                                if (have[j] >= 0) retire(gtab, have[j], old[j]);
                                tags[tg[j] & 15] = tg[j];
                            }
                        }
                    }
                });
                // d/d f of rank j = (g . p_{j+1} - g . p_j) / q belongs to the key of that rank
                float df[4];
#pragma unroll
                for (int j = 0; j < 4; ++j) df[j] = (dm[j + 1] - dm[j]) / (float)G::q;
                const int o0 = ord & 3, o1 = (ord >> 2) & 3, o2 = (ord >> 4) & 3;
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const float dk = o0 == k ? df[0] : o1 == k ? df[1] : o2 == k ? df[2] : df[3];
                    if (k == 0) own += dk;
                    else {
                        int dy, dx;
                        sample_offset(r, di[k - 1], dj[k - 1], dy, dx);
                        float *tp = gxt_own + dy * TW + dx;
                        *tp = *tp + (valid ? dk : 0.0f);
                    }
                }
            }
            // the tile onto the image: position (ty, tx) is pixel (4 by - HALO + ty, 4 bx - HALO + tx) clamped into the plane
            *gxt_own += valid ? own : 0.0f;
            if (block < nblock) {
                const int ty0 = (brem / bw) * 4 - HALO, tx0 = (brem % bw) * 4 - HALO;
#pragma unroll
                for (int i = 0; i < (TN + 15) / 16; ++i) {
                    const int q = e + 16 * i;
                    if (TN % 16 != 0 && q >= TN) continue;
                    const float v = gxt[q];
                    // (row and column of q written as shift and mask where TW is 8: from q / TW and q % TW the compiler no longer hoists the column's
                    // clamp out of the unrolled loop, and the HALO = 2 instance would not be the kernel it was)
                    if (v != 0.0f)
                        atomicAdd(&gplane[imin(imax(ty0 + (HALO == 2 ? q >> 3 : q / TW), 0), a.H - 1) * a.W + imin(imax(tx0 + (HALO == 2 ? q & 7 : q % TW), 0), a.W - 1)], v);
                }
            }
        }
        // the group's cache leaves, then the image or the band goes into the table gradient, 16 lanes per row
#pragma unroll 1
        for (int c = 0; c < 16; ++c) {
            const int tg = tags[c];
            if (tg >= 0) retire(gtab, tg, cache[c * 16 + e]);
        }
        lds_adds_done();
        __syncthreads();
        for (int i = threadIdx.x; i < IMG; i += NT) {      // (i % 16 == e: NT is a multiple of 16)
            const float v = s_img[i];
            if (v != 0.0f) atomicAdd(&gtab[RES ? i : ftiv_band_row<IV>(i >> 4) * EL + e], v);
        }
        __syncthreads();
    }
}

template <int IV, int U>
static hipError_t launch_ftiv_fwd(const FtIvArgs &a, int num_cus, hipStream_t st) {
    const long long nsite = (long long)a.B * a.C * a.H * a.W;
    const long long ntile = (nsite + kFtIvFwdNT - 1) / kFtIvFwdNT;
    if (ntile <= 0 || ntile > 0x7fffffffLL) return hipErrorInvalidValue;
    const size_t tables = (size_t)a.M * IvGeom<IV>::rows * U * U * 4;
    if (tables <= (size_t)kFtIvLdsBudget) {
        // persistent workgroups (the tables are staged once per workgroup), as many per CU as fit its LDS, at most 4
        const hipError_t e = raise_lds_limit((const void *)ft_interval_stage_fwd<IV, U, true>, kFtIvLdsBudget);
        if (e != hipSuccess) return e;
        long long per_cu = (160 * 1024) / (long long)tables;
        per_cu = per_cu > 4 ? 4 : per_cu;
        const long long nb = ntile < per_cu * num_cus ? ntile : per_cu * num_cus;
        hipLaunchKernelGGL((ft_interval_stage_fwd<IV, U, true>), dim3((unsigned)nb), dim3(kFtIvFwdNT), tables, st, a);
    } else {
        hipLaunchKernelGGL((ft_interval_stage_fwd<IV, U, false>), dim3((unsigned)ntile), dim3(kFtIvFwdNT), 0, st, a);
    }
    return hipGetLastError();
}

template <int IV, int U, int HALO>
static hipError_t launch_ftiv_bwd(FtIvArgs a, int num_cus, hipStream_t st) {
    constexpr int image = IvGeom<IV>::rows * U * U;
    constexpr bool RES = image * 4 <= kFtIvLdsBudget;
    long long ntile;
    if constexpr (U == 4) ntile = ((long long)a.B * a.C * ((a.H + 3) / 4) * ((a.W + 3) / 4) + kFtIvB4Groups - 1) / kFtIvB4Groups;
    else ntile = ((long long)a.B * a.C * a.H * a.W + kFtIvNT - 1) / kFtIvNT;
    if (ntile <= 0 || ntile > 0x7fffffffLL) return hipErrorInvalidValue;
    // a workgroup walks `per` consecutive tiles, so that the image is zeroed and flushed once per that many: of one to four
    // workgroups per slot (a CU holds `fit` of them at a time) the split whose last round wastes least, the coarser one on a tie
    constexpr int lds_bytes = U == 4 ? ftiv_bwd4_lds(RES ? image : kFtIvBandRows<IV> * 16, HALO) : ftiv_bwd_lds<U>(RES ? image : 0);
    constexpr int fit = U == 4 ? 1 : (160 * 1024 / lds_bytes < 8 ? 160 * 1024 / lds_bytes : 8);
    const long long slots = (long long)num_cus * fit;
    long long per = 0, best = 0;
    for (int k = 1; k <= 4; ++k) {
        const long long p = (ntile + k * slots - 1) / (k * slots);
        const long long cost = (((ntile + p - 1) / p + slots - 1) / slots) * p;
        if (!per || cost < best) per = p, best = cost;
    }
    a.tiles_per_wg = (int)per;
    const long long nb = (ntile + per - 1) / per;
    if constexpr (U == 4) {
        constexpr int lds = lds_bytes;
        const hipError_t e = raise_lds_limit((const void *)ft_interval_stage_bwd4<IV, RES, HALO>, lds);
        if (e != hipSuccess) return e;
        hipLaunchKernelGGL((ft_interval_stage_bwd4<IV, RES, HALO>), dim3((unsigned)nb), dim3(kFtIvB4Sites), (size_t)lds, st, a);
    } else {
        constexpr int lds = lds_bytes;
        const hipError_t e = raise_lds_limit((const void *)ft_interval_stage_bwd<IV, U, RES, HALO>, lds);
        if (e != hipSuccess) return e;
        hipLaunchKernelGGL((ft_interval_stage_bwd<IV, U, RES, HALO>), dim3((unsigned)nb), dim3(kFtIvNT), (size_t)lds, st, a);
    }
    return hipGetLastError();
}

// HALO: 2 for the lists of s, d, y, 3 when the list holds one of e, h, o (ft_halo()); the forward kernels have no halo
template <int IV, int HALO>
static hipError_t launch_ftiv(const FtIvArgs &a, bool backward, int num_cus, hipStream_t st) {
    switch (a.u * 2 + (backward ? 1 : 0)) {
        case 2: return launch_ftiv_fwd<IV, 1>(a, num_cus, st);
        case 3: return launch_ftiv_bwd<IV, 1, HALO>(a, num_cus, st);
        case 4: return launch_ftiv_fwd<IV, 2>(a, num_cus, st);
        case 5: return launch_ftiv_bwd<IV, 2, HALO>(a, num_cus, st);
        case 6: return launch_ftiv_fwd<IV, 3>(a, num_cus, st);
        case 7: return launch_ftiv_bwd<IV, 3, HALO>(a, num_cus, st);
        case 8: return launch_ftiv_fwd<IV, 4>(a, num_cus, st);
        case 9: return launch_ftiv_bwd<IV, 4, HALO>(a, num_cus, st);
        default: return hipErrorInvalidValue;
    }
}

// one stage, forward or backward, of a filled FtIvArgs at interval 5 or 6 (mulut_ft.h)
hipError_t launch_ft_interval_stage(const FtIvArgs &a, int interval, bool backward, int halo, int num_cus, hipStream_t st) {
    if (halo > 2) return interval == 5 ? launch_ftiv<5, 3>(a, backward, num_cus, st) : launch_ftiv<6, 3>(a, backward, num_cus, st);
    return interval == 5 ? launch_ftiv<5, 2>(a, backward, num_cus, st) : launch_ftiv<6, 2>(a, backward, num_cus, st);
}

}  // namespace mulut
