// mulut_ft.hip -- LUT-aware fine-tuning kernels: the differentiable twin of the inference path.
//
// Reference: MuLUT.InterpTorchBatch + MuLUT.forward, sr/model.py:69-312 (driver sr/3_finetune_lut.py).
// One kernel pair per STAGE:
//   ft_stage_fwd  per LR site and channel: all modes x 4 rotations; each pass is the reference's float32
//                 expression  ((((q-f1)*p0 + (f1-f2)*p1) + (f2-f3)*p2) + (f3-f4)*p3) + f4*p4, /q  (no FMA
//                 contraction), accumulated as  pred = round(pred + pass)  after EVERY pass (:308), then
//                 x = round(clamp(pred/avg + bias, 0, 255)) (:309).
//   ft_stage_bwd  recomputes the stage forward (for the clamp mask), then scatters
//                   d/d(table row j)  = w_j/q * g            (atomic add into the quantised-table gradient)
//                   d/d(f of rank j)  = sum_e g*(p_j - p_{j-1})/q   (atomic add into the input gradient at
//                                       the clamped source pixel: replicate-pad and rot90 backward)
//                 rounding is BPDA identity (:59-67), clamp passes gradient inside [0,255] inclusive.
// The simplex case at TIES is the reference's 24-branch cascade with strict '>' (:191-282): forward
// values do not depend on it, gradients do.
// Tables are passed already quantised (clamp(round(w*127),-127,127), :74-76) by the Python module, which
// also applies that step's backward (x127, clamp mask).
#include <hip/hip_runtime.h>

#include <cstring>
#include <type_traits>

#include "mulut_kernels.h"

#pragma clang fp contract(off)

#include "mulut_ft.h"

#ifndef MULUT_FT_ABL
#define MULUT_FT_ABL 0      // timing-only ablations (tools/ab_bench.py variants ftabl*): never in the product build
#endif

namespace mulut {

// table row of every tube-band slot (-1: the slot holds no row), built at compile time: the flush of a workgroup's band sums walks the
// slots instead of re-deriving (A, B, C, D) -> slot for 16 x 125 candidates per mode
struct FtTubeRows { int row[kTubeSlots]; };
constexpr FtTubeRows ft_make_tube_rows() {
    FtTubeRows t{};
    for (int i = 0; i < kTubeSlots; ++i) t.row[i] = -1;
    for (int A = 0; A < kL; ++A)
        for (int B = (A < 2 ? 0 : A - 2); B < kL && B <= A + 2; ++B)
            for (int C = (A < 2 ? 0 : A - 2); C < kL && C <= A + 2; ++C)
                for (int D = (A < 2 ? 0 : A - 2); D < kL && D <= A + 2; ++D)
                    if (tube_contains(A, B, C, D)) t.row[tube_slot(A, B, C, D)] = A * kStrideA + B * kStrideB + C * kStrideC + D;
    return t;
}
__device__ const FtTubeRows kFtTubeRows = ft_make_tube_rows();

// (FtPass and ft_pass_setup(), the per-pass set-up of every kernel here: mulut_ft.h)

// pred after all passes of the stage for one site (the order of additions and roundings is the reference's)
template <int U>
__device__ __forceinline__ void ft_site_forward(const FtArgs &a, const float *plane, int y, int x, float (&pred)[U * U]) {
#pragma unroll
    for (int e = 0; e < U * U; ++e) pred[e] = 0.0f;
    for (int m = 0; m < a.M; ++m) {
        const float *tab = a.w[m];
        const int di[3] = {a.di[m][0], a.di[m][1], a.di[m][2]}, dj[3] = {a.dj[m][0], a.dj[m][1], a.dj[m][2]};
        static_for<0, 4>([&](auto R) {
            constexpr int r = R;
            FtPass p;
            ft_pass_setup(plane, a.H, a.W, y, x, r, di, dj, p);
            const float *r0 = tab + (long long)p.idx[0] * (U * U), *r1 = tab + (long long)p.idx[1] * (U * U);
            const float *r2 = tab + (long long)p.idx[2] * (U * U), *r3 = tab + (long long)p.idx[3] * (U * U);
            const float *r4 = tab + (long long)p.idx[4] * (U * U);
            static_for<0, U * U>([&](auto E) {
                constexpr int eo = E;                                   // block position sy*U+sx
                constexpr int e = row_elem(r, eo / U, eo % U, U);       // table element landing there
                const float val = ((((p.wt[0] * r0[e] + p.wt[1] * r1[e]) + p.wt[2] * r2[e]) + p.wt[3] * r3[e]) + p.wt[4] * r4[e]) /
                                  (float)kQ;
                pred[eo] = rintf(pred[eo] + val);                       // pred += ...; pred = round_func(pred)
            });
        });
    }
}

template <int U>
__global__ void __launch_bounds__(256) ft_stage_fwd(FtArgs a) {
    const long long nsite = (long long)a.B * a.C * a.H * a.W;
    const long long s = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= nsite) return;
    const int x = (int)(s % a.W), y = (int)((s / a.W) % a.H);
    const long long bc = s / ((long long)a.W * a.H);
    const float *plane = a.x + bc * a.H * a.W;
    float pred[U * U];
    ft_site_forward<U>(a, plane, y, x, pred);
    const float avg = a.is_last ? (float)a.M : (float)(4 * a.M), bias = a.is_last ? 0.0f : 127.0f;
    float *po = a.out + bc * (long long)(a.H * U) * (a.W * U);
    uint32_t inside = 0;
    static_for<0, U * U>([&](auto E) {
        constexpr int eo = E;
        const float t0 = pred[eo] / avg + bias;
        inside |= (t0 >= 0.0f && t0 <= 255.0f) ? 1u << eo : 0u;
        const float t = fminf(fmaxf(t0, 0.0f), 255.0f);
        po[(long long)(y * U + eo / U) * (a.W * U) + (x * U + eo % U)] = rintf(t);
    });
    if (a.inside) a.inside[s] = (uint16_t)inside;
}

// g = dL/d pred of one site: the clamp's mask (saved by the forward, or from the stage forward recomputed here), then d(pred / avg)
template <int U, class F>
__device__ __forceinline__ void ft_site_g(const FtArgs &a, const float *plane, long long bc, int y, int x, bool valid, F &&put) {
    constexpr int EL = U * U;
    const float avg = a.is_last ? (float)a.M : (float)(4 * a.M), bias = a.is_last ? 0.0f : 127.0f;
    const float *pg = a.gout + bc * (long long)(a.H * U) * (a.W * U);
    if (a.inside) {
        const uint32_t inside = valid ? a.inside[(bc * a.H + y) * a.W + x] : 0u;
        static_for<0, EL>([&](auto E) {
            constexpr int eo = E;
            const float go = pg[(long long)(y * U + eo / U) * (a.W * U) + (x * U + eo % U)];
            put(eo, ((inside >> eo) & 1u) ? go / avg : 0.0f);
        });
    } else {
        float pred[EL];
#if MULUT_FT_ABL == 2
        for (int q = 0; q < EL; ++q) pred[q] = 100.0f;
#else
        ft_site_forward<U>(a, plane, y, x, pred);
#endif
        static_for<0, EL>([&](auto E) {
            constexpr int eo = E;
            const float t = pred[eo] / avg + bias;
            const float go = pg[(long long)(y * U + eo / U) * (a.W * U) + (x * U + eo % U)];
            put(eo, (valid && t >= 0.0f && t <= 255.0f) ? go / avg : 0.0f);
        });
    }
}

// Backward of one stage.  A workgroup owns 256 consecutive sites.  Per site (one thread): recompute the stage forward for
// the clamp mask, g = dL/d pred; then per pass the five rows' dot products with g give the input gradient (one atomic
// per rank into the source pixel: adjacent sites hit adjacent floats, i.e. well-shaped 256-byte atomic instructions).
// The TABLE gradient is not scattered from the site threads (64 lanes -> 64 different rows = 64 memory-side atomic
// requests per instruction): every pass writes its (row, weight / q) items to LDS and the workgroup redistributes them
//   u > 1 : EPL lanes per item, one per row element: a wave instruction adds whole 16-float rows (64-byte segments);
//   u == 1: one float per item: items inside the tube (991 rows, the ones smooth content uses) are summed into a
//           per-workgroup LDS copy of the tube band with ds_add_f32 and flushed once per workgroup as contiguous
//           atomics; items outside it go to global memory directly.
// HALO (2 or 3): the pixels the tiles of the input gradient stage around their sites, i.e. the largest key offset of the stage's
// patterns -- 2 for s, d, y, 3 with one of e, h, o in the list.  A compile-time constant: the instances of HALO = 2 are the kernels
// as they were before the 4 x 4 patterns, instruction for instruction (tools/asm_compare.py).
constexpr int kFtGxTile = 1024;        // floats of a wave's input-gradient tile (ft_stage_bwd)
template <int U, int HALO>
__global__ void __launch_bounds__(256) ft_stage_bwd(FtArgs a) {
    static_assert(HALO == 2 || HALO == 3, "halo of the input-gradient tile");
    constexpr int EL = U * U, EPL = EL <= 1 ? 1 : EL <= 4 ? 4 : 16, NT = 256;
    __shared__ float s_g[NT][EL + 1];
    __shared__ int s_idx[5][NT];
    __shared__ float s_wq[5][NT];
    __shared__ float s_band[U == 1 ? kMaxFtModes * kTubeSlots : 1];
    __shared__ float s_gxt[NT / 64][kFtGxTile];
    const long long nsite = (long long)a.B * a.C * a.H * a.W;
    const long long s = (long long)blockIdx.x * NT + threadIdx.x;
    const bool valid = s < nsite;
    const long long sc = valid ? s : nsite - 1;                 // surplus threads shadow the last site and contribute nothing
    const int x = (int)(sc % a.W), y = (int)((sc / a.W) % a.H);
    const long long bc = sc / ((long long)a.W * a.H);
    const float *plane = a.x + bc * a.H * a.W;
    float *gplane = a.gx + bc * a.H * a.W;
    // The input gradient: a pass gives d/d f of each key to that key's pixel.  The site's own pixel (key a) is summed in a register; for
    // key b, c or d the target is the site's pixel plus an offset that is the same for every site of the pass, so the 64 consecutive
    // sites of a WAVE hit 64 different positions of the wave's private tile -- the rows its sites lie in plus HALO on either side, each
    // plane with its own halo rows and columns (unclamped coordinates: replicate padding is applied when the tile is folded onto the
    // image at the end): a plain LDS read + add + write per key, no atomic (36 LDS float adds per site before, 83 % of this kernel's
    // launch with the LDS pipeline busy).  When the tile does not fit (crops wider than ~140; a single row of 64 sites needs
    // (rows + 2 HALO) * (W + 2 HALO) <= 1024 floats) the adds go to memory.
    const int lane = (int)threadIdx.x & 63;
    float *tile = s_gxt[threadIdx.x >> 6];
    const int PWd = a.W + 2 * HALO, PHt = a.H + 2 * HALO;
    auto padded_row = [&](long long R) { return R + 2 * HALO * (R / a.H) + HALO; };      // stacked image row (plane * H + y) -> row of the padded stack
    const long long w0 = (long long)blockIdx.x * NT + (threadIdx.x & ~63u);
    const long long R0 = (w0 < nsite ? w0 : nsite - 1) / a.W, R1 = (w0 + 63 < nsite ? w0 + 63 : nsite - 1) / a.W;
    const long long pr0 = padded_row(R0) - HALO;
    const long long t_rows = padded_row(R1) + HALO - pr0 + 1;
    const int t_n = t_rows * PWd <= kFtGxTile ? (int)(t_rows * PWd) : 0;      // 0: does not fit
    for (int i = lane; i < t_n; i += 64) tile[i] = 0.0f;                      // (wave-private, and LDS serves a wave in order: no barrier)
    const int t_own = (int)(padded_row(bc * a.H + y) - pr0) * PWd + x + HALO;
    if constexpr (U == 1)
        for (int i = threadIdx.x; i < a.M * kTubeSlots; i += NT) s_band[i] = 0.0f;
    float g[EL];
    ft_site_g<U>(a, plane, bc, y, x, valid, [&](int eo, float v) {
        g[eo] = v;
        s_g[threadIdx.x][eo] = v;
    });
    __syncthreads();      // the band and the gradient rows must be zero before any wave adds into them
    float own = 0.0f;
    for (int m = 0; m < a.M; ++m) {
        const float *tab = a.w[m];
        float *gtab = a.gw[m];
        const int di[3] = {a.di[m][0], a.di[m][1], a.di[m][2]}, dj[3] = {a.dj[m][0], a.dj[m][1], a.dj[m][2]};
#pragma unroll 1
        for (int r = 0; r < 4; ++r) {
            FtPass p;
            ft_pass_setup(plane, a.H, a.W, y, x, r, di, dj, p);
            float dsum[5];   // sum_e g * p_j[e]
#pragma unroll
            for (int j = 0; j < 5; ++j) {
                const float *row = tab + (long long)p.idx[j] * EL;
                float acc = 0.0f;
#pragma unroll
                for (int eo = 0; eo < EL; ++eo) {
                    const int e = r == 0 ? eo : r == 1 ? (U - 1 - eo % U) * U + eo / U : r == 2 ? EL - 1 - eo : (eo % U) * U + (U - 1 - eo / U);   // row_elem
                    acc += g[eo] * row[e];
                }
                dsum[j] = acc;
                const float wq = p.wt[j] / (float)kQ;
                if constexpr (U == 1) {
                    // one float per item: LDS tube band when the pass is inside the tube, else global memory.  Neighbouring sites of smooth
                    // content hit the SAME slot, and an LDS float add serialises over its lanes and again over equal addresses (this
                    // kernel's LDS pipeline was busy 83 % of the launch on 96 such adds per site): the lanes of a 16-lane row that share
                    // the row leader's slot are summed by DPP first and added once, by the leader; the others add on their own.
                    // (All 256 threads are here: the broadcast and the row sum read every lane.)
                    const float v = wq * g[0];
                    const int slot = p.in_tube ? m * kTubeSlots + p.tslot[j] : -1;
                    const int lead = ft_bcast<0>(slot);
                    const bool with_lead = slot == lead && slot >= 0;
                    const float sum = ft_sum16(with_lead ? v : 0.0f);
                    if ((threadIdx.x & 15) == 0 && lead >= 0 && sum != 0.0f) lds_add_f32(&s_band[lead], sum);
                    if (!with_lead && v != 0.0f) {
                        if (slot >= 0) lds_add_f32(&s_band[slot], v);
                        else atomicAdd(&gtab[p.idx[j]], v);
                    }
                } else {
                    s_idx[j][threadIdx.x] = valid ? p.idx[j] : -1;
                    s_wq[j][threadIdx.x] = wq;
                }
            }
            // d/d f of rank j = (p_{j+1} - p_j) . g / q belongs to the key of that rank
            float df[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) df[j] = (dsum[j + 1] - dsum[j]) / (float)kQ;
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
                            float *t = tile + t_own + dy * PWd + dx;
                            *t = *t + dk;
                        }
                    } else if (dk != 0.0f) atomicAdd(&gplane[imin(imax(y + dy, 0), a.H - 1) * a.W + imin(imax(x + dx, 0), a.W - 1)], dk);
                }
            }
            if constexpr (U > 1) {
                __syncthreads();
                const int e = (int)threadIdx.x % EPL;
                const int eo = eo_of_elem<U>(r, e < EL ? e : 0);
                for (int it = (int)threadIdx.x / EPL; it < 5 * NT; it += NT / EPL) {
                    const int j = it / NT, si = it % NT;
                    const int idx = s_idx[j][si];
                    if (e < EL && idx >= 0) {
                        const float v = s_wq[j][si] * s_g[si][eo];
                        if (v != 0.0f) atomicAdd(&gtab[(long long)idx * EL + e], v);
                    }
                }
                __syncthreads();
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
    lds_adds_done();
    __syncthreads();
    if constexpr (U == 1) {
        // flush the workgroup's tube-band sums: contiguous floats, a wave adds 256 bytes at a time
        for (int m = 0; m < a.M; ++m) {
            float *gtab = a.gw[m];
            for (int sl = threadIdx.x; sl < kTubeSlots; sl += NT) {
                const int row = kFtTubeRows.row[sl];
                const float v = s_band[m * kTubeSlots + sl];
                if (row >= 0 && v != 0.0f) atomicAdd(&gtab[row], v);
            }
        }
    }
}

// Backward of a stage with 16-float rows (u == 4), kFtB4Sites sites per workgroup.  Photograph-like batches send thousands of
// sites to the same few hundred table rows, and float adds are dear wherever they meet: memory-side atomics serialise per
// address, and an LDS float add (ds_add_f32) occupies the CU's LDS pipeline for 48 cycles per wave instruction whatever its
// addresses (tools/ubench/ubench_lds_atomic.hip; an integer add or a plain write takes 3.8, read + add + write of a private
// address 7).  So the table gradient is summed on three levels:
//   1. a 16-lane group (lane = row element) owns 16 sites (a 4x4 block) and a PRIVATE 16-entry cache of band rows in LDS, direct
//      mapped by slot mod 16 -- the 16 corners of one MSB cell have 16 different residues (the tube strides are 11, 2, 12, 8
//      mod 16), so a group whose sites stay inside a cell never evicts.  A hit is read + add + write, no atomic;
//   2. an evicted entry (the sites moved on to another cell) and, at the end of a mode, every entry goes into the workgroup's LDS
//      copy of the tube band (1041 x 16 floats) with ds_add_f32;
//   3. the band is flushed once per workgroup and mode as contiguous memory-side atomics.
// Passes outside the tube add to global memory directly (16 lanes per row: 64-byte segments).
// The sites of a group ARE its 16 lanes, so nothing crosses a wave and nothing goes through LDS items: a site lane keeps the five
// (table row | tube slot, weight / q) of its pass in registers and the group reads them with DPP row broadcasts; the 80 table rows of
// a pass (one coalesced 64-byte read per site and vertex) are requested before the first is used.  The group then walks its sites
// ONE SITE AT A TIME, all five vertices together: a site's vertices are corners of one cell, i.e. five DIFFERENT cache entries, so
// their five tag + entry reads, adds and writes are independent and in flight together (round 3 walked vertex by vertex, one
// dependent LDS round trip per site and vertex, at 2 waves per SIMD: the kernel waited 60 % of its wave cycles).  The dot products
// g . row -- the input gradient's ingredient -- are 16-lane DPP sums and stay in the site's lane.  The cache tags sit in LDS next to
// the entries (one broadcast read each).  No barrier inside a mode.
// The INPUT gradient: a pass gives d/d f of each key to that key's pixel.  The site's own pixel (key a) is summed in a register; for
// key b, c or d the target is the site's pixel plus an offset that is the same for every site of the pass, so the 16 sites of a
// group hit 16 DIFFERENT positions of the group's tile (its 4 x 4 block and a halo of HALO, unclamped: 8 x 8 floats, 10 x 10 at
// HALO = 3): a plain LDS read + add
// + write per key, no atomic.  The tile goes to memory once, at the end, folded onto the image (replicate padding: a position
// outside the plane belongs to the border pixel) -- 4 memory-side atomics per site instead of 37.
// LDS: [ band gradient 1041 x 16 f32 ][ g of the sites, 17 floats each ][ caches: 16 x 16 f32 per group ][ tags: 16 per group ]
//      [ input-gradient tiles: (4 + 2 HALO)^2 f32 per group ]
constexpr int kFtB4Sites = 512, kFtB4Groups = kFtB4Sites / 16;
constexpr int ft_b4_tile(int halo) { return (4 + 2 * halo) * (4 + 2 * halo); }      // floats of a group's input-gradient tile
constexpr int ft_b4_lds(int halo) {
    return kTubeSlots * 16 * 4 + kFtB4Sites * 17 * 4 + kFtB4Groups * 16 * 16 * 4 + kFtB4Groups * 16 * 4 + kFtB4Groups * ft_b4_tile(halo) * 4;
}
constexpr int kFtB4Lds = ft_b4_lds(2);
static_assert(kFtB4Lds == 144448 && kFtB4Lds <= 160 * 1024, "ft_stage_bwd4: LDS");
static_assert(ft_b4_lds(3) == 149056 && ft_b4_lds(3) <= 160 * 1024, "ft_stage_bwd4, HALO = 3: LDS");      // one workgroup per CU either way

template <int HALO>
__global__ void __launch_bounds__(kFtB4Sites) ft_stage_bwd4(FtArgs a) {
    static_assert(HALO == 2 || HALO == 3, "halo of the input-gradient tile");
    constexpr int U = 4, EL = 16, NT = kFtB4Sites, NG = kFtB4Groups, TW = 4 + 2 * HALO, TN = ft_b4_tile(HALO);
    extern __shared__ __attribute__((aligned(16))) uint8_t ft_smem[];
    float *s_band = (float *)ft_smem;
    float (*s_g)[17] = (float (*)[17])(ft_smem + kTubeSlots * 16 * 4);
    float *s_cache = (float *)(ft_smem + kTubeSlots * 16 * 4 + NT * 17 * 4);
    int *s_tag = (int *)(s_cache + NG * 256);             // [NG][16]
    float *s_gxt = (float *)(s_tag + NG * 16);            // [NG][TW][TW]
    // a group's 16 sites are a 4x4 block of one plane (lane = 4 * row + column): neighbours in both directions share MSB cells, so
    // the group's cache sees fewer cell changes than with 16 sites along a row; lanes beyond the plane shadow its last site
    const int e = (int)threadIdx.x & 15, grp = (int)threadIdx.x >> 4, first = grp * 16;
    const int bw = (a.W + 3) / 4, bh = (a.H + 3) / 4;
    const long long nblock = (long long)a.B * a.C * bh * bw, block = (long long)blockIdx.x * NG + grp;
    const long long blk = block < nblock ? block : nblock - 1;
    const long long bc = blk / ((long long)bh * bw);
    const int brem = (int)(blk % ((long long)bh * bw));
    const int y0 = (brem / bw) * 4 + (e >> 2), x0 = (brem % bw) * 4 + (e & 3);
    const bool valid = block < nblock && y0 < a.H && x0 < a.W;
    const int y = imin(y0, a.H - 1), x = imin(x0, a.W - 1);
    const float *plane = a.x + bc * a.H * a.W;
    float *gplane = a.gx + bc * a.H * a.W;
    float *gxt = s_gxt + grp * TN;
#pragma unroll
    for (int i = 0; i < (TN + 15) / 16; ++i)
        if (TN % 16 == 0 || e + 16 * i < TN) gxt[e + 16 * i] = 0.0f;      // (only this group touches its tile, and LDS serves a wave in order)
    float *gxt_own = gxt + (HALO + (e >> 2)) * TW + HALO + (e & 3);
    ft_site_g<U>(a, plane, bc, y, x, valid, [&](int eo, float v) { s_g[threadIdx.x][eo] = v; });
    float *cache = s_cache + grp * 256;      // [16 entries][16 elements]
    int *tags = s_tag + grp * 16;            // slot held by entry c, -1: none
    float own = 0.0f;
    for (int m = 0; m < a.M; ++m) {
        const float *tab = a.w[m];
        float *gtab = a.gw[m];
        const int di[3] = {a.di[m][0], a.di[m][1], a.di[m][2]}, dj[3] = {a.dj[m][0], a.dj[m][1], a.dj[m][2]};
        for (int i = threadIdx.x; i < kTubeSlots * 16; i += NT) s_band[i] = 0.0f;
        tags[e] = -1;
        __syncthreads();      // band zeroed (and, first trip, s_g written) before any group adds into it
#pragma unroll 1
        for (int r = 0; r < 4; ++r) {
            // this lane's site, per vertex: byte offset of the table row, tube slot (-1: the pass is outside the tube -- all five or
            // none) and weight / q; a lane without a site has row 0, weight 0
            int roff[5], slotv[5], ord;
            float wq[5];
            {
                FtPass p;
                ft_pass_setup(plane, a.H, a.W, y, x, r, di, dj, p);
#pragma unroll
                for (int j = 0; j < 5; ++j) {
                    roff[j] = valid ? p.idx[j] * (EL * 4) : 0;
                    slotv[j] = valid && p.in_tube ? p.tslot[j] : -1;
                    wq[j] = valid ? p.wt[j] / (float)kQ : 0.0f;
                }
                ord = p.ord;
            }
            const int eo = eo_of_elem<U>(r, e);
            const char *tabe = (const char *)tab;
            float rowv[16][5];
            static_for<0, 16>([&](auto K) {
#pragma unroll
                for (int j = 0; j < 5; ++j) rowv[K][j] = *(const float *)(tabe + (uint32_t)(ft_bcast<K>(roff[j]) + e * 4));
            });
            float dm[5] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f};      // g . row of this lane's site, per vertex
            static_for<0, 16>([&](auto K) {
                asm volatile("" : : : "memory");      // one site at a time: keeps the scheduler from opening every site's reads and sums at once (registers)
                const float gv = s_g[first + K][eo];
                int slot[5];
                float v[5], d[5];
#pragma unroll
                for (int j = 0; j < 5; ++j) {
                    slot[j] = ft_bcast<K>(slotv[j]);
                    v[j] = ft_bcast<K>(wq[j]) * gv;
                    d[j] = ft_sum16(gv * rowv[K][j]);
                }
                if (e == K) {
#pragma unroll
                    for (int j = 0; j < 5; ++j) dm[j] = d[j];
                }
#if MULUT_FT_ABL != 4
                if (slot[0] >= 0) {      // inside the tube (uniform in the group)
                    int tg[5];
                    float old[5];
#pragma unroll
                    for (int j = 0; j < 5; ++j) {
                        tg[j] = tags[slot[j] & 15];
                        old[j] = cache[(slot[j] & 15) * 16 + e];
                    }
#pragma unroll
                    for (int j = 0; j < 5; ++j) {
                        // hit: old + v; miss: v, and the entry's sum goes into the band
                        const bool hit = tg[j] == slot[j];
                        cache[(slot[j] & 15) * 16 + e] = hit ? old[j] + v[j] : v[j];
                        if (!hit) {
                            if (tg[j] >= 0) lds_add_f32(&s_band[tg[j] * 16 + e], old[j]);
                            tags[slot[j] & 15] = slot[j];
                        }
                    }
                } else {
#pragma unroll
                    for (int j = 0; j < 5; ++j) {
                        // (the broadcast outside the lane-divergent test below: a DPP read of a lane that is switched off returns 0)
                        const uint32_t off = (uint32_t)(ft_bcast<K>(roff[j]) + e * 4);
                        if (v[j] != 0.0f) atomicAdd((float *)((char *)gtab + off), v[j]);
                    }
                }
#endif
            });
            // d/d f of rank j = (g . p_{j+1} - g . p_j) / q belongs to the key of that rank
            float df[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) df[j] = (dm[j + 1] - dm[j]) / (float)kQ;
            const int o0 = ord & 3, o1 = (ord >> 2) & 3, o2 = (ord >> 4) & 3;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const float dk = o0 == k ? df[0] : o1 == k ? df[1] : o2 == k ? df[2] : df[3];
                if (k == 0) own += dk;
#if MULUT_FT_ABL != 3
                else {
                    int dy, dx;
                    sample_offset(r, di[k - 1], dj[k - 1], dy, dx);
                    float *t = gxt_own + dy * TW + dx;
                    *t = *t + dk;
                }
#endif
            }
        }
        // the group's cache into the band, then the band's rows (tube rows of anchor MSB A, 16 lanes per row) into the table gradient
#pragma unroll 1
        for (int c = 0; c < 16; ++c) {
            const int t = tags[c];
            if (t >= 0) lds_add_f32(&s_band[t * 16 + e], cache[c * 16 + e]);
        }
        lds_adds_done();
        __syncthreads();
        for (int sl = grp; sl < kTubeSlots; sl += NG) {
            const int row = kFtTubeRows.row[sl];
            const float v = s_band[sl * 16 + e];
            if (row >= 0 && v != 0.0f) atomicAdd(&gtab[(long long)row * EL + e], v);
        }
        __syncthreads();
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

// HALO: 2 for the lists of s, d, y, 3 when the list holds one of e, h, o (ft_halo()); the forward kernels read their keys through
// clamped gathers with run-time offsets and have no halo
template <int U, int HALO>
static hipError_t launch_ft(const FtArgs &a, bool backward, hipStream_t st) {
    const long long nsite = (long long)a.B * a.C * a.H * a.W;
    const long long nb = (nsite + 255) / 256;
    if (nb <= 0 || nb > 0x7fffffffLL) return hipErrorInvalidValue;
    if (backward && U == 4) {
        {
            const hipError_t e = mulut::raise_lds_limit((const void *)ft_stage_bwd4<HALO>, 160 * 1024);
            if (e != hipSuccess) return e;
        }
        const long long nblock4 = (long long)a.B * a.C * ((a.H + 3) / 4) * ((a.W + 3) / 4);      // 4x4 site blocks, one per 16-lane group
        const long long nb4 = (nblock4 + kFtB4Groups - 1) / kFtB4Groups;
        hipLaunchKernelGGL(ft_stage_bwd4<HALO>, dim3((unsigned)nb4), dim3(kFtB4Sites), (size_t)ft_b4_lds(HALO), st, a);
    } else if (backward) hipLaunchKernelGGL((ft_stage_bwd<U, HALO>), dim3((unsigned)nb), dim3(256), 0, st, a);
    else hipLaunchKernelGGL(ft_stage_fwd<U>, dim3((unsigned)nb), dim3(256), 0, st, a);
    return hipGetLastError();
}

template <int HALO>
static hipError_t launch_ft_u(const FtArgs &a, bool backward, hipStream_t st) {
    return a.u == 1 ? launch_ft<1, HALO>(a, backward, st) : a.u == 2 ? launch_ft<2, HALO>(a, backward, st)
         : a.u == 3 ? launch_ft<3, HALO>(a, backward, st) : launch_ft<4, HALO>(a, backward, st);
}

hipError_t launch_ft_stage(const FtArgs &a, bool backward, int halo, hipStream_t st) {
    return halo > 2 ? launch_ft_u<3>(a, backward, st) : launch_ft_u<2>(a, backward, st);
}

// The module's quantisation step and its backward (sr/model.py:74-76: weight = clamp(round_func(weight * 127), -127, 127), round_func a
// BPDA identity), for all tables of a stage in one launch: as torch operations they are six launches per table and direction.
struct FtQuantArgs {
    const float *w[kMaxFtModes];
    float *o[kMaxFtModes];
    long long n;
};
template <bool BACKWARD>
__global__ void __launch_bounds__(256) ft_quantize_kernel(FtQuantArgs a) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= a.n) return;
    const int m = (int)blockIdx.y;
    const float r = rintf(a.w[m][i] * 127.0f);          // torch.round: half to even
    if (BACKWARD) a.o[m][i] = a.o[m][i] * ((r >= -127.0f && r <= 127.0f) ? 1.0f : 0.0f) * 127.0f;      // the clamp passes gradient inside [-127, 127] inclusive
    else a.o[m][i] = r != r ? r : fminf(fmaxf(r, -127.0f), 127.0f);      // torch.clamp keeps NaN (fminf / fmaxf drop it): a diverged run must show
}

// The optimiser's step (sr/3_finetune_lut.py:86: Adam, L2 weight decay in the gradient, no amsgrad) over every table of a run in one
// launch.  Parameters and moments are float32 in memory, as the reference holds them; the arithmetic between the loads and the three
// stores is float64, so each stored value is the float64 Adam's, rounded once -- the step is bound by its seven memory streams and the
// float64 operations cost it nothing.  The bias corrections come from the host (1 - beta^step, in double).
constexpr int kMaxAdamTensors = 32;
struct FtAdamArgs {
    float *p[kMaxAdamTensors], *m[kMaxAdamTensors], *v[kMaxAdamTensors];
    const float *g[kMaxAdamTensors];
    long long n[kMaxAdamTensors];
    double beta1, beta2, eps, weight_decay, step_size, bc2_sqrt;
};
__global__ void __launch_bounds__(256) ft_adam_kernel(FtAdamArgs a) {
    const int t = (int)blockIdx.y;
    const long long n = a.n[t], stride = (long long)gridDim.x * 256;
    float *__restrict__ P = a.p[t], *__restrict__ M = a.m[t], *__restrict__ V = a.v[t];
    const float *__restrict__ G = a.g[t];
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += stride) {
        double p = (double)P[i], g = (double)G[i];
        if (a.weight_decay != 0.0) g += a.weight_decay * p;
        const double m = (double)M[i] + (g - (double)M[i]) * (1.0 - a.beta1);
        const double v = (double)V[i] * a.beta2 + (1.0 - a.beta2) * g * g;
        p -= a.step_size * (m / (sqrt(v) / a.bc2_sqrt + a.eps));
        P[i] = (float)p;
        M[i] = (float)m;
        V[i] = (float)v;
    }
}

}  // namespace mulut

using namespace mulut;

int mulut_ft_adam(int device, float *const *params, const float *const *grads, float *const *exp_avg, float *const *exp_avg_sq,
                  const long long *n, int T, long long step, double lr, double beta1, double beta2, double eps, double weight_decay,
                  void *stream) {
    if (!params || !grads || !exp_avg || !exp_avg_sq || !n || T < 1 || step < 1) return MULUT_EINVAL;
    if (!(beta1 >= 0.0 && beta1 < 1.0 && beta2 >= 0.0 && beta2 < 1.0)) return MULUT_EINVAL;
    for (int t = 0; t < T; ++t)
        if (!params[t] || !grads[t] || !exp_avg[t] || !exp_avg_sq[t] || n[t] <= 0) return MULUT_EINVAL;
    if (hipSetDevice(device) != hipSuccess) return MULUT_ENODEVICE;
    const double bc1 = 1.0 - pow(beta1, (double)step), bc2 = 1.0 - pow(beta2, (double)step);
    for (int t0 = 0; t0 < T; t0 += kMaxAdamTensors) {
        FtAdamArgs a;
        memset(&a, 0, sizeof(a));
        const int cnt = T - t0 < kMaxAdamTensors ? T - t0 : kMaxAdamTensors;
        long long most = 0;
        for (int t = 0; t < cnt; ++t) {
            a.p[t] = params[t0 + t];
            a.g[t] = grads[t0 + t];
            a.m[t] = exp_avg[t0 + t];
            a.v[t] = exp_avg_sq[t0 + t];
            a.n[t] = n[t0 + t];
            most = a.n[t] > most ? a.n[t] : most;
        }
        a.beta1 = beta1, a.beta2 = beta2, a.eps = eps, a.weight_decay = weight_decay, a.step_size = lr / bc1, a.bc2_sqrt = sqrt(bc2);
        long long nb = (most + 255) / 256;
        if (nb > 4096) nb = 4096;      // grid-stride beyond that: 2^20 threads per table keep every CU busy
        hipLaunchKernelGGL(ft_adam_kernel, dim3((unsigned)nb, (unsigned)cnt), dim3(256), 0, (hipStream_t)stream, a);
    }
    return hipGetLastError() == hipSuccess ? MULUT_OK : MULUT_EHIP;
}

static int ft_quantize(int device, const float *const *w, float *const *o, int M, long long n, bool backward, void *stream) {
    if (!w || !o || n <= 0) return MULUT_EINVAL;
    if (M < 1 || M > kMaxFtModes) return MULUT_EUNSUPPORTED;
    FtQuantArgs a;
    memset(&a, 0, sizeof(a));
    for (int m = 0; m < M; ++m) {
        if (!w[m] || !o[m]) return MULUT_EINVAL;
        a.w[m] = w[m];
        a.o[m] = o[m];
    }
    a.n = n;
    const long long nb = (n + 255) / 256;
    if (nb > 0x7fffffffLL) return MULUT_EINVAL;
    if (hipSetDevice(device) != hipSuccess) return MULUT_ENODEVICE;
    if (backward) hipLaunchKernelGGL(ft_quantize_kernel<true>, dim3((unsigned)nb, (unsigned)M), dim3(256), 0, (hipStream_t)stream, a);
    else hipLaunchKernelGGL(ft_quantize_kernel<false>, dim3((unsigned)nb, (unsigned)M), dim3(256), 0, (hipStream_t)stream, a);
    return hipGetLastError() == hipSuccess ? MULUT_OK : MULUT_EHIP;
}

// The one host path of a stage call.  A request is what an entry point was given; a rule is what its family asks of it.  The order of
// the checks -- and so which MULUT_E* code a bad call gets -- is part of the ABI: the family's early pointer, ft_fill (mulut_ft.h),
// the call's own output pointers; all before the device is touched.
struct FtRequest {
    int device, interval;
    const float *const *weights_q;
    const char *modes;
    int is_last, u;
    const float *x;
    int B, C, H, W;
    float *out;                 // forward
    const uint16_t *inside;
    const float *grad_out;      // backward
    float *const *grad_wq;
    float *grad_x;
    void *stream;
};
enum FtEarly { kFtEarlyNone, kFtEarlyInside, kFtEarlyGradWq };
struct FtRule {
    int iv_lo, iv_hi;   // intervals the family accepts (else MULUT_EUNSUPPORTED)
    int max_reach;      // largest pattern reach: 2 = s, d, y; 3 = e, h, o as well
    bool need_mask;     // `inside` is required
    FtEarly early;      // the pointer tested ahead of everything else (kFtEarlyGradWq: of a backward call)
};
static const FtRule kFtPlain = {4, 4, 2, false, kFtEarlyNone};          // mulut_ft_stage_forward / _backward: the backward recomputes the mask
static const FtRule kFtMask = {4, 4, 2, true, kFtEarlyInside};          // mulut_ft_stage_forward_mask / _backward_mask
static const FtRule kFtInterval = {5, 6, 2, true, kFtEarlyGradWq};      // mulut_ft_interval_stage_*
static const FtRule kFtWide = {4, 6, 3, true, kFtEarlyGradWq};          // mulut_ft_wide_stage_*

static int ft_num_cus(int device) {
    static int cus[64];
    if (device < 0 || device >= 64) return 256;
    if (!cus[device]) {
        int n = 0;
        if (hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, device) != hipSuccess || n < 1) n = 256;
        cus[device] = n;
    }
    return cus[device];
}

// Args: FtArgs (interval 4) or FtIvArgs (5 and 6) -- exactly one is filled per call
template <class Args>
static int ft_stage_as(const FtRule &rule, const FtRequest &q, bool backward) {
    Args a;
    const int rc = ft_fill(a, q.interval >= rule.iv_lo && q.interval <= rule.iv_hi, q.weights_q, q.grad_wq, q.modes, q.is_last, q.u, q.x, q.inside,
                           rule.need_mask, rule.max_reach, q.B, q.C, q.H, q.W);
    if (rc) return rc;
    if (backward ? !q.grad_out || !q.grad_wq || !q.grad_x : !q.out) return MULUT_EINVAL;
    a.out = q.out;
    a.gout = q.grad_out;
    a.gx = q.grad_x;
    if (hipSetDevice(q.device) != hipSuccess) return MULUT_ENODEVICE;
    const int halo = backward ? ft_halo(a) : 2;      // (the forward kernels have no halo)
    hipError_t e;
    if constexpr (std::is_same<Args, FtArgs>::value) e = launch_ft_stage(a, backward, halo, (hipStream_t)q.stream);
    else e = launch_ft_interval_stage(a, q.interval, backward, halo, ft_num_cus(q.device), (hipStream_t)q.stream);
    return e == hipSuccess ? MULUT_OK : MULUT_EHIP;
}

static int ft_stage(const FtRule &rule, const FtRequest &q, bool backward) {
    if (rule.early == kFtEarlyInside && !q.inside) return MULUT_EINVAL;
    if (rule.early == kFtEarlyGradWq && backward && !q.grad_wq) return MULUT_EINVAL;
    return q.interval == 4 ? ft_stage_as<FtArgs>(rule, q, backward) : ft_stage_as<FtIvArgs>(rule, q, backward);
}

extern "C" {

int mulut_ft_quantize(int device, const float *const *weights, float *const *weights_q, int M, long long n, void *stream) {
    return ft_quantize(device, weights, weights_q, M, n, false, stream);
}

int mulut_ft_quantize_backward(int device, const float *const *weights, float *const *grad, int M, long long n, void *stream) {
    return ft_quantize(device, weights, grad, M, n, true, stream);
}

int mulut_ft_stage_forward(int device, const float *const *weights_q, const char *modes, int is_last, int u, const float *x,
                           int B, int C, int H, int W, float *out, void *stream) {
    return ft_stage(kFtPlain, {device, 4, weights_q, modes, is_last, u, x, B, C, H, W, out, nullptr, nullptr, nullptr, nullptr, stream}, false);
}

int mulut_ft_stage_backward(int device, const float *const *weights_q, const char *modes, int is_last, int u, const float *x,
                            const float *grad_out, int B, int C, int H, int W, float *const *grad_wq, float *grad_x,
                            void *stream) {
    return ft_stage(kFtPlain, {device, 4, weights_q, modes, is_last, u, x, B, C, H, W, nullptr, nullptr, grad_out, grad_wq, grad_x, stream}, true);
}

int mulut_ft_stage_forward_mask(int device, const float *const *weights_q, const char *modes, int is_last, int u, const float *x,
                                int B, int C, int H, int W, float *out, unsigned short *inside, void *stream) {
    return ft_stage(kFtMask, {device, 4, weights_q, modes, is_last, u, x, B, C, H, W, out, inside, nullptr, nullptr, nullptr, stream}, false);
}

int mulut_ft_stage_backward_mask(int device, const float *const *weights_q, const char *modes, int is_last, int u, const float *x,
                                 const float *grad_out, const unsigned short *inside, int B, int C, int H, int W,
                                 float *const *grad_wq, float *grad_x, void *stream) {
    return ft_stage(kFtMask, {device, 4, weights_q, modes, is_last, u, x, B, C, H, W, nullptr, inside, grad_out, grad_wq, grad_x, stream}, true);
}

// MuLUT.forward's stage at interval 5 / 6 (sr/model.py:289-312 with :42-44, 78-80), and autograd's backward of it
int mulut_ft_interval_stage_forward(int device, int interval, const float *const *weights_q, const char *modes, int is_last, int u,
                                    const float *x, int B, int C, int H, int W, float *out, unsigned short *inside, void *stream) {
    return ft_stage(kFtInterval, {device, interval, weights_q, modes, is_last, u, x, B, C, H, W, out, inside, nullptr, nullptr, nullptr, stream}, false);
}

int mulut_ft_interval_stage_backward(int device, int interval, const float *const *weights_q, const char *modes, int is_last, int u,
                                     const float *x, const float *grad_out, const unsigned short *inside, int B, int C, int H, int W,
                                     float *const *grad_wq, float *grad_x, void *stream) {
    return ft_stage(kFtInterval, {device, interval, weights_q, modes, is_last, u, x, B, C, H, W, nullptr, inside, grad_out, grad_wq, grad_x, stream}, true);
}

// The same stage for any list over s, d, y, e, h, o at interval 4, 5 or 6 (sr/model.py:69-312; the reference's module stops at s, d, y
// with "more sampling modes can be implemented similarly", :119-121 -- the 4 x 4 taps are common/network.py:173-215).  A list with one
// of e, h, o runs the backward kernels' HALO = 3 instances; a list without runs what the families above run, launch for launch.
int mulut_ft_wide_stage_forward(int device, int interval, const float *const *weights_q, const char *modes, int is_last, int u,
                                const float *x, int B, int C, int H, int W, float *out, unsigned short *inside, void *stream) {
    return ft_stage(kFtWide, {device, interval, weights_q, modes, is_last, u, x, B, C, H, W, out, inside, nullptr, nullptr, nullptr, stream}, false);
}

int mulut_ft_wide_stage_backward(int device, int interval, const float *const *weights_q, const char *modes, int is_last, int u,
                                 const float *x, const float *grad_out, const unsigned short *inside, int B, int C, int H, int W,
                                 float *const *grad_wq, float *grad_x, void *stream) {
    return ft_stage(kFtWide, {device, interval, weights_q, modes, is_last, u, x, B, C, H, W, nullptr, inside, grad_out, grad_wq, grad_x, stream}, true);
}

}  // extern "C"
