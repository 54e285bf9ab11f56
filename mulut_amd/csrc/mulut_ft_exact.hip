// mulut_ft_exact.hip -- the bit-reproducible backward of a fine-tune stage: fixed-point gradient sums.
//
// Reference: MuLUT.InterpTorchBatch + MuLUT.forward, sr/model.py:69-312 (autograd's backward of it; driver sr/3_finetune_lut.py).
// The backward kernels of mulut_ft.hip and mulut_ft_interval.hip sum their contributions with float32 atomics, so their last bits
// depend on the order in which the hardware runs the waves.  Here every contribution -- the same float32 expressions, written once
// in mulut_ft_exact.h -- is converted to a 64-bit fixed-point integer at a scale taken from max |grad_out| and the shape of the
// call, the integers are added (any order gives the same sum) and each sum is converted to float32 once.  One call is four launches:
//   fx_clear       zeroes the caller's workspace (its content on entry is irrelevant)
//   fx_gmax        integer maximum of |grad_out|'s bit patterns into word 0 of the workspace
//   fx_accumulate  one thread per site; table sums int64 [M][rows][u*u], input sums int64 [B][C][H][W], 64-bit integer atomics:
//                  into a workgroup-private band (interval 4: the tube) or image (5 at u = 1, 6) of the table sums in LDS, flushed
//                  once per workgroup and mode, and memory-side for what lies outside it.  u > 1: as in ft_stage_bwd the site threads
//                  hand (row, weight) items to the workgroup through LDS and 4 or 16 lanes add one row each -- a wave instruction
//                  adds whole rows, 128 contiguous bytes at u = 4 -- instead of 64 lanes adding to 64 different rows.  The site's
//                  own pixel is summed in a register, as an integer.
//   fx_finish      dst += float((double)sum * 2^-S) for every non-zero sum: one float add per element, none where the sum is 0
// Serves every list over s, d, y, e, h, o at the intervals 4, 5, 6 and u = 1..4 from one kernel template.
#include <hip/hip_runtime.h>

#include <cstring>

#include "mulut_kernels.h"

#pragma clang fp contract(off)

#include "mulut_ft_exact.h"

namespace mulut {

struct FxArgs {
    FtArgs f;                    // tables, destinations, x, grad_out, the mask, the shape and the key offsets (ft_fill())
    unsigned long long *ws;      // the caller's workspace (fx_ws_words())
    long long nsite, ntab;       // B C H W; M rows u*u
    int rows, reach;
    int tiles_per_wg;            // consecutive tiles of 256 sites a workgroup of fx_accumulate walks
};

__global__ void __launch_bounds__(256) fx_clear(unsigned long long *ws, long long n) {
    const long long stride = (long long)gridDim.x * 256;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += stride) ws[i] = 0ull;
}

__global__ void __launch_bounds__(256) fx_gmax(const float *gout, long long n, unsigned long long *ws) {
    __shared__ uint32_t s_max;
    if (threadIdx.x == 0) s_max = 0u;
    __syncthreads();
    uint32_t mx = 0u;
    const long long stride = (long long)gridDim.x * 256;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += stride) {
        const uint32_t b = (uint32_t)ft_bits(gout[i]) & 0x7fffffffu;
        mx = b > mx ? b : mx;
    }
    if (mx) atomicMax(&s_max, mx);
    __syncthreads();
    if (threadIdx.x == 0 && s_max) atomicMax((uint32_t *)ws, s_max);      // (low half of word 0)
}

// The workgroup's private copy of the table sums, int64 in LDS: what a batch of natural crops adds to the SAME few hundred rows
// (memory-side atomics serialise per address: 46 ms for the final stage at 256 x 48 x 48 without it, profiles/ft_exact_bench.json)
// is added on chip and goes to memory once per workgroup and mode.  Integer sums in LDS cannot change the result.
//   interval 4          the 1041-slot tube band (mulut_core.h): the rows of every pass whose four MSBs span at most one step;
//                       a pass outside the tube adds to memory.  8 KB at u = 1, 133 KB at u = 4: one mode at a time
//   interval 6          the whole table (625 rows)
//   interval 5, u = 1   the whole table (6,561 rows, 52 KB); u > 1: none (memory-side atomics only)
template <int IV, int U>
struct FxLds {
    static constexpr int EL = U * U, NT = 256;
    static constexpr int slots = IV == 4 ? kTubeSlots : IV == 6 ? IvGeom<6>::rows : U == 1 ? IvGeom<5>::rows : 0;
    static constexpr int band_bytes = slots * EL * 8;
    static constexpr int item_bytes = U == 1 ? 0 : NT * (EL + 1) * 4 + 2 * 5 * NT * 4;      // g of the sites, (row | slot, weight) of a pass
    static constexpr int bytes = band_bytes + item_bytes;
    static_assert(bytes <= 160 * 1024, "fx_accumulate: LDS");
};
static_assert(FxLds<4, 4>::bytes == 160896, "fx_accumulate<4, 4>: one workgroup per CU");

// table row of every tube-band slot (-1: the slot holds no row), for the flush of an interval-4 band
struct FxTubeRows { int row[kTubeSlots]; };
constexpr FxTubeRows fx_make_tube_rows() {
    FxTubeRows t{};
    for (int i = 0; i < kTubeSlots; ++i) t.row[i] = -1;
    for (int A = 0; A < kL; ++A)
        for (int B = (A < 2 ? 0 : A - 2); B < kL && B <= A + 2; ++B)
            for (int C = (A < 2 ? 0 : A - 2); C < kL && C <= A + 2; ++C)
                for (int D = (A < 2 ? 0 : A - 2); D < kL && D <= A + 2; ++D)
                    if (tube_contains(A, B, C, D)) t.row[tube_slot(A, B, C, D)] = A * kStrideA + B * kStrideB + C * kStrideC + D;
    return t;
}
__device__ const FxTubeRows kFxTubeRows = fx_make_tube_rows();

// 64-bit integer add into LDS as ds_add_u64 (an atomicAdd next to a global one on the other branch is merged with it into one flat
// atomic on a selected pointer, as mulut_ft.h notes for the float form; the flat form reaches LDS through the texture path)
__device__ __forceinline__ void fx_lds_add(unsigned long long *p, unsigned long long v) {
    __hip_atomic_fetch_add((__attribute__((address_space(3))) unsigned long long *)p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}

// Persistent workgroups: tiles_per_wg consecutive tiles of 256 sites each, one mode at a time, so that the band is zeroed and
// flushed once per workgroup and mode.
template <int IV, int U>
__global__ void __launch_bounds__(256) fx_accumulate(FxArgs A) {
    using G = IvGeom<IV>;
    using LD = FxLds<IV, U>;
    constexpr int EL = U * U, EPL = EL <= 1 ? 1 : EL <= 4 ? 4 : 16, NT = 256, SLOTS = LD::slots;
    extern __shared__ __attribute__((aligned(16))) unsigned char fx_smem[];
    unsigned long long *s_band = (unsigned long long *)fx_smem;                        // [SLOTS][EL]
    float (*s_g)[EL + 1] = (float (*)[EL + 1])(fx_smem + LD::band_bytes);              // [NT][EL + 1]      (u > 1)
    int (*s_idx)[NT] = (int (*)[NT])(fx_smem + LD::band_bytes + NT * (EL + 1) * 4);    // [5][NT]: row, or -(slot + 2) inside the band, -1: no site
    float (*s_wt)[NT] = (float (*)[NT])(fx_smem + LD::band_bytes + NT * (EL + 1) * 4 + 5 * NT * 4);
    const FtArgs &a = A.f;
    const uint32_t gbits = *(const uint32_t *)A.ws;
    if (gbits == 0u) return;      // grad_out is all zeros (uniform in the launch): no contribution
    const int Sw = fx_scale_w(gbits, A.nsite), Sx = fx_scale_x(gbits, U, a.M, A.reach, a.H, a.W);
    const long long ntile = (A.nsite + NT - 1) / NT;
    const long long t0 = (long long)blockIdx.x * A.tiles_per_wg, t1 = t0 + A.tiles_per_wg < ntile ? t0 + A.tiles_per_wg : ntile;
    const float avg = a.is_last ? (float)a.M : (float)(4 * a.M);
    for (int m = 0; m < a.M; ++m) {
        const float *tab = a.w[m];
        unsigned long long *wtab = A.ws + 1 + (long long)m * A.rows * EL;
        const int di[3] = {a.di[m][0], a.di[m][1], a.di[m][2]}, dj[3] = {a.dj[m][0], a.dj[m][1], a.dj[m][2]};
        if constexpr (SLOTS > 0) {
            for (int i = threadIdx.x; i < SLOTS * EL; i += NT) s_band[i] = 0ull;
            __syncthreads();      // the band is zero before any wave adds into it
        }
        for (long long t = t0; t < t1; ++t) {
            const long long s = t * NT + threadIdx.x;
            const bool valid = s < A.nsite;
            const long long sc = valid ? s : A.nsite - 1;      // surplus threads shadow the last site and contribute nothing
            const int x = (int)(sc % a.W), y = (int)((sc / a.W) % a.H);
            const long long bc = sc / ((long long)a.W * a.H);
            const float *plane = a.x + bc * a.H * a.W;
            unsigned long long *wx = A.ws + 1 + A.ntab + bc * a.H * a.W;      // the plane's input sums
            float g[EL];
            fx_site_g<U>(a.gout + bc * (long long)(a.H * U) * (a.W * U), a.W, y, x, valid ? (uint32_t)a.inside[sc] : 0u, avg, g);
            if constexpr (U > 1) {
                // (own row only; the last barrier of the tile before -- or the one behind the zeroing -- lies between its readers and this)
#pragma unroll
                for (int eo = 0; eo < EL; ++eo) s_g[threadIdx.x][eo] = g[eo];
            }
            long long own = 0;
#pragma unroll 1
            for (int r = 0; r < 4; ++r) {
                FxPass p;
                fx_pass<IV>(plane, a.H, a.W, y, x, r, di, dj, p);
                float dk[4];
                fx_key_grads<IV, U>(tab, p, r, g, dk);
                if constexpr (U == 1) {
                    if (valid) {
#pragma unroll
                        for (int j = 0; j < 5; ++j) {
                            const long long v = fx_quant(fx_table_term(p.wt[j], (float)G::q, g[0]), Sw);
                            const int slot = SLOTS == 0 ? -1 : IV == 4 ? p.slot[j] : p.idx[j];
                            if (v) {
                                if (slot >= 0) fx_lds_add(&s_band[slot], (unsigned long long)v);
                                else atomicAdd(&wtab[p.idx[j]], (unsigned long long)v);
                            }
                        }
                    }
                } else {
#pragma unroll
                    for (int j = 0; j < 5; ++j) {
                        const int slot = SLOTS == 0 ? -1 : IV == 4 ? p.slot[j] : p.idx[j];
                        s_idx[j][threadIdx.x] = !valid ? -1 : slot >= 0 ? -(slot + 2) : p.idx[j];
                        s_wt[j][threadIdx.x] = p.wt[j];
                    }
                }
                if (valid) {
                    own += fx_quant(dk[0], Sx);
#pragma unroll
                    for (int k = 1; k < 4; ++k) {
                        int dy, dx;
                        sample_offset(r, di[k - 1], dj[k - 1], dy, dx);
                        const long long v = fx_quant(dk[k], Sx);
                        if (v) atomicAdd(&wx[imin(imax(y + dy, 0), a.H - 1) * a.W + imin(imax(x + dx, 0), a.W - 1)], (unsigned long long)v);
                    }
                }
                if constexpr (U > 1) {
                    __syncthreads();      // (every thread of the workgroup is here: surplus threads walk the passes of the last site)
                    const int e = (int)threadIdx.x % EPL;
                    const int eo = eo_of_elem<U>(r, e < EL ? e : 0);
                    for (int it = (int)threadIdx.x / EPL; it < 5 * NT; it += NT / EPL) {
                        const int j = it / NT, si = it % NT;
                        const int idx = s_idx[j][si];
                        if (e < EL && idx != -1) {
                            const long long v = fx_quant(fx_table_term(s_wt[j][si], (float)G::q, s_g[si][eo]), Sw);
                            if (v) {
                                if (idx < 0) fx_lds_add(&s_band[(-idx - 2) * EL + e], (unsigned long long)v);
                                else atomicAdd(&wtab[(long long)idx * EL + e], (unsigned long long)v);
                            }
                        }
                    }
                    __syncthreads();
                }
            }
            if (valid && own) atomicAdd(&wx[y * a.W + x], (unsigned long long)own);
        }
        if constexpr (SLOTS > 0) {
            // the workgroup's sums into the workspace: contiguous words, zeros skipped
            __syncthreads();
            for (int i = threadIdx.x; i < SLOTS * EL; i += NT) {
                const unsigned long long v = s_band[i];
                if (v == 0ull) continue;
                const int row = IV == 4 ? kFxTubeRows.row[i / EL] : i / EL;
                if (row >= 0) atomicAdd(&wtab[(long long)row * EL + i % EL], v);
            }
            __syncthreads();      // (the next mode zeroes the band)
        }
    }
}

__global__ void __launch_bounds__(256) fx_finish(FxArgs A) {
    const FtArgs &a = A.f;
    const uint32_t gbits = *(const uint32_t *)A.ws;
    if (gbits == 0u) return;
    const int Sw = fx_scale_w(gbits, A.nsite), Sx = fx_scale_x(gbits, a.u, a.M, A.reach, a.H, a.W);
    const long long per = A.ntab / a.M, n = A.ntab + A.nsite, stride = (long long)gridDim.x * 256;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += stride) {
        const long long sum = (long long)A.ws[1 + i];
        if (sum == 0) continue;      // an element nothing was added to is not written
        if (i < A.ntab) {
            float *d = a.gw[i / per] + i % per;
            *d = *d + fx_result(sum, Sw);
        } else {
            float *d = a.gx + (i - A.ntab);
            *d = *d + fx_result(sum, Sx);
        }
    }
}

// The device's CU count, asked once per device (not capturable: the warm-up call of the capture contract does it)
static int fx_num_cus(int device) {
    static int cus[64];
    if (device < 0 || device >= 64) return 256;
    if (!cus[device]) {
        int n = 0;
        if (hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, device) != hipSuccess || n < 1) n = 256;
        cus[device] = n;
    }
    return cus[device];
}

template <int IV, int U>
static hipError_t launch_fx_accumulate_u(FxArgs A, int num_cus, hipStream_t st) {
    using LD = FxLds<IV, U>;
    const long long ntile = (A.nsite + 255) / 256;
    // as many workgroups as the chip holds at a time (a CU holds `fit` of them), each walking `per` consecutive tiles
    constexpr int fit = LD::bytes == 0 ? 8 : (160 * 1024 / LD::bytes < 8 ? 160 * 1024 / LD::bytes : 8);
    const long long slots = (long long)num_cus * fit;
    const long long per = LD::slots == 0 ? 1 : (ntile + slots - 1) / slots;
    A.tiles_per_wg = (int)per;
    const long long nb = (ntile + per - 1) / per;
    if (LD::bytes > 0) {
        const hipError_t e = raise_lds_limit((const void *)fx_accumulate<IV, U>, 160 * 1024);
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL((fx_accumulate<IV, U>), dim3((unsigned)nb), dim3(256), (size_t)LD::bytes, st, A);
    return hipGetLastError();
}

template <int IV>
static hipError_t launch_fx_accumulate(const FxArgs &A, int num_cus, hipStream_t st) {
    switch (A.f.u) {
        case 1: return launch_fx_accumulate_u<IV, 1>(A, num_cus, st);
        case 2: return launch_fx_accumulate_u<IV, 2>(A, num_cus, st);
        case 3: return launch_fx_accumulate_u<IV, 3>(A, num_cus, st);
        default: return launch_fx_accumulate_u<IV, 4>(A, num_cus, st);
    }
}

// The argument checks of both entry points, in the ABI's order (include/mulut.h): the family's early pointer and ft_fill() as for
// mulut_ft_wide_stage_backward, the call's own pointers, then the size of the problem.  (The query has no pointers to test and passes
// stand-ins.)  Returns MULUT_OK and the workspace's size in words, or the refusal.
constexpr long long kFxMaxSites = 0x7fffffffLL;
static int fx_check(FxArgs &A, int interval, const float *const *weights_q, const char *modes, int is_last, int u, const float *x,
                    const float *grad_out, const uint16_t *inside, int B, int C, int H, int W, float *const *grad_wq, const float *grad_x,
                    long long *words) {
    memset(&A, 0, sizeof(A));
    if (!grad_wq) return MULUT_EINVAL;
    const int rc = ft_fill(A.f, interval >= 4 && interval <= 6, weights_q, grad_wq, modes, is_last, u, x, inside, true, 3, B, C, H, W);
    if (rc) return rc;
    if (!grad_out || !grad_x) return MULUT_EINVAL;
    // (ft_fill leaves the problem's size open: the stage kernels refuse a grid beyond 2^31 - 1 at launch; here it decides the scale)
    const long long planes = (long long)B * C, plane = (long long)H * W;
    if (planes > kFxMaxSites || plane > kFxMaxSites || planes * plane > kFxMaxSites) return MULUT_EUNSUPPORTED;
    A.nsite = planes * plane;
    A.rows = interval_rows(interval);
    A.ntab = (long long)A.f.M * A.rows * (u * u);
    A.reach = ft_halo(A.f);
    *words = fx_ws_words(A.f.M, A.rows, u, A.nsite);
    return MULUT_OK;
}

}  // namespace mulut

using namespace mulut;

extern "C" {

long long mulut_ft_exact_ws_bytes(int interval, const char *modes, int u, int B, int C, int H, int W) {
    // stand-ins for the pointers a query does not have: never followed
    static const float probe = 0.0f;
    static float sink = 0.0f;
    const float *w[kMaxFtModes];
    float *gw[kMaxFtModes];
    for (int m = 0; m < kMaxFtModes; ++m) w[m] = &probe, gw[m] = &sink;
    FxArgs A;
    long long words = 0;
    const int rc = fx_check(A, interval, w, modes, 0, u, &probe, &probe, (const uint16_t *)&probe, B, C, H, W, gw, &sink, &words);
    return rc ? (long long)rc : words * 8;
}

int mulut_ft_exact_stage_backward(int device, int interval, const float *const *weights_q, const char *modes, int is_last, int u,
                                  const float *x, const float *grad_out, const unsigned short *inside, int B, int C, int H, int W,
                                  float *const *grad_wq, float *grad_x, void *ws, long long ws_bytes, void *stream) {
    FxArgs A;
    long long words = 0;
    const int rc = fx_check(A, interval, weights_q, modes, is_last, u, x, grad_out, inside, B, C, H, W, grad_wq, grad_x, &words);
    if (rc) return rc;
    if (!ws || ((uintptr_t)ws & 7u)) return MULUT_EINVAL;
    if (ws_bytes < words * 8) return MULUT_EWORKSPACE;
    A.f.gout = grad_out;
    A.f.gx = grad_x;
    A.ws = (unsigned long long *)ws;
    if (hipSetDevice(device) != hipSuccess) return MULUT_ENODEVICE;
    hipStream_t st = (hipStream_t)stream;
    auto blocks = [](long long n, long long most) { const long long nb = (n + 255) / 256; return (unsigned)(nb < most ? nb : most); };      // grid-stride beyond that
    hipLaunchKernelGGL(fx_clear, dim3(blocks(words, 8192)), dim3(256), 0, st, A.ws, words);
    // (every workgroup ends in one atomic on the same word, and those serialise: 8192 of them were most of this launch's 0.13 ms at 9.4 M floats)
    hipLaunchKernelGGL(fx_gmax, dim3(blocks(A.nsite * (u * u), 1024)), dim3(256), 0, st, grad_out, A.nsite * (u * u), A.ws);
    const int cus = fx_num_cus(device);
    const hipError_t e = interval == 4 ? launch_fx_accumulate<4>(A, cus, st) : interval == 5 ? launch_fx_accumulate<5>(A, cus, st) : launch_fx_accumulate<6>(A, cus, st);
    if (e != hipSuccess) return MULUT_EHIP;
    hipLaunchKernelGGL(fx_finish, dim3(blocks(A.ntab + A.nsite, 8192)), dim3(256), 0, st, A);
    return hipGetLastError() == hipSuccess ? MULUT_OK : MULUT_EHIP;
}

}  // extern "C"
