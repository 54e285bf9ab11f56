// ft_exact_memory_atomics_only.hip -- NOT BUILT.  The first correct form of mulut_amd/csrc/mulut_ft_exact.hip: every table sum goes
// to the workspace with a memory-side 64-bit atomic, nothing is kept in LDS.  Same bytes as the shipped kernel (the tests of
// tests/test_gpu_ft_fixed.py passed on it); on natural crops the hot rows serialise at the memory side: fx_accumulate<4, 4> 46.3 ms
// and <4, 1> 10.4 ms per step at 256 x 48 x 48 against 2.9 and 0.21 ms with the workgroup's band in LDS, the step 56.0 ms against
// 3.7 (33x the default step instead of 2.1x); on uniform noise the two forms take the same time (6.95 ms).  Numbers:
// profiles/ft_exact_bench_memory_atomics_only.json.  Kept for its launcher-free simplicity as the form to fall back to when reading
// the shipped kernel.
//
// Reference: MuLUT.InterpTorchBatch + MuLUT.forward, sr/model.py:69-312 (autograd's backward of it; driver sr/3_finetune_lut.py).
// The backward kernels of mulut_ft.hip and mulut_ft_interval.hip sum their contributions with float32 atomics, so their last bits
// depend on the order in which the hardware runs the waves.  Here every contribution -- the same float32 expressions, written once
// in mulut_ft_exact.h -- is converted to a 64-bit fixed-point integer at a scale taken from max |grad_out| and the shape of the
// call, the integers are added (any order gives the same sum) and each sum is converted to float32 once.  One call is four launches:
//   fx_clear       zeroes the caller's workspace (its content on entry is irrelevant)
//   fx_gmax        integer maximum of |grad_out|'s bit patterns into word 0 of the workspace
//   fx_accumulate  one thread per site; table sums int64 [M][rows][u*u], input sums int64 [B][C][H][W], memory-side 64-bit
//                  integer atomics.  u > 1: as in ft_stage_bwd the site threads hand (row, weight) items to the workgroup through
//                  LDS and 4 or 16 lanes add one row each -- a wave instruction adds whole rows, 128 contiguous bytes at u = 4 --
//                  instead of 64 lanes adding to 64 different rows.  The site's own pixel is summed in a register, as an integer.
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

template <int IV, int U>
__global__ void __launch_bounds__(256) fx_accumulate(FxArgs A) {
    using G = IvGeom<IV>;
    constexpr int EL = U * U, EPL = EL <= 1 ? 1 : EL <= 4 ? 4 : 16, NT = 256;
    __shared__ float s_g[U == 1 ? 1 : NT][EL + 1];
    __shared__ int s_idx[U == 1 ? 1 : 5][NT];
    __shared__ float s_wt[U == 1 ? 1 : 5][NT];
    const FtArgs &a = A.f;
    const uint32_t gbits = *(const uint32_t *)A.ws;
    if (gbits == 0u) return;      // grad_out is all zeros (uniform in the launch): no contribution
    const int Sw = fx_scale_w(gbits, A.nsite), Sx = fx_scale_x(gbits, U, a.M, A.reach, a.H, a.W);
    const long long s = (long long)blockIdx.x * NT + threadIdx.x;
    const bool valid = s < A.nsite;
    const long long sc = valid ? s : A.nsite - 1;      // surplus threads shadow the last site and contribute nothing
    const int x = (int)(sc % a.W), y = (int)((sc / a.W) % a.H);
    const long long bc = sc / ((long long)a.W * a.H);
    const float *plane = a.x + bc * a.H * a.W;
    unsigned long long *wx = A.ws + 1 + A.ntab + bc * a.H * a.W;      // the plane's input sums
    const float avg = a.is_last ? (float)a.M : (float)(4 * a.M);
    float g[EL];
    fx_site_g<U>(a.gout + bc * (long long)(a.H * U) * (a.W * U), a.W, y, x, valid ? (uint32_t)a.inside[sc] : 0u, avg, g);
    if constexpr (U > 1) {
#pragma unroll
        for (int eo = 0; eo < EL; ++eo) s_g[threadIdx.x][eo] = g[eo];
    }
    long long own = 0;
    for (int m = 0; m < a.M; ++m) {
        const float *tab = a.w[m];
        unsigned long long *wtab = A.ws + 1 + (long long)m * A.rows * EL;
        const int di[3] = {a.di[m][0], a.di[m][1], a.di[m][2]}, dj[3] = {a.dj[m][0], a.dj[m][1], a.dj[m][2]};
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
                        const long long t = fx_quant(fx_table_term(p.wt[j], (float)G::q, g[0]), Sw);
                        if (t) atomicAdd(&wtab[p.idx[j]], (unsigned long long)t);
                    }
                }
            } else {
#pragma unroll
                for (int j = 0; j < 5; ++j) {
                    s_idx[j][threadIdx.x] = valid ? p.idx[j] : -1;
                    s_wt[j][threadIdx.x] = p.wt[j];
                }
            }
            if (valid) {
                own += fx_quant(dk[0], Sx);
#pragma unroll
                for (int k = 1; k < 4; ++k) {
                    int dy, dx;
                    sample_offset(r, di[k - 1], dj[k - 1], dy, dx);
                    const long long t = fx_quant(dk[k], Sx);
                    if (t) atomicAdd(&wx[imin(imax(y + dy, 0), a.H - 1) * a.W + imin(imax(x + dx, 0), a.W - 1)], (unsigned long long)t);
                }
            }
            if constexpr (U > 1) {
                __syncthreads();      // (every thread of the workgroup is here: surplus threads walk the passes of the last site)
                const int e = (int)threadIdx.x % EPL;
                const int eo = eo_of_elem<U>(r, e < EL ? e : 0);
                for (int it = (int)threadIdx.x / EPL; it < 5 * NT; it += NT / EPL) {
                    const int j = it / NT, si = it % NT;
                    const int idx = s_idx[j][si];
                    if (e < EL && idx >= 0) {
                        const long long t = fx_quant(fx_table_term(s_wt[j][si], (float)G::q, s_g[si][eo]), Sw);
                        if (t) atomicAdd(&wtab[(long long)idx * EL + e], (unsigned long long)t);
                    }
                }
                __syncthreads();
            }
        }
    }
    if (valid && own) atomicAdd(&wx[y * a.W + x], (unsigned long long)own);
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

template <int IV>
static void launch_fx_accumulate(const FxArgs &A, unsigned nb, hipStream_t st) {
    switch (A.f.u) {
        case 1: hipLaunchKernelGGL((fx_accumulate<IV, 1>), dim3(nb), dim3(256), 0, st, A); break;
        case 2: hipLaunchKernelGGL((fx_accumulate<IV, 2>), dim3(nb), dim3(256), 0, st, A); break;
        case 3: hipLaunchKernelGGL((fx_accumulate<IV, 3>), dim3(nb), dim3(256), 0, st, A); break;
        default: hipLaunchKernelGGL((fx_accumulate<IV, 4>), dim3(nb), dim3(256), 0, st, A); break;
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
    auto blocks = [](long long n) { const long long nb = (n + 255) / 256; return (unsigned)(nb < 8192 ? nb : 8192); };      // grid-stride beyond that
    hipLaunchKernelGGL(fx_clear, dim3(blocks(words)), dim3(256), 0, st, A.ws, words);
    hipLaunchKernelGGL(fx_gmax, dim3(blocks(A.nsite * (u * u))), dim3(256), 0, st, grad_out, A.nsite * (u * u), A.ws);
    const unsigned nb = (unsigned)((A.nsite + 255) / 256);
    if (interval == 4) launch_fx_accumulate<4>(A, nb, st);
    else if (interval == 5) launch_fx_accumulate<5>(A, nb, st);
    else launch_fx_accumulate<6>(A, nb, st);
    hipLaunchKernelGGL(fx_finish, dim3(blocks(A.ntab + A.nsite)), dim3(256), 0, st, A);
    return hipGetLastError() == hipSuccess ? MULUT_OK : MULUT_EHIP;
}

}  // extern "C"
