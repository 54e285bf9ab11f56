// mulut_eval.hip -- device-side evaluation of a super-resolved frame against its ground truth:
// Y-channel PSNR and SSIM exactly as the reference's test script computes them
//   y = _rgb2ycbcr(img)[:, :, 0]            common/utils.py:42-60   (BT.601 studio swing, float64)
//   PSNR(y_gt, y_out, shave=scale)          common/utils.py:63-72   (float32 difference, border shaved)
//   cal_ssim(y_gt, y_out)                   common/utils.py:75-101  (11x11 Gaussian sigma 1.5, 'valid', float64)
// used at sr/4_test_lut.py:313-315.  Not on the inference hot path: it saves the D2H copy of two HR frames
// per image when a whole benchmark set is scored.  Two kernels, each leaving one float64 partial sum per
// workgroup; the host adds the partials in index order (deterministic).
//
// The list form (mulut_eval_plan_*: the validation loop of sr/3_finetune_lut.py:23-65 scored in one stream-ordered call) runs the SAME
// two workgroup bodies over many pairs of different sizes: workgroup g of a launch looks up (item, block or tile) in a map built once
// by the host, leaves its partial in the plan's workspace, and eval_sum_kernel then adds each item's partials in index order, one
// lane per sum -- the additions mulut_eval_y's host makes, so mulut_eval_finish gives the same two doubles bit for bit.  Workgroups
// of the squared error whose first pixel lies beyond the item (blocks >= ceil(interior / 256)) would only add +0.0 to a sum that is
// never negative, and are not launched.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <new>
#include <vector>

#include "../../include/mulut.h"

namespace {

__device__ __forceinline__ double luma(const uint8_t *p) {
    // first row of T (common/utils.py:46) and O[0] = 16
    return (double)p[0] * 0.256788235294118 + (double)p[1] * 0.504129411764706 + (double)p[2] * 0.097905882352941 + 16.0;
}

constexpr int kSseThreads = 256;

constexpr int kSseBlocks = 1024;

// sum over the shaved interior of (float32(y_out) - float32(y_gt))^2, squared in float32 as the reference does: block `blk` of a
// grid-stride assignment over `blocks` x kSseThreads threads (always kSseBlocks); the block's sum is returned to thread 0
__device__ __forceinline__ double sse_block(const uint8_t *gt, const uint8_t *out, int H, int W, int shave, unsigned blk, unsigned blocks) {
    const int h = H - 2 * shave, w = W - 2 * shave;
    const long long n = (long long)h * w;
    double acc = 0.0;
    for (long long i = (long long)blk * kSseThreads + threadIdx.x; i < n; i += (long long)blocks * kSseThreads) {
        const int y = (int)(i / w) + shave, x = (int)(i % w) + shave;
        const size_t o = ((size_t)y * W + x) * 3;
        const float d = (float)luma(out + o) - (float)luma(gt + o);
        acc += (double)(d * d);
    }
    __shared__ double s[kSseThreads];
    s[threadIdx.x] = acc;
    __syncthreads();
    for (int k = kSseThreads / 2; k > 0; k >>= 1) {
        if ((int)threadIdx.x < k) s[threadIdx.x] += s[threadIdx.x + k];
        __syncthreads();
    }
    return s[0];
}

// (always launched with kSseBlocks workgroups)
__global__ void __launch_bounds__(kSseThreads) sse_y_kernel(const uint8_t *gt, const uint8_t *out, int H, int W, int shave,
                                                           double *partial) {
    const double v = sse_block(gt, out, H, W, shave, blockIdx.x, gridDim.x);
    if (threadIdx.x == 0) partial[blockIdx.x] = v;
}

constexpr int kWin = 11, kT = 32;          // window, output tile edge
constexpr int kP = kT + kWin - 1;          // 42: input patch edge

struct Gauss {
    double k[kWin];
};

// one workgroup = one 32x32 tile of the 'valid' SSIM map; both luma patches staged in LDS as float64 (a pixel outside the image is
// read only for tile positions that are masked); thread 0 stores the tile's sum to DST.  The body of ssim_y_kernel and of
// ssim_list_kernel, over the names gt, out, H, W and g of the kernel it stands in.  A macro and not a function on purpose:
// moved into an inline function, ssim_y_kernel was compiled to another instruction stream (rolled window loops, another set of
// contracted multiply-adds) and its sums changed in the last bit on some pairs; as a macro the kernel is the text it was, token for
// token, and compiles to the instructions it had (tools/asm_compare.py).
#define MULUT_SSIM_TILE(TILE, DST) \
    __shared__ double sa[kP * kP], sb[kP * kP];                                                      \
    __shared__ double red[256];                                                                      \
    const int oh = H - (kWin - 1), ow = W - (kWin - 1);                                              \
    const int tiles_x = (ow + kT - 1) / kT;                                                          \
    const int ty0 = (int)((TILE) / tiles_x) * kT, tx0 = (int)((TILE) % tiles_x) * kT;                \
    for (int i = threadIdx.x; i < kP * kP; i += 256) {                                               \
        int y = ty0 + i / kP, x = tx0 + i % kP;                                                      \
        y = y < H ? y : H - 1;                                                                       \
        x = x < W ? x : W - 1;                                                                       \
        const size_t o = ((size_t)y * W + x) * 3;                                                    \
        sa[i] = luma(gt + o);                                                                        \
        sb[i] = luma(out + o);                                                                       \
    }                                                                                                \
    __syncthreads();                                                                                 \
    const double C1 = (0.01 * 255) * (0.01 * 255), C2 = (0.03 * 255) * (0.03 * 255);                 \
    const int lx = threadIdx.x % kT, ly0 = (int)(threadIdx.x / kT) * 4;                              \
    double sum = 0.0;                                                                                \
    for (int q = 0; q < 4; ++q) {                                                                    \
        const int ly = ly0 + q;                                                                      \
        if (ty0 + ly >= oh || tx0 + lx >= ow) continue;                                              \
        double m1 = 0, m2 = 0, s11 = 0, s22 = 0, s12 = 0;                                            \
        for (int i = 0; i < kWin; ++i) {                                                             \
            const double *ra = sa + (ly + i) * kP + lx, *rb = sb + (ly + i) * kP + lx;               \
            for (int j = 0; j < kWin; ++j) {                                                         \
                const double wgt = g.k[i] * g.k[j], a = ra[j], b = rb[j];                            \
                m1 += wgt * a;                                                                       \
                m2 += wgt * b;                                                                       \
                s11 += wgt * (a * a);                                                                \
                s22 += wgt * (b * b);                                                                \
                s12 += wgt * (a * b);                                                                \
            }                                                                                        \
        }                                                                                            \
        const double v1 = s11 - m1 * m1, v2 = s22 - m2 * m2, cov = s12 - m1 * m2;                    \
        sum += ((2 * m1 * m2 + C1) * (2 * cov + C2)) / ((m1 * m1 + m2 * m2 + C1) * (v1 + v2 + C2));  \
    }                                                                                                \
    red[threadIdx.x] = sum;                                                                          \
    __syncthreads();                                                                                 \
    for (int k = 128; k > 0; k >>= 1) {                                                              \
        if ((int)threadIdx.x < k) red[threadIdx.x] += red[threadIdx.x + k];                          \
        __syncthreads();                                                                             \
    }                                                                                                \
    if (threadIdx.x == 0) (DST) = red[0];

__global__ void __launch_bounds__(256) ssim_y_kernel(const uint8_t *gt, const uint8_t *out, int H, int W, Gauss g, double *partial) {
    MULUT_SSIM_TILE(blockIdx.x, partial[blockIdx.x]);
}

// ---- the list form: many pairs of different sizes, one launch per kernel
struct EvalItem {                 // one pair as the kernels see it
    long long gt_off, out_off;    // bytes into the ground-truth pool / the output pool
    long long part;               // the item's partials in the workspace: nsse block sums, then ntile tile sums
    int H, W, nsse, ntile;
};
struct EvalGroup {                // workgroup -> (item, block or tile of that item)
    int item, idx;
};
constexpr int kSumThreads = 64;

}  // namespace

namespace mulut {

__global__ void __launch_bounds__(kSseThreads) sse_list_kernel(const uint8_t *gt_pool, const uint8_t *out_pool, const EvalItem *items,
                                                              const EvalGroup *map, int shave, double *ws) {
    const EvalGroup m = map[blockIdx.x];
    const EvalItem it = items[m.item];
    const double v = sse_block(gt_pool + it.gt_off, out_pool + it.out_off, it.H, it.W, shave, (unsigned)m.idx, (unsigned)kSseBlocks);
    if (threadIdx.x == 0) ws[it.part + m.idx] = v;
}

__global__ void __launch_bounds__(256) ssim_list_kernel(const uint8_t *gt_pool, const uint8_t *out_pool, const EvalItem *items,
                                                       const EvalGroup *map, Gauss g, double *ws) {
    const EvalGroup m = map[blockIdx.x];
    const EvalItem it = items[m.item];
    const uint8_t *gt = gt_pool + it.gt_off, *out = out_pool + it.out_off;
    const int H = it.H, W = it.W;
    MULUT_SSIM_TILE((unsigned)m.idx, ws[it.part + it.nsse + m.idx]);
}

// one workgroup (one wave) per item: its partials in index order, first the block sums, then the tile sums -- the additions
// mulut_eval_y's host makes, blocks that hold +0.0 left out.  The wave fetches 64 partials at a time; lane 0 adds them one by one.
__global__ void __launch_bounds__(kSumThreads) eval_sum_kernel(const EvalItem *items, const double *ws, double *sums) {
    __shared__ double buf[kSumThreads];
    const EvalItem it = items[blockIdx.x];
    for (int which = 0; which < 2; ++which) {
        const double *p = ws + it.part + (which ? it.nsse : 0);
        const int n = which ? it.ntile : it.nsse;
        double acc = 0.0;
        for (int c = 0; c < n; c += kSumThreads) {
            if (c + (int)threadIdx.x < n) buf[threadIdx.x] = p[c + threadIdx.x];
            __syncthreads();
            if (threadIdx.x == 0) {
                const int m = n - c < kSumThreads ? n - c : kSumThreads;
                for (int j = 0; j < m; ++j) acc += buf[j];
            }
            __syncthreads();
        }
        if (threadIdx.x == 0) sums[2 * (long long)blockIdx.x + which] = acc;
    }
}

}  // namespace mulut

namespace {

long long ssim_tiles(int H, int W) {
    const long long oh = H - (kWin - 1), ow = W - (kWin - 1);
    if (oh <= 0 || ow <= 0) return 0;
    return ((oh + kT - 1) / kT) * ((ow + kT - 1) / kT);
}

// blocks of the squared error that see a pixel: block b starts at pixel 256 b of the first grid-stride pass
long long sse_blocks(int H, int W, int shave) {
    const long long n = (long long)(H - 2 * shave) * (W - 2 * shave);
    const long long b = (n + kSseThreads - 1) / kSseThreads;
    return b < kSseBlocks ? b : kSseBlocks;
}

Gauss make_gauss() {   // cv2.getGaussianKernel(11, 1.5): exp(-(i-5)^2 / (2 sigma^2)), normalised (common/utils.py:78)
    Gauss g;
    double tot = 0;
    for (int i = 0; i < kWin; ++i) { g.k[i] = std::exp(-((i - 5.0) * (i - 5.0)) / (2.0 * 1.5 * 1.5)); tot += g.k[i]; }
    for (int i = 0; i < kWin; ++i) g.k[i] /= tot;
    return g;
}

// an image of H x W x 3 bytes at `off` lies inside a pool of `pool` bytes (no product here can overflow 64 bits)
bool image_inside(long long off, int H, int W, long long pool) {
    if (off < 0 || pool < 0) return false;
    const long long px = (long long)H * W;
    if (px > pool / 3) return false;
    return off <= pool - px * 3;
}

}  // namespace

struct mulut_eval_plan {
    int device, n, shave;
    unsigned sse_groups, ssim_groups;
    unsigned char *dev;           // one allocation: items, the two maps, the partial sums
    size_t sse_map_at, ssim_map_at, ws_at;
};

extern "C" {

long long mulut_eval_ws_doubles(int H, int W) { return (long long)kSseBlocks + ssim_tiles(H, W); }

/* the last four lines of PSNR and cal_ssim's mean: common/utils.py:63-72,101 */
int mulut_eval_finish(double sse, double ssim_sum, int H, int W, int shave, double *psnr, double *ssim) {
    if (!psnr || !ssim || H <= 0 || W <= 0 || shave < 0) return MULUT_EINVAL;
    if (H - 2LL * shave <= 0 || W - 2LL * shave <= 0 || H < kWin || W < kWin) return MULUT_ESHAPE;
    const double n = (double)(H - 2 * shave) * (double)(W - 2 * shave);
    const double rmse = std::sqrt((double)(float)(sse / n));   // np.mean of a float32 array is a float32
    *psnr = 20.0 * std::log10(255.0 / rmse);
    *ssim = ssim_sum / ((double)(H - (kWin - 1)) * (double)(W - (kWin - 1)));
    return MULUT_OK;
}

int mulut_eval_y(int device, const void *gt_hwc, const void *out_hwc, int H, int W, int shave, double *ws, long long ws_doubles,
                 double *psnr, double *ssim, void *stream) {
    if (!gt_hwc || !out_hwc || !ws || !psnr || !ssim || H <= 0 || W <= 0 || shave < 0) return MULUT_EINVAL;
    if (H - 2 * shave <= 0 || W - 2 * shave <= 0 || H < kWin || W < kWin) return MULUT_ESHAPE;
    const long long tiles = ssim_tiles(H, W);
    if (ws_doubles < kSseBlocks + tiles) return MULUT_EWORKSPACE;
    if (hipSetDevice(device) != hipSuccess) return MULUT_ENODEVICE;
    hipStream_t st = (hipStream_t)stream;
    const Gauss g = make_gauss();
    hipLaunchKernelGGL(sse_y_kernel, dim3(kSseBlocks), dim3(kSseThreads), 0, st, (const uint8_t *)gt_hwc, (const uint8_t *)out_hwc, H, W,
                       shave, ws);
    hipLaunchKernelGGL(ssim_y_kernel, dim3((unsigned)tiles), dim3(256), 0, st, (const uint8_t *)gt_hwc, (const uint8_t *)out_hwc, H, W, g,
                       ws + kSseBlocks);
    if (hipGetLastError() != hipSuccess) return MULUT_EHIP;
    std::vector<double> h((size_t)(kSseBlocks + tiles));
    if (hipMemcpyAsync(h.data(), ws, h.size() * sizeof(double), hipMemcpyDeviceToHost, st) != hipSuccess) return MULUT_EHIP;
    if (hipStreamSynchronize(st) != hipSuccess) return MULUT_EHIP;
    double sse = 0, s = 0;
    for (int i = 0; i < kSseBlocks; ++i) sse += h[i];
    for (long long i = 0; i < tiles; ++i) s += h[kSseBlocks + i];
    return mulut_eval_finish(sse, s, H, W, shave, psnr, ssim);
}

/* sr/3_finetune_lut.py:23-65 (the scoring of :56-58 for a whole list of pairs) */
int mulut_eval_plan_create(int device, const mulut_eval_item *items, int n, int shave, mulut_eval_plan **out_plan) {
    if (!out_plan) return MULUT_EINVAL;
    *out_plan = nullptr;
    if (!items || n < 1 || shave < 0) return MULUT_EINVAL;
    for (int i = 0; i < n; ++i)
        if (items[i].H < kWin || items[i].W < kWin || items[i].H <= 2LL * shave || items[i].W <= 2LL * shave) return MULUT_ESHAPE;
    for (int i = 0; i < n; ++i)
        if (!image_inside(items[i].gt_off, items[i].H, items[i].W, items[i].gt_pool_bytes) ||
            !image_inside(items[i].out_off, items[i].H, items[i].W, items[i].out_pool_bytes))
            return MULUT_EINVAL;
    long long sse_groups = 0, ssim_groups = 0;
    for (int i = 0; i < n; ++i) {      // (an item adds fewer than 2^53 tiles: the running sums stay far inside 64 bits)
        sse_groups += sse_blocks(items[i].H, items[i].W, shave);
        ssim_groups += ssim_tiles(items[i].H, items[i].W);
        if (sse_groups >= (1LL << 31) || ssim_groups >= (1LL << 31)) return MULUT_EUNSUPPORTED;
    }
    const size_t sse_map_at = (size_t)n * sizeof(EvalItem), ssim_map_at = sse_map_at + (size_t)sse_groups * sizeof(EvalGroup);
    const size_t ws_at = ssim_map_at + (size_t)ssim_groups * sizeof(EvalGroup);
    static_assert(sizeof(EvalItem) % 8 == 0 && sizeof(EvalGroup) == 8, "the workspace of doubles starts 8-aligned");
    std::vector<unsigned char> host;
    try {
        host.resize(ws_at);
    } catch (const std::bad_alloc &) {
        return MULUT_EUNSUPPORTED;
    }
    EvalItem *hi = reinterpret_cast<EvalItem *>(host.data());
    EvalGroup *ma = reinterpret_cast<EvalGroup *>(host.data() + sse_map_at), *mb = reinterpret_cast<EvalGroup *>(host.data() + ssim_map_at);
    long long part = 0;
    for (int i = 0; i < n; ++i) {
        const int nsse = (int)sse_blocks(items[i].H, items[i].W, shave), ntile = (int)ssim_tiles(items[i].H, items[i].W);
        hi[i] = EvalItem{items[i].gt_off, items[i].out_off, part, items[i].H, items[i].W, nsse, ntile};
        for (int k = 0; k < nsse; ++k) *ma++ = EvalGroup{i, k};
        for (int k = 0; k < ntile; ++k) *mb++ = EvalGroup{i, k};
        part += (long long)nsse + ntile;
    }
    if (hipSetDevice(device) != hipSuccess) return MULUT_ENODEVICE;
    mulut_eval_plan *p = new (std::nothrow) mulut_eval_plan{device, n, shave, (unsigned)sse_groups, (unsigned)ssim_groups, nullptr,
                                                            sse_map_at, ssim_map_at, ws_at};
    if (!p) return MULUT_EHIP;
    if (hipMalloc(reinterpret_cast<void **>(&p->dev), ws_at + (size_t)part * sizeof(double)) != hipSuccess) {
        delete p;
        return MULUT_EHIP;
    }
    if (hipMemcpy(p->dev, host.data(), ws_at, hipMemcpyHostToDevice) != hipSuccess) {
        (void)hipFree(p->dev);
        delete p;
        return MULUT_EHIP;
    }
    *out_plan = p;
    return MULUT_OK;
}

int mulut_eval_plan_destroy(mulut_eval_plan *plan) {
    if (!plan) return MULUT_EINVAL;
    int rc = MULUT_OK;
    if (hipSetDevice(plan->device) != hipSuccess) rc = MULUT_ENODEVICE;
    else if (hipFree(plan->dev) != hipSuccess) rc = MULUT_EHIP;
    delete plan;
    return rc;
}

/* sr/3_finetune_lut.py:56-58 */
int mulut_eval_plan_run(const mulut_eval_plan *plan, const void *gt_pool, const void *out_pool, double *sums, void *stream) {
    if (!plan || !gt_pool || !out_pool || !sums) return MULUT_EINVAL;
    if (hipSetDevice(plan->device) != hipSuccess) return MULUT_ENODEVICE;
    hipStream_t st = (hipStream_t)stream;
    const EvalItem *items = reinterpret_cast<const EvalItem *>(plan->dev);
    const EvalGroup *ma = reinterpret_cast<const EvalGroup *>(plan->dev + plan->sse_map_at);
    const EvalGroup *mb = reinterpret_cast<const EvalGroup *>(plan->dev + plan->ssim_map_at);
    double *ws = reinterpret_cast<double *>(plan->dev + plan->ws_at);
    hipLaunchKernelGGL(mulut::sse_list_kernel, dim3(plan->sse_groups), dim3(kSseThreads), 0, st, (const uint8_t *)gt_pool, (const uint8_t *)out_pool,
                       items, ma, plan->shave, ws);
    hipLaunchKernelGGL(mulut::ssim_list_kernel, dim3(plan->ssim_groups), dim3(256), 0, st, (const uint8_t *)gt_pool, (const uint8_t *)out_pool,
                       items, mb, make_gauss(), ws);
    hipLaunchKernelGGL(mulut::eval_sum_kernel, dim3((unsigned)plan->n), dim3(kSumThreads), 0, st, items, (const double *)ws, sums);
    return hipGetLastError() == hipSuccess ? MULUT_OK : MULUT_EHIP;
}

}  // extern "C"

