// mulut_ft_data.hip -- the fine-tune loop's training batches, cut on the device from a device-resident training set.
//
// Reference: DIV2K.__getitem__, sr/data.py:91-121 (restated by CropProvider.next(), mulut_amd/finetune_lut.py): a random pair, a
// random sz x sz window of one colour channel of its LR image and the scale-times window of its HR image, np.fliplr, np.flipud,
// np.rot90(., k), astype(float32) / 255.0.  The reference draws and cuts in DataLoader workers (sr/data.py:27-49) and copies the
// float batch to the device; here the pairs lie in device memory as the uint8 bytes the PNGs hold, the host draws only the six
// integers of a sample (pair, i, j, c, flips, k) and one launch cuts, turns and converts the whole batch.
//
//   ft_crop_kernel    a workgroup of 4 waves takes up to 8 consecutive 32 x 32 tiles of ONE sample's two output planes (im, then lb),
//                     a wave one tile at a time in a tile of LDS of its own -- no workgroup barrier after the start.  The draw and
//                     the pair are read and vetted once per workgroup, so a tile's only trip to memory before its stores is its
//                     16 byte loads per lane, all in flight together.  (First written as persistent workgroups over single tiles, each
//                     tile re-reading draw and pair and crossing two barriers: 37 us for bs 256 x 48 x 48 x4 against 9.5 us for a
//                     plain fill of the outputs -- three dependent trips to memory per 4 KB stored.)  With A the n x n window
//                     (n = sz, or sz * scale), out[y][x] = A[u][v] where
//                        (p, q) = (y, x) | (x, n-1-y) | (n-1-y, n-1-x) | (n-1-x, y)   for k = 0 | 1 | 2 | 3   (np.rot90)
//                        u = flipud ? n-1-p : p,   v = fliplr ? n-1-q : q,
//                     an affine map whose byte strides per y and per x are worked out once per tile.
//                     For k odd an output row walks a source column, so the tile is LOADED with the lanes along the source row
//                     (bytes `ch` apart, one or two cache lines per 32 lanes) and turned in LDS: the loader writes tile[y][x]
//                     with x or y along the lanes, as the turn asks, and the writer always reads 4 consecutive x of a row and
//                     stores 16 bytes.  The row stride of 33 floats keeps both the turned write and the row read off shared
//                     banks.  Where sz * scale is not a multiple of 4 or an output base is not 16-byte aligned, and at the right
//                     edge of a plane, the writer stores single floats.
//                     byte -> float32(byte) / 255.0f comes from a 256-entry table evaluated by the host compiler (IEEE division,
//                     whatever the device's division flags are) and staged in LDS once per workgroup.
// The draws are device-resident, so the host cannot vet them: the kernel does, once per workgroup, with compares that are uniform
// in it.  A sample that fails is written as zeros and counted once in *bad; no address is formed from it.
//
//   ft_val_pack_kernel  the other end of the loop's data: the module's output for one validation image (float32 planar, 0..1) to the
//                     packed bytes the validation scores and saves, sr/3_finetune_lut.py:50-54 -- times 255, clamp, round half to
//                     even -- in one launch, into a slot of a pool at any byte address.
#include <hip/hip_runtime.h>

#include "../../include/mulut.h"

namespace mulut {

constexpr int kCropTile = 32, kCropStride = kCropTile + 1, kCropWaves = 4, kCropNT = 64 * kCropWaves, kCropChunk = 2 * kCropWaves;

struct CropTable {
    float v[256];
};
constexpr CropTable make_crop_table() {
    CropTable t{};
    for (int b = 0; b < 256; ++b) t.v[b] = (float)b / 255.0f;
    return t;
}
__device__ const CropTable kCropTable = make_crop_table();

struct CropArgs {
    const unsigned char *pool;
    long long pool_bytes;
    const mulut_ft_pair *pairs;
    const int *draws;
    float *im, *lb;
    int *bad;
    int n_pairs, B, sz, scale;
    int t_lr, t_hr;      // tiles per side of an im / lb plane
    int vec_lr, vec_hr;  // 16-byte stores allowed on that plane
    int chunks;          // workgroups per sample: ceil((t_lr^2 + t_hr^2) / kCropChunk)
};

// an image of h x w x ch bytes at `off` lies inside the pool (no product here can overflow 64 bits)
__device__ __forceinline__ bool crop_image_inside(long long off, int h, int w, int ch, long long pool_bytes) {
    if (h <= 0 || w <= 0 || ch <= 0 || off < 0) return false;
    const long long px = (long long)h * w;
    if (px > pool_bytes / ch) return false;
    return off <= pool_bytes - px * ch;
}

__global__ void __launch_bounds__(kCropNT) ft_crop_kernel(CropArgs a) {
    static_assert(kCropNT == 256, "one table entry per thread");
    __shared__ float s_tab[256];
    __shared__ float s_tiles[kCropWaves][kCropTile * kCropStride];
    s_tab[threadIdx.x] = kCropTable.v[threadIdx.x];
    const int b = (int)(blockIdx.x / (unsigned)a.chunks), chunk = (int)(blockIdx.x % (unsigned)a.chunks);
    const int wave = (int)threadIdx.x >> 6, lane = (int)threadIdx.x & 63;
    // ---- the sample's draw and pair, vetted (everything here is uniform in the workgroup)
    const int *d = a.draws + (long long)b * 6;
    const int pi = d[0], i = d[1], j = d[2], c = d[3], flips = d[4], k = d[5] & 3;
    bool ok = pi >= 0 && pi < a.n_pairs && i >= 0 && j >= 0 && c >= 0;
    mulut_ft_pair p = {};
    if (ok) {
        p = a.pairs[pi];
        ok = c < p.ch && crop_image_inside(p.lr_off, p.lr_h, p.lr_w, p.ch, a.pool_bytes) &&
             crop_image_inside(p.hr_off, p.hr_h, p.hr_w, p.ch, a.pool_bytes) &&
             i <= p.lr_h - a.sz && j <= p.lr_w - a.sz &&                                       // i + sz <= lr_h, j + sz <= lr_w
             ((long long)i + a.sz) * a.scale <= p.hr_h && ((long long)j + a.sz) * a.scale <= p.hr_w;
    }
    if (!ok && chunk == 0 && threadIdx.x == 0 && a.bad) atomicAdd(a.bad, 1);      // once per sample
    __syncthreads();      // the table is staged
    float *tile = s_tiles[wave];
    const int n_lr_tiles = a.t_lr * a.t_lr, per_sample = n_lr_tiles + a.t_hr * a.t_hr;
    const int t_end = (chunk + 1) * kCropChunk < per_sample ? (chunk + 1) * kCropChunk : per_sample;
    const int lx = lane & 31, ly = lane >> 5;        // loader: 2 rows of 32 lanes, 16 times
    const int wx = (lane & 7) * 4, wy = lane >> 3;   // writer: 4 consecutive x of one of 8 rows, 4 times
    for (int t = chunk * kCropChunk + wave; t < t_end; t += kCropWaves) {
        const bool hr = t >= n_lr_tiles;
        const int r = hr ? t - n_lr_tiles : t;
        const int tps = hr ? a.t_hr : a.t_lr, s = hr ? a.scale : 1, n = a.sz * s;
        const int Y0 = (r / tps) * kCropTile, X0 = (r % tps) * kCropTile;
        if (ok) {
            const long long off = hr ? p.hr_off : p.lr_off;
            const int w = hr ? p.hr_w : p.lr_w, ch = p.ch;
            // u = uc + uy * y + ux * x and v likewise, coefficients in {-1, 0, 1}: the source byte of (y, x) is src + y * cy + x * cx
            const bool turn = k & 1;
            int pc = k >= 2 ? n - 1 : 0, ps = k >= 2 ? -1 : 1;                 // p = pc + ps * (turn ? x : y)
            int qc = k == 1 || k == 2 ? n - 1 : 0, qs = k == 1 || k == 2 ? -1 : 1;      // q = qc + qs * (turn ? y : x)
            if (flips & 2) pc = n - 1 - pc, ps = -ps;                          // u = n-1-p
            if (flips & 1) qc = n - 1 - qc, qs = -qs;                          // v = n-1-q
            const long long row = (long long)w * ch;
            const long long cy = turn ? (long long)qs * ch : ps * row, cx = turn ? ps * row : (long long)qs * ch;
            const unsigned char *src = a.pool + off + (((long long)i * s + pc) * w + ((long long)j * s + qc)) * ch + c;      // (y, x) = (0, 0)
            unsigned char byte[16];
#pragma unroll
            for (int q = 0; q < 16; ++q) {
                // lanes along the source row: along x, or along y when the tile is turned
                const int along = lx, across = ly + 2 * q;
                const int y = Y0 + (turn ? along : across), x = X0 + (turn ? across : along);
                byte[q] = y < n && x < n ? src[y * cy + x * cx] : 0;
            }
#pragma unroll
            for (int q = 0; q < 16; ++q) {
                const int along = lx, across = ly + 2 * q;
                tile[(turn ? along : across) * kCropStride + (turn ? across : along)] = s_tab[byte[q]];
            }
        }
        __builtin_amdgcn_wave_barrier();      // (the tile is this wave's own, and LDS serves a wave in order)
        float *plane = (hr ? a.lb : a.im) + (long long)b * n * n;
        const bool vec = hr ? a.vec_hr : a.vec_lr;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int yl = wy + 8 * q, y = Y0 + yl, x = X0 + wx;
            if (y < n && x < n) {
                float4 o = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
                if (ok) {
                    const float *tp = tile + yl * kCropStride + wx;
                    o = make_float4(tp[0], tp[1], tp[2], tp[3]);      // (columns past n hold zeros that are never stored)
                }
                const long long at = (long long)y * n + x;
                if (vec && x + 3 < n) {
                    *reinterpret_cast<float4 *>(plane + at) = o;
                    asm volatile("" ::: "memory");      // (keeps the compiler from sharing part of this store with the path below)
                } else {
                    float *ps = plane + at;
                    ps[0] = o.x;
                    if (x + 1 < n) ps[1] = o.y;
                    if (x + 2 < n) ps[2] = o.z;
                    if (x + 3 < n) ps[3] = o.w;
                }
            }
        }
        __builtin_amdgcn_wave_barrier();      // (the next tile's writes stay behind these reads)
    }
}

constexpr int kPackNT = 256;

// rintf rounds half to even in the default rounding mode, as torch.round and np.round do
__device__ __forceinline__ unsigned char pack_byte(float v) { return (unsigned char)rintf(fminf(fmaxf(v * 255.0f, 0.0f), 255.0f)); }

// one lane per pixel: three coalesced plane loads, three byte stores (a wave writes 192 consecutive bytes; any address)
__global__ void __launch_bounds__(kPackNT) ft_val_pack_kernel(const float *pred, int n, unsigned char *out) {
    const int i = (int)(blockIdx.x * (unsigned)kPackNT + threadIdx.x);
    if (i >= n) return;
    const unsigned char r = pack_byte(pred[i]), g = pack_byte(pred[(size_t)n + i]), b = pack_byte(pred[2 * (size_t)n + i]);
    unsigned char *o = out + 3 * (size_t)i;
    o[0] = r;
    o[1] = g;
    o[2] = b;
}

}  // namespace mulut

/* sr/3_finetune_lut.py:50-54 */
extern "C" int mulut_ft_val_pack(int device, const float *pred, int H, int W, unsigned char *out_hwc, void *stream) {
    using namespace mulut;
    if (!pred || !out_hwc) return MULUT_EINVAL;
    if (H <= 0 || W <= 0) return MULUT_EINVAL;
    const long long n = (long long)H * W;
    if (n > ((1LL << 31) - 1) / 3) return MULUT_EUNSUPPORTED;      // H * W * 3 >= 2^31 (n * 3 itself may leave 64 bits)
    if (hipSetDevice(device) != hipSuccess) return MULUT_ENODEVICE;
    hipLaunchKernelGGL(ft_val_pack_kernel, dim3((unsigned)((n + kPackNT - 1) / kPackNT)), dim3(kPackNT), 0, (hipStream_t)stream, pred, (int)n,
                       out_hwc);
    return hipGetLastError() == hipSuccess ? MULUT_OK : MULUT_EHIP;
}

extern "C" int mulut_ft_crop_batch(int device, const unsigned char *pool, long long pool_bytes, const mulut_ft_pair *pairs, int n_pairs,
                                   const int *draws, int B, int sz, int scale, float *im, float *lb, int *bad, void *stream) {
    using namespace mulut;
    if (!pool || !pairs || !draws || !im || !lb) return MULUT_EINVAL;
    if (B <= 0 || sz <= 0 || n_pairs <= 0 || pool_bytes <= 0) return MULUT_EINVAL;
    if (scale < 1 || scale > 4) return MULUT_EUNSUPPORTED;
    const long long n_hr = (long long)sz * scale;
    if (n_hr >= (1LL << 31) || n_hr * n_hr >= (1LL << 31) || (long long)B * (n_hr * n_hr) >= (1LL << 31)) return MULUT_EUNSUPPORTED;
    CropArgs a;
    a.pool = pool;
    a.pool_bytes = pool_bytes;
    a.pairs = pairs;
    a.draws = draws;
    a.im = im;
    a.lb = lb;
    a.bad = bad;
    a.n_pairs = n_pairs;
    a.B = B;
    a.sz = sz;
    a.scale = scale;
    a.t_lr = (sz + kCropTile - 1) / kCropTile;
    a.t_hr = ((int)n_hr + kCropTile - 1) / kCropTile;
    // a plane starts at base + b * n * n floats: every row of it is 16-byte aligned when the base is and n % 4 == 0
    a.vec_lr = sz % 4 == 0 && (uintptr_t)im % 16 == 0;
    a.vec_hr = n_hr % 4 == 0 && (uintptr_t)lb % 16 == 0;
    a.chunks = (a.t_lr * a.t_lr + a.t_hr * a.t_hr + kCropChunk - 1) / kCropChunk;
    const long long nb = (long long)B * a.chunks;      // (a chunk stores at least one float of lb: fewer than 2^31)
    if (hipSetDevice(device) != hipSuccess) return MULUT_ENODEVICE;
    hipLaunchKernelGGL(ft_crop_kernel, dim3((unsigned)nb), dim3(kCropNT), 0, (hipStream_t)stream, a);
    return hipGetLastError() == hipSuccess ? MULUT_OK : MULUT_EHIP;
}
