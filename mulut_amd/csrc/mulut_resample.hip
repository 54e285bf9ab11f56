// mulut_resample.hip -- LR images made on the device: Pillow's bicubic resampling of 8-bit images, byte for byte.
//
// Reference: sr/Test_dataset.py:24-25, img.resize((w // s, h // s), resample=Image.BICUBIC) for s = 2, 3, 4 -- the step that makes
// LR_bicubic/X{s}/ (LR/X{s}/) from HR/.  Pillow resamples 8-bit images in fixed point (ImagingResampleHorizontal_8bpc / Vertical_8bpc):
// normalised double coefficients per output position, rounded to integers at 22 fractional bits; an int accumulator that starts at
// 1 << 21; clip(acc >> 22) to 0..255; a horizontal pass into a uint8 image, then a vertical pass over THAT.  An axis whose size does
// not change is skipped.  sum|k| * 255 + 2^21 stays below 2^31 (1.33e9 at most on 2040 -> 510, 1080 -> 4320 and their like), so int32
// accumulators are exact.
//
//   rs_coeffs          the host's precompute_coeffs + normalize_coeffs_8bpc for one axis, in double, in Pillow's operation order and
//                      with contraction off (hipcc fuses a * b + c by default; Pillow's build does not).
//   resample_kernel    a workgroup of 4 waves walks 1 to 4 output tiles of 16 (growing images: 64) rows x 256 bytes down one tile column.  Per tile:
//                      phase 1 writes the horizontal pass of the input rows the tile's vertical taps span into LDS as bytes (a thread
//                      owns one dword column: its four bytes' xmin and the 4 x KH coefficients lie in LDS, staged once per
//                      workgroup); phase 2 reads a row of 64 dwords per wave and tap (conflict-free), sums the vertical taps of four
//                      bytes and stores a dword.  Nothing intermediate goes to memory.  With both images packed (HWC) and C <= 4 the
//                      256 bytes of a row are whole pixels (252 at C = 3), lanes along the bytes; any other layout or C runs one
//                      channel per workgroup with the pixel and channel strides of its layout.
// The kernel computes no coefficient: rows, xmin and n come from the device tables of a plan (the horizontal rows transposed, tap-major,
// so the staging reads are coalesced).  The plan's host half also bounds the LDS a tile needs; what does not fit 64 KiB is refused.
#include <hip/hip_runtime.h>

#include <cmath>
#include <new>
#include <vector>

#include "../../include/mulut.h"

struct mulut_resample_plan {
    int device;
    int in_h, in_w, out_h, out_w;
    int kh, kv;            // taps per row of the two tables (0: the axis is skipped)
    int tile_h;            // output rows of a tile: 16, or 64 when the image grows downwards (few input rows under many output rows)
    int span_rows;         // the most input rows a tile's vertical taps span
    int32_t *tab;          // device: khT [kh][out_w] (a row's n is its zero tail), xmin [out_w], kv [out_h][kv], ymin [out_h], nv [out_h]
};

namespace mulut {

constexpr int kRsRowBytes = 256, kRsTileH = 16, kRsTileHUp = 64, kRsWaves = 4, kRsNT = 64 * kRsWaves, kRsLdsMax = 64 * 1024;
constexpr int kRsWalkMax = 4, kRsTilesPerWalk = 2048;      // a workgroup walks up to 4 tiles once a call has 2048 tiles per tile walked
constexpr int kRsPrecision = 22;

// bytes of a tile row in use when a pixel is cc bytes: whole pixels and whole dwords
__host__ __device__ constexpr int rs_tile_bytes(int cc) { return kRsRowBytes / (4 * cc) * (4 * cc); }

static double rs_bicubic(double x) {
#pragma clang fp contract(off)
    const double a = -0.5;
    if (x < 0.0) x = -x;
    if (x < 1.0) return ((a + 2.0) * x - (a + 3.0)) * x * x + 1;
    if (x < 2.0) return (((x - 5) * x + 8) * x - 4) * a;
    return 0.0;
}

// taps per row for in -> out, or 0 when they do not fit an int comfortably
static int rs_ksize(int in, int out) {
#pragma clang fp contract(off)
    double fs = (double)in / out;
    if (fs < 1.0) fs = 1.0;
    const double support = 2.0 * fs;
    if (support > (double)(1 << 20)) return 0;
    return (int)ceil(support) * 2 + 1;
}

// kk [out][ksize] (zero beyond n), xmin [out], n [out]
static void rs_coeffs(int in, int out, int ksize, int32_t *kk, int32_t *xmin_out, int32_t *n_out) {
#pragma clang fp contract(off)
    const double scale = (double)in / out;
    double fs = scale;
    if (fs < 1.0) fs = 1.0;
    const double support = 2.0 * fs, ss = 1.0 / fs;
    std::vector<double> k((size_t)ksize);
    for (int xx = 0; xx < out; ++xx) {
        const double center = (xx + 0.5) * scale;
        double ww = 0.0;
        int xmin = (int)(center - support + 0.5);
        if (xmin < 0) xmin = 0;
        int xmax = (int)(center + support + 0.5);
        if (xmax > in) xmax = in;
        xmax -= xmin;
        for (int x = 0; x < xmax; ++x) {
            const double w = rs_bicubic((x + xmin - center + 0.5) * ss);
            k[x] = w;
            ww += w;
        }
        int32_t *row = kk + (size_t)xx * ksize;
        for (int x = 0; x < xmax; ++x) {
            if (ww != 0.0) k[x] /= ww;
            row[x] = k[x] < 0 ? (int)(-0.5 + k[x] * (1 << kRsPrecision)) : (int)(0.5 + k[x] * (1 << kRsPrecision));
        }
        for (int x = xmax; x < ksize; ++x) row[x] = 0;
        xmin_out[xx] = xmin;
        n_out[xx] = xmax;
    }
}

struct ResampleArgs {
    const unsigned char *in;
    unsigned char *out;
    const int *kh, *xmin, *kv, *ymin, *nv;
    long long in_img, in_chan, out_img, out_chan;      // bytes from image n to n + 1 and from channel c to c + 1
    int in_row, in_px, out_row, out_px;                // bytes from row y to y + 1 and from pixel x to x + 1
    int in_h, in_w, out_h, out_w, KH, KV;              // KH / KV 0: that pass is skipped
    int groups, tiles_x, tiles_y, walkers_y, span_rows;
    int tile_h, walk;                                  // output rows of a tile; tiles a workgroup walks down its column
};

// The empty asm keeps each clipped value a value of its own.  Without it the compiler fuses two of these into one
// v_ashr_pk_u8_i32 and ORs the dword's other two bytes onto the result as if its upper half were zero; on the MI355X it is not,
// and bytes 2 and 3 of every dword came out OR-ed with stale bits (tests/test_gpu_resample.py caught it).
__device__ __forceinline__ int rs_clip8(int acc) {
    int v = acc >> kRsPrecision;
    v = v < 0 ? 0 : v > 255 ? 255 : v;
    asm volatile("" : "+v"(v));
    return v;
}

// CC: channels of a pixel taken together (both images packed, lanes along the bytes of a row); 1: one channel, any strides
template <int CC>
__global__ void __launch_bounds__(kRsNT) resample_kernel(ResampleArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char rs_lds[];
    constexpr int TB = rs_tile_bytes(CC), TP = TB / CC;
    int4 *s_kh = reinterpret_cast<int4 *>(rs_lds);                                              // [KH][64]: tap t of this thread's 4 bytes
    unsigned *s_rows = reinterpret_cast<unsigned *>(rs_lds + (size_t)a.KH * kRsRowBytes * 4);   // [span_rows][64]
    unsigned b = blockIdx.x;
    const int tx = (int)(b % (unsigned)a.tiles_x);
    b /= (unsigned)a.tiles_x;
    const int wy = (int)(b % (unsigned)a.walkers_y);
    b /= (unsigned)a.walkers_y;
    const int g = (int)(b % (unsigned)a.groups), n = (int)(b / (unsigned)a.groups);
    const int d = (int)threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6);
    const int X0 = tx * TP;                                              // the tile column's first output pixel
    const int valid = (a.out_w - X0) * CC < TB ? (a.out_w - X0) * CC : TB;      // bytes of the tile row inside the image
    const unsigned char *in = a.in + n * a.in_img + (long long)g * CC * a.in_chan;
    unsigned char *out = a.out + n * a.out_img + (long long)g * CC * a.out_chan;
    const bool skip_h = a.KH == 0, skip_v = a.KV == 0;
    // ---- this thread's four byte columns: first tap, channel, and (staged) the coefficients; a column outside the image reads
    // pixel 0 with zero coefficients and is never stored
    int xm[4], cc[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int j = 4 * d + q, xx = X0 + j / CC;
        const bool ok = j < valid;
        cc[q] = CC == 1 ? 0 : j % CC;
        xm[q] = !ok ? 0 : skip_h ? xx : a.xmin[xx];
    }
    for (int idx = (int)threadIdx.x; idx < a.KH * kRsRowBytes; idx += kRsNT) {
        const int t = idx >> 8, j = idx & (kRsRowBytes - 1);
        reinterpret_cast<int *>(rs_lds)[idx] = j < valid ? a.kh[(long long)t * a.out_w + X0 + j / CC] : 0;
    }
    __syncthreads();
    const int ty_end = (wy + 1) * a.walk < a.tiles_y ? (wy + 1) * a.walk : a.tiles_y;
    for (int ty = wy * a.walk; ty < ty_end; ++ty) {
        const int oy0 = ty * a.tile_h, oyl = (oy0 + a.tile_h < a.out_h ? oy0 + a.tile_h : a.out_h) - 1;
        // xmin and xmin + n do not decrease along an axis: the tile's taps span [ya, yb)
        const int ya = skip_v ? oy0 : a.ymin[oy0], yb = skip_v ? oyl + 1 : a.ymin[oyl] + a.nv[oyl];
        const int span = yb - ya < a.span_rows ? yb - ya : a.span_rows;      // (the plan's host half sized span_rows as this maximum)
        // ---- phase 1: the horizontal pass of rows ya .. yb, rounded and clipped to bytes, into LDS
        // (a wave takes two rows per trip and the taps four at a time: 32 byte loads in flight, none waited for on its own)
        for (int r = wave; r < span; r += 2 * kRsWaves) {
            const int r1 = r + kRsWaves < span ? r + kRsWaves : r;      // (the last trip may hold one row: done twice)
            const unsigned char *row0 = in + (long long)(ya + r) * a.in_row, *row1 = in + (long long)(ya + r1) * a.in_row;
            unsigned w0 = 0, w1 = 0;
            if (skip_h) {
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const int off = xm[q] * a.in_px + cc[q];
                    w0 |= (unsigned)row0[off] << (8 * q);
                    w1 |= (unsigned)row1[off] << (8 * q);
                }
            } else {
                int acc0[4], acc1[4];
#pragma unroll
                for (int q = 0; q < 4; ++q) acc0[q] = acc1[q] = 1 << (kRsPrecision - 1);
#pragma unroll 4
                for (int t = 0; t < a.KH; ++t) {
                    const int4 k = s_kh[t * 64 + d];      // zero beyond a column's own n: the clamped load below then adds nothing
                    const int kq[4] = {k.x, k.y, k.z, k.w};
#pragma unroll
                    for (int q = 0; q < 4; ++q) {
                        const int x = xm[q] + t < a.in_w ? xm[q] + t : a.in_w - 1;
                        const int off = x * a.in_px + cc[q];
                        acc0[q] += (int)row0[off] * kq[q];
                        acc1[q] += (int)row1[off] * kq[q];
                    }
                }
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    w0 |= (unsigned)rs_clip8(acc0[q]) << (8 * q);
                    w1 |= (unsigned)rs_clip8(acc1[q]) << (8 * q);
                }
            }
            s_rows[r * 64 + d] = w0;
            s_rows[r1 * 64 + d] = w1;
        }
        __syncthreads();
        // ---- phase 2: the vertical pass over those bytes; a wave takes a row of the tile at a time
        for (int ly = wave; oy0 + ly <= oyl; ly += kRsWaves) {
            const int oy = oy0 + ly;
            unsigned w;
            if (skip_v) {
                w = s_rows[(oy - ya) * 64 + d];
            } else {
                const int y0 = a.ymin[oy] - ya, nv = a.nv[oy];
                const int *kp = a.kv + (long long)oy * a.KV;
                int acc[4] = {1 << (kRsPrecision - 1), 1 << (kRsPrecision - 1), 1 << (kRsPrecision - 1), 1 << (kRsPrecision - 1)};
                for (int t = 0; t < nv && y0 + t < span; ++t) {
                    const unsigned s = s_rows[(y0 + t) * 64 + d];
                    const int k = kp[t];
#pragma unroll
                    for (int q = 0; q < 4; ++q) acc[q] += (int)((s >> (8 * q)) & 255u) * k;
                }
                w = 0;
#pragma unroll
                for (int q = 0; q < 4; ++q) w |= (unsigned)rs_clip8(acc[q]) << (8 * q);
            }
            const int j = 4 * d;
            if (j < valid) {
                const int px = CC == 1 ? a.out_px : 1;      // bytes between this thread's columns
                unsigned char *p = out + (long long)oy * a.out_row + (long long)(X0 * CC + j) * px;
                if (px == 1 && j + 3 < valid && (reinterpret_cast<uintptr_t>(p) & 3) == 0) {
                    *reinterpret_cast<unsigned *>(p) = w;
                } else {
#pragma unroll
                    for (int q = 0; q < 4; ++q)
                        if (j + q < valid) p[q * px] = (unsigned char)(w >> (8 * q));
                }
            }
        }
        __syncthreads();      // the next tile's phase 1 stays behind these reads
    }
}

// the most input rows the vertical taps of one tile of tile_h output rows span
static int rs_span_rows(int out_h, int tile_h, const int32_t *ymin, const int32_t *nv) {
    int span = 0;
    for (int oy0 = 0; oy0 < out_h; oy0 += tile_h) {
        int lo = ymin[oy0], hi = 0;
        for (int oy = oy0; oy < out_h && oy < oy0 + tile_h; ++oy) {
            lo = ymin[oy] < lo ? ymin[oy] : lo;
            hi = ymin[oy] + nv[oy] > hi ? ymin[oy] + nv[oy] : hi;
        }
        span = hi - lo > span ? hi - lo : span;
    }
    return span;
}

}  // namespace mulut

/* sr/Test_dataset.py:24-25 */
extern "C" int mulut_resample_coeffs(int in, int out, int32_t *kk, int32_t *xmin, int32_t *n, long long cap) {
    using namespace mulut;
    if (!kk || !xmin || !n || in < 1 || out < 1) return MULUT_EINVAL;
    const int ksize = rs_ksize(in, out);
    if (ksize == 0) return MULUT_EUNSUPPORTED;
    if ((long long)out * ksize > cap) return MULUT_EWORKSPACE;
    rs_coeffs(in, out, ksize, kk, xmin, n);
    return ksize;
}

/* sr/Test_dataset.py:24-25 */
extern "C" int mulut_resample_plan_create(int device, int in_h, int in_w, int out_h, int out_w, mulut_resample_plan **out_plan) {
    using namespace mulut;
    if (!out_plan) return MULUT_EINVAL;
    *out_plan = nullptr;
    if (in_h < 1 || in_w < 1 || out_h < 1 || out_w < 1) return MULUT_EINVAL;
    if ((long long)in_h * in_w >= (1LL << 31) || (long long)out_h * out_w >= (1LL << 31)) return MULUT_EUNSUPPORTED;
    const int kh = in_w == out_w ? 0 : rs_ksize(in_w, out_w), kv = in_h == out_h ? 0 : rs_ksize(in_h, out_h);
    if ((in_w != out_w && kh == 0) || (in_h != out_h && kv == 0)) return MULUT_EUNSUPPORTED;
    const long long ints = (long long)out_w * (kh + 1) + (long long)out_h * (kv + 2);
    if (ints >= (1LL << 28)) return MULUT_EUNSUPPORTED;
    std::vector<int32_t> host;
    try {
        host.resize((size_t)ints);
    } catch (const std::bad_alloc &) {
        return MULUT_EUNSUPPORTED;
    }
    // horizontal: computed row-major, uploaded tap-major
    int32_t *khT = host.data(), *xmin = khT + (size_t)kh * out_w;
    int32_t *kvp = xmin + out_w, *ymin = kvp + (size_t)kv * out_h, *nv = ymin + out_h;
    if (kh) {
        std::vector<int32_t> rows((size_t)out_w * kh), nh((size_t)out_w);
        rs_coeffs(in_w, out_w, kh, rows.data(), xmin, nh.data());
        for (int xx = 0; xx < out_w; ++xx)
            for (int t = 0; t < kh; ++t) khT[(size_t)t * out_w + xx] = rows[(size_t)xx * kh + t];
    } else {
        for (int xx = 0; xx < out_w; ++xx) xmin[xx] = xx;
    }
    const int tile_h = out_h > in_h ? kRsTileHUp : kRsTileH;
    int span = tile_h;
    if (kv) {
        rs_coeffs(in_h, out_h, kv, kvp, ymin, nv);
        span = rs_span_rows(out_h, tile_h, ymin, nv);
    } else {
        for (int oy = 0; oy < out_h; ++oy) ymin[oy] = oy, nv[oy] = 1;
    }
    // the LDS of a workgroup: its coefficient rows and the rows of a tile
    if ((long long)kh * kRsRowBytes * 4 + (long long)span * kRsRowBytes > kRsLdsMax) return MULUT_EUNSUPPORTED;
    if (hipSetDevice(device) != hipSuccess) return MULUT_ENODEVICE;
    mulut_resample_plan *p = new (std::nothrow) mulut_resample_plan{device, in_h, in_w, out_h, out_w, kh, kv, tile_h, span, nullptr};
    if (!p) return MULUT_EHIP;
    if (hipMalloc(reinterpret_cast<void **>(&p->tab), (size_t)ints * sizeof(int32_t)) != hipSuccess) {
        delete p;
        return MULUT_EHIP;
    }
    if (hipMemcpy(p->tab, host.data(), (size_t)ints * sizeof(int32_t), hipMemcpyHostToDevice) != hipSuccess) {
        (void)hipFree(p->tab);
        delete p;
        return MULUT_EHIP;
    }
    *out_plan = p;
    return MULUT_OK;
}

extern "C" int mulut_resample_plan_destroy(mulut_resample_plan *plan) {
    if (!plan) return MULUT_EINVAL;
    int rc = MULUT_OK;
    if (hipSetDevice(plan->device) != hipSuccess) rc = MULUT_ENODEVICE;
    else if (hipFree(plan->tab) != hipSuccess) rc = MULUT_EHIP;
    delete plan;
    return rc;
}

/* sr/Test_dataset.py:24-25 */
extern "C" int mulut_resample_run(const mulut_resample_plan *plan, const uint8_t *in, int in_layout, uint8_t *out, int out_layout,
                                  int N, int C, void *stream) {
    using namespace mulut;
    if (!plan || !in || !out || N < 1 || C < 1) return MULUT_EINVAL;
    if ((in_layout != MULUT_LAYOUT_CHW && in_layout != MULUT_LAYOUT_HWC) || (out_layout != MULUT_LAYOUT_CHW && out_layout != MULUT_LAYOUT_HWC))
        return MULUT_EINVAL;
    const mulut_resample_plan &p = *plan;
    const long long in_plane = (long long)p.in_h * p.in_w, out_plane = (long long)p.out_h * p.out_w;
    // the kernel's offsets inside one image are 32-bit: a packed image counts all its channels, a planar one a plane
    if ((in_layout == MULUT_LAYOUT_HWC && in_plane * C >= (1LL << 31)) || (out_layout == MULUT_LAYOUT_HWC && out_plane * C >= (1LL << 31)))
        return MULUT_EUNSUPPORTED;
    const bool packed = in_layout == MULUT_LAYOUT_HWC && out_layout == MULUT_LAYOUT_HWC && C <= 4;
    const int cc = packed ? C : 1;
    ResampleArgs a;
    a.in = in;
    a.out = out;
    a.kh = p.tab;
    a.xmin = a.kh + (size_t)p.kh * p.out_w;
    a.kv = a.xmin + p.out_w;
    a.ymin = a.kv + (size_t)p.kv * p.out_h;
    a.nv = a.ymin + p.out_h;
    a.in_img = in_plane * C;
    a.out_img = out_plane * C;
    a.in_chan = in_layout == MULUT_LAYOUT_HWC ? 1 : in_plane;
    a.out_chan = out_layout == MULUT_LAYOUT_HWC ? 1 : out_plane;
    a.in_px = in_layout == MULUT_LAYOUT_HWC ? C : 1;
    a.out_px = out_layout == MULUT_LAYOUT_HWC ? C : 1;
    a.in_row = p.in_w * a.in_px;
    a.out_row = p.out_w * a.out_px;
    a.in_h = p.in_h;
    a.in_w = p.in_w;
    a.out_h = p.out_h;
    a.out_w = p.out_w;
    a.KH = p.kh;
    a.KV = p.kv;
    a.groups = packed ? 1 : C;
    const int tp = rs_tile_bytes(cc) / cc;
    a.tiles_x = (p.out_w + tp - 1) / tp;
    a.tile_h = p.tile_h;
    a.tiles_y = (p.out_h + p.tile_h - 1) / p.tile_h;
    const long long tiles = (long long)N * a.groups * a.tiles_y * a.tiles_x;
    a.walk = tiles / kRsTilesPerWalk >= kRsWalkMax ? kRsWalkMax : tiles / kRsTilesPerWalk >= 1 ? (int)(tiles / kRsTilesPerWalk) : 1;
    a.walkers_y = (a.tiles_y + a.walk - 1) / a.walk;
    a.span_rows = p.span_rows;
    const long long per_image = (long long)a.groups * a.walkers_y * a.tiles_x;
    if (per_image >= (1LL << 31) || per_image * N >= (1LL << 31)) return MULUT_EUNSUPPORTED;
    const size_t lds = (size_t)p.kh * kRsRowBytes * 4 + (size_t)p.span_rows * kRsRowBytes;
    if (hipSetDevice(p.device) != hipSuccess) return MULUT_ENODEVICE;
    const dim3 grid((unsigned)(per_image * N)), block(kRsNT);
    hipStream_t st = (hipStream_t)stream;
    switch (cc) {
        case 1: hipLaunchKernelGGL(resample_kernel<1>, grid, block, lds, st, a); break;
        case 2: hipLaunchKernelGGL(resample_kernel<2>, grid, block, lds, st, a); break;
        case 3: hipLaunchKernelGGL(resample_kernel<3>, grid, block, lds, st, a); break;
        default: hipLaunchKernelGGL(resample_kernel<4>, grid, block, lds, st, a); break;
    }
    return hipGetLastError() == hipSuccess ? MULUT_OK : MULUT_EHIP;
}
