// mulut_net.hip -- the fused forward of the SR network: one site body (four tap values in, u*u values of tanh(conv6(...)) out)
// on the f32-input MFMA, under three launch forms.
//
// Reference: common/network.py:62-105 (MuLUTUnit, dense=True) is the site body; sr/2_transfer_to_lut.py:12-41,86-109 the grid form
// (mulut_net_table); sr/1_train_model.py:33-35 one rotation pass (mulut_net_pass); :26-45 in the 'valid' phase, with :101, one
// stage (mulut_net_stage).  In that phase every stage maps bytes to bytes, so no float image exists anywhere: the taps are read
// as bytes and divided by 255 in the kernel, every pass value is rounded to an integer as it leaves the site body, and the
// stage's average / bias / round / clip runs on the integer sum.
//
// The site body.  A wave owns 32 sites (the lane; both lane halves hold the same site and different features), a workgroup of four
// waves 128.  Activations stay in registers from the taps to tanh: mulut_net.h explains why an MFMA result register is the next
// layer's B operand as it stands.  Only the weights move: the unit's packed stream (181 KiB + biases at nf = 64) is read from
// memory -- from L2 in practice, every workgroup reads the same bytes -- in 16 KiB chunks, each staged ONCE per workgroup into one of
// two LDS buffers (the next chunk is in flight, in registers, under the 64 MFMAs of the current one) and read from there by the four
// waves, four steps per 16-byte LDS load.  One barrier per chunk.  No scratch, no atomics, nothing intermediate in global memory.
#include <hip/hip_runtime.h>

#include <cstring>
#include <new>
#include <type_traits>
#include <vector>

#include "../../include/mulut.h"
#include "mulut_net.h"

struct mulut_net_unit {
    int device, nf, u, mt;
    long long floats;
    float *w;      // device: the packed stream
};

namespace mulut {

void net_pack(int nf, int u, const float *const w[6], const float *const b[6], float *out) {
    const int MT = net_tiles(nf);
    memset(out, 0, (size_t)net_stream_floats(MT) * sizeof(float));
    for (int L = 1; L <= 6; ++L) {
        const int tiles = L == 6 ? 1 : MT, in_f = L == 1 ? 4 : (L - 1) * nf;
        const float *W = w[L - 1], *B = b[L - 1];
        for (int mt = 0; mt < tiles; ++mt) {
            const int base = net_step_base(MT, L, mt);
            for (int lane = 0; lane < 64; ++lane) {
                const int i = lane & 31, h = lane >> 5;
                int out_row;      // the logical output this lane's A row feeds, or -1: padding
                if (L < 6) {
                    out_row = mt * 32 + i < nf ? mt * 32 + i : -1;
                } else {
                    const int hh = (i >> 2) & 1, r = (i & 3) + 4 * (i >> 3);      // i = net_row(r, hh)
                    out_row = r < 8 && 8 * hh + r < u * u ? 8 * hh + r : -1;
                }
                if (out_row < 0) continue;
                if (h == 0) out[net_step_float(base, lane)] = B[out_row];
                if (L == 1) {
                    out[net_step_float(base + 1, lane)] = W[out_row * 4 + h];
                    out[net_step_float(base + 2, lane)] = W[out_row * 4 + 2 + h];
                    continue;
                }
                for (int s = 0; s < L - 1; ++s)
                    for (int t = 0; t < MT; ++t)
                        for (int reg = 0; reg < 16; ++reg) {
                            const int f = t * 32 + net_row(reg, h);
                            if (f < nf) out[net_step_float(base + 1 + (s * MT + t) * 16 + reg, lane)] = W[(size_t)out_row * in_f + s * nf + f];
                        }
            }
        }
    }
}

typedef float f32x16 __attribute__((ext_vector_type(16)));

template <int B, int E, class F>
__device__ __forceinline__ void net_static_for(F &&f) {
    if constexpr (B < E) {
        f(std::integral_constant<int, B>{});
        net_static_for<B + 1, E>(f);
    }
}

// a workgroup's walk down weight streams: chunk 0 of `cur` is in LDS buffer `par` when a site body begins, and chunk 0 of `next`
// is in buffer `par` (updated) when it ends
struct NetStream {
    const float4 *cur, *next;
    float4 *lds;
    float4 pf[4], wq;
    int par, tid, lane;
};

__device__ __forceinline__ void net_fetch(NetStream &s, const float4 *chunk) {
#pragma unroll
    for (int j = 0; j < 4; ++j) s.pf[j] = chunk[j * kNetNT + s.tid];
}

__device__ __forceinline__ void net_put(NetStream &s, int c) {
    float4 *buf = s.lds + ((c & 1) ^ s.par) * kNetChunkVec4;
#pragma unroll
    for (int j = 0; j < 4; ++j) buf[j * kNetNT + s.tid] = s.pf[j];
}

// before the first body of a workgroup
__device__ __forceinline__ void net_stream_begin(NetStream &s, const float4 *first, float4 *lds) {
    s.lds = lds;
    s.par = 0;
    s.tid = (int)threadIdx.x;
    s.lane = s.tid & 63;
    net_fetch(s, first);
    net_put(s, 0);
    __syncthreads();
}

template <int MT, int G>
__device__ __forceinline__ void net_step(NetStream &s, float b, f32x16 &acc) {
    constexpr int NC = net_chunks(MT), c = G / kNetChunkSteps;
    if constexpr (G % kNetChunkSteps == 0) {
        if constexpr (c > 0) {
            net_put(s, c);      // buffer c & 1 was last read in chunk c - 2: every wave has passed the barrier of chunk c - 1 since
            __syncthreads();
        }
        net_fetch(s, c + 1 < NC ? s.cur + (c + 1) * kNetChunkVec4 : s.next);
    }
    if constexpr (G % 4 == 0) s.wq = s.lds[((c & 1) ^ s.par) * kNetChunkVec4 + ((G % kNetChunkSteps) / 4) * 64 + s.lane];
    const float a = (G & 3) == 0 ? s.wq.x : (G & 3) == 1 ? s.wq.y : (G & 3) == 2 ? s.wq.z : s.wq.w;
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, acc, 0, 0, 0);
}

// t0, t1: this lane's tap values of steps 1 and 2 -- (a, c) in lane half 0, (b, d) in half 1.  y[r]: output 8 * h + r (valid below u*u).
template <int MT, int U>
__device__ __forceinline__ void net_site_body(NetStream &s, float t0, float t1, float (&y)[8]) {
    const float one = s.lane < 32 ? 1.0f : 0.0f;
    f32x16 x[5][MT];
    net_static_for<1, 6>([&](auto Lc) __attribute__((always_inline)) {
        constexpr int L = decltype(Lc)::value;
        net_static_for<0, MT>([&](auto mc) __attribute__((always_inline)) {
            constexpr int mt = decltype(mc)::value, base = net_step_base(MT, L, mt);
            f32x16 acc;
#pragma unroll
            for (int q = 0; q < 16; ++q) acc[q] = 0.0f;
            net_step<MT, base>(s, one, acc);
            if constexpr (L == 1) {
                net_step<MT, base + 1>(s, t0, acc);
                net_step<MT, base + 2>(s, t1, acc);
            } else {
                net_static_for<0, (L - 1) * MT * 16>([&](auto kc) __attribute__((always_inline)) {
                    constexpr int k = decltype(kc)::value;
                    net_step<MT, base + 1 + k>(s, x[k / (MT * 16)][(k / 16) % MT][k % 16], acc);
                });
            }
#pragma unroll
            for (int q = 0; q < 16; ++q) x[L - 1][mt][q] = fmaxf(acc[q], 0.0f);
        });
    });
    constexpr int base6 = net_step_base(MT, 6, 0);
    f32x16 acc;
#pragma unroll
    for (int q = 0; q < 16; ++q) acc[q] = 0.0f;
    net_step<MT, base6>(s, one, acc);
    net_static_for<0, 5 * MT * 16>([&](auto kc) __attribute__((always_inline)) {
        constexpr int k = decltype(kc)::value;
        net_step<MT, base6 + 1 + k>(s, x[k / (MT * 16)][(k / 16) % MT][k % 16], acc);
    });
    constexpr int NC = net_chunks(MT);
    net_put(s, NC);
    __syncthreads();
    s.par ^= NC & 1;
    constexpr int RN = U * U < 8 ? U * U : 8;
#pragma unroll
    for (int r = 0; r < 8; ++r) y[r] = r < RN ? tanhf(acc[r]) : 0.0f;
}

// round(127 * y) of sr/1_train_model.py:34-35 and round(clamp(y, -1, 1) * 127) of sr/2_transfer_to_lut.py:108-109: tanh stays inside
// [-1, 1], the clamp only makes that explicit; torch.round is round-half-even
__device__ __forceinline__ int net_q127(float y) { return (int)__builtin_rintf(fminf(fmaxf(y, -1.0f), 1.0f) * 127.0f); }

// ---- rotations by index arithmetic.  rot90^r(x)[i][j] = x[net_unrot(r, i, j, H, W)] for an H x W image x (torch.rot90 over dims 2, 3)
__device__ __forceinline__ void net_unrot(int r, int i, int j, int H, int W, int &y, int &x) {
    y = r == 0 ? i : r == 1 ? j : r == 2 ? H - 1 - i : H - 1 - j;
    x = r == 0 ? j : r == 1 ? W - 1 - i : r == 2 ? W - 1 - j : i;
}
__device__ __forceinline__ void net_rot(int r, int y, int x, int H, int W, int &i, int &j) {
    i = r == 0 ? y : r == 1 ? W - 1 - x : r == 2 ? H - 1 - y : x;
    j = r == 0 ? x : r == 1 ? y : r == 2 ? W - 1 - x : H - 1 - y;
}

// The two tap values of this lane half for the site that pixel (y, x) of the un-rotated plane is in rotation r: taps k = h and 2 + h
// of the pattern (`taps`: di | dj << 4 in byte k), replicate-padded on the bottom and right of the ROTATED image (mode_pad_dict)
__device__ __forceinline__ void net_taps(const unsigned char *plane, int H, int W, int r, int y, int x, unsigned taps, int h, float &t0, float &t1) {
    int i, j;
    net_rot(r, y, x, H, W, i, j);
    const int Hr = (r & 1) ? W : H, Wr = (r & 1) ? H : W;
    float t[2];
#pragma unroll
    for (int q = 0; q < 2; ++q) {
        const unsigned tp = taps >> (8 * (2 * q + h));
        int ii = i + (int)(tp & 15u), jj = j + (int)((tp >> 4) & 15u), yy, xx;
        ii = ii < Hr ? ii : Hr - 1;
        jj = jj < Wr ? jj : Wr - 1;
        net_unrot(r, ii, jj, H, W, yy, xx);
        t[q] = (float)plane[yy * W + xx] / 255.0f;
    }
    t0 = t[0];
    t1 = t[1];
}

// ---- grid form: row i of the table is the site (a, b, c, d) = the base-L digits of i, a slowest
template <int MT, int U>
__global__ void __launch_bounds__(kNetNT) net_table_kernel(const float4 *w, signed char *rows, int L, int interval, int total) {
    __shared__ float4 lds[2 * kNetChunkVec4];
    NetStream s;
    s.cur = s.next = w;
    net_stream_begin(s, w, lds);
    const int h = s.lane >> 5;
    const int site = (int)blockIdx.x * kNetSites + (s.tid >> 6) * kNetTileSites + (s.lane & 31);
    int i = site < total ? site : total - 1;
    const int d = i % L;
    i /= L;
    const int c = i % L;
    i /= L;
    const int b = i % L, a = i / L;
    const int v0 = (h ? b : a) << interval, v1 = (h ? d : c) << interval;      // 0, q, ..., 256 - q, 255
    float y[8];
    net_site_body<MT, U>(s, (float)(v0 < 255 ? v0 : 255) / 255.0f, (float)(v1 < 255 ? v1 : 255) / 255.0f, y);
    if (site >= total) return;
    signed char *p = rows + (long long)site * (U * U);
    if (U == 4 && (reinterpret_cast<uintptr_t>(rows) & 7) == 0) {
        unsigned lo = 0, hi = 0;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            lo |= ((unsigned)net_q127(y[r]) & 255u) << (8 * r);
            hi |= ((unsigned)net_q127(y[4 + r]) & 255u) << (8 * r);
        }
        *reinterpret_cast<uint2 *>(p + 8 * h) = make_uint2(lo, hi);
    } else {
#pragma unroll
        for (int r = 0; r < 8; ++r)
            if (8 * h + r < U * U) p[8 * h + r] = (signed char)net_q127(y[r]);
    }
}

// ---- pass form: int8 [planes][H*U][W*U] = rot90^-r(round(127 * net(pad(rot90^r(x) / 255))))
template <int MT, int U>
__global__ void __launch_bounds__(kNetNT) net_pass_kernel(const float4 *w, const unsigned char *in, signed char *out, int H, int W, int r,
                                                          unsigned taps, int total) {
    __shared__ float4 lds[2 * kNetChunkVec4];
    NetStream s;
    s.cur = s.next = w;
    net_stream_begin(s, w, lds);
    const int h = s.lane >> 5;
    const int site = (int)blockIdx.x * kNetSites + (s.tid >> 6) * kNetTileSites + (s.lane & 31);
    const int px = site < total ? site : total - 1;
    const int plane = px / (H * W), y0 = (px % (H * W)) / W, x0 = px % W;
    float t0, t1, y[8];
    net_taps(in + (long long)plane * H * W, H, W, r, y0, x0, taps, h, t0, t1);
    net_site_body<MT, U>(s, t0, t1, y);
    if (site >= total) return;
    int i, j;
    net_rot(r, y0, x0, H, W, i, j);
    signed char *po = out + (long long)plane * (H * U) * (W * U);
#pragma unroll
    for (int q = 0; q < 8; ++q) {
        const int o = 8 * h + q;
        if (o < U * U) {
            int Y, X;
            net_unrot(r, i * U + o / U, j * U + o % U, H * U, W * U, Y, X);
            po[Y * (W * U) + X] = (signed char)net_q127(y[q]);
        }
    }
}

// ---- stage form
struct NetStageArgs {
    const float4 *w[MULUT_MAX_MODES];
    unsigned taps[MULUT_MAX_MODES];
    const unsigned char *in;
    unsigned char *out;
    int M, is_last, H, W, total;
};

// Integer round-half-even of n / D (D > 0), clipped to a byte.  sr/1_train_model.py:36-43 computes pred / avg_factor + bias in
// float32 and rounds that.  pred is an integer with |pred| <= 127 * 4 * M and avg_factor D is M or 4 * M <= 32, so the exact quotient
// is either an integer, a tie (k + 1/2, exactly representable, and so is the sum with the bias 127), or at least 1 / (2 * D) >= 1 / 64
// away from the nearest tie; float32 carries |pred / D + 127| < 2^10 with an error below 2^-13, which can reach neither.  Hence
// round-half-even of the rational is the reference's float32 result, bit for bit.
__device__ __forceinline__ int net_rhe_clip(int n, int D) {
    int q = n / D, rem = n % D;
    if (rem < 0) {
        rem += D;
        --q;
    }
    if (2 * rem > D || (2 * rem == D && (q & 1))) ++q;
    return q < 0 ? 0 : q > 255 ? 255 : q;
}

// A lane pair owns pixel (y, x) of the un-rotated image and its U x U output block for the whole stage: in rotation r the site that
// produces this block is the pixel's own position in the rotated frame, with the block's sub-pixels rotated along.  The integer sums
// sit in a wave-private LDS tile, [output][site]: in a pass a lane adds the outputs it computed to where they land un-rotated (which
// may be the other lane half's slot), and LDS operations of a wave execute in order, so no synchronisation beyond program order is
// needed.
template <int MT, int U>
__global__ void __launch_bounds__(kNetNT) net_stage_kernel(NetStageArgs a) {
    __shared__ float4 lds[2 * kNetChunkVec4];
    __shared__ int sums[kNetWaves][16][kNetTileSites];
    NetStream s;
    net_stream_begin(s, a.w[0], lds);
    const int h = s.lane >> 5, sl = s.lane & 31, wave = s.tid >> 6;
    const int site = (int)blockIdx.x * kNetSites + wave * kNetTileSites + sl;
    const int px = site < a.total ? site : a.total - 1;
    const int H = a.H, W = a.W;
    const int plane = px / (H * W), y0 = (px % (H * W)) / W, x0 = px % W;
    const unsigned char *pin = a.in + (long long)plane * H * W;
    int(*acc)[kNetTileSites] = sums[wave];
#pragma unroll
    for (int q = 0; q < 8; ++q) acc[8 * h + q][sl] = 0;
    for (int m = 0; m < a.M; ++m) {
        const unsigned taps = a.taps[m];
        for (int r = 0; r < 4; ++r) {
            s.cur = a.w[m];
            s.next = r < 3 ? a.w[m] : a.w[m + 1 < a.M ? m + 1 : m];
            float t0, t1, y[8];
            net_taps(pin, H, W, r, y0, x0, taps, h, t0, t1);
            net_site_body<MT, U>(s, t0, t1, y);
#pragma unroll
            for (int q = 0; q < 8; ++q) {
                const int o = 8 * h + q;
                if (o < U * U) {
                    const int si = o / U, sj = o % U;
                    const int sy = r == 0 ? si : r == 1 ? sj : r == 2 ? U - 1 - si : U - 1 - sj;
                    const int sx = r == 0 ? sj : r == 1 ? U - 1 - si : r == 2 ? U - 1 - sj : si;
                    acc[sy * U + sx][sl] += net_q127(y[q]);
                }
            }
        }
    }
    if (site >= a.total) return;
    const int D = a.is_last ? a.M : 4 * a.M, bias = a.is_last ? 0 : 127 * D;
    unsigned char *po = a.out + (long long)plane * (H * U) * (W * U);
    if (U == 4 && (reinterpret_cast<uintptr_t>(a.out) & 3) == 0) {
#pragma unroll
        for (int row = 0; row < 2; ++row) {
            unsigned v = 0;
#pragma unroll
            for (int q = 0; q < 4; ++q) v |= (unsigned)net_rhe_clip(acc[8 * h + 4 * row + q][sl] + bias, D) << (8 * q);
            *reinterpret_cast<unsigned *>(po + (y0 * 4 + 2 * h + row) * (W * 4) + x0 * 4) = v;
        }
    } else {
#pragma unroll
        for (int q = 0; q < 8; ++q) {
            const int o = 8 * h + q;
            if (o < U * U) po[(y0 * U + o / U) * (W * U) + x0 * U + o % U] = (unsigned char)net_rhe_clip(acc[o][sl] + bias, D);
        }
    }
}

// di | dj << 4 per tap a, b, c, d (common/network.py:150-227), or 0xffffffff for an unknown letter
static unsigned net_pattern(char mode) {
    switch (mode) {
        case 's': return 0x11011000u;
        case 'd': return 0x22022000u;
        case 'y': return 0x12211100u;
        case 'e': return 0x33033000u;
        case 'h': return 0x23322200u;
        case 'o': return 0x13312200u;
        default: return 0xffffffffu;
    }
}

static int net_image_sites(int N, int C, int H, int W, int u, int *sites) {
    if (N < 1 || C < 1 || H < 1 || W < 1) return MULUT_EINVAL;
    const long long px = (long long)N * C;
    if (px >= (1LL << 31) || (long long)H * W >= (1LL << 31) || px * H * W * u * u >= (1LL << 31)) return MULUT_EUNSUPPORTED;
    *sites = (int)(px * H * W);
    return MULUT_OK;
}

#define MULUT_NET_LAUNCH(kernel, mt, u, ...)                                                               \
    do {                                                                                                   \
        if ((mt) == 1) {                                                                                   \
            switch (u) {                                                                                   \
                case 1: hipLaunchKernelGGL((kernel<1, 1>), grid, block, 0, st, __VA_ARGS__); break;        \
                case 2: hipLaunchKernelGGL((kernel<1, 2>), grid, block, 0, st, __VA_ARGS__); break;        \
                case 3: hipLaunchKernelGGL((kernel<1, 3>), grid, block, 0, st, __VA_ARGS__); break;        \
                default: hipLaunchKernelGGL((kernel<1, 4>), grid, block, 0, st, __VA_ARGS__); break;       \
            }                                                                                              \
        } else {                                                                                           \
            switch (u) {                                                                                   \
                case 1: hipLaunchKernelGGL((kernel<2, 1>), grid, block, 0, st, __VA_ARGS__); break;        \
                case 2: hipLaunchKernelGGL((kernel<2, 2>), grid, block, 0, st, __VA_ARGS__); break;        \
                case 3: hipLaunchKernelGGL((kernel<2, 3>), grid, block, 0, st, __VA_ARGS__); break;        \
                default: hipLaunchKernelGGL((kernel<2, 4>), grid, block, 0, st, __VA_ARGS__); break;       \
            }                                                                                              \
        }                                                                                                  \
    } while (0)

}  // namespace mulut

/* common/network.py:62-105 (the weights of one MuLUTUnit, dense=True) */
extern "C" int mulut_net_unit_create(int device, int nf, int u, const float *const w[6], const float *const b[6], mulut_net_unit **out) {
    using namespace mulut;
    if (!out) return MULUT_EINVAL;
    *out = nullptr;
    if (!w || !b) return MULUT_EINVAL;
    for (int l = 0; l < 6; ++l)
        if (!w[l] || !b[l]) return MULUT_EINVAL;
    if (nf < 1 || nf > kNetMaxNf || u < 1 || u > kNetMaxU) return MULUT_EUNSUPPORTED;
    const int mt = net_tiles(nf);
    const long long floats = net_stream_floats(mt);
    std::vector<float> host;
    try {
        host.resize((size_t)floats);
    } catch (const std::bad_alloc &) {
        return MULUT_EUNSUPPORTED;
    }
    net_pack(nf, u, w, b, host.data());
    if (hipSetDevice(device) != hipSuccess) return MULUT_ENODEVICE;
    mulut_net_unit *p = new (std::nothrow) mulut_net_unit{device, nf, u, mt, floats, nullptr};
    if (!p) return MULUT_EHIP;
    if (hipMalloc(reinterpret_cast<void **>(&p->w), (size_t)floats * sizeof(float)) != hipSuccess) {
        delete p;
        return MULUT_EHIP;
    }
    if (hipMemcpy(p->w, host.data(), (size_t)floats * sizeof(float), hipMemcpyHostToDevice) != hipSuccess) {
        (void)hipFree(p->w);
        delete p;
        return MULUT_EHIP;
    }
    *out = p;
    return MULUT_OK;
}

extern "C" int mulut_net_unit_destroy(mulut_net_unit *unit) {
    if (!unit) return MULUT_EINVAL;
    int rc = MULUT_OK;
    if (hipSetDevice(unit->device) != hipSuccess) rc = MULUT_ENODEVICE;
    else if (hipFree(unit->w) != hipSuccess) rc = MULUT_EHIP;
    delete unit;
    return rc;
}

/* sr/2_transfer_to_lut.py:12-41 (the grid) and :86-109 (the network on it, clamp, * 127, round, int8) */
extern "C" int mulut_net_table(const mulut_net_unit *unit, int interval, int8_t *rows_dev, void *stream) {
    using namespace mulut;
    if (!unit || !rows_dev) return MULUT_EINVAL;
    if (interval < 4 || interval > 6) return MULUT_EUNSUPPORTED;
    const int L = (256 >> interval) + 1, total = L * L * L * L;
    if (hipSetDevice(unit->device) != hipSuccess) return MULUT_ENODEVICE;
    const dim3 grid((unsigned)((total + kNetSites - 1) / kNetSites)), block(kNetNT);
    hipStream_t st = (hipStream_t)stream;
    const float4 *w = reinterpret_cast<const float4 *>(unit->w);
    MULUT_NET_LAUNCH(net_table_kernel, unit->mt, unit->u, w, reinterpret_cast<signed char *>(rows_dev), L, interval, total);
    return hipGetLastError() == hipSuccess ? MULUT_OK : MULUT_EHIP;
}

/* sr/1_train_model.py:33-35: one (mode, rotation) term of mulut_predict, before it is added to pred */
extern "C" int mulut_net_pass(const mulut_net_unit *unit, char mode, int r, const uint8_t *in, int N, int C, int H, int W, int8_t *out,
                              void *stream) {
    using namespace mulut;
    if (!unit || !in || !out || r < 0 || r > 3) return MULUT_EINVAL;
    const unsigned taps = net_pattern(mode);
    if (taps == 0xffffffffu) return MULUT_EINVAL;
    int total = 0;
    const int rc = net_image_sites(N, C, H, W, unit->u, &total);
    if (rc != MULUT_OK) return rc;
    if (hipSetDevice(unit->device) != hipSuccess) return MULUT_ENODEVICE;
    const dim3 grid((unsigned)(((long long)total + kNetSites - 1) / kNetSites)), block(kNetNT);
    hipStream_t st = (hipStream_t)stream;
    const float4 *w = reinterpret_cast<const float4 *>(unit->w);
    MULUT_NET_LAUNCH(net_pass_kernel, unit->mt, unit->u, w, in, reinterpret_cast<signed char *>(out), H, W, r, taps, total);
    return hipGetLastError() == hipSuccess ? MULUT_OK : MULUT_EHIP;
}

/* sr/1_train_model.py:29-43 in the 'valid' phase (and :101 for the last stage): one stage, bytes to bytes */
extern "C" int mulut_net_stage(const mulut_net_unit *const units[], const char *modes, int is_last, const uint8_t *in, uint8_t *out, int N,
                               int C, int H, int W, void *stream) {
    using namespace mulut;
    if (!units || !modes || !in || !out) return MULUT_EINVAL;
    const size_t M = strnlen(modes, MULUT_MAX_MODES + 1);
    if (M < 1) return MULUT_EINVAL;
    if (M > MULUT_MAX_MODES) return MULUT_EUNSUPPORTED;
    NetStageArgs a;
    memset(&a, 0, sizeof(a));
    for (size_t m = 0; m < M; ++m) {
        if (!units[m]) return MULUT_EINVAL;
        a.taps[m] = net_pattern(modes[m]);
        if (a.taps[m] == 0xffffffffu) return MULUT_EINVAL;
        if (units[m]->u != units[0]->u || units[m]->mt != units[0]->mt || units[m]->device != units[0]->device) return MULUT_ESHAPE;
        a.w[m] = reinterpret_cast<const float4 *>(units[m]->w);
    }
    const int u = units[0]->u, mt = units[0]->mt;
    const int rc = net_image_sites(N, C, H, W, u, &a.total);
    if (rc != MULUT_OK) return rc;
    a.in = in;
    a.out = out;
    a.M = (int)M;
    a.is_last = is_last ? 1 : 0;
    a.H = H;
    a.W = W;
    if (hipSetDevice(units[0]->device) != hipSuccess) return MULUT_ENODEVICE;
    const dim3 grid((unsigned)(((long long)a.total + kNetSites - 1) / kNetSites)), block(kNetNT);
    hipStream_t st = (hipStream_t)stream;
    MULUT_NET_LAUNCH(net_stage_kernel, mt, u, a);
    return hipGetLastError() == hipSuccess ? MULUT_OK : MULUT_EHIP;
}
