// mulut_net_dev.h -- what mulut_net.hip (inference forms) and mulut_net_train.hip (training forms) share: the unit and its allocation,
// the walk down a weight stream, the site body, the rotations' index arithmetic, the taps, the stage loop, and the stage calls' argument
// checks and launch.
#ifndef MULUT_NET_DEV_H_
#define MULUT_NET_DEV_H_

#include <hip/hip_runtime.h>

#include <cstring>
#include <new>
#include <type_traits>

#include "../../include/mulut.h"
#include "mulut_net.h"

struct mulut_net_unit {
    int device, nf, u, mt;
    long long floats;
    float *w;      // device: the packed stream
    float *wb;     // device: the backward stream (mulut_net_unit_create_train), or NULL
};

namespace mulut {

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

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
    f32x4 pf[4];      // a native vector: a chunk in flight is four loads and four stores, never a copy through memory
    float4 wq;
    int par, tid, lane;
};

__device__ __forceinline__ void net_fetch(NetStream &s, const float4 *chunk) {
#pragma unroll
    for (int j = 0; j < 4; ++j) s.pf[j] = reinterpret_cast<const f32x4 *>(chunk)[j * kNetNT + s.tid];
}

__device__ __forceinline__ void net_put(NetStream &s, int c) {
    float4 *buf = s.lds + ((c & 1) ^ s.par) * kNetChunkVec4;
#pragma unroll
    for (int j = 0; j < 4; ++j) reinterpret_cast<f32x4 *>(buf)[j * kNetNT + s.tid] = s.pf[j];
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

// step G of a stream of NC chunks; TAIL: chunk 0 of `next` is fetched under the last chunk (a walk that ends its workgroup has none)
template <int NC, int G, bool TAIL = true>
__device__ __forceinline__ void net_step_of(NetStream &s, float b, f32x16 &acc) {
    constexpr int c = G / kNetChunkSteps;
    if constexpr (G % kNetChunkSteps == 0) {
        if constexpr (c > 0) {
            net_put(s, c);      // buffer c & 1 was last read in chunk c - 2: every wave has passed the barrier of chunk c - 1 since
            __syncthreads();
        }
        if constexpr (c + 1 < NC) net_fetch(s, s.cur + (c + 1) * kNetChunkVec4);
        else if constexpr (TAIL) net_fetch(s, s.next);
    }
    if constexpr (G % 4 == 0) s.wq = s.lds[((c & 1) ^ s.par) * kNetChunkVec4 + ((G % kNetChunkSteps) / 4) * 64 + s.lane];
    const float a = (G & 3) == 0 ? s.wq.x : (G & 3) == 1 ? s.wq.y : (G & 3) == 2 ? s.wq.z : s.wq.w;
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, acc, 0, 0, 0);
}

template <int MT, int G>
__device__ __forceinline__ void net_step(NetStream &s, float b, f32x16 &acc) {
    net_step_of<net_chunks(MT), G>(s, b, acc);
}

// The six layers.  t0, t1: this lane's tap values of steps 1 and 2 -- (a, c) in lane half 0, (b, d) in half 1.  x[L - 1][mt]: the
// post-ReLU tile mt of layer L; acc: layer 6 before tanh, register r of lane half h being output 8 * h + r.
template <int MT>
__device__ __forceinline__ void net_site_layers(NetStream &s, float t0, float t1, f32x16 (&x)[5][MT], f32x16 &acc) {
    const float one = s.lane < 32 ? 1.0f : 0.0f;
    net_static_for<1, 6>([&](auto Lc) __attribute__((always_inline)) {
        constexpr int L = decltype(Lc)::value;
        net_static_for<0, MT>([&](auto mc) __attribute__((always_inline)) {
            constexpr int mt = decltype(mc)::value, base = net_step_base(MT, L, mt);
            f32x16 a;
#pragma unroll
            for (int q = 0; q < 16; ++q) a[q] = 0.0f;
            net_step<MT, base>(s, one, a);
            if constexpr (L == 1) {
                net_step<MT, base + 1>(s, t0, a);
                net_step<MT, base + 2>(s, t1, a);
            } else {
                net_static_for<0, (L - 1) * MT * 16>([&](auto kc) __attribute__((always_inline)) {
                    constexpr int k = decltype(kc)::value;
                    net_step<MT, base + 1 + k>(s, x[k / (MT * 16)][(k / 16) % MT][k % 16], a);
                });
            }
#pragma unroll
            for (int q = 0; q < 16; ++q) x[L - 1][mt][q] = fmaxf(a[q], 0.0f);
        });
    });
    constexpr int base6 = net_step_base(MT, 6, 0);
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
}

// y[r]: output 8 * h + r (valid below u*u)
template <int MT, int U>
__device__ __forceinline__ void net_site_body(NetStream &s, float t0, float t1, float (&y)[8]) {
    f32x16 x[5][MT], acc;
    net_site_layers<MT>(s, t0, t1, x, acc);
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

// a tap as the network sees it: a byte of the 'valid' phase is divided by 255, a float of the 'train' phase is the value itself
__device__ __forceinline__ float net_tap_value(unsigned char v) { return (float)v / 255.0f; }
__device__ __forceinline__ float net_tap_value(float v) { return v; }

// Where tap k of the pattern (`taps`: di | dj << 4 in byte k) of the site that pixel (y, x) of the un-rotated plane is in rotation r
// lies in that plane: replicate-padded on the bottom and right of the ROTATED image (mode_pad_dict)
__device__ __forceinline__ int net_tap_index(int H, int W, int r, int y, int x, unsigned taps, int k) {
    int i, j;
    net_rot(r, y, x, H, W, i, j);
    const int Hr = (r & 1) ? W : H, Wr = (r & 1) ? H : W;
    const unsigned tp = taps >> (8 * k);
    int ii = i + (int)(tp & 15u), jj = j + (int)((tp >> 4) & 15u), yy, xx;
    ii = ii < Hr ? ii : Hr - 1;
    jj = jj < Wr ? jj : Wr - 1;
    net_unrot(r, ii, jj, H, W, yy, xx);
    return yy * W + xx;
}

// The two tap values of this lane half: taps k = h and 2 + h
template <class T>
__device__ __forceinline__ void net_taps(const T *plane, int H, int W, int r, int y, int x, unsigned taps, int h, float &t0, float &t1) {
    t0 = net_tap_value(plane[net_tap_index(H, W, r, y, x, taps, h)]);
    t1 = net_tap_value(plane[net_tap_index(H, W, r, y, x, taps, 2 + h)]);
}

// ---- stage form
template <class T, class O>
struct NetStageArgs {
    const float4 *w[MULUT_MAX_MODES];
    unsigned taps[MULUT_MAX_MODES];
    const T *in;
    O *out;
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
// needed.  O = unsigned char: the stage's epilogue in integers; O = float: the sums themselves (the 'train' phase's pred).
// (net_list_kernel of mulut_net_list.hip holds a COPY of the loop over modes and rotations below, its taps apart: shared through one
// function it changed this body's instructions.  A change to the accumulation or the sub-pixel rotation here goes there too.)
template <int MT, int U, class T, class O>
__device__ __forceinline__ void net_stage_body(const NetStageArgs<T, O> &a, float4 *lds, int (*sums)[16][kNetTileSites]) {
    NetStream s;
    net_stream_begin(s, a.w[0], lds);
    const int h = s.lane >> 5, sl = s.lane & 31, wave = s.tid >> 6;
    const int site = (int)blockIdx.x * kNetSites + wave * kNetTileSites + sl;
    const int px = site < a.total ? site : a.total - 1;
    const int H = a.H, W = a.W;
    const int plane = px / (H * W), y0 = (px % (H * W)) / W, x0 = px % W;
    const T *pin = a.in + (long long)plane * H * W;
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
    O *po = a.out + (long long)plane * (H * U) * (W * U);
    if constexpr (std::is_same<O, float>::value) {
#pragma unroll
        for (int q = 0; q < 8; ++q) {
            const int o = 8 * h + q;
            if (o < U * U) po[(y0 * U + o / U) * (W * U) + x0 * U + o % U] = (float)acc[o][sl];
        }
    } else {
        const int D = a.is_last ? a.M : 4 * a.M, bias = a.is_last ? 0 : 127 * D;
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
}

// di | dj << 4 per tap a, b, c, d (common/network.py:150-227), or 0xffffffff for an unknown letter
inline unsigned net_pattern(char mode) {
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

inline int net_image_sites(int N, int C, int H, int W, int u, int *sites) {
    if (N < 1 || C < 1 || H < 1 || W < 1) return MULUT_EINVAL;
    const long long px = (long long)N * C;
    if (px >= (1LL << 31) || (long long)H * W >= (1LL << 31) || px * H * W * u * u >= (1LL << 31)) return MULUT_EUNSUPPORTED;
    *sites = (int)(px * H * W);
    return MULUT_OK;
}

// the common argument checks of the stage calls: the mode list, the units' agreement; fills w (stream 0: forward, 1: backward) and taps
inline int net_stage_units(const mulut_net_unit *const units[], const char *modes, int backward, const float4 **w, unsigned *taps, int *M_out) {
    const size_t M = strnlen(modes, MULUT_MAX_MODES + 1);
    if (M < 1) return MULUT_EINVAL;
    if (M > MULUT_MAX_MODES) return MULUT_EUNSUPPORTED;
    for (size_t m = 0; m < M; ++m) {
        if (!units[m]) return MULUT_EINVAL;
        taps[m] = net_pattern(modes[m]);
        if (taps[m] == 0xffffffffu) return MULUT_EINVAL;
        if (units[m]->u != units[0]->u || units[m]->mt != units[0]->mt || units[m]->device != units[0]->device) return MULUT_ESHAPE;
        if (backward && !units[m]->wb) return MULUT_EINVAL;
        w[m] = reinterpret_cast<const float4 *>(backward ? units[m]->wb : units[m]->w);
    }
    *M_out = (int)M;
    return MULUT_OK;
}

// One allocation per unit: the forward stream, uploaded from `host`, or (host NULL: a training unit) both streams, zeroed.
// mulut_net_unit_destroy frees w.
inline int net_unit_new(int device, int nf, int u, const float *host, mulut_net_unit **out) {
    const int mt = net_tiles(nf);
    const long long floats = net_stream_floats(mt);
    const size_t bytes = (size_t)(floats + (host ? 0 : net_bwd_stream_floats(mt))) * sizeof(float);
    if (hipSetDevice(device) != hipSuccess) return MULUT_ENODEVICE;
    mulut_net_unit *p = new (std::nothrow) mulut_net_unit{device, nf, u, mt, floats, nullptr, nullptr};
    if (!p) return MULUT_EHIP;
    if (hipMalloc(reinterpret_cast<void **>(&p->w), bytes) != hipSuccess) {
        delete p;
        return MULUT_EHIP;
    }
    if ((host ? hipMemcpy(p->w, host, bytes, hipMemcpyHostToDevice) : hipMemset(p->w, 0, bytes)) != hipSuccess) {
        (void)hipFree(p->w);
        delete p;
        return MULUT_EHIP;
    }
    if (!host) p->wb = p->w + floats;
    *out = p;
    return MULUT_OK;
}

// kernel<MT, U> over `sites` sites, one workgroup per kNetSites of them, on `stream`
#define MULUT_NET_LAUNCH_U(kernel, MT, U, sites, stream, ...)                                                           \
    hipLaunchKernelGGL((kernel<MT, U>), dim3((unsigned)(((long long)(sites) + kNetSites - 1) / kNetSites)), dim3(kNetNT), 0, \
                       (hipStream_t)(stream), __VA_ARGS__)
#define MULUT_NET_LAUNCH_MT(kernel, MT, u, sites, stream, ...)                                   \
    switch (u) {                                                                                 \
        case 1: MULUT_NET_LAUNCH_U(kernel, MT, 1, sites, stream, __VA_ARGS__); break;            \
        case 2: MULUT_NET_LAUNCH_U(kernel, MT, 2, sites, stream, __VA_ARGS__); break;            \
        case 3: MULUT_NET_LAUNCH_U(kernel, MT, 3, sites, stream, __VA_ARGS__); break;            \
        default: MULUT_NET_LAUNCH_U(kernel, MT, 4, sites, stream, __VA_ARGS__); break;           \
    }
#define MULUT_NET_LAUNCH(kernel, mt, u, sites, stream, ...)                                      \
    do {                                                                                         \
        if ((mt) == 1) MULUT_NET_LAUNCH_MT(kernel, 1, u, sites, stream, __VA_ARGS__)             \
        else MULUT_NET_LAUNCH_MT(kernel, 2, u, sites, stream, __VA_ARGS__)                       \
    } while (0)

}  // namespace mulut
#endif
