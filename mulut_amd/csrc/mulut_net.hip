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

#include "mulut_net_dev.h"

namespace mulut {

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

// ---- stage form (the body is net_stage_body of mulut_net_dev.h)
template <int MT, int U>
__global__ void __launch_bounds__(kNetNT) net_stage_kernel(NetStageArgs<unsigned char, unsigned char> a) {
    __shared__ float4 lds[2 * kNetChunkVec4];
    __shared__ int sums[kNetWaves][16][kNetTileSites];
    net_stage_body<MT, U>(a, lds, sums);
}

}  // namespace mulut

/* common/network.py:62-105 (the weights of one MuLUTUnit, dense=True) */
extern "C" int mulut_net_unit_create(int device, int nf, int u, const float *const w[6], const float *const b[6], mulut_net_unit **out) {
    using namespace mulut;
    if (!out) return MULUT_EINVAL;
    *out = nullptr;
    if (!net_have_params(w, b)) return MULUT_EINVAL;
    if (!net_unit_ok(nf, u)) return MULUT_EUNSUPPORTED;
    std::vector<float> host;
    try {
        host.resize((size_t)net_stream_floats(net_tiles(nf)));
    } catch (const std::bad_alloc &) {
        return MULUT_EUNSUPPORTED;
    }
    net_pack(nf, u, w, b, host.data());
    return net_unit_new(device, nf, u, host.data(), out);
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
    const float4 *w = reinterpret_cast<const float4 *>(unit->w);
    MULUT_NET_LAUNCH(net_table_kernel, unit->mt, unit->u, total, stream, w, reinterpret_cast<signed char *>(rows_dev), L, interval, total);
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
    const float4 *w = reinterpret_cast<const float4 *>(unit->w);
    MULUT_NET_LAUNCH(net_pass_kernel, unit->mt, unit->u, total, stream, w, in, reinterpret_cast<signed char *>(out), H, W, r, taps, total);
    return hipGetLastError() == hipSuccess ? MULUT_OK : MULUT_EHIP;
}

/* sr/1_train_model.py:29-43 in the 'valid' phase (and :101 for the last stage): one stage, bytes to bytes */
extern "C" int mulut_net_stage(const mulut_net_unit *const units[], const char *modes, int is_last, const uint8_t *in, uint8_t *out, int N,
                               int C, int H, int W, void *stream) {
    using namespace mulut;
    if (!units || !modes || !in || !out) return MULUT_EINVAL;
    NetStageArgs<unsigned char, unsigned char> a;
    memset(&a, 0, sizeof(a));
    int rc = net_stage_units(units, modes, 0, a.w, a.taps, &a.M);
    if (rc != MULUT_OK) return rc;
    const int u = units[0]->u, mt = units[0]->mt;
    rc = net_image_sites(N, C, H, W, u, &a.total);
    if (rc != MULUT_OK) return rc;
    a.in = in;
    a.out = out;
    a.is_last = is_last ? 1 : 0;
    a.H = H;
    a.W = W;
    if (hipSetDevice(units[0]->device) != hipSuccess) return MULUT_ENODEVICE;
    MULUT_NET_LAUNCH(net_stage_kernel, mt, u, a.total, stream, a);
    return hipGetLastError() == hipSuccess ? MULUT_OK : MULUT_EHIP;
}
