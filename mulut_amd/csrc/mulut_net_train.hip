// mulut_net_train.hip -- training the SR network on the fused site body of mulut_net.hip: units whose streams follow parameters that
// live on the device, the 'train'-phase stage forward, and the backward.
//
// Reference: sr/1_train_model.py:26-45 (`mulut_predict(..., 'train')`), :194-197 (loss, backward).  Per stage the reference sums 4 M
// terms round(127 * net(pad(rot^r(x)))) rotated back; what follows the sum (average, bias, clamp, BPDA round, / 255) is element-wise
// and stays with the caller.  mulut_net_stage_sum is that sum; mulut_net_stage_backward is its gradient with round as the identity
// (round_func, :48-55): given g = dL/dsum it returns dL/dx and dL/d(every weight and bias of the stage's M units).
//
// The backward of one (mode, rotation) pass is two kernels over a caller-owned workspace (layout: mulut_net.h):
//   net_bwd_site_kernel   per 128-site workgroup: the forward again, keeping the five post-ReLU tiles; delta_6 = 127 g (1 - y^2) with g
//                         read where the site's u x u block lands un-rotated; then source layers 5..1 on the MFMA from the backward
//                         stream, masked by x > 0 in place; x_s and delta_s go to the workspace as delta_s is made.  With gx, the tap
//                         gradient W_1^T delta_1 is added to gx at the four (clamped, un-rotated) tap positions with float atomics.
//   net_wgrad_kernel      dW_L[out][in] = sum over sites of delta_L[out][site] xcat_L[in][site] and db_L = sum of delta_L: one launch
//                         for all six layers, a workgroup per (out tile, in tile) pair and site split; its four waves' tiles are added
//                         in wave order and the result is added to the split's own copy of the gradient.  No atomics.
// After the four rotations of a unit net_wgrad_reduce_kernel adds the kNetGradSplits copies in index order into gw / gb, so these are
// bit-identical from run to run (gx is not: float atomics).
//
// mulut_net_stage_backward_exact makes gx a function of its inputs too, without atomics and without fixed point.  Its site kernel,
// net_bwd_site_taps_kernel (the same body, the other compile-time form), STORES the four tap gradients of a site into a tap buffer
// [4][ts] of the workspace, and after the last chunk of a pass net_gx_gather_kernel, one thread per input pixel, adds the terms that
// land on its pixel in the fixed order include/mulut.h defines, found by index arithmetic.  gw / gb are the bits of the other backward.
#include "mulut_net_dev.h"

namespace mulut {

// one thread per float of either stream
__global__ void __launch_bounds__(256) net_pack_kernel(NetParams p, int nf, int u, int MT, float *fwd, int fwd_floats, float *bwd, int bwd_floats) {
    const int idx = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (idx >= fwd_floats + bwd_floats) return;
    const int f = idx < fwd_floats ? idx : idx - fwd_floats;
    const int g = (f >> 8) * 4 + (f & 3), lane = (f >> 2) & 63;      // the inverse of net_step_float
    if (idx < fwd_floats) fwd[f] = net_fwd_value(nf, u, MT, g, lane, p);
    else bwd[f] = net_bwd_value(nf, u, MT, g, lane, p);
}

template <int MT, int U>
__global__ void __launch_bounds__(kNetNT) net_stage_sum_kernel(NetStageArgs<float, float> a) {
    __shared__ float4 lds[2 * kNetChunkVec4];
    __shared__ int sums[kNetWaves][16][kNetTileSites];
    net_stage_body<MT, U>(a, lds, sums);
}

struct NetBwdArgs {
    const float4 *wf, *wb;
    const float *x, *g;
    float *gx, *ws;
    long long cs;      // sites per workspace row
    unsigned taps;
    int r, u, nf, H, W, total, site0;
};

// The site body in its two forms.  TAPS false: the tap gradient is added into a.gx with float atomics.  TAPS true: a.gx is the pass's
// tap buffer t, float [4][ts] with the site as the fast index, and row k of the site's column is STORED -- 32 consecutive floats per
// wave and tap; net_gx_gather_kernel sums them per pixel in a fixed order.
template <int MT, bool TAPS>
__device__ __forceinline__ void net_bwd_site_body(const NetBwdArgs &a, long long ts, float4 *lds) {
    NetStream s;
    s.cur = a.wf;
    s.next = a.wb;
    net_stream_begin(s, a.wf, lds);
    const int h = s.lane >> 5, sl = s.lane & 31, wave = s.tid >> 6;
    const int local = (int)blockIdx.x * kNetSites + wave * kNetTileSites + sl;      // < cs: the grid covers no more than the chunk
    const long long site = (long long)a.site0 + local;
    const bool valid = site < a.total;
    const int px = valid ? (int)site : a.total - 1;
    const int H = a.H, W = a.W, U = a.u, nf = a.nf;
    const int plane = px / (H * W), y0 = (px % (H * W)) / W, x0 = px % W;
    const float *pin = a.x + (long long)plane * H * W;
    float t0, t1;
    net_taps(pin, H, W, a.r, y0, x0, a.taps, h, t0, t1);
    f32x16 x[5][MT], acc;
    net_site_layers<MT>(s, t0, t1, x, acc);
    s.cur = a.wb;      // chunk 0 of the backward stream is in LDS now; the walk down it is the workgroup's last
    float *wsl = a.ws + local;
    const long long cs = a.cs;
    wsl[h * cs] = t0;
    wsl[(2 + h) * cs] = t1;
    // delta_6: g where output o of this site lands un-rotated -- the inverse of net_pass_kernel's store
    typedef float f32x8 __attribute__((ext_vector_type(8)));
    f32x8 d6;
    {
        int i, j;
        net_rot(a.r, y0, x0, H, W, i, j);
        const float *pg = a.g + (long long)plane * (H * U) * (W * U);
#pragma unroll
        for (int q = 0; q < 8; ++q) {
            const int o = 8 * h + q;
            float v = 0.0f;
            if (o < U * U) {
                if (valid) {
                    int Y, X;
                    net_unrot(a.r, i * U + o / U, j * U + o % U, H * U, W * U, Y, X);
                    const float y = tanhf(acc[q]);
                    v = 127.0f * pg[Y * (W * U) + X] * (1.0f - y * y);
                }
                wsl[(4 + 10 * nf + o) * cs] = v;
            }
            d6[q] = v;
        }
    }
    constexpr int NCB = net_bwd_chunks(MT);
    f32x16 d[5][MT];
    net_static_for<0, 5>([&](auto sc) __attribute__((always_inline)) {
        constexpr int S = 5 - decltype(sc)::value;      // source layer 5..1
        net_static_for<0, MT>([&](auto tc) __attribute__((always_inline)) {
            constexpr int t = decltype(tc)::value, base = net_bwd_step_base(MT, S, t);
            f32x16 gacc;
#pragma unroll
            for (int q = 0; q < 16; ++q) gacc[q] = 0.0f;
            net_static_for<0, 8>([&](auto kc) __attribute__((always_inline)) {
                constexpr int k = decltype(kc)::value;
                net_step_of<NCB, base + k, false>(s, d6[k], gacc);
            });
            net_static_for<0, (5 - S) * MT * 16>([&](auto kc) __attribute__((always_inline)) {
                constexpr int k = decltype(kc)::value;
                net_step_of<NCB, base + 8 + k, false>(s, d[4 - k / (MT * 16)][(k / 16) % MT][k % 16], gacc);
            });
#pragma unroll
            for (int q = 0; q < 16; ++q) {
                const float xv = x[S - 1][t][q], dv = xv > 0.0f ? gacc[q] : 0.0f;
                d[S - 1][t][q] = dv;
                const int f = 32 * t + net_row(q, h);
                if (f < nf) {
                    wsl[(4 + (S - 1) * nf + f) * cs] = xv;
                    wsl[(4 + (4 + S) * nf + f) * cs] = dv;
                }
            }
        });
    });
    if (a.gx == nullptr) return;      // uniform over the workgroup
    constexpr int tap_base = net_bwd_step_base(MT, 0, 0);
    f32x16 gacc;
#pragma unroll
    for (int q = 0; q < 16; ++q) gacc[q] = 0.0f;
    net_static_for<0, MT * 16>([&](auto kc) __attribute__((always_inline)) {
        constexpr int k = decltype(kc)::value;
        net_step_of<NCB, tap_base + k, false>(s, d[0][k / 16][k % 16], gacc);
    });
    if (valid && h == 0) {
        if constexpr (TAPS) {
#pragma unroll
            for (int q = 0; q < 4; ++q) a.gx[q * ts + site] = gacc[q];
        } else {
            float *pgx = a.gx + (long long)plane * H * W;
#pragma unroll
            for (int q = 0; q < 4; ++q) atomicAdd(pgx + net_tap_index(H, W, a.r, y0, x0, a.taps, q), gacc[q]);
        }
    }
}

template <int MT>
__global__ void __launch_bounds__(kNetNT) net_bwd_site_kernel(NetBwdArgs a) {
    __shared__ float4 lds[2 * kNetChunkVec4];
    net_bwd_site_body<MT, false>(a, 0, lds);
}

template <int MT>
__global__ void __launch_bounds__(kNetNT) net_bwd_site_taps_kernel(NetBwdArgs a, long long ts) {
    __shared__ float4 lds[2 * kNetChunkVec4];
    net_bwd_site_body<MT, true>(a, ts, lds);
}

// gx of one (pattern, rotation) pass from its tap buffer: the definition of mulut_net_gx_gather (include/mulut.h), one thread per
// input pixel.  Tap k = (di, dj) of the site at (i, j) of the ROTATED frame reads (min(i + di, Hr - 1), min(j + dj, Wr - 1)), so row i'
// receives from i' - di below the last row and from every i in [max(0, Hr - 1 - di), Hr - 1] on it, and columns likewise: a rectangle
// of sites, which is a rectangle of the un-rotated plane too, walked there row by row -- ascending in the index the site kernel
// numbers sites with.
struct NetGatherArgs {
    const float *t;
    float *gx;
    long long ts;
    unsigned taps;
    int r, H, W, total, accumulate;
};

__global__ void __launch_bounds__(256) net_gx_gather_kernel(NetGatherArgs a) {
    const int idx = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (idx >= a.total) return;
    const int H = a.H, W = a.W, r = a.r;
    const int plane = idx / (H * W), p = idx % (H * W), y = p / W, x = p % W;
    const int Hr = (r & 1) ? W : H, Wr = (r & 1) ? H : W;
    int ip, jp;
    net_rot(r, y, x, H, W, ip, jp);
    const float *tp = a.t + (long long)plane * H * W;
    float acc = a.accumulate ? a.gx[idx] : 0.0f;
    for (int k = 0; k < 4; ++k) {
        const unsigned tpn = a.taps >> (8 * k);
        const int di = (int)(tpn & 15u), dj = (int)((tpn >> 4) & 15u);
        int i_lo = ip - di, i_hi = ip - di, j_lo = jp - dj, j_hi = jp - dj;
        if (ip == Hr - 1) i_hi = ip;
        if (jp == Wr - 1) j_hi = jp;
        i_lo = i_lo > 0 ? i_lo : 0;
        j_lo = j_lo > 0 ? j_lo : 0;
        if (i_lo > i_hi || j_lo > j_hi) continue;
        int ya, xa, yb, xb;
        net_unrot(r, i_lo, j_lo, H, W, ya, xa);
        net_unrot(r, i_hi, j_hi, H, W, yb, xb);
        const int y_lo = ya < yb ? ya : yb, y_hi = ya < yb ? yb : ya, x_lo = xa < xb ? xa : xb, x_hi = xa < xb ? xb : xa;
        const float *tk = tp + k * a.ts;
        for (int y0 = y_lo; y0 <= y_hi; ++y0)
            for (int x0 = x_lo; x0 <= x_hi; ++x0) acc = acc + tk[y0 * W + x0];
    }
    a.gx[idx] = acc;
}

struct NetWgradArgs {
    const float *ws;
    float *partial;      // [kNetGradSplits][P]
    long long cs;
    int nf, u, groups, P;      // groups: 32-site groups of the chunk to sum over
};

// the (layer, out tile, in tile) pairs of a unit; the last in tile of a layer is the bias (B = 1)
__host__ __device__ inline int net_wgrad_pairs(int nf, int u) {
    int n = 0;
    for (int L = 1; L <= 6; ++L) n += ((net_layer_out(nf, u, L) + 31) / 32) * ((net_layer_in(nf, L) + 31) / 32 + 1);
    return n;
}

__global__ void __launch_bounds__(kNetNT) net_wgrad_kernel(NetWgradArgs a) {
    __shared__ float red[kNetWaves - 1][16][64];
    const int nf = a.nf, u = a.u;
    int p = (int)blockIdx.x, L = 1, out_f = nf, in_f = 4, IT = 2, off_w = 0, off_b = 0;
    for (int l = 1; l <= 6; ++l) off_b += net_layer_out(nf, u, l) * net_layer_in(nf, l);
    for (;; ++L) {
        out_f = net_layer_out(nf, u, L);
        in_f = net_layer_in(nf, L);
        IT = (in_f + 31) / 32 + 1;
        const int n = ((out_f + 31) / 32) * IT;
        if (p < n) break;
        p -= n;
        off_w += out_f * in_f;
        off_b += out_f;
    }
    const int ot = p / IT, it = p % IT;
    const bool bias = it == IT - 1;
    const int z = (int)blockIdx.y, lane = (int)threadIdx.x & 63, wave = (int)threadIdx.x >> 6, i = lane & 31, h = lane >> 5;
    const bool dvalid = ot * 32 + i < out_f, xvalid = !bias && it * 32 + i < in_f;
    const long long drow = (L < 6 ? 4 + (4 + L) * nf : 4 + 10 * nf) + (dvalid ? ot * 32 + i : 0);
    const long long xrow = (L == 1 ? 0 : 4) + (xvalid ? it * 32 + i : 0);
    const float *pa = a.ws + drow * a.cs + 16 * h, *pb = a.ws + xrow * a.cs + 16 * h;
    f32x16 acc;
#pragma unroll
    for (int q = 0; q < 16; ++q) acc[q] = 0.0f;
    const float4 zero = make_float4(0.0f, 0.0f, 0.0f, 0.0f), ones = make_float4(1.0f, 1.0f, 1.0f, 1.0f);
    for (int g = z + kNetGradSplits * wave; g < a.groups; g += kNetGradSplits * kNetWaves) {
        const float4 *qa = reinterpret_cast<const float4 *>(pa + (long long)g * 32), *qb = reinterpret_cast<const float4 *>(pb + (long long)g * 32);
        float4 A[4], B[4];
#pragma unroll
        for (int v = 0; v < 4; ++v) {
            A[v] = dvalid ? qa[v] : zero;
            B[v] = bias ? ones : xvalid ? qb[v] : zero;
        }
#pragma unroll
        for (int v = 0; v < 4; ++v) {
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(A[v].x, B[v].x, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(A[v].y, B[v].y, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(A[v].z, B[v].z, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(A[v].w, B[v].w, acc, 0, 0, 0);
        }
    }
    if (wave > 0) {
#pragma unroll
        for (int q = 0; q < 16; ++q) red[wave - 1][q][lane] = acc[q];
    }
    __syncthreads();
    if (wave > 0) return;
    float *dst = a.partial + (long long)z * a.P;
#pragma unroll
    for (int q = 0; q < 16; ++q) {
        const float v = ((acc[q] + red[0][q][lane]) + red[1][q][lane]) + red[2][q][lane];
        const int out = ot * 32 + net_row(q, h), in = it * 32 + i;      // result register q of lane (i, h): row net_row(q, h), column i
        if (out >= out_f) continue;
        if (bias) {
            if (i == 0) dst[off_b + out] += v;
        } else if (in < in_f) {
            dst[off_w + out * in_f + in] += v;
        }
    }
}

struct NetGradOut {
    float *p[12];      // dW_1..dW_6, db_1..db_6
    int end[12];       // where each ends in a copy of the gradient
};

__global__ void __launch_bounds__(256) net_wgrad_reduce_kernel(const float *partial, int P, NetGradOut o) {
    const int idx = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (idx >= P) return;
    float v = partial[idx];
    for (int z = 1; z < kNetGradSplits; ++z) v += partial[(long long)z * P + idx];
    float *dst = nullptr;
#pragma unroll
    for (int k = 0; k < 12; ++k)
        if (dst == nullptr && idx < o.end[k]) dst = o.p[k] + (idx - (k ? o.end[k - 1] : 0));
    *dst = v;
}

static long long net_partial_bytes(int nf, int u) {
    const long long b = (long long)kNetGradSplits * net_param_floats(nf, u) * (long long)sizeof(float);
    return (b + 255) / 256 * 256;
}

// the tap buffer of a pass: float [4][ts], ts the pass's sites rounded up to 128
static long long net_tap_bytes(long long ts) { return 4 * ts * (long long)sizeof(float); }

static void net_gx_gather_launch(unsigned taps, int r, const float *t, long long ts, int total, int H, int W, float *gx, bool accumulate, hipStream_t st) {
    NetGatherArgs a{t, gx, ts, taps, r, H, W, total, accumulate ? 1 : 0};
    hipLaunchKernelGGL(net_gx_gather_kernel, dim3((unsigned)(((long long)total + 255) / 256)), dim3(256), 0, st, a);
}

}  // namespace mulut

/* a unit for training: both streams allocated and zeroed, to be filled by mulut_net_unit_load_dev */
extern "C" int mulut_net_unit_create_train(int device, int nf, int u, mulut_net_unit **out) {
    using namespace mulut;
    if (!out) return MULUT_EINVAL;
    *out = nullptr;
    if (!net_unit_ok(nf, u)) return MULUT_EUNSUPPORTED;
    return net_unit_new(device, nf, u, nullptr, out);
}

/* the host packs, for tests of the device pack: the stream mulut_net_unit_create uploads (backward 0) or the backward stream (1) */
extern "C" long long mulut_net_pack_host(int nf, int u, const float *const w[6], const float *const b[6], int backward, float *out, long long cap) {
    using namespace mulut;
    if (!net_have_params(w, b) || !out || backward < 0 || backward > 1) return MULUT_EINVAL;
    if (!net_unit_ok(nf, u)) return MULUT_EUNSUPPORTED;
    const long long n = backward ? net_bwd_stream_floats(net_tiles(nf)) : net_stream_floats(net_tiles(nf));
    if (cap < n) return MULUT_EWORKSPACE;
    if (backward) net_pack_bwd(nf, u, w, out);
    else net_pack(nf, u, w, b, out);
    return n;
}

extern "C" int mulut_net_unit_load_dev(mulut_net_unit *unit, const float *const w_dev[6], const float *const b_dev[6], void *stream) {
    using namespace mulut;
    if (!unit || !net_have_params(w_dev, b_dev)) return MULUT_EINVAL;
    NetParams p;
    for (int l = 0; l < 6; ++l) p.w[l] = w_dev[l], p.b[l] = b_dev[l];
    if (hipSetDevice(unit->device) != hipSuccess) return MULUT_ENODEVICE;
    const int ff = (int)unit->floats, bf = unit->wb ? (int)net_bwd_stream_floats(unit->mt) : 0;
    hipLaunchKernelGGL(net_pack_kernel, dim3((unsigned)((ff + bf + 255) / 256)), dim3(256), 0, (hipStream_t)stream, p, unit->nf, unit->u, unit->mt,
                       unit->w, ff, unit->wb, bf);
    return hipGetLastError() == hipSuccess ? MULUT_OK : MULUT_EHIP;
}

extern "C" long long mulut_net_unit_read(const mulut_net_unit *unit, int backward, float *host, long long cap) {
    using namespace mulut;
    if (!unit || !host || backward < 0 || backward > 1) return MULUT_EINVAL;
    if (backward && !unit->wb) return MULUT_EINVAL;
    const long long n = backward ? net_bwd_stream_floats(unit->mt) : unit->floats;
    if (cap < n) return MULUT_EWORKSPACE;
    if (hipSetDevice(unit->device) != hipSuccess) return MULUT_ENODEVICE;
    if (hipDeviceSynchronize() != hipSuccess) return MULUT_EHIP;
    if (hipMemcpy(host, backward ? unit->wb : unit->w, (size_t)n * sizeof(float), hipMemcpyDeviceToHost) != hipSuccess) return MULUT_EHIP;
    return n;
}

/* sr/1_train_model.py:30-35: pred of one stage in the 'train' phase, before :36-43 */
extern "C" int mulut_net_stage_sum(const mulut_net_unit *const units[], const char *modes, const float *x, int N, int C, int H, int W, float *pred,
                                   void *stream) {
    using namespace mulut;
    if (!units || !modes || !x || !pred) return MULUT_EINVAL;
    NetStageArgs<float, float> a;
    memset(&a, 0, sizeof(a));
    int rc = net_stage_units(units, modes, 0, a.w, a.taps, &a.M);
    if (rc != MULUT_OK) return rc;
    const int u = units[0]->u, mt = units[0]->mt;
    rc = net_image_sites(N, C, H, W, u, &a.total);
    if (rc != MULUT_OK) return rc;
    a.in = x;
    a.out = pred;
    a.H = H;
    a.W = W;
    if (hipSetDevice(units[0]->device) != hipSuccess) return MULUT_ENODEVICE;
    MULUT_NET_LAUNCH(net_stage_sum_kernel, mt, u, a.total, stream, a);
    return hipGetLastError() == hipSuccess ? MULUT_OK : MULUT_EHIP;
}

extern "C" long long mulut_net_backward_ws_bytes(int nf, int u, long long sites) {
    using namespace mulut;
    if (sites < 1) return MULUT_EINVAL;
    if (!net_unit_ok(nf, u) || sites >= (1LL << 31)) return MULUT_EUNSUPPORTED;
    const long long cs = (sites + kNetSites - 1) / kNetSites * kNetSites;
    return net_partial_bytes(nf, u) + cs * net_ws_rows(nf, u) * (long long)sizeof(float);
}

// Both backwards.  exact: the workspace holds the pass's tap buffer, float [4][ts], between the partial copies and the rows; the site
// kernel stores a site's tap gradient there and, after the last chunk of a pass, net_gx_gather_kernel writes (first pass of the stage)
// or adds to gx.
static int net_backward(const mulut_net_unit *const units[], const char *modes, const float *x, const float *g, int N, int C, int H, int W, void *ws,
                        long long ws_bytes, float *gx, float *const gw[], float *const gb[], void *stream, bool exact) {
    using namespace mulut;
    if (!units || !modes || !x || !g || !ws || !gw || !gb) return MULUT_EINVAL;
    const float4 *wf[MULUT_MAX_MODES], *wb[MULUT_MAX_MODES];
    unsigned taps[MULUT_MAX_MODES];
    int M = 0, total = 0;
    int rc = net_stage_units(units, modes, 0, wf, taps, &M);
    if (rc == MULUT_OK) rc = net_stage_units(units, modes, 1, wb, taps, &M);
    if (rc != MULUT_OK) return rc;
    for (int k = 0; k < 6 * M; ++k)
        if (!gw[k] || !gb[k]) return MULUT_EINVAL;
    const int u = units[0]->u, mt = units[0]->mt, nf = units[0]->nf;
    for (int m = 0; m < M; ++m)
        if (units[m]->nf != nf) return MULUT_ESHAPE;
    rc = net_image_sites(N, C, H, W, u, &total);
    if (rc != MULUT_OK) return rc;
    if (reinterpret_cast<uintptr_t>(ws) & 255) return MULUT_EINVAL;
    const long long need = ((long long)total + kNetSites - 1) / kNetSites * kNetSites;
    const long long pbytes = net_partial_bytes(nf, u), row_bytes = net_ws_rows(nf, u) * (long long)sizeof(float);
    const long long tbytes = exact ? net_tap_bytes(need) : 0;
    if (ws_bytes < pbytes + tbytes + kNetSites * row_bytes) return MULUT_EWORKSPACE;
    long long cs = (ws_bytes - pbytes - tbytes) / row_bytes / kNetSites * kNetSites;
    if (cs > need) cs = need;
    if (hipSetDevice(units[0]->device) != hipSuccess) return MULUT_ENODEVICE;
    hipStream_t st = (hipStream_t)stream;
    float *partial = static_cast<float *>(ws), *t = reinterpret_cast<float *>(static_cast<char *>(ws) + pbytes);
    float *rows = reinterpret_cast<float *>(static_cast<char *>(ws) + pbytes + tbytes);
    const int P = net_param_floats(nf, u), pairs = net_wgrad_pairs(nf, u);
    for (int m = 0; m < M; ++m) {
        if (hipMemsetAsync(partial, 0, (size_t)kNetGradSplits * P * sizeof(float), st) != hipSuccess) return MULUT_EHIP;
        for (int r = 0; r < 4; ++r) {
            for (long long site0 = 0; site0 < total; site0 += cs) {
                const long long n = total - site0 < cs ? total - site0 : cs;
                const int blocks = (int)((n + kNetSites - 1) / kNetSites);
                NetBwdArgs a{wf[m], wb[m], x, g, exact && gx ? t : gx, rows, cs, taps[m], r, u, nf, H, W, total, (int)site0};
                if (exact) {
                    if (mt == 1) hipLaunchKernelGGL(net_bwd_site_taps_kernel<1>, dim3((unsigned)blocks), dim3(kNetNT), 0, st, a, need);
                    else hipLaunchKernelGGL(net_bwd_site_taps_kernel<2>, dim3((unsigned)blocks), dim3(kNetNT), 0, st, a, need);
                } else {
                    if (mt == 1) hipLaunchKernelGGL(net_bwd_site_kernel<1>, dim3((unsigned)blocks), dim3(kNetNT), 0, st, a);
                    else hipLaunchKernelGGL(net_bwd_site_kernel<2>, dim3((unsigned)blocks), dim3(kNetNT), 0, st, a);
                }
                NetWgradArgs wa{rows, partial, cs, nf, u, blocks * kNetWaves, P};
                hipLaunchKernelGGL(net_wgrad_kernel, dim3((unsigned)pairs, kNetGradSplits), dim3(kNetNT), 0, st, wa);
            }
            if (exact && gx) net_gx_gather_launch(taps[m], r, t, need, total, H, W, gx, m > 0 || r > 0, st);
        }
        NetGradOut o;
        int end = 0;
        for (int k = 0; k < 12; ++k) {      // dW_1..dW_6, then db_1..db_6
            const int L = k % 6 + 1;
            end += net_layer_out(nf, u, L) * (k < 6 ? net_layer_in(nf, L) : 1);
            o.p[k] = (k < 6 ? gw : gb)[6 * m + k % 6];
            o.end[k] = end;
        }
        hipLaunchKernelGGL(net_wgrad_reduce_kernel, dim3((unsigned)((P + 255) / 256)), dim3(256), 0, st, partial, P, o);
    }
    return hipGetLastError() == hipSuccess ? MULUT_OK : MULUT_EHIP;
}

extern "C" int mulut_net_stage_backward(const mulut_net_unit *const units[], const char *modes, const float *x, const float *g, int N, int C, int H,
                                        int W, void *ws, long long ws_bytes, float *gx, float *const gw[], float *const gb[], void *stream) {
    return net_backward(units, modes, x, g, N, C, H, W, ws, ws_bytes, gx, gw, gb, stream, false);
}

extern "C" long long mulut_net_backward_exact_ws_bytes(int nf, int u, long long chunk_sites, long long total_sites) {
    using namespace mulut;
    if (total_sites < 1) return MULUT_EINVAL;
    const long long base = mulut_net_backward_ws_bytes(nf, u, chunk_sites);
    if (base < 0) return base;
    if (total_sites >= (1LL << 31)) return MULUT_EUNSUPPORTED;
    return base + net_tap_bytes((total_sites + kNetSites - 1) / kNetSites * kNetSites);
}

extern "C" int mulut_net_stage_backward_exact(const mulut_net_unit *const units[], const char *modes, const float *x, const float *g, int N, int C,
                                              int H, int W, void *ws, long long ws_bytes, float *gx, float *const gw[], float *const gb[],
                                              void *stream) {
    return net_backward(units, modes, x, g, N, C, H, W, ws, ws_bytes, gx, gw, gb, stream, true);
}

extern "C" int mulut_net_gx_gather(int device, char mode, int r, const float *t, long long ts, int N, int C, int H, int W, float *gx, int accumulate,
                                   void *stream) {
    using namespace mulut;
    if (!t || !gx || r < 0 || r > 3) return MULUT_EINVAL;
    const unsigned taps = net_pattern(mode);
    if (taps == 0xffffffffu) return MULUT_EINVAL;
    int total = 0;
    const int rc = net_image_sites(N, C, H, W, 1, &total);
    if (rc != MULUT_OK) return rc;
    if (ts < total) return MULUT_EINVAL;
    if (hipSetDevice(device) != hipSuccess) return MULUT_ENODEVICE;
    net_gx_gather_launch(taps, r, t, ts, total, H, W, gx, accumulate != 0, (hipStream_t)stream);
    return hipGetLastError() == hipSuccess ? MULUT_OK : MULUT_EHIP;
}
