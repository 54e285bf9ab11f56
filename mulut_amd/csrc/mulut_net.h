// mulut_net.h -- the weight stream of mulut_net.hip: what the host packs and the kernels walk, in one place.
//
// A unit is the reference's MuLUTUnit with dense=True (common/network.py:62-105): conv1 4 -> nf, conv2..conv5 densely connected
// (layer L reads the (L-1)*nf features of all layers before it), conv6 5*nf -> u*u, tanh.  The kernels compute Y^T = W * X^T on
// v_mfma_f32_32x32x2_f32: an M-tile is 32 output features, a site tile 32 sites (the lane), and one MFMA ("step") sums over TWO
// input features, one per lane half.  nf is padded to MT = 1 or 2 M-tiles with zero weights and zero biases, u*u to one M-tile.
//
// The result of a step sequence leaves, in register `reg` of lane half h, output feature row(reg, h) = (reg & 3) + 8 * (reg >> 2) + 4 * h
// of the tile.  That register IS the B operand of a later step that sums over the feature pair {row(reg, 0), row(reg, 1)}: the host
// puts W[out][that feature] into the A operand of that step, and no activation ever moves between lanes.
//
// Step order (= stream order): layers 1..5, M-tile mt = 0..MT-1 of the layer, then
//     step 0                 bias: A = bias[out] in lane half 0, 0 in half 1; the kernel's B is 1 in half 0, 0 in half 1
//     layer 1: steps 1, 2    taps (a, b) and (c, d)
//     layers 2..5            for source layer s = 1..L-1, source tile t, reg = 0..15: features s, 32 * t + row(reg, h)
// then layer 6 (one M-tile) in the same way over s = 1..5.  Its 32 physical output rows hold the u*u outputs so that register
// r = 0..7 of lane half h is output o = 8 * h + r (pixel-shuffle order si * u + sj).
// Step g lies at float ((g / 4) * 64 + lane) * 4 + (g & 3): a lane reads four steps with one 16-byte LDS load.  The stream is cut
// into chunks of kNetChunkSteps steps (16 KiB), zero-padded to whole chunks.
#ifndef MULUT_NET_H_
#define MULUT_NET_H_

namespace mulut {

constexpr int kNetWaves = 4, kNetNT = 64 * kNetWaves, kNetTileSites = 32, kNetSites = kNetTileSites * kNetWaves;
constexpr int kNetChunkSteps = 64, kNetChunkFloats = kNetChunkSteps * 64, kNetChunkVec4 = kNetChunkFloats / 4;
constexpr int kNetMaxNf = 64, kNetMaxU = 4;
__host__ __device__ constexpr bool net_unit_ok(int nf, int u) { return nf >= 1 && nf <= kNetMaxNf && u >= 1 && u <= kNetMaxU; }
// input / output features of layer L (1..6): conv(L) is [net_layer_out][net_layer_in]
__host__ __device__ constexpr int net_layer_in(int nf, int L) { return L == 1 ? 4 : (L - 1) * nf; }
__host__ __device__ constexpr int net_layer_out(int nf, int u, int L) { return L == 6 ? u * u : nf; }

__host__ __device__ constexpr int net_row(int reg, int h) { return (reg & 3) + 8 * (reg >> 2) + 4 * h; }
// steps of one M-tile of layer L (1..6), bias step included
__host__ __device__ constexpr int net_layer_steps(int mt_count, int L) { return 1 + (L == 1 ? 2 : 16 * mt_count * (L - 1)); }
// first step of M-tile mt of layer L
__host__ __device__ constexpr int net_step_base(int mt_count, int L, int mt) {
    int g = 0;
    for (int l = 1; l < L; ++l) g += mt_count * net_layer_steps(mt_count, l);
    return g + mt * net_layer_steps(mt_count, L);
}
__host__ __device__ constexpr int net_steps(int mt_count) { return net_step_base(mt_count, 6, 0) + net_layer_steps(mt_count, 6); }
__host__ __device__ constexpr int net_chunks(int mt_count) { return (net_steps(mt_count) + kNetChunkSteps - 1) / kNetChunkSteps; }
__host__ __device__ constexpr int net_tiles(int nf) { return nf <= 32 ? 1 : 2; }
__host__ __device__ constexpr long long net_stream_floats(int mt_count) { return (long long)net_chunks(mt_count) * kNetChunkFloats; }
__host__ __device__ constexpr long long net_step_float(int g, int lane) { return ((long long)(g >> 2) * 64 + lane) * 4 + (g & 3); }

// ---- the backward stream (mulut_net_train.hip): the transposed weights in the same step format, for G^T = W^T * D^T.
//
// delta of layer L = 1..5 leaves its MFMA in register `reg` of lane half h as feature 32 * mt + net_row(reg, h) of M-tile mt, in the
// layout of x; delta of layer 6 is made in registers 0..7 of both halves, register r of half h being output 8 * h + r.  Either is the
// B operand of a step that sums over that pair of OUTPUTS of layer L, and the A operand of that step is W_L[out of half h][input
// feature i of the source tile] in lane (i, h).  The result tile is the gradient of the source tile (s, t) in the layout of x[s][t],
// so the ReLU mask x > 0 is applied register by register.
//
// Step order: source layers s = 5, 4, ..., 1 (delta_s needs every delta_L, L > s), source tile t = 0..MT-1 of the layer, then
//     steps 0..7             layer 6: reg = 0..7, A = W_6[8 * h + reg][(s - 1) * nf + 32 * t + i]
//     then L = 5, ..., s + 1 for M-tile mt of layer L, reg = 0..15: A = W_L[32 * mt + row(reg, h)][(s - 1) * nf + 32 * t + i]
// and last the tap gradient W_1^T * delta_1: M-tile mt, reg = 0..15, A = W_1[32 * mt + row(reg, h)][i] for i < 4 -- taps a..d arrive
// in registers 0..3 of lane half 0.  No bias steps.  Float position, chunking and zero padding are the forward stream's.
__host__ __device__ constexpr int net_bwd_tile_steps(int mt_count, int s) { return 8 + 16 * mt_count * (5 - s); }
// first step of source tile t of source layer s (5..1); s = 0: the tap-gradient steps
__host__ __device__ constexpr int net_bwd_step_base(int mt_count, int s, int t) {
    int g = 0;
    for (int l = 5; l > s; --l) g += mt_count * net_bwd_tile_steps(mt_count, l);
    return g + (s > 0 ? t * net_bwd_tile_steps(mt_count, s) : 0);
}
__host__ __device__ constexpr int net_bwd_steps(int mt_count) { return net_bwd_step_base(mt_count, 0, 0) + 16 * mt_count; }
__host__ __device__ constexpr int net_bwd_chunks(int mt_count) { return (net_bwd_steps(mt_count) + kNetChunkSteps - 1) / kNetChunkSteps; }
__host__ __device__ constexpr long long net_bwd_stream_floats(int mt_count) { return (long long)net_bwd_chunks(mt_count) * kNetChunkFloats; }

// What both streams hold at (step g, lane), computed rather than scattered: these two functions ARE the streams' definition.  The device
// pack runs one thread per float of a stream and the host packs, net_pack and net_pack_bwd below, are loops over them.  w[l] / b[l] are conv(l+1) as
// [out][in] / [out]; the backward stream reads no bias.
struct NetParams {
    const float *w[6], *b[6];
};
// false if a pointer is missing
inline bool net_have_params(const float *const w[6], const float *const b[6]) {
    if (!w || !b) return false;
    for (int l = 0; l < 6; ++l)
        if (!w[l] || !b[l]) return false;
    return true;
}
// (Both spell a layer's input features out, 4 or (L - 1) * nf, and do not call net_layer_in: net_pack_kernel inlines them, and with
// the call its instructions are no longer the ones that were measured.)
__host__ __device__ inline float net_fwd_value(int nf, int u, int MT, int g, int lane, const NetParams &p) {
    const int i = lane & 31, h = lane >> 5;
    int base = 0;
    for (int L = 1; L <= 6; ++L) {
        const int tiles = L == 6 ? 1 : MT, ls = net_layer_steps(MT, L);
        if (g >= base + tiles * ls) {
            base += tiles * ls;
            continue;
        }
        const int mt = (g - base) / ls, k = (g - base) % ls, in_f = L == 1 ? 4 : (L - 1) * nf;
        int out_row;
        if (L < 6) {
            out_row = mt * 32 + i < nf ? mt * 32 + i : -1;
        } else {
            const int hh = (i >> 2) & 1, r = (i & 3) + 4 * (i >> 3);      // i = net_row(r, hh)
            out_row = r < 8 && 8 * hh + r < u * u ? 8 * hh + r : -1;
        }
        if (out_row < 0) return 0.0f;
        if (k == 0) return h == 0 ? p.b[L - 1][out_row] : 0.0f;
        if (L == 1) return p.w[0][out_row * 4 + 2 * (k - 1) + h];
        const int s = (k - 1) / (MT * 16), t = ((k - 1) / 16) % MT, f = t * 32 + net_row((k - 1) % 16, h);
        return f < nf ? p.w[L - 1][(long long)out_row * in_f + s * nf + f] : 0.0f;
    }
    return 0.0f;      // the tail of the last chunk
}
__host__ __device__ inline float net_bwd_value(int nf, int u, int MT, int g, int lane, const NetParams &p) {
    const int i = lane & 31, h = lane >> 5;
    int base = 0;
    for (int s = 5; s >= 1; --s) {
        const int ts = net_bwd_tile_steps(MT, s);
        if (g >= base + MT * ts) {
            base += MT * ts;
            continue;
        }
        const int t = (g - base) / ts, k = (g - base) % ts, f = 32 * t + i;
        if (f >= nf) return 0.0f;
        const int col = (s - 1) * nf + f;
        if (k < 8) return 8 * h + k < u * u ? p.w[5][(long long)(8 * h + k) * (5 * nf) + col] : 0.0f;
        const int L = 5 - (k - 8) / (MT * 16), mt = ((k - 8) / 16) % MT, orow = 32 * mt + net_row((k - 8) % 16, h);
        return orow < nf ? p.w[L - 1][(long long)orow * ((L - 1) * nf) + col] : 0.0f;
    }
    if (g < base + 16 * MT && i < 4) {
        const int orow = 32 * ((g - base) / 16) + net_row((g - base) % 16, h);
        return orow < nf ? p.w[0][orow * 4 + i] : 0.0f;
    }
    return 0.0f;
}
// the host packs, each a loop over its stream's function: `out` has net_stream_floats / net_bwd_stream_floats(net_tiles(nf)) floats
inline void net_pack(int nf, int u, const float *const w[6], const float *const b[6], float *out) {
    const int MT = net_tiles(nf);
    NetParams p;
    for (int l = 0; l < 6; ++l) p.w[l] = w[l], p.b[l] = b[l];
    for (int g = 0; g < net_chunks(MT) * kNetChunkSteps; ++g)
        for (int lane = 0; lane < 64; ++lane) out[net_step_float(g, lane)] = net_fwd_value(nf, u, MT, g, lane, p);
}
inline void net_pack_bwd(int nf, int u, const float *const w[6], float *out) {
    const int MT = net_tiles(nf);
    NetParams p;
    for (int l = 0; l < 6; ++l) p.w[l] = w[l], p.b[l] = nullptr;
    for (int g = 0; g < net_bwd_chunks(MT) * kNetChunkSteps; ++g)
        for (int lane = 0; lane < 64; ++lane) out[net_step_float(g, lane)] = net_bwd_value(nf, u, MT, g, lane, p);
}

// ---- the workspace of the backward (mulut_net_train.hip), one (mode, rotation) pass of a chunk of `cs` sites (a multiple of 128):
// float [rows][cs], a row being one feature and the site the fast index, behind kNetGradSplits partial copies of the unit's gradient.
//     rows 0..3                          taps a..d                     (xcat of layer 1)
//     rows 4 + (s - 1) * nf + f          x_s[f], s = 1..5              (xcat of layer L >= 2 is rows 4 .. 4 + (L - 1) * nf)
//     rows 4 + 5 * nf + (L - 1) * nf + f delta_L[f], L = 1..5
//     rows 4 + 10 * nf + o               delta_6[o], o < u * u
// The site kernel's wave writes, per register, 32 consecutive sites of two rows: two whole 128-byte lines.  The weight-gradient kernel's
// wave reads 32 consecutive sites of 32 rows per operand and step group: a lane takes 16 sites of its row (64 bytes, lane half h the
// sites 16 * h ..) as four 16-byte loads, and MFMA v * 4 + c of the group contracts sites 4 * v + c and 16 + 4 * v + c -- the order of a
// sum's terms is free as long as both operands agree on it.
// (mulut_net_stage_backward_exact puts the tap buffer of a whole pass, float [4][sites rounded up to 128], between the partial copies
// and the rows: include/mulut.h.)
constexpr int kNetGradSplits = 16;
__host__ __device__ constexpr int net_ws_rows(int nf, int u) { return 4 + 10 * nf + u * u; }
// floats of one copy of a unit's gradient: dW_1..dW_6 as [out][in], then db_1..db_6
__host__ __device__ constexpr int net_param_floats(int nf, int u) {
    int n = 0;
    for (int L = 1; L <= 6; ++L) n += net_layer_out(nf, u, L) * (net_layer_in(nf, L) + 1);
    return n;
}

}  // namespace mulut
#endif
