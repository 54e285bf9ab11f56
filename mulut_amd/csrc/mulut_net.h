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

// the host pack (mulut_net.hip): `out` has net_stream_floats(net_tiles(nf)) floats; w[l] / b[l] are conv(l+1) as [out][in] / [out]
void net_pack(int nf, int u, const float *const w[6], const float *const b[6], float *out);

}  // namespace mulut
#endif
