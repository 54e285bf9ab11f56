// net_gx_host.cpp -- the host model of the gather-form input gradient (mulut_net_gx_gather of include/mulut.h) and, with its own main,
// the host halves of the three entry points of the bit-reproducible backward (mulut_amd/csrc/mulut_net_train.hip) against fake_hip.cpp.
//
// The model holds the definition as nested loops that SCATTER in the order pass, plane, k, site: tap k of the site anchored at pixel
// (y0, x0), in rotation r, lies at one pixel of the plane, and a pixel so receives its terms tap by tap and, within a tap, by
// ascending site -- exactly the order of the contract's gather.  Plain float adds; built with -ffp-contract=off.  The index
// arithmetic is restated here in plain C++ (sr/1_train_model.py:33-35: rot90, replicate padding on the bottom and right of the rotated
// image, the pattern's four taps) and shares nothing with the kernels' headers; tests/test_net_exact_cpu.py pins it to torch autograd.
//
// Two builds: -DNET_GX_NO_MAIN as a shared object for ctypes (tests/net_exact_cases.py), and as a program under AddressSanitizer and
// UndefinedBehaviorSanitizer (tests/test_net_exact_cpu.py), where main also checks the scatter against the gather by SEARCH on
// random floats of mixed magnitude, every refusal of the three calls, each decided without a launch, and the launch sequence of an
// exact backward over a workspace of two chunks.  It prints one line per check and exits with the number of unexpected ones.
#include <cstdint>
#include <cstring>

namespace {

// di | dj << 4 per tap a, b, c, d (common/network.py:150-227); 0 for an unknown letter (no pattern is all zeros)
unsigned gx_pattern(char mode) {
    switch (mode) {
        case 's': return 0x11011000u;
        case 'd': return 0x22022000u;
        case 'y': return 0x12211100u;
        case 'e': return 0x33033000u;
        case 'h': return 0x23322200u;
        case 'o': return 0x13312200u;
        default: return 0u;
    }
}

// rot90^r(x)[i][j] = x[y][x] (torch.rot90 over dims 2, 3, counter-clockwise)
void gx_unrot(int r, int i, int j, int H, int W, int &y, int &x) {
    switch (r) {
        case 0: y = i, x = j; break;
        case 1: y = j, x = W - 1 - i; break;
        case 2: y = H - 1 - i, x = W - 1 - j; break;
        default: y = H - 1 - j, x = i; break;
    }
}
void gx_rot(int r, int y, int x, int H, int W, int &i, int &j) {
    switch (r) {
        case 0: i = y, j = x; break;
        case 1: i = W - 1 - x, j = y; break;
        case 2: i = H - 1 - y, j = W - 1 - x; break;
        default: i = x, j = H - 1 - y; break;
    }
}

// the pixel of the un-rotated plane that tap k of the site anchored at pixel (y0, x0) reads in rotation r
int gx_tap_pixel(int H, int W, int r, int y0, int x0, unsigned taps, int k) {
    int i, j, y, x;
    gx_rot(r, y0, x0, H, W, i, j);
    const int Hr = (r & 1) ? W : H, Wr = (r & 1) ? H : W;
    int ii = i + (int)((taps >> (8 * k)) & 15u), jj = j + (int)((taps >> (8 * k + 4)) & 15u);
    if (ii > Hr - 1) ii = Hr - 1;
    if (jj > Wr - 1) jj = Wr - 1;
    gx_unrot(r, ii, jj, H, W, y, x);
    return y * W + x;
}

}  // namespace

// one pass: t = float [4][ts], gx = float [N * C][H * W].  Returns 0, or -1 for an unknown letter / rotation
extern "C" int net_gx_host_pass(char mode, int r, const float *t, long long ts, int N, int C, int H, int W, float *gx, int accumulate) {
    const unsigned taps = gx_pattern(mode);
    if (taps == 0u || r < 0 || r > 3) return -1;
    const long long hw = (long long)H * W, planes = (long long)N * C;
    if (!accumulate)
        for (long long p = 0; p < planes * hw; ++p) gx[p] = 0.0f;
    for (long long plane = 0; plane < planes; ++plane)
        for (int k = 0; k < 4; ++k)
            for (int s = 0; s < (int)hw; ++s) {
                float *dst = gx + plane * hw + gx_tap_pixel(H, W, r, s / W, s % W, taps, k);
                *dst = *dst + t[k * ts + plane * hw + s];
            }
    return 0;
}

// a stage: the passes in the backward's order (mode in the order of `modes`, then r = 0..3), t = float [4 M][4][ts]
extern "C" int net_gx_host_stage(const char *modes, const float *t, long long ts, int N, int C, int H, int W, float *gx) {
    const int M = (int)strlen(modes);
    for (int pass = 0; pass < 4 * M; ++pass)
        if (net_gx_host_pass(modes[pass / 4], pass % 4, t + (long long)pass * 4 * ts, ts, N, C, H, W, gx, pass > 0) != 0) return -1;
    return 0;
}

#ifndef NET_GX_NO_MAIN
#include <cstdlib>

#include "net_host_common.h"

static const float *const kX = (const float *)0x10000000;
static float *const kOut = (float *)0x50000000;
static void *const kWs = (void *)0x70000000;

// the contract as it is written: per pixel, per tap, the sites found by SEARCH in ascending order
static void gather_by_search(char mode, int r, const float *t, long long ts, int N, int C, int H, int W, float *gx, int accumulate) {
    const unsigned taps = gx_pattern(mode);
    const int hw = H * W;
    for (int plane = 0; plane < N * C; ++plane)
        for (int p = 0; p < hw; ++p) {
            float acc = accumulate ? gx[(size_t)plane * hw + p] : 0.0f;
            for (int k = 0; k < 4; ++k)
                for (int s = 0; s < hw; ++s)
                    if (gx_tap_pixel(H, W, r, s / W, s % W, taps, k) == p) acc = acc + t[k * ts + (long long)plane * hw + s];
            gx[(size_t)plane * hw + p] = acc;
        }
}

static void model_case(const char *modes, int N, int C, int H, int W, int slack) {
    const int M = (int)strlen(modes), total = N * C * H * W;
    const long long ts = total + slack;
    std::vector<float> t((size_t)(4 * M) * 4 * (size_t)ts);
    for (auto &v : t) {      // mixed magnitudes: the order of a pixel's adds is visible in the bits
        const float m = rnd();
        v = std::ldexp(m, (int)(rnd() * 20.0f));
    }
    std::vector<float> a((size_t)total, NAN), b((size_t)total, NAN);
    int rc = net_gx_host_stage(modes, t.data(), ts, N, C, H, W, a.data());
    for (int pass = 0; pass < 4 * M; ++pass) gather_by_search(modes[pass / 4], pass % 4, t.data() + (size_t)pass * 4 * (size_t)ts, ts, N, C, H, W, b.data(), pass > 0);
    char what[128];
    snprintf(what, sizeof(what), "model %s %d x %d x %d x %d slack %d: scatter is the gather by search, bit for bit", modes, N, C, H, W, slack);
    check(what, rc == 0 && memcmp(a.data(), b.data(), (size_t)total * sizeof(float)) == 0);
}

int main() {
    using namespace mulut;
    g_seed = 9876u;
    const int shapes[6][4] = {{1, 3, 1, 1}, {1, 1, 1, 9}, {1, 1, 9, 1}, {2, 3, 5, 7}, {1, 1, 33, 17}, {2, 1, 17, 33}};
    for (auto &sh : shapes) {
        model_case("sdyeho", sh[0], sh[1], sh[2], sh[3], 0);
        model_case("oh", sh[0], sh[1], sh[2], sh[3], 128);
    }
    {
        float one[4] = {1, 2, 3, 4}, out = 0;
        check("model refuses an unknown letter and a rotation outside 0..3",
              net_gx_host_pass('x', 0, one, 1, 1, 1, 1, 1, &out, 0) == -1 && net_gx_host_pass('s', 4, one, 1, 1, 1, 1, 1, &out, 0) == -1 &&
                  net_gx_host_pass('s', 0, one, 1, 1, 1, 1, 1, &out, 0) == 0 && out == 10.0f);
    }
    Weights m8, m64;
    make(m8, 8, 2, false);
    make(m64, 64, 4, false);
    mulut_net_unit *t8 = nullptr, *t24 = nullptr, *t24u2 = nullptr, *t64 = nullptr, *plain64 = nullptr;
    expect("create_train nf 8 u 2", mulut_net_unit_create_train(0, 8, 2, &t8), MULUT_OK, "malloc 131072 | memset 131072");
    expect("create_train nf 24 u 4", mulut_net_unit_create_train(0, 24, 4, &t24), MULUT_OK, "malloc 131072 | memset 131072");
    expect("create_train nf 24 u 2", mulut_net_unit_create_train(0, 24, 2, &t24u2), MULUT_OK, "malloc 131072 | memset 131072");
    expect("create_train nf 64 u 4", mulut_net_unit_create_train(0, 64, 4, &t64), MULUT_OK, "malloc 409600 | memset 409600");
    expect("create nf 64 u 4", mulut_net_unit_create(0, 64, 4, m64.wp, m64.bp, &plain64), MULUT_OK, "malloc 212992 | memcpy 212992");
    g_wrong += !t8 || !t24 || !t24u2 || !t64 || !plain64;
    const mulut_net_unit *list[9] = {t64, t64, t64, t64, t64, t64, t64, t64, t64};
    // ---- mulut_net_backward_exact_ws_bytes: the old figure plus 16 bytes per site of the whole pass, rounded up to 128 sites
    const long long p64 = 16LL * 46672 * 4, row64 = 660LL * 4;
    expect("exact_ws_bytes chunk 0", mulut_net_backward_exact_ws_bytes(64, 4, 0, 128), MULUT_EINVAL, "");
    expect("exact_ws_bytes total 0", mulut_net_backward_exact_ws_bytes(64, 4, 128, 0), MULUT_EINVAL, "");
    expect("exact_ws_bytes nf 65", mulut_net_backward_exact_ws_bytes(65, 4, 128, 128), MULUT_EUNSUPPORTED, "");
    expect("exact_ws_bytes u 5", mulut_net_backward_exact_ws_bytes(64, 5, 128, 128), MULUT_EUNSUPPORTED, "");
    expect("exact_ws_bytes 2^31 chunk sites", mulut_net_backward_exact_ws_bytes(64, 4, 1LL << 31, 128), MULUT_EUNSUPPORTED, "");
    expect("exact_ws_bytes 2^31 total sites", mulut_net_backward_exact_ws_bytes(64, 4, 128, 1LL << 31), MULUT_EUNSUPPORTED, "");
    expect("exact_ws_bytes 128, 128", mulut_net_backward_exact_ws_bytes(64, 4, 128, 128), p64 + 128 * row64 + 16 * 128, "");
    expect("exact_ws_bytes 128, 200", mulut_net_backward_exact_ws_bytes(64, 4, 128, 200), p64 + 128 * row64 + 16 * 256, "");
    expect("exact_ws_bytes 129, 73728", mulut_net_backward_exact_ws_bytes(64, 4, 129, 73728), p64 + 256 * row64 + 16 * 73728, "");
    // ---- mulut_net_gx_gather
    const float *kT = kX;
    expect("gather null t", mulut_net_gx_gather(0, 's', 0, nullptr, 128, 1, 1, 8, 8, kOut, 0, nullptr), MULUT_EINVAL, "");
    expect("gather null gx", mulut_net_gx_gather(0, 's', 0, kT, 128, 1, 1, 8, 8, nullptr, 0, nullptr), MULUT_EINVAL, "");
    expect("gather r -1", mulut_net_gx_gather(0, 's', -1, kT, 128, 1, 1, 8, 8, kOut, 0, nullptr), MULUT_EINVAL, "");
    expect("gather r 4", mulut_net_gx_gather(0, 's', 4, kT, 128, 1, 1, 8, 8, kOut, 0, nullptr), MULUT_EINVAL, "");
    expect("gather mode x", mulut_net_gx_gather(0, 'x', 0, kT, 128, 1, 1, 8, 8, kOut, 0, nullptr), MULUT_EINVAL, "");
    expect("gather mode S", mulut_net_gx_gather(0, 'S', 0, kT, 128, 1, 1, 8, 8, kOut, 0, nullptr), MULUT_EINVAL, "");
    for (int v = 0; v >= -1; --v) {
        expect("gather N < 1", mulut_net_gx_gather(0, 's', 0, kT, 128, v, 1, 8, 8, kOut, 0, nullptr), MULUT_EINVAL, "");
        expect("gather C < 1", mulut_net_gx_gather(0, 's', 0, kT, 128, 1, v, 8, 8, kOut, 0, nullptr), MULUT_EINVAL, "");
        expect("gather H < 1", mulut_net_gx_gather(0, 's', 0, kT, 128, 1, 1, v, 8, kOut, 0, nullptr), MULUT_EINVAL, "");
        expect("gather W < 1", mulut_net_gx_gather(0, 's', 0, kT, 128, 1, 1, 8, v, kOut, 0, nullptr), MULUT_EINVAL, "");
    }
    expect("gather ts one short", mulut_net_gx_gather(0, 's', 0, kT, 63, 1, 1, 8, 8, kOut, 0, nullptr), MULUT_EINVAL, "");
    expect("gather 2^31 pixels", mulut_net_gx_gather(0, 's', 0, kT, 1LL << 32, 2, 1, 1 << 15, 1 << 15, kOut, 0, nullptr), MULUT_EUNSUPPORTED, "");
    expect("gather 2^31 pixels a plane", mulut_net_gx_gather(0, 's', 0, kT, 1LL << 32, 1, 1, 1 << 16, 1 << 15, kOut, 0, nullptr), MULUT_EUNSUPPORTED, "");
    expect("gather device 3", mulut_net_gx_gather(3, 's', 0, kT, 128, 1, 1, 8, 8, kOut, 0, nullptr), MULUT_ENODEVICE, "");
    expect("gather s 8 x 8, ts exact", mulut_net_gx_gather(0, 's', 0, kT, 64, 1, 1, 8, 8, kOut, 0, nullptr), MULUT_OK,
           "launch net_gx_gather_kernel grid 1,1,1 block 256,1,1 lds 0");
    expect("gather o 2 x 3 x 65 x 33 r 3 accumulate", mulut_net_gx_gather(0, 'o', 3, kT, 12928, 2, 3, 65, 33, kOut, 1, (void *)0x77), MULUT_OK,
           "launch net_gx_gather_kernel grid 51,1,1 block 256,1,1 lds 0");
    // ---- mulut_net_stage_backward_exact: the refusals of mulut_net_stage_backward
    float *gw[12], *gb[12];
    for (int k = 0; k < 12; ++k) gw[k] = kOut + 4096 * k, gb[k] = kOut + 4096 * (12 + k);
    const long long big = 1LL << 30;
    expect("exact null units", mulut_net_stage_backward_exact(nullptr, "sd", kX, kX, 1, 3, 8, 8, kWs, big, kOut, gw, gb, nullptr), MULUT_EINVAL, "");
    expect("exact null modes", mulut_net_stage_backward_exact(list, nullptr, kX, kX, 1, 3, 8, 8, kWs, big, kOut, gw, gb, nullptr), MULUT_EINVAL, "");
    expect("exact null x", mulut_net_stage_backward_exact(list, "sd", nullptr, kX, 1, 3, 8, 8, kWs, big, kOut, gw, gb, nullptr), MULUT_EINVAL, "");
    expect("exact null g", mulut_net_stage_backward_exact(list, "sd", kX, nullptr, 1, 3, 8, 8, kWs, big, kOut, gw, gb, nullptr), MULUT_EINVAL, "");
    expect("exact null ws", mulut_net_stage_backward_exact(list, "sd", kX, kX, 1, 3, 8, 8, nullptr, big, kOut, gw, gb, nullptr), MULUT_EINVAL, "");
    expect("exact null gw", mulut_net_stage_backward_exact(list, "sd", kX, kX, 1, 3, 8, 8, kWs, big, kOut, nullptr, gb, nullptr), MULUT_EINVAL, "");
    expect("exact null gb", mulut_net_stage_backward_exact(list, "sd", kX, kX, 1, 3, 8, 8, kWs, big, kOut, gw, nullptr, nullptr), MULUT_EINVAL, "");
    expect("exact no mode", mulut_net_stage_backward_exact(list, "", kX, kX, 1, 3, 8, 8, kWs, big, kOut, gw, gb, nullptr), MULUT_EINVAL, "");
    expect("exact nine modes", mulut_net_stage_backward_exact(list, "sdysdysdy", kX, kX, 1, 3, 8, 8, kWs, big, kOut, gw, gb, nullptr), MULUT_EUNSUPPORTED, "");
    expect("exact mode x", mulut_net_stage_backward_exact(list, "sx", kX, kX, 1, 3, 8, 8, kWs, big, kOut, gw, gb, nullptr), MULUT_EINVAL, "");
    {
        const mulut_net_unit *no_stream[2] = {t64, plain64};
        expect("exact of a unit without a backward stream", mulut_net_stage_backward_exact(no_stream, "sd", kX, kX, 1, 3, 8, 8, kWs, big, kOut, gw, gb, nullptr),
               MULUT_EINVAL, "");
        const mulut_net_unit *two_nf[2] = {t8, t24};
        expect("exact units of two nf", mulut_net_stage_backward_exact(two_nf, "sd", kX, kX, 1, 3, 8, 8, kWs, big, kOut, gw, gb, nullptr), MULUT_ESHAPE, "");
        const mulut_net_unit *one_width[2] = {t8, t24u2};      // (those differ in u as well; these only in nf)
        expect("exact units of two nf, one u and one padded width", mulut_net_stage_backward_exact(one_width, "sy", kX, kX, 2, 3, 5, 7, kWs, big, kOut, gw, gb, nullptr),
               MULUT_ESHAPE, "");
        float *hole[12];
        for (int k = 0; k < 12; ++k) hole[k] = gw[k];
        hole[7] = nullptr;
        expect("exact null gw[7]", mulut_net_stage_backward_exact(list, "sd", kX, kX, 1, 3, 8, 8, kWs, big, kOut, hole, gb, nullptr), MULUT_EINVAL, "");
        expect("exact null gb[7]", mulut_net_stage_backward_exact(list, "sd", kX, kX, 1, 3, 8, 8, kWs, big, kOut, gw, hole, nullptr), MULUT_EINVAL, "");
    }
    for (int v = 0; v >= -1; --v) {
        expect("exact C < 1", mulut_net_stage_backward_exact(list, "sd", kX, kX, 1, v, 8, 8, kWs, big, kOut, gw, gb, nullptr), MULUT_EINVAL, "");
        expect("exact H < 1", mulut_net_stage_backward_exact(list, "sd", kX, kX, 1, 3, v, 8, kWs, big, kOut, gw, gb, nullptr), MULUT_EINVAL, "");
    }
    expect("exact 2^31 outputs", mulut_net_stage_backward_exact(list, "sd", kX, kX, 1, 2, 1 << 13, 1 << 13, kWs, big, kOut, gw, gb, nullptr), MULUT_EUNSUPPORTED, "");
    expect("exact misaligned ws", mulut_net_stage_backward_exact(list, "sd", kX, kX, 1, 3, 8, 8, (char *)kWs + 128, big, kOut, gw, gb, nullptr), MULUT_EINVAL, "");
    // 1 x 1 x 10 x 20 = 200 sites: the tap region is that of 256
    const long long smallest = p64 + 16 * 256 + 128 * row64;
    expect("exact smallest workspace is mulut_net_backward_exact_ws_bytes(nf, u, 128, sites)", mulut_net_backward_exact_ws_bytes(64, 4, 128, 200), smallest, "");
    expect("exact ws one byte short", mulut_net_stage_backward_exact(list, "s", kX, kX, 1, 1, 10, 20, kWs, smallest - 1, kOut, gw, gb, nullptr), MULUT_EWORKSPACE, "");
    expect("exact ws of the other backward (no tap region)", mulut_net_stage_backward_exact(list, "s", kX, kX, 1, 1, 10, 20, kWs, p64 + 128 * row64, kOut, gw, gb, nullptr),
           MULUT_EWORKSPACE, "");
    {
        // one mode, 200 sites over a workspace of 128: per rotation two chunks (a site launch and a weight-gradient launch each), then the
        // gather over the 200 pixels; after the four rotations the reduction.  gx NULL: no gather, the other launches the same
        const std::string site = "launch net_bwd_site_taps_kernel<2> grid 1,1,1 block 256,1,1 lds 0", wg = "launch net_wgrad_kernel grid 63,16,1 block 256,1,1 lds 0";
        const std::string gather = "launch net_gx_gather_kernel grid 1,1,1 block 256,1,1 lds 0", reduce = "launch net_wgrad_reduce_kernel grid 183,1,1 block 256,1,1 lds 0";
        std::string with = "memset 2987008", without = "memset 2987008";
        for (int r = 0; r < 4; ++r) {
            with += " | " + site + " | " + wg + " | " + site + " | " + wg + " | " + gather;
            without += " | " + site + " | " + wg + " | " + site + " | " + wg;
        }
        void *real = aligned_alloc(256, (size_t)smallest);      // (the fake hipMemsetAsync writes the partial copies for real)
        expect("exact s 10 x 20 over the smallest workspace", mulut_net_stage_backward_exact(list, "s", kX, kX, 1, 1, 10, 20, real, smallest, kOut, gw, gb, (void *)0x77),
               MULUT_OK, with + " | " + reduce);
        expect("exact s 10 x 20, gx NULL", mulut_net_stage_backward_exact(list, "s", kX, kX, 1, 1, 10, 20, real, smallest, nullptr, gw, gb, nullptr), MULUT_OK,
               without + " | " + reduce);
        free(real);
        // two modes, one chunk: 8 passes of site, weight gradient, gather; a memset and a reduction per mode
        const size_t big_ws = (size_t)(p64 + 16 * 256 + 256 * row64);
        real = aligned_alloc(256, big_ws);
        const std::string site2 = "launch net_bwd_site_taps_kernel<2> grid 2,1,1 block 256,1,1 lds 0";
        std::string two;
        for (int m = 0; m < 2; ++m) {
            two += std::string(m ? " | " : "") + "memset 2987008";
            for (int r = 0; r < 4; ++r) two += " | " + site2 + " | " + wg + " | " + gather;
            two += " | " + reduce;
        }
        expect("exact sd 10 x 20 in one chunk", mulut_net_stage_backward_exact(list, "sd", kX, kX, 1, 1, 10, 20, real, (long long)big_ws, kOut, gw, gb, nullptr), MULUT_OK, two);
        free(real);
    }
    {
        const mulut_net_unit *narrow[1] = {t8};
        const long long p8 = (16LL * net_param_floats(8, 2) * 4 + 255) / 256 * 256, ws8 = p8 + 16 * 128 + 128LL * net_ws_rows(8, 2) * 4;
        void *real = aligned_alloc(256, (size_t)ws8);
        char memset8[64];
        snprintf(memset8, sizeof(memset8), "memset %lld", 16LL * net_param_floats(8, 2) * 4);
        std::string want = memset8;
        for (int r = 0; r < 4; ++r)
            want += " | launch net_bwd_site_taps_kernel<1> grid 1,1,1 block 256,1,1 lds 0 | launch net_wgrad_kernel grid 13,16,1 block 256,1,1 lds 0 | "
                    "launch net_gx_gather_kernel grid 1,1,1 block 256,1,1 lds 0";
        char red[96];
        snprintf(red, sizeof(red), " | launch net_wgrad_reduce_kernel grid %d,1,1 block 256,1,1 lds 0", (net_param_floats(8, 2) + 255) / 256);
        expect("exact y nf 8 on 1 x 3 x 5 x 7", mulut_net_stage_backward_exact(narrow, "y", kX, kX, 1, 3, 5, 7, real, ws8, kOut, gw, gb, nullptr), MULUT_OK, want + red);
        free(real);
    }
    expect("destroy nf 8", mulut_net_unit_destroy(t8), MULUT_OK, "free 131072");
    expect("destroy nf 24", mulut_net_unit_destroy(t24), MULUT_OK, "free 131072");
    expect("destroy nf 24 u 2", mulut_net_unit_destroy(t24u2), MULUT_OK, "free 131072");
    expect("destroy nf 64", mulut_net_unit_destroy(t64), MULUT_OK, "free 409600");
    expect("destroy plain", mulut_net_unit_destroy(plain64), MULUT_OK, "free 212992");
    printf("%d unexpected\n", g_wrong);
    return g_wrong;
}
#endif
