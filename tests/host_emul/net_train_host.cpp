// net_train_host.cpp -- the host half of the training entry points (mulut_amd/csrc/mulut_net_train.hip) on the CPU against fake_hip.cpp:
// the backward stream (net_bwd_value of mulut_net.h, through the host pack) walked as net_bwd_site_kernel's MFMA sequence walks it
// against plain transposed matrices -- the forward stream has the same single definition, net_fwd_value, and net_host.cpp walks what
// it produces against a plain-loop MLP over nf {1, 8, 24, 32, 33, 64} x u 1..4, so no forward comparison is made here; every
// refusal of the six calls, each decided without touching the device; what a training unit allocates and frees; and the launch
// sequence of a backward over a workspace of two chunks.  tests/test_net_train_cpu.py builds it under AddressSanitizer and
// UndefinedBehaviorSanitizer and runs it as a program; it prints one line per check and exits with the number of lines that are not
// what this file expects.  No kernel runs, so the device pointers are made-up addresses that nothing follows.
#include <cstdlib>

#include "net_host_common.h"

static const float *const kX = (const float *)0x10000000;
static float *const kOut = (float *)0x50000000;
static void *const kWs = (void *)0x70000000;

static void pack_case(int nf, int u) {
    using namespace mulut;
    Weights m;
    make(m, nf, u, false);
    const int MT = net_tiles(nf);
    // ---- the stream walked step by step against plain transposed matrices, for one vector of deltas
    std::vector<float> bw((size_t)net_bwd_stream_floats(MT));
    net_pack_bwd(nf, u, m.wp, bw.data());
    std::vector<double> delta[6];
    for (int l = 0; l < 6; ++l) {
        delta[l].resize(l == 5 ? (size_t)u * u : (size_t)nf);
        for (auto &v : delta[l]) v = rnd();
    }
    // B operand of a step: register reg of lane half h of delta_L's tile mt is feature 32 mt + row(reg, h), 0 on padding
    auto dval = [&](int L, int mt, int reg, int h) {
        if (L == 6) return reg < 8 && 8 * h + reg < u * u ? delta[5][(size_t)(8 * h + reg)] : 0.0;
        const int f = 32 * mt + net_row(reg, h);
        return f < nf ? delta[L - 1][(size_t)f] : 0.0;
    };
    double worst = 0;
    for (int s = 5; s >= 0; --s)
        for (int t = 0; t < (s == 0 ? 1 : MT); ++t) {
            double acc[32] = {0};
            const int base = net_bwd_step_base(MT, s, t);
            auto step = [&](int g, double b0, double b1) {
                for (int i = 0; i < 32; ++i)
                    acc[i] += (double)bw[(size_t)net_step_float(g, i)] * b0 + (double)bw[(size_t)net_step_float(g, i + 32)] * b1;
            };
            if (s > 0) {
                for (int reg = 0; reg < 8; ++reg) step(base + reg, dval(6, 0, reg, 0), dval(6, 0, reg, 1));
                for (int k = 0; k < (5 - s) * MT * 16; ++k) {
                    const int L = 5 - k / (MT * 16), mt = (k / 16) % MT, reg = k % 16;
                    step(base + 8 + k, dval(L, mt, reg, 0), dval(L, mt, reg, 1));
                }
            } else {
                for (int k = 0; k < MT * 16; ++k) step(base + k, dval(1, k / 16, k % 16, 0), dval(1, k / 16, k % 16, 1));
            }
            for (int i = 0; i < 32; ++i) {      // row i of the result tile: input feature 32 t + i of source layer s (or tap i)
                double want = 0;
                if (s == 0) {
                    if (i < 4)
                        for (int o = 0; o < nf; ++o) want += (double)m.w[0][(size_t)o * 4 + i] * delta[0][(size_t)o];
                } else if (32 * t + i < nf) {
                    const int col = (s - 1) * nf + 32 * t + i;
                    for (int L = s + 1; L <= 6; ++L) {
                        const int in = (L - 1) * nf, out = L == 6 ? u * u : nf;
                        for (int o = 0; o < out; ++o) want += (double)m.w[L - 1][(size_t)o * in + col] * delta[L - 1][(size_t)o];
                    }
                }
                worst = std::fmax(worst, std::fabs(want - acc[i]));
            }
        }
    size_t nonzero = 0, want_nonzero = 0;
    for (float v : bw) nonzero += v != 0.0f;
    for (int l = 0; l < 6; ++l)
        for (float v : m.w[l]) want_nonzero += v != 0.0f;
    // (every weight appears exactly once: W_1 in the tap steps, W_L (L >= 2) once per source block; biases nowhere)
    char what[128];
    snprintf(what, sizeof(what), "pack nf %d u %d: backward %d steps in %d chunks, worst |walk - plain| %.2e", nf, u, net_bwd_steps(MT), net_bwd_chunks(MT), worst);
    // double sums of at most 330 products of float values below 1: 330 * 2^-53
    check(what, worst < 1e-12 && nonzero == want_nonzero);
}

int main() {
    using namespace mulut;
    g_seed = 4321u;
    check("backward steps at one tile 216, at two 752", net_bwd_steps(1) == 216 && net_bwd_steps(2) == 752 && net_bwd_chunks(1) == 4 && net_bwd_chunks(2) == 12);
    check("workspace rows and gradient floats at nf 64 u 4", net_ws_rows(64, 4) == 660 && net_param_floats(64, 4) == 46672);
    for (int nf : {1, 8, 24, 32, 33, 64})
        for (int u : {1, 2, 3, 4}) pack_case(nf, u);
    Weights m8, m64;
    make(m8, 8, 2, false);
    make(m64, 64, 4, false);
    mulut_net_unit *unit = (mulut_net_unit *)0x1, *t8 = nullptr, *t64 = nullptr, *t64b = nullptr, *t24 = nullptr, *t24u2 = nullptr, *plain64 = nullptr;
    // ---- mulut_net_unit_create_train
    expect("create_train null out", mulut_net_unit_create_train(0, 8, 2, nullptr), MULUT_EINVAL, "");
    expect("create_train nf 0", mulut_net_unit_create_train(0, 0, 2, &unit), MULUT_EUNSUPPORTED, "");
    expect("create_train nf 65", mulut_net_unit_create_train(0, 65, 2, &unit), MULUT_EUNSUPPORTED, "");
    expect("create_train u 0", mulut_net_unit_create_train(0, 8, 0, &unit), MULUT_EUNSUPPORTED, "");
    expect("create_train u 5", mulut_net_unit_create_train(0, 8, 5, &unit), MULUT_EUNSUPPORTED, "");
    expect("create_train device 3", mulut_net_unit_create_train(3, 8, 2, &unit), MULUT_ENODEVICE, "");
    g_wrong += unit != nullptr;
    // both streams in one allocation: 4 + 4 chunks of 16 KiB at one tile, 13 + 12 at two
    expect("create_train nf 8 u 2", mulut_net_unit_create_train(0, 8, 2, &t8), MULUT_OK, "malloc 131072 | memset 131072");
    expect("create_train nf 64 u 4", mulut_net_unit_create_train(0, 64, 4, &t64), MULUT_OK, "malloc 409600 | memset 409600");
    expect("create_train nf 64 u 4 again", mulut_net_unit_create_train(0, 64, 4, &t64b), MULUT_OK, "malloc 409600 | memset 409600");
    expect("create_train nf 24 u 4", mulut_net_unit_create_train(0, 24, 4, &t24), MULUT_OK, "malloc 131072 | memset 131072");
    expect("create_train nf 24 u 2", mulut_net_unit_create_train(0, 24, 2, &t24u2), MULUT_OK, "malloc 131072 | memset 131072");
    expect("create nf 64 u 4", mulut_net_unit_create(0, 64, 4, m64.wp, m64.bp, &plain64), MULUT_OK, "malloc 212992 | memcpy 212992");
    g_wrong += !t8 || !t64 || !t64b || !t24 || !t24u2 || !plain64;
    // ---- mulut_net_unit_load_dev (the pointers are device pointers: nothing follows them here)
    expect("load_dev null unit", mulut_net_unit_load_dev(nullptr, m8.wp, m8.bp, nullptr), MULUT_EINVAL, "");
    expect("load_dev null w", mulut_net_unit_load_dev(t8, nullptr, m8.bp, nullptr), MULUT_EINVAL, "");
    expect("load_dev null b", mulut_net_unit_load_dev(t8, m8.wp, nullptr, nullptr), MULUT_EINVAL, "");
    for (int l = 0; l < 6; ++l) {
        const float *wp[6], *bp[6];
        for (int k = 0; k < 6; ++k) wp[k] = m8.wp[k], bp[k] = m8.bp[k];
        wp[l] = nullptr;
        expect("load_dev null w[l]", mulut_net_unit_load_dev(t8, wp, bp, nullptr), MULUT_EINVAL, "");
        wp[l] = m8.wp[l];
        bp[l] = nullptr;
        expect("load_dev null b[l]", mulut_net_unit_load_dev(t8, wp, bp, nullptr), MULUT_EINVAL, "");
    }
    expect("load_dev nf 8", mulut_net_unit_load_dev(t8, m8.wp, m8.bp, nullptr), MULUT_OK, "launch net_pack_kernel grid 128,1,1 block 256,1,1 lds 0");
    expect("load_dev nf 64", mulut_net_unit_load_dev(t64, m64.wp, m64.bp, (void *)0x77), MULUT_OK, "launch net_pack_kernel grid 400,1,1 block 256,1,1 lds 0");
    expect("load_dev of a unit without a backward stream", mulut_net_unit_load_dev(plain64, m64.wp, m64.bp, nullptr), MULUT_OK,
           "launch net_pack_kernel grid 208,1,1 block 256,1,1 lds 0");
    // ---- mulut_net_pack_host / mulut_net_unit_read
    std::vector<float> buf(1 << 17);
    expect("pack_host null w", mulut_net_pack_host(8, 2, nullptr, m8.bp, 0, buf.data(), (long long)buf.size()), MULUT_EINVAL, "");
    expect("pack_host null out", mulut_net_pack_host(8, 2, m8.wp, m8.bp, 0, nullptr, (long long)buf.size()), MULUT_EINVAL, "");
    expect("pack_host which 2", mulut_net_pack_host(8, 2, m8.wp, m8.bp, 2, buf.data(), (long long)buf.size()), MULUT_EINVAL, "");
    expect("pack_host nf 65", mulut_net_pack_host(65, 2, m8.wp, m8.bp, 0, buf.data(), (long long)buf.size()), MULUT_EUNSUPPORTED, "");
    expect("pack_host small cap", mulut_net_pack_host(8, 2, m8.wp, m8.bp, 1, buf.data(), 16383), MULUT_EWORKSPACE, "");
    expect("pack_host forward", mulut_net_pack_host(8, 2, m8.wp, m8.bp, 0, buf.data(), (long long)buf.size()), 16384, "");
    expect("pack_host backward", mulut_net_pack_host(64, 4, m64.wp, m64.bp, 1, buf.data(), (long long)buf.size()), 12 * 4096, "");
    expect("read null unit", mulut_net_unit_read(nullptr, 0, buf.data(), (long long)buf.size()), MULUT_EINVAL, "");
    expect("read null host", mulut_net_unit_read(t8, 0, nullptr, (long long)buf.size()), MULUT_EINVAL, "");
    expect("read which 2", mulut_net_unit_read(t8, 2, buf.data(), (long long)buf.size()), MULUT_EINVAL, "");
    expect("read backward of a unit without", mulut_net_unit_read(plain64, 1, buf.data(), (long long)buf.size()), MULUT_EINVAL, "");
    expect("read small cap", mulut_net_unit_read(t8, 1, buf.data(), 100), MULUT_EWORKSPACE, "");
    expect("read backward nf 8", mulut_net_unit_read(t8, 1, buf.data(), (long long)buf.size()), 16384, "wait device | memcpy 65536");
    // ---- mulut_net_stage_sum
    const mulut_net_unit *list[9] = {t64, t64b, t64, t64, t64, t64, t64, t64, t64};
    expect("sum null units", mulut_net_stage_sum(nullptr, "sd", kX, 1, 3, 8, 8, kOut, nullptr), MULUT_EINVAL, "");
    expect("sum null modes", mulut_net_stage_sum(list, nullptr, kX, 1, 3, 8, 8, kOut, nullptr), MULUT_EINVAL, "");
    expect("sum null x", mulut_net_stage_sum(list, "sd", nullptr, 1, 3, 8, 8, kOut, nullptr), MULUT_EINVAL, "");
    expect("sum null pred", mulut_net_stage_sum(list, "sd", kX, 1, 3, 8, 8, nullptr, nullptr), MULUT_EINVAL, "");
    expect("sum no mode", mulut_net_stage_sum(list, "", kX, 1, 3, 8, 8, kOut, nullptr), MULUT_EINVAL, "");
    expect("sum nine modes", mulut_net_stage_sum(list, "sdysdysdy", kX, 1, 3, 8, 8, kOut, nullptr), MULUT_EUNSUPPORTED, "");
    expect("sum mode x", mulut_net_stage_sum(list, "sx", kX, 1, 3, 8, 8, kOut, nullptr), MULUT_EINVAL, "");
    {
        const mulut_net_unit *hole[2] = {t64, nullptr};
        expect("sum null unit in the list", mulut_net_stage_sum(hole, "sd", kX, 1, 3, 8, 8, kOut, nullptr), MULUT_EINVAL, "");
        const mulut_net_unit *mixed_w[2] = {t64, t8};
        expect("sum units of two widths", mulut_net_stage_sum(mixed_w, "sd", kX, 1, 3, 8, 8, kOut, nullptr), MULUT_ESHAPE, "");
        const mulut_net_unit *mixed_u[2] = {t24u2, t24};
        expect("sum units of two u", mulut_net_stage_sum(mixed_u, "sd", kX, 1, 3, 8, 8, kOut, nullptr), MULUT_ESHAPE, "");
        const mulut_net_unit *one_width[2] = {t8, t24u2};      // nf 8 and nf 24: one u, one padded width -- the forward takes them
        expect("sum units of two nf under one padded width", mulut_net_stage_sum(one_width, "sy", kX, 2, 3, 5, 7, kOut, nullptr), MULUT_OK,
               "launch net_stage_sum_kernel<1, 2> grid 2,1,1 block 256,1,1 lds 0");
    }
    for (int v = 0; v >= -1; --v) {
        expect("sum N < 1", mulut_net_stage_sum(list, "sd", kX, v, 3, 8, 8, kOut, nullptr), MULUT_EINVAL, "");
        expect("sum W < 1", mulut_net_stage_sum(list, "sd", kX, 1, 3, 8, v, kOut, nullptr), MULUT_EINVAL, "");
    }
    expect("sum 2^31 outputs", mulut_net_stage_sum(list, "sd", kX, 1, 2, 1 << 13, 1 << 13, kOut, nullptr), MULUT_EUNSUPPORTED, "");
    expect("sum sd 65 x 33 x 3 x 2", mulut_net_stage_sum(list, "sd", kX, 2, 3, 65, 33, kOut, nullptr), MULUT_OK,
           "launch net_stage_sum_kernel<2, 4> grid 101,1,1 block 256,1,1 lds 0");
    {
        const mulut_net_unit *narrow[1] = {t8};
        expect("sum y nf 8", mulut_net_stage_sum(narrow, "y", kX, 1, 3, 5, 7, kOut, (void *)0x77), MULUT_OK,
               "launch net_stage_sum_kernel<1, 2> grid 1,1,1 block 256,1,1 lds 0");
        const mulut_net_unit *mixed[1] = {plain64};      // a forward needs no backward stream
        expect("sum of a unit of mulut_net_unit_create", mulut_net_stage_sum(mixed, "s", kX, 1, 1, 1, 1, kOut, nullptr), MULUT_OK,
               "launch net_stage_sum_kernel<2, 4> grid 1,1,1 block 256,1,1 lds 0");
    }
    // ---- mulut_net_backward_ws_bytes: 16 copies of the gradient (rounded up to 256 bytes) + rows x sites rounded up to 128
    expect("ws_bytes sites 0", mulut_net_backward_ws_bytes(64, 4, 0), MULUT_EINVAL, "");
    expect("ws_bytes nf 65", mulut_net_backward_ws_bytes(65, 4, 128), MULUT_EUNSUPPORTED, "");
    expect("ws_bytes u 5", mulut_net_backward_ws_bytes(64, 5, 128), MULUT_EUNSUPPORTED, "");
    expect("ws_bytes 2^31 sites", mulut_net_backward_ws_bytes(64, 4, 1LL << 31), MULUT_EUNSUPPORTED, "");
    const long long p64 = 16LL * 46672 * 4, row64 = 660LL * 4;
    expect("ws_bytes nf 64 u 4 sites 1", mulut_net_backward_ws_bytes(64, 4, 1), p64 + 128 * row64, "");
    expect("ws_bytes nf 64 u 4 sites 129", mulut_net_backward_ws_bytes(64, 4, 129), p64 + 256 * row64, "");
    // ---- mulut_net_stage_backward
    float *gw[12], *gb[12];
    for (int k = 0; k < 12; ++k) gw[k] = kOut + 4096 * k, gb[k] = kOut + 4096 * (12 + k);
    const long long big = 1LL << 30;
    expect("backward null units", mulut_net_stage_backward(nullptr, "sd", kX, kX, 1, 3, 8, 8, kWs, big, kOut, gw, gb, nullptr), MULUT_EINVAL, "");
    expect("backward null modes", mulut_net_stage_backward(list, nullptr, kX, kX, 1, 3, 8, 8, kWs, big, kOut, gw, gb, nullptr), MULUT_EINVAL, "");
    expect("backward null x", mulut_net_stage_backward(list, "sd", nullptr, kX, 1, 3, 8, 8, kWs, big, kOut, gw, gb, nullptr), MULUT_EINVAL, "");
    expect("backward null g", mulut_net_stage_backward(list, "sd", kX, nullptr, 1, 3, 8, 8, kWs, big, kOut, gw, gb, nullptr), MULUT_EINVAL, "");
    expect("backward null ws", mulut_net_stage_backward(list, "sd", kX, kX, 1, 3, 8, 8, nullptr, big, kOut, gw, gb, nullptr), MULUT_EINVAL, "");
    expect("backward null gw", mulut_net_stage_backward(list, "sd", kX, kX, 1, 3, 8, 8, kWs, big, kOut, nullptr, gb, nullptr), MULUT_EINVAL, "");
    expect("backward null gb", mulut_net_stage_backward(list, "sd", kX, kX, 1, 3, 8, 8, kWs, big, kOut, gw, nullptr, nullptr), MULUT_EINVAL, "");
    expect("backward no mode", mulut_net_stage_backward(list, "", kX, kX, 1, 3, 8, 8, kWs, big, kOut, gw, gb, nullptr), MULUT_EINVAL, "");
    expect("backward nine modes", mulut_net_stage_backward(list, "sdysdysdy", kX, kX, 1, 3, 8, 8, kWs, big, kOut, gw, gb, nullptr), MULUT_EUNSUPPORTED, "");
    expect("backward mode x", mulut_net_stage_backward(list, "sx", kX, kX, 1, 3, 8, 8, kWs, big, kOut, gw, gb, nullptr), MULUT_EINVAL, "");
    {
        const mulut_net_unit *no_stream[2] = {t64, plain64};
        expect("backward of a unit without a backward stream", mulut_net_stage_backward(no_stream, "sd", kX, kX, 1, 3, 8, 8, kWs, big, kOut, gw, gb, nullptr),
               MULUT_EINVAL, "");
        const mulut_net_unit *two_nf[2] = {t8, t24};      // one feature tile each, yet different rows in the workspace
        expect("backward units of two nf", mulut_net_stage_backward(two_nf, "sd", kX, kX, 1, 3, 8, 8, kWs, big, kOut, gw, gb, nullptr), MULUT_ESHAPE, "");
        const mulut_net_unit *one_width[2] = {t8, t24u2};      // (those differ in u as well; these only in nf)
        expect("backward units of two nf, one u and one padded width", mulut_net_stage_backward(one_width, "sy", kX, kX, 2, 3, 5, 7, kWs, big, kOut, gw, gb, nullptr),
               MULUT_ESHAPE, "");
        float *hole[12];
        for (int k = 0; k < 12; ++k) hole[k] = gw[k];
        hole[7] = nullptr;
        expect("backward null gw[7]", mulut_net_stage_backward(list, "sd", kX, kX, 1, 3, 8, 8, kWs, big, kOut, hole, gb, nullptr), MULUT_EINVAL, "");
        expect("backward null gb[7]", mulut_net_stage_backward(list, "sd", kX, kX, 1, 3, 8, 8, kWs, big, kOut, gw, hole, nullptr), MULUT_EINVAL, "");
    }
    for (int v = 0; v >= -1; --v) {
        expect("backward C < 1", mulut_net_stage_backward(list, "sd", kX, kX, 1, v, 8, 8, kWs, big, kOut, gw, gb, nullptr), MULUT_EINVAL, "");
        expect("backward H < 1", mulut_net_stage_backward(list, "sd", kX, kX, 1, 3, v, 8, kWs, big, kOut, gw, gb, nullptr), MULUT_EINVAL, "");
    }
    expect("backward 2^31 outputs", mulut_net_stage_backward(list, "sd", kX, kX, 1, 2, 1 << 13, 1 << 13, kWs, big, kOut, gw, gb, nullptr), MULUT_EUNSUPPORTED, "");
    expect("backward misaligned ws", mulut_net_stage_backward(list, "sd", kX, kX, 1, 3, 8, 8, (char *)kWs + 128, big, kOut, gw, gb, nullptr), MULUT_EINVAL, "");
    expect("backward ws one byte short", mulut_net_stage_backward(list, "sd", kX, kX, 1, 3, 8, 8, kWs, p64 + 128 * row64 - 1, kOut, gw, gb, nullptr),
           MULUT_EWORKSPACE, "");
    {
        // one mode, 1 x 1 x 10 x 20 = 200 sites over a workspace of 128: per rotation two chunks (one workgroup each: 128 and 72 sites),
        // each a site launch and a weight-gradient launch over the 63 (out tile, in tile) pairs of nf 64 u 4; then the reduction
        const std::string site = "launch net_bwd_site_kernel<2> grid 1,1,1 block 256,1,1 lds 0", wg = "launch net_wgrad_kernel grid 63,16,1 block 256,1,1 lds 0";
        std::string want = "memset 2987008";
        for (int k = 0; k < 8; ++k) want += " | " + site + " | " + wg;
        want += " | launch net_wgrad_reduce_kernel grid 183,1,1 block 256,1,1 lds 0";
        void *real = aligned_alloc(256, (size_t)(p64 + 128 * row64));      // (the fake hipMemsetAsync writes the partial copies for real)
        expect("backward s 10 x 20 over the smallest workspace", mulut_net_stage_backward(list, "s", kX, kX, 1, 1, 10, 20, real, p64 + 128 * row64, nullptr, gw, gb, (void *)0x77),
               MULUT_OK, want);
        free(real);
    }
    // ---- destroy: one allocation each
    expect("destroy nf 8", mulut_net_unit_destroy(t8), MULUT_OK, "free 131072");
    expect("destroy nf 64", mulut_net_unit_destroy(t64), MULUT_OK, "free 409600");
    expect("destroy nf 64", mulut_net_unit_destroy(t64b), MULUT_OK, "free 409600");
    expect("destroy nf 24", mulut_net_unit_destroy(t24), MULUT_OK, "free 131072");
    expect("destroy nf 24 u 2", mulut_net_unit_destroy(t24u2), MULUT_OK, "free 131072");
    expect("destroy plain", mulut_net_unit_destroy(plain64), MULUT_OK, "free 212992");
    printf("%d unexpected\n", g_wrong);
    return g_wrong;
}
