// net_host.cpp -- the host half of mulut_net_* (mulut_amd/csrc/mulut_net.hip) on the CPU against fake_hip.cpp: the weight pack walked
// step by step as the kernel's MFMA sequence walks it (mulut_net.h) against a plain-loop evaluation of the same MLP; the zero padding
// of a narrow unit; every refusal of the five calls, each decided without touching the device; what a unit allocates, copies and
// frees; and the launch configurations of the three forms.  tests/test_net_cpu.py builds it under AddressSanitizer and
// UndefinedBehaviorSanitizer and runs it as a program; it prints one line per check and exits with the number of lines that are not
// what this file expects.  No kernel runs, so the image pointers are made-up addresses that nothing follows.
#include "net_host_common.h"

static const uint8_t *const kIn = (const uint8_t *)0x10000000;
static uint8_t *const kOut = (uint8_t *)0x50000000;

// common/network.py:62-105 as plain loops, in double
static void plain(const Weights &m, const float t[4], double *y) {
    std::vector<double> x(t, t + 4), feat;
    for (int l = 0; l < 6; ++l) {
        const int in = l == 0 ? 4 : l * m.nf, out = l == 5 ? m.u * m.u : m.nf;
        const std::vector<double> &src = l == 0 ? x : feat;
        std::vector<double> o((size_t)out);
        for (int i = 0; i < out; ++i) {
            double a = m.b[l][i];
            for (int k = 0; k < in; ++k) a += (double)m.w[l][(size_t)i * in + k] * src[k];
            o[i] = l == 5 ? std::tanh(a) : (a > 0 ? a : 0);
        }
        if (l == 5) {
            for (int i = 0; i < out; ++i) y[i] = o[i];
        } else {
            feat.insert(feat.end(), o.begin(), o.end());      // dense: torch.cat([x, relu(conv(x))])
        }
    }
}

// the stream walked as net_site_body walks it, for one site: an MFMA step adds A[row][half 0] * B[half 0] + A[row][half 1] * B[half 1]
// to each of the 32 rows in k order, and register reg of half h of the result is row net_row(reg, h)
static void walk(const std::vector<float> &st, int MT, int u, const float t[4], float *y) {
    using namespace mulut;
    std::vector<float> x((size_t)5 * MT * 16 * 2);      // [layer][tile][reg][half]
    auto step = [&](int g, float b0, float b1, float *acc) {
        for (int i = 0; i < 32; ++i) {
            acc[i] = std::fmaf(st[(size_t)net_step_float(g, i)], b0, acc[i]);
            acc[i] = std::fmaf(st[(size_t)net_step_float(g, i + 32)], b1, acc[i]);
        }
    };
    for (int L = 1; L <= 6; ++L)
        for (int mt = 0; mt < (L == 6 ? 1 : MT); ++mt) {
            float acc[32] = {0};
            const int base = net_step_base(MT, L, mt);
            step(base, 1.0f, 0.0f, acc);
            if (L == 1) {
                step(base + 1, t[0], t[1], acc);
                step(base + 2, t[2], t[3], acc);
            } else {
                for (int k = 0; k < (L - 1) * MT * 16; ++k) step(base + 1 + k, x[(size_t)k * 2], x[(size_t)k * 2 + 1], acc);
            }
            if (L < 6) {
                for (int reg = 0; reg < 16; ++reg)
                    for (int h = 0; h < 2; ++h) x[((size_t)((L - 1) * MT + mt) * 16 + reg) * 2 + h] = std::fmax(acc[net_row(reg, h)], 0.0f);
            } else {
                for (int o = 0; o < u * u; ++o) y[o] = std::tanh(acc[net_row(o & 7, o >> 3)]);
            }
        }
}

static void pack_case(int nf, int u) {
    using namespace mulut;
    Weights m;
    make(m, nf, u, true);
    const int MT = net_tiles(nf);
    std::vector<float> st((size_t)net_stream_floats(MT));
    net_pack(nf, u, m.wp, m.bp, st.data());
    double worst = 0;
    const float sites[5][4] = {{0, 0, 0, 0}, {1, 1, 1, 1}, {0.25f, 0.5f, 0.75f, 1.0f}, {16 / 255.0f, 240 / 255.0f, 1 / 255.0f, 128 / 255.0f}, {1, 0, 0.5f, 0.1f}};
    for (auto &t : sites) {
        double want[16];
        float got[16];
        plain(m, t, want);
        walk(st, MT, u, t, got);
        for (int o = 0; o < u * u; ++o) worst = std::fmax(worst, std::fabs(want[o] - (double)got[o]));
    }
    // what the pack leaves zero: every A row of a padded output, every step of a padded feature, the tail of the last chunk
    size_t nonzero = 0, want_nonzero = 0;
    for (float v : st) nonzero += v != 0.0f;
    for (int l = 0; l < 6; ++l) {
        for (float v : m.w[l]) want_nonzero += v != 0.0f;
        for (float v : m.b[l]) want_nonzero += v != 0.0f;
    }
    char what[96];
    snprintf(what, sizeof(what), "pack nf %d u %d: %d steps in %d chunks, worst |walk - plain| %.2e", nf, u, net_steps(MT), net_chunks(MT), worst);
    // float32 against double: at most 320 products of O(1) magnitude per sum, 2^-24 each, then tanh (slope <= 1)
    check(what, worst < 2e-6 && nonzero == want_nonzero);
}

int main() {
    using namespace mulut;
    g_seed = 12345u;
    check("steps at one tile 248, at two 815", net_steps(1) == 248 && net_steps(2) == 815 && net_chunks(1) == 4 && net_chunks(2) == 13);
    for (int nf : {1, 8, 24, 32, 33, 64})
        for (int u : {1, 2, 3, 4}) pack_case(nf, u);
    Weights m8, m64, m64u1;
    make(m8, 8, 2, true);
    make(m64, 64, 4, true);
    make(m64u1, 64, 1, true);
    mulut_net_unit *unit = (mulut_net_unit *)0x1, *u8 = nullptr, *u64 = nullptr, *u64b = nullptr, *u64u1 = nullptr;
    // ---- mulut_net_unit_create: refusals before the device is touched; *unit is NULL afterwards
    expect("create null out", mulut_net_unit_create(0, 8, 2, m8.wp, m8.bp, nullptr), MULUT_EINVAL, "");
    expect("create null w", mulut_net_unit_create(0, 8, 2, nullptr, m8.bp, &unit), MULUT_EINVAL, "");
    expect("create null b", mulut_net_unit_create(0, 8, 2, m8.wp, nullptr, &unit), MULUT_EINVAL, "");
    g_wrong += unit != nullptr;
    for (int l = 0; l < 6; ++l) {
        const float *wp[6], *bp[6];
        for (int k = 0; k < 6; ++k) wp[k] = m8.wp[k], bp[k] = m8.bp[k];
        wp[l] = nullptr;
        expect("create null w[l]", mulut_net_unit_create(0, 8, 2, wp, bp, &unit), MULUT_EINVAL, "");
        wp[l] = m8.wp[l];
        bp[l] = nullptr;
        expect("create null b[l]", mulut_net_unit_create(0, 8, 2, wp, bp, &unit), MULUT_EINVAL, "");
    }
    expect("create nf 0", mulut_net_unit_create(0, 0, 2, m8.wp, m8.bp, &unit), MULUT_EUNSUPPORTED, "");
    expect("create nf 65", mulut_net_unit_create(0, 65, 2, m8.wp, m8.bp, &unit), MULUT_EUNSUPPORTED, "");
    expect("create u 0", mulut_net_unit_create(0, 8, 0, m8.wp, m8.bp, &unit), MULUT_EUNSUPPORTED, "");
    expect("create u 5", mulut_net_unit_create(0, 8, 5, m8.wp, m8.bp, &unit), MULUT_EUNSUPPORTED, "");
    expect("create device 3", mulut_net_unit_create(3, 8, 2, m8.wp, m8.bp, &unit), MULUT_ENODEVICE, "");
    g_wrong += unit != nullptr;
    // ---- units: one allocation and one copy of the whole stream (4 or 13 chunks of 16 KiB)
    expect("create nf 8 u 2", mulut_net_unit_create(0, 8, 2, m8.wp, m8.bp, &u8), MULUT_OK, "malloc 65536 | memcpy 65536");
    expect("create nf 64 u 4", mulut_net_unit_create(0, 64, 4, m64.wp, m64.bp, &u64), MULUT_OK, "malloc 212992 | memcpy 212992");
    expect("create nf 64 u 4 again", mulut_net_unit_create(0, 64, 4, m64.wp, m64.bp, &u64b), MULUT_OK, "malloc 212992 | memcpy 212992");
    expect("create nf 64 u 1", mulut_net_unit_create(0, 64, 1, m64u1.wp, m64u1.bp, &u64u1), MULUT_OK, "malloc 212992 | memcpy 212992");
    g_wrong += !u8 || !u64 || !u64b || !u64u1;
    int8_t *rows = (int8_t *)kOut;
    // ---- mulut_net_table
    expect("table null unit", mulut_net_table(nullptr, 4, rows, nullptr), MULUT_EINVAL, "");
    expect("table null rows", mulut_net_table(u64, 4, nullptr, nullptr), MULUT_EINVAL, "");
    expect("table interval 3", mulut_net_table(u64, 3, rows, nullptr), MULUT_EUNSUPPORTED, "");
    expect("table interval 7", mulut_net_table(u64, 7, rows, nullptr), MULUT_EUNSUPPORTED, "");
    // 83,521 = 652 * 128 + 65, 6,561 = 51 * 128 + 33, 625 = 4 * 128 + 113: tails of 1, 1 and 17 rows past a 32-row tile
    expect("table interval 4", mulut_net_table(u64, 4, rows, nullptr), MULUT_OK, "launch net_table_kernel<2, 4> grid 653,1,1 block 256,1,1 lds 0");
    expect("table interval 5", mulut_net_table(u64, 5, rows, (void *)0x77), MULUT_OK, "launch net_table_kernel<2, 4> grid 52,1,1 block 256,1,1 lds 0");
    expect("table interval 6", mulut_net_table(u8, 6, rows, nullptr), MULUT_OK, "launch net_table_kernel<1, 2> grid 5,1,1 block 256,1,1 lds 0");
    check("tails past a 32-row tile are 1, 1 and 17", 83521 % 32 == 1 && 6561 % 32 == 1 && 625 % 32 == 17);
    // ---- mulut_net_pass
    expect("pass null unit", mulut_net_pass(nullptr, 's', 0, kIn, 1, 3, 8, 8, rows, nullptr), MULUT_EINVAL, "");
    expect("pass null in", mulut_net_pass(u64, 's', 0, nullptr, 1, 3, 8, 8, rows, nullptr), MULUT_EINVAL, "");
    expect("pass null out", mulut_net_pass(u64, 's', 0, kIn, 1, 3, 8, 8, nullptr, nullptr), MULUT_EINVAL, "");
    expect("pass r -1", mulut_net_pass(u64, 's', -1, kIn, 1, 3, 8, 8, rows, nullptr), MULUT_EINVAL, "");
    expect("pass r 4", mulut_net_pass(u64, 's', 4, kIn, 1, 3, 8, 8, rows, nullptr), MULUT_EINVAL, "");
    expect("pass mode x", mulut_net_pass(u64, 'x', 0, kIn, 1, 3, 8, 8, rows, nullptr), MULUT_EINVAL, "");
    expect("pass mode S", mulut_net_pass(u64, 'S', 0, kIn, 1, 3, 8, 8, rows, nullptr), MULUT_EINVAL, "");
    for (int v = 0; v >= -1; --v) {
        expect("pass N < 1", mulut_net_pass(u64, 's', 0, kIn, v, 3, 8, 8, rows, nullptr), MULUT_EINVAL, "");
        expect("pass C < 1", mulut_net_pass(u64, 's', 0, kIn, 1, v, 8, 8, rows, nullptr), MULUT_EINVAL, "");
        expect("pass H < 1", mulut_net_pass(u64, 's', 0, kIn, 1, 3, v, 8, rows, nullptr), MULUT_EINVAL, "");
        expect("pass W < 1", mulut_net_pass(u64, 's', 0, kIn, 1, 3, 8, v, rows, nullptr), MULUT_EINVAL, "");
    }
    expect("pass 2^31 output bytes", mulut_net_pass(u64, 's', 0, kIn, 1, 2, 1 << 13, 1 << 13, rows, nullptr), MULUT_EUNSUPPORTED, "");
    expect("pass 2^31 planes", mulut_net_pass(u64, 's', 0, kIn, 1 << 16, 1 << 15, 1, 1, rows, nullptr), MULUT_EUNSUPPORTED, "");
    expect("pass 2^31 pixels a plane", mulut_net_pass(u64u1, 's', 0, kIn, 1, 1, 1 << 16, 1 << 15, rows, nullptr), MULUT_EUNSUPPORTED, "");
    expect("pass one short of 2^31 output bytes", mulut_net_pass(u64u1, 's', 0, kIn, 1, 1, 0x7fffffff, 1, rows, nullptr), MULUT_OK,
           "launch net_pass_kernel<2, 1> grid 16777216,1,1 block 256,1,1 lds 0");
    for (const char *mode = "sdyeho"; *mode; ++mode)
        expect("pass 33 x 65 x 3", mulut_net_pass(u64, *mode, 3, kIn, 1, 3, 33, 65, rows, nullptr), MULUT_OK,
               "launch net_pass_kernel<2, 4> grid 51,1,1 block 256,1,1 lds 0");
    expect("pass 1 x 1", mulut_net_pass(u8, 'y', 1, kIn, 1, 1, 1, 1, rows, (void *)0x77), MULUT_OK, "launch net_pass_kernel<1, 2> grid 1,1,1 block 256,1,1 lds 0");
    // ---- mulut_net_stage
    const mulut_net_unit *list[9] = {u64, u64b, u64, u64, u64, u64, u64, u64, u64};
    expect("stage null units", mulut_net_stage(nullptr, "sd", 1, kIn, kOut, 1, 3, 8, 8, nullptr), MULUT_EINVAL, "");
    expect("stage null modes", mulut_net_stage(list, nullptr, 1, kIn, kOut, 1, 3, 8, 8, nullptr), MULUT_EINVAL, "");
    expect("stage null in", mulut_net_stage(list, "sd", 1, nullptr, kOut, 1, 3, 8, 8, nullptr), MULUT_EINVAL, "");
    expect("stage null out", mulut_net_stage(list, "sd", 1, kIn, nullptr, 1, 3, 8, 8, nullptr), MULUT_EINVAL, "");
    expect("stage no mode", mulut_net_stage(list, "", 1, kIn, kOut, 1, 3, 8, 8, nullptr), MULUT_EINVAL, "");
    expect("stage nine modes", mulut_net_stage(list, "sdysdysdy", 1, kIn, kOut, 1, 3, 8, 8, nullptr), MULUT_EUNSUPPORTED, "");
    expect("stage mode x", mulut_net_stage(list, "sx", 1, kIn, kOut, 1, 3, 8, 8, nullptr), MULUT_EINVAL, "");
    {
        const mulut_net_unit *hole[2] = {u64, nullptr};
        expect("stage null unit in the list", mulut_net_stage(hole, "sd", 1, kIn, kOut, 1, 3, 8, 8, nullptr), MULUT_EINVAL, "");
        const mulut_net_unit *mixed_u[2] = {u64, u64u1};
        expect("stage units of two u", mulut_net_stage(mixed_u, "sd", 1, kIn, kOut, 1, 3, 8, 8, nullptr), MULUT_ESHAPE, "");
        const mulut_net_unit *mixed_w[2] = {u64, u8};
        expect("stage units of two widths", mulut_net_stage(mixed_w, "sd", 1, kIn, kOut, 1, 3, 8, 8, nullptr), MULUT_ESHAPE, "");
    }
    for (int v = 0; v >= -1; --v) {
        expect("stage N < 1", mulut_net_stage(list, "sd", 1, kIn, kOut, v, 3, 8, 8, nullptr), MULUT_EINVAL, "");
        expect("stage C < 1", mulut_net_stage(list, "sd", 1, kIn, kOut, 1, v, 8, 8, nullptr), MULUT_EINVAL, "");
        expect("stage H < 1", mulut_net_stage(list, "sd", 1, kIn, kOut, 1, 3, v, 8, nullptr), MULUT_EINVAL, "");
        expect("stage W < 1", mulut_net_stage(list, "sd", 1, kIn, kOut, 1, 3, 8, v, nullptr), MULUT_EINVAL, "");
    }
    expect("stage 2^31 output bytes", mulut_net_stage(list, "sd", 1, kIn, kOut, 1, 2, 1 << 13, 1 << 13, nullptr), MULUT_EUNSUPPORTED, "");
    expect("stage sd 65 x 33 x 3 x 2", mulut_net_stage(list, "sd", 1, kIn, kOut, 2, 3, 65, 33, nullptr), MULUT_OK,
           "launch net_stage_kernel<2, 4> grid 101,1,1 block 256,1,1 lds 0");
    expect("stage eight modes", mulut_net_stage(list, "sdyehosd", 0, kIn, kOut, 1, 1, 1, 1, (void *)0x77), MULUT_OK,
           "launch net_stage_kernel<2, 4> grid 1,1,1 block 256,1,1 lds 0");
    {
        const mulut_net_unit *narrow[1] = {u8};
        expect("stage y nf 8", mulut_net_stage(narrow, "y", 1, kIn, kOut, 1, 3, 5, 7, nullptr), MULUT_OK,
               "launch net_stage_kernel<1, 2> grid 1,1,1 block 256,1,1 lds 0");
    }
    // ---- destroy
    expect("destroy null", mulut_net_unit_destroy(nullptr), MULUT_EINVAL, "");
    expect("destroy nf 8", mulut_net_unit_destroy(u8), MULUT_OK, "free 65536");
    expect("destroy nf 64", mulut_net_unit_destroy(u64), MULUT_OK, "free 212992");
    expect("destroy nf 64", mulut_net_unit_destroy(u64b), MULUT_OK, "free 212992");
    expect("destroy nf 64", mulut_net_unit_destroy(u64u1), MULUT_OK, "free 212992");
    printf("%d unexpected\n", g_wrong);
    return g_wrong;
}
