// resample_host.cpp -- the host half of mulut_resample_* (mulut_amd/csrc/mulut_resample.hip) on the CPU against fake_hip.cpp: every
// refusal code, each decided without touching the device; what a plan allocates, copies and frees; the launch configuration of a
// run; and a sweep of the coefficient tables with every tap inside [0, in).  tests/test_resample_cpu.py builds it under
// AddressSanitizer and UndefinedBehaviorSanitizer and runs it as a program; it prints one line per call and exits with the number
// of lines that are not what this file expects.  The kernel never runs, so the image pointers are made-up addresses that nothing
// follows.
#include <cstdio>
#include <string>
#include <vector>

#include "../../include/mulut.h"

std::vector<std::string> &fake_hip_events();
void fake_hip_flush();

static const uint8_t *const kIn = (const uint8_t *)0x10000000;
static uint8_t *const kOut = (uint8_t *)0x50000000;
static int g_wrong = 0;

static void expect(const char *what, int rc, int want_rc, const std::string &want_event) {
    fake_hip_flush();
    std::vector<std::string> &ev = fake_hip_events();
    std::string got;
    for (auto &s : ev) got += (got.empty() ? "" : " | ") + s;
    ev.clear();
    const bool ok = rc == want_rc && got == want_event;
    printf("%s -> %d [%s]%s\n", what, rc, got.c_str(), ok ? "" : "   UNEXPECTED");
    g_wrong += !ok;
}

// the tables of in -> out: rows zero beyond n, every tap inside [0, in), n within the row, each row summing to about 2^22
static void sweep(int in, int out, long long *axes) {
    int32_t probe[1], px[1], pn[1];
    const int taps_in_1 = mulut_resample_coeffs(in, 1, probe, px, pn, 0);      // (too small on purpose: only the refusal is wanted)
    if (taps_in_1 != MULUT_EWORKSPACE) {
        printf("coeffs %d -> 1 with cap 0 -> %d   UNEXPECTED\n", in, taps_in_1);
        ++g_wrong;
    }
    // in / out stays below 8 in this sweep (in < 2 * s * out): support below 16, at most 33 taps
    std::vector<int32_t> kk((size_t)out * 33), xmin((size_t)out), n((size_t)out);
    const int got = mulut_resample_coeffs(in, out, kk.data(), xmin.data(), n.data(), (long long)kk.size());
    bool ok = got >= 5 && (long long)got * out <= (long long)kk.size();
    for (int xx = 0; ok && xx < out; ++xx) {
        ok = xmin[xx] >= 0 && n[xx] >= 1 && n[xx] <= got && xmin[xx] + n[xx] <= in;
        long long sum = 0;
        for (int t = 0; ok && t < got; ++t) {
            const int32_t k = kk[(size_t)xx * got + t];
            if (t >= n[xx] && k != 0) ok = false;
            sum += k;
        }
        if (sum < (1 << 22) - 64 || sum > (1 << 22) + 64) ok = false;
    }
    if (!ok) {
        printf("coeffs %d -> %d: taps %d   UNEXPECTED\n", in, out, got);
        ++g_wrong;
    }
    ++*axes;
}

int main() {
    int32_t kk[64], xm[4], nn[4];
    mulut_resample_plan *plan = (mulut_resample_plan *)0x1;
    // ---- mulut_resample_coeffs: needs no device, so no event in any line
    expect("coeffs null kk", mulut_resample_coeffs(8, 2, nullptr, xm, nn, 64), MULUT_EINVAL, "");
    expect("coeffs null xmin", mulut_resample_coeffs(8, 2, kk, nullptr, nn, 64), MULUT_EINVAL, "");
    expect("coeffs null n", mulut_resample_coeffs(8, 2, kk, xm, nullptr, 64), MULUT_EINVAL, "");
    for (int v = 0; v >= -1; --v) {
        expect("coeffs in < 1", mulut_resample_coeffs(v, 2, kk, xm, nn, 64), MULUT_EINVAL, "");
        expect("coeffs out < 1", mulut_resample_coeffs(8, v, kk, xm, nn, 64), MULUT_EINVAL, "");
    }
    expect("coeffs 2^31-1 -> 1", mulut_resample_coeffs(0x7fffffff, 1, kk, xm, nn, 64), MULUT_EUNSUPPORTED, "");
    expect("coeffs cap one short", mulut_resample_coeffs(8, 2, kk, xm, nn, 2 * 17 - 1), MULUT_EWORKSPACE, "");
    expect("coeffs 8 -> 2", mulut_resample_coeffs(8, 2, kk, xm, nn, 2 * 17), 17, "");
    expect("coeffs 2 -> 4", mulut_resample_coeffs(2, 4, kk, xm, nn, 64), 5, "");
    // ---- mulut_resample_plan_create: refusals before the device is touched; *plan is NULL afterwards
    expect("plan null out", mulut_resample_plan_create(0, 8, 8, 2, 2, nullptr), MULUT_EINVAL, "");
    for (int v = 0; v >= -1; --v) {
        expect("plan in_h < 1", mulut_resample_plan_create(0, v, 8, 2, 2, &plan), MULUT_EINVAL, "");
        expect("plan in_w < 1", mulut_resample_plan_create(0, 8, v, 2, 2, &plan), MULUT_EINVAL, "");
        expect("plan out_h < 1", mulut_resample_plan_create(0, 8, 8, v, 2, &plan), MULUT_EINVAL, "");
        expect("plan out_w < 1", mulut_resample_plan_create(0, 8, 8, 2, v, &plan), MULUT_EINVAL, "");
        g_wrong += plan != nullptr;
    }
    expect("plan in plane 2^31", mulut_resample_plan_create(0, 1 << 16, 1 << 15, 2, 2, &plan), MULUT_EUNSUPPORTED, "");
    expect("plan out plane 2^31", mulut_resample_plan_create(0, 2, 2, 1 << 15, 1 << 16, &plan), MULUT_EUNSUPPORTED, "");
    expect("plan taps beyond 2^20", mulut_resample_plan_create(0, 1, 0x7ffffff0, 1, 1, &plan), MULUT_EUNSUPPORTED, "");
    expect("plan rows beyond the LDS", mulut_resample_plan_create(0, 1600, 64, 100, 64, &plan), MULUT_EUNSUPPORTED, "");
    expect("plan taps beyond the LDS", mulut_resample_plan_create(0, 64, 1600, 64, 100, &plan), MULUT_EUNSUPPORTED, "");
    g_wrong += plan != nullptr;
    expect("plan device 3", mulut_resample_plan_create(3, 8, 8, 2, 2, &plan), MULUT_ENODEVICE, "");
    g_wrong += plan != nullptr;
    // ---- a plan: one allocation of out_w * (17 + 1) + out_h * (17 + 2) int32, one copy; runs launch once and do nothing else
    expect("plan 1356 x 2040 -> 339 x 510", mulut_resample_plan_create(0, 1356, 2040, 339, 510, &plan), MULUT_OK, "malloc 62484 | memcpy 62484");
    g_wrong += plan == nullptr;
    // refusals of a run, with a real plan and pointers nothing may follow
    expect("run null plan", mulut_resample_run(nullptr, kIn, MULUT_LAYOUT_HWC, kOut, MULUT_LAYOUT_HWC, 1, 3, nullptr), MULUT_EINVAL, "");
    expect("run null in", mulut_resample_run(plan, nullptr, MULUT_LAYOUT_HWC, kOut, MULUT_LAYOUT_HWC, 1, 3, nullptr), MULUT_EINVAL, "");
    expect("run null out", mulut_resample_run(plan, kIn, MULUT_LAYOUT_HWC, nullptr, MULUT_LAYOUT_HWC, 1, 3, nullptr), MULUT_EINVAL, "");
    for (int v = 0; v >= -1; --v) {
        expect("run N < 1", mulut_resample_run(plan, kIn, MULUT_LAYOUT_HWC, kOut, MULUT_LAYOUT_HWC, v, 3, nullptr), MULUT_EINVAL, "");
        expect("run C < 1", mulut_resample_run(plan, kIn, MULUT_LAYOUT_HWC, kOut, MULUT_LAYOUT_HWC, 1, v, nullptr), MULUT_EINVAL, "");
    }
    expect("run layout 2", mulut_resample_run(plan, kIn, 2, kOut, MULUT_LAYOUT_HWC, 1, 3, nullptr), MULUT_EINVAL, "");
    expect("run layout -1", mulut_resample_run(plan, kIn, MULUT_LAYOUT_CHW, kOut, -1, 1, 3, nullptr), MULUT_EINVAL, "");
    expect("run packed image of 2^31 bytes", mulut_resample_run(plan, kIn, MULUT_LAYOUT_HWC, kOut, MULUT_LAYOUT_CHW, 1, 777, nullptr),
           MULUT_EUNSUPPORTED, "");
    expect("run 2^31 workgroups", mulut_resample_run(plan, kIn, MULUT_LAYOUT_CHW, kOut, MULUT_LAYOUT_CHW, 1 << 20, 171, nullptr),
           MULUT_EUNSUPPORTED, "");
    // launches: packed RGB (7 tile columns of 84 pixels x 22 tiles of 16 rows, one per workgroup in so small a call; 17 KiB of taps + 76 rows of 256 bytes),
    // planar and mixed layouts (one channel per workgroup, 2 tile columns of 256 pixels), a batch, a stream
    expect("run HWC C 3", mulut_resample_run(plan, kIn, MULUT_LAYOUT_HWC, kOut, MULUT_LAYOUT_HWC, 1, 3, nullptr), MULUT_OK,
           "launch resample_kernel<3> grid 154,1,1 block 256,1,1 lds 36864");
    expect("run CHW C 3", mulut_resample_run(plan, kIn, MULUT_LAYOUT_CHW, kOut, MULUT_LAYOUT_CHW, 1, 3, nullptr), MULUT_OK,
           "launch resample_kernel<1> grid 132,1,1 block 256,1,1 lds 36864");
    expect("run HWC -> CHW C 3 N 5", mulut_resample_run(plan, kIn + 1, MULUT_LAYOUT_HWC, kOut + 3, MULUT_LAYOUT_CHW, 5, 3, (void *)0x77), MULUT_OK,
           "launch resample_kernel<1> grid 660,1,1 block 256,1,1 lds 36864");
    expect("run HWC C 1", mulut_resample_run(plan, kIn, MULUT_LAYOUT_HWC, kOut, MULUT_LAYOUT_HWC, 1, 1, nullptr), MULUT_OK,
           "launch resample_kernel<1> grid 44,1,1 block 256,1,1 lds 36864");
    expect("run HWC C 4", mulut_resample_run(plan, kIn, MULUT_LAYOUT_HWC, kOut, MULUT_LAYOUT_HWC, 1, 4, nullptr), MULUT_OK,
           "launch resample_kernel<4> grid 176,1,1 block 256,1,1 lds 36864");
    expect("run HWC C 5", mulut_resample_run(plan, kIn, MULUT_LAYOUT_HWC, kOut, MULUT_LAYOUT_HWC, 1, 5, nullptr), MULUT_OK,
           "launch resample_kernel<1> grid 220,1,1 block 256,1,1 lds 36864");
    expect("destroy", mulut_resample_plan_destroy(plan), MULUT_OK, "free 62484");
    expect("destroy null", mulut_resample_plan_destroy(nullptr), MULUT_EINVAL, "");
    // one axis unchanged: no table and no LDS for the skipped pass (x4 across: 5 taps; 16 rows of a tile pass through)
    expect("plan 40 x 50 -> 40 x 200", mulut_resample_plan_create(0, 40, 50, 40, 200, &plan), MULUT_OK, "malloc 5120 | memcpy 5120");
    expect("run across only", mulut_resample_run(plan, kIn, MULUT_LAYOUT_HWC, kOut, MULUT_LAYOUT_HWC, 2, 3, nullptr), MULUT_OK,
           "launch resample_kernel<3> grid 18,1,1 block 256,1,1 lds 9216");
    expect("destroy", mulut_resample_plan_destroy(plan), MULUT_OK, "free 5120");
    expect("plan 40 x 50 -> 10 x 50", mulut_resample_plan_create(0, 40, 50, 10, 50, &plan), MULUT_OK, "malloc 960 | memcpy 960");
    expect("run down only", mulut_resample_run(plan, kIn, MULUT_LAYOUT_CHW, kOut, MULUT_LAYOUT_HWC, 1, 2, nullptr), MULUT_OK,
           "launch resample_kernel<1> grid 2,1,1 block 256,1,1 lds 10240");
    expect("destroy", mulut_resample_plan_destroy(plan), MULUT_OK, "free 960");
    // ---- the coefficient sweep: in = 1 .. 600 with out = in / s and in * s, and the sizes of real frames
    long long axes = 0;
    for (int in = 1; in <= 600; ++in)
        for (int s = 2; s <= 4; ++s) {
            if (in / s) sweep(in, in / s, &axes);
            sweep(in, in * s, &axes);
        }
    const int pairs[4][2] = {{2040, 510}, {2041, 510}, {1356, 339}, {1080, 4320}};
    for (auto &p : pairs) sweep(p[0], p[1], &axes);
    printf("%lld axes swept\n", axes);
    printf("%d unexpected\n", g_wrong);
    return g_wrong;
}
