// abi_host.cpp -- drives the library's C ABI (include/mulut.h) on the CPU against fake_hip.cpp and prints, per ABI call, its
// return code and what it asked of the runtime: allocations, frees, copies, waits, events and launch configurations.
// tests/test_host_abi_cpu.py builds it with the host half of every file of the library under AddressSanitizer,
// UndefinedBehaviorSanitizer and LeakSanitizer and compares the output with tests/golden/host_abi_trace.txt.
//   --skip-destroy : leaves the last context alive, so that LeakSanitizer has something to report (the test's control)
// Kernels never run, so image and table pointers given to compute calls are made-up addresses that nothing follows.
#include <algorithm>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/mulut.h"

std::vector<std::string> &fake_hip_events();
void fake_hip_flush();

static const uint8_t *const kIn = (const uint8_t *)0x10000000;
static uint8_t *const kOut = (uint8_t *)0x20000000;
static std::vector<int8_t> g_rows;      // 83521 x 16 seeded int8 values: every table is cut from it
static long g_mallocs = 0;              // malloc events since the last reset (the reserve contract)

// prints "<call> -> rc" and the events of the call; sort_release: the frees and event destructions among themselves sorted (the
// order in which the members of a context die is not behaviour)
static int done(int rc, bool sort_release, const char *fmt, ...) {
    fake_hip_flush();
    char buf[256];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    std::vector<std::string> &ev = fake_hip_events();
    if (sort_release) {
        auto rel = [](const std::string &s) { return s.compare(0, 5, "free ") == 0 || s == "event_destroy"; };
        std::vector<std::string> r;
        for (auto &s : ev)
            if (rel(s)) r.push_back(s);
        std::sort(r.begin(), r.end());
        size_t k = 0;
        for (auto &s : ev)
            if (rel(s)) s = r[k++];
    }
    printf("%s -> %d\n", buf, rc);
    // runs of one repeated line are folded
    for (size_t i = 0; i < ev.size();) {
        size_t j = i;
        while (j < ev.size() && ev[j] == ev[i]) ++j;
        if (j - i > 1) printf("  %s x%zu\n", ev[i].c_str(), j - i);
        else printf("  %s\n", ev[i].c_str());
        if (ev[i].compare(0, 7, "malloc ") == 0) g_mallocs += (long)(j - i);
        i = j;
    }
    ev.clear();
    return rc;
}

static int rows_of(int interval) { return interval == 4 ? 83521 : interval == 5 ? 6561 : 625; }

static mulut_ctx *create() {
    mulut_ctx *c = nullptr;
    done(mulut_create(0, &c), false, "create");
    return c;
}
static void set_luts(mulut_ctx *c, int stages, const char *modes, int scale, int interval) {
    for (int s = 1; s <= stages; ++s)
        for (const char *m = modes; *m; ++m) {
            if (strchr(modes, *m) != m) continue;       // a repeated pattern has one table
            const int v = s == stages ? scale * scale : 1;
            done(mulut_set_lut(c, s, *m, g_rows.data(), rows_of(interval), v), false, "set_lut s%d %c v%d", s, *m, v);
        }
}
static mulut_ctx *model(int stages, const char *modes, int scale, int interval) {
    mulut_ctx *c = create();
    done(mulut_configure(c, stages, modes, scale, interval), true, "configure %d %s x%d iv%d", stages, modes, scale, interval);
    set_luts(c, stages, modes, scale, interval);
    return c;
}
static void destroy(mulut_ctx *c) { done(mulut_destroy(c), true, "destroy"); }
static int pipeline(mulut_ctx *c, int N, int H, int W, int C, int layout) {
    return done(mulut_pipeline(c, kIn, kOut, N, H, W, C, layout, nullptr), false, "pipeline %dx%dx%dx%d %s", N, H, W, C, layout ? "hwc" : "chw");
}
static void names(mulut_ctx *c) { printf("kernels: %s | %s\n", mulut_kernel_name(c, 0), mulut_kernel_name(c, 1)); }
static void tune(mulut_ctx *c, const char *key, int v) { done(mulut_set_tuning(c, key, v), false, "tuning %s %d", key, v); }

// ---------------------------------------------------------------------------------------------------------------- inference
static void inference() {
    // every route of the stage plan: the default tuning at every scale, then each tuning key that picks another route, on a
    // reserved context -- which must then allocate nothing
    for (int scale = 1; scale <= 4; ++scale) {
        printf("# sdy x%d\n", scale);
        mulut_ctx *c = model(2, "sdy", scale, 4);
        names(c);
        pipeline(c, 2, 70, 90, 3, MULUT_LAYOUT_HWC);
        pipeline(c, 2, 70, 90, 3, MULUT_LAYOUT_HWC);
        done(mulut_reserve(c, 3, 80, 100, 4), false, "reserve 3x80x100x4");
        g_mallocs = 0;
        static const struct { const char *key; int v, back; } keys[] = {
            {"final_stage_kernel", 1, 0}, {"final_stage_kernel", 5, 0}, {"final_stage_kernel", 6, 0}, {"first_stage_kernel", 2, 0},
            {"first_stage_kernel", 3, 0}, {"detail_kernel", 1, 0}, {"tube_pipelined", 0, 1}, {"stat_from_first_stage", 0, 1},
        };
        for (auto &k : keys) {
            if (scale < 4 && k.key[1] != 'i') continue;       // (the other keys choose among the x4 routes only)
            tune(c, k.key, k.v);
            names(c);
            pipeline(c, 3, 80, 100, 3, MULUT_LAYOUT_HWC);
            if (scale == 4) pipeline(c, 1, 33, 41, 1, MULUT_LAYOUT_CHW);
            tune(c, k.key, k.back);
        }
        pipeline(c, 2, 64, 64, 4, MULUT_LAYOUT_CHW);
        pipeline(c, 2, 64, 64, 4, MULUT_LAYOUT_HWC);
        printf("mallocs after reserve: %ld\n", g_mallocs);
        destroy(c);
    }
    printf("# mode lists\n");
    for (const char *modes : {"sdysd", "ssd"}) {
        mulut_ctx *c = model(2, modes, 4, 4);
        names(c);
        pipeline(c, 2, 70, 90, 3, MULUT_LAYOUT_HWC);
        tune(c, "tube_pipelined", 0);
        pipeline(c, 2, 70, 90, 3, MULUT_LAYOUT_HWC);
        destroy(c);
    }
    for (int scale : {1, 4}) {
        mulut_ctx *c = model(2, "sdyeho", scale, 4);
        names(c);
        printf("halo %d\n", mulut_halo(c));
        pipeline(c, 2, 70, 90, 3, MULUT_LAYOUT_HWC);
        pipeline(c, 1, 33, 41, 4, MULUT_LAYOUT_CHW);
        destroy(c);
    }
    printf("# intervals 5 and 6\n");
    for (int iv : {5, 6})
        for (const char *modes : {"sdy", "se"}) {
            mulut_ctx *c = model(2, modes, 4, iv);
            names(c);
            pipeline(c, 2, 70, 90, 3, MULUT_LAYOUT_HWC);
            pipeline(c, 1, 33, 41, 1, MULUT_LAYOUT_CHW);
            done(mulut_pass(c, 2, 's', 1, kIn, 20, 30, 1, (int32_t *)kOut, nullptr), false, "pass s2 s r1");
            destroy(c);
        }

    printf("# channels, layouts, single stages, strips\n");
    mulut_ctx *c = model(2, "sdy", 4, 4);
    for (int C : {1, 3, 4})
        for (int layout : {MULUT_LAYOUT_CHW, MULUT_LAYOUT_HWC}) pipeline(c, 2, 40, 52, C, layout);
    for (int stage : {1, 2})
        for (int C : {1, 3, 4})
            done(mulut_stage(c, stage, kIn, MULUT_LAYOUT_HWC, kOut, MULUT_LAYOUT_CHW, 2, 40, 52, C, nullptr), false, "stage %d C%d hwc->chw", stage, C);
    done(mulut_stage(c, 3, kIn, 0, kOut, 0, 1, 8, 8, 1, nullptr), false, "stage 3 (beyond the model)");
    printf("halo %d\n", mulut_halo(c));
    done(mulut_pipeline_rows(c, kIn, 16, 40, kOut, 20, 52, 2, 100, 90, 3, MULUT_LAYOUT_HWC, nullptr), false, "pipeline_rows [20,52) of 100, band [16,56)");
    done(mulut_pipeline_rows(c, kIn, 0, 30, kOut, 0, 26, 2, 100, 90, 3, MULUT_LAYOUT_CHW, nullptr), false, "pipeline_rows [0,26) of 100, band [0,30)");
    done(mulut_pipeline_rows(c, kIn, 18, 36, kOut, 20, 52, 2, 100, 90, 3, MULUT_LAYOUT_HWC, nullptr), false, "pipeline_rows [20,52) of 100, band [18,54)");
    done(mulut_pipeline_rows(c, kIn, 16, 40, kOut, 52, 20, 2, 100, 90, 3, MULUT_LAYOUT_HWC, nullptr), false, "pipeline_rows, y0 > y1");
    done(mulut_pipeline(c, kIn, kOut, 1, 1 << 30, 8, 1, MULUT_LAYOUT_CHW, nullptr), false, "pipeline, 2^30 rows");
    done(mulut_pipeline(c, nullptr, kOut, 1, 8, 8, 1, MULUT_LAYOUT_CHW, nullptr), false, "pipeline, no input");

    printf("# timing, probes, passes\n");
    done(mulut_set_stage_timing(c, 1), false, "timing on");
    done(mulut_set_stage_timing(c, 1), false, "timing on again");
    pipeline(c, 2, 40, 52, 3, MULUT_LAYOUT_HWC);
    float ms[8];
    done(mulut_last_stage_ms(c, ms, 8), false, "last_stage_ms");
    done(mulut_last_kernel_ms(c, ms, 8), false, "last_kernel_ms");
    tune(c, "first_stage_kernel", 2);
    tune(c, "final_stage_kernel", 1);
    pipeline(c, 2, 40, 52, 3, MULUT_LAYOUT_HWC);
    tune(c, "first_stage_kernel", 0);
    tune(c, "final_stage_kernel", 0);
    done(mulut_set_stage_timing(c, 0), false, "timing off");
    pipeline(c, 2, 40, 52, 3, MULUT_LAYOUT_HWC);
    done(mulut_last_stage_ms(c, ms, 8), false, "last_stage_ms");
    uint32_t ctr[32];
    done(mulut_last_detail_counters(c, ctr, 32, nullptr), false, "last_detail_counters");
    std::vector<unsigned long long> words(MULUT_DEBUG_WORDS);
    done(mulut_debug_read(c, words.data(), 16, 1, nullptr), false, "debug_read 16, reset");
    done(mulut_debug_read(c, words.data(), MULUT_DEBUG_WORDS + 5, 0, nullptr), false, "debug_read all");
    pipeline(c, 2, 40, 52, 3, MULUT_LAYOUT_HWC);
    for (int stage : {1, 2})
        for (int r : {0, 3}) done(mulut_pass(c, stage, 'y', r, kIn, 20, 30, 2, (int32_t *)kOut, nullptr), false, "pass s%d y r%d", stage, r);
    done(mulut_pass(c, 1, 'e', 0, kIn, 20, 30, 2, (int32_t *)kOut, nullptr), false, "pass of a table not set");
    done(mulut_pass(c, 1, 'q', 0, kIn, 20, 30, 2, (int32_t *)kOut, nullptr), false, "pass of an unknown pattern");

    printf("# tables\n");
    done(mulut_set_lut(c, 2, 'd', g_rows.data(), 83521, 16), false, "set_lut s2 d v16 on a filled slot");
    done(mulut_set_lut(c, 2, 'd', g_rows.data(), 83521, 4), false, "set_lut s2 d v4 on a filled slot");
    pipeline(c, 1, 16, 16, 1, MULUT_LAYOUT_CHW);
    done(mulut_set_lut(c, 2, 'd', g_rows.data(), 83521, 16), false, "set_lut s2 d v16 on a filled slot");
    done(mulut_set_lut(c, 1, 'd', g_rows.data(), 83521, 1), false, "set_lut s1 d v1 on a filled slot");
    done(mulut_set_lut(c, 2, 'e', g_rows.data(), 83521, 16), false, "set_lut s2 e v16");
    done(mulut_set_lut(c, 2, 'e', g_rows.data(), 83521, 1), false, "set_lut s2 e v1 on a filled slot");
    done(mulut_set_lut(c, 2, 'e', g_rows.data(), 6561, 1), false, "set_lut, rows of another interval");
    done(mulut_set_lut(c, 2, 'e', g_rows.data(), 83521, 5), false, "set_lut, v_num 5");
    done(mulut_set_lut(c, 9, 'e', g_rows.data(), 83521, 1), false, "set_lut, stage 9");
    done(mulut_configure(c, 2, "sdy", 4, 7), true, "configure, interval 7");
    done(mulut_configure(c, 2, "sxy", 4, 4), true, "configure, unknown pattern");
    done(mulut_configure(c, 3, "sd", 2, 4), true, "configure 3 sd x2 iv4");
    pipeline(c, 1, 16, 16, 1, MULUT_LAYOUT_CHW);
    done(mulut_configure(c, 2, "sdy", 4, 5), true, "configure 2 sdy x4 iv5 (another interval)");
    pipeline(c, 1, 16, 16, 1, MULUT_LAYOUT_CHW);
    set_luts(c, 2, "sdy", 4, 5);
    pipeline(c, 1, 16, 16, 1, MULUT_LAYOUT_CHW);

    printf("# two contexts\n");
    mulut_ctx *d = model(1, "s", 2, 4);
    pipeline(d, 1, 16, 16, 1, MULUT_LAYOUT_CHW);
    pipeline(c, 1, 16, 16, 1, MULUT_LAYOUT_CHW);
    destroy(c);
    pipeline(d, 1, 20, 20, 1, MULUT_LAYOUT_CHW);
    destroy(d);
    mulut_ctx *none = nullptr;
    done(mulut_create(1, &none), false, "create on device 1");
    done(mulut_create(0, nullptr), false, "create, no result pointer");
    done(mulut_destroy(nullptr), true, "destroy, no context");
    mulut_ctx *fresh = create();
    pipeline(fresh, 1, 16, 16, 1, MULUT_LAYOUT_CHW);
    done(mulut_reserve(fresh, 1, 16, 16, 1), false, "reserve before configure");
    destroy(fresh);
}

// --------------------------------------------------------------------------------------------------------------- fine-tuning
struct FtReq {
    int interval, u, is_last, B, C, H, W;
    const float *const *w;
    const char *modes;
    const float *x;
    float *out;
    unsigned short *inside;
    const float *gout;
    float *const *gw;
    float *gx;
};
static const char *const kFtNames[8] = {"stage_forward", "stage_backward", "stage_forward_mask", "stage_backward_mask",
                                        "interval_stage_forward", "interval_stage_backward", "wide_stage_forward", "wide_stage_backward"};
static int ft_call(int ep, const FtReq &r) {
    switch (ep) {
        case 0: return mulut_ft_stage_forward(0, r.w, r.modes, r.is_last, r.u, r.x, r.B, r.C, r.H, r.W, r.out, nullptr);
        case 1: return mulut_ft_stage_backward(0, r.w, r.modes, r.is_last, r.u, r.x, r.gout, r.B, r.C, r.H, r.W, r.gw, r.gx, nullptr);
        case 2: return mulut_ft_stage_forward_mask(0, r.w, r.modes, r.is_last, r.u, r.x, r.B, r.C, r.H, r.W, r.out, r.inside, nullptr);
        case 3: return mulut_ft_stage_backward_mask(0, r.w, r.modes, r.is_last, r.u, r.x, r.gout, r.inside, r.B, r.C, r.H, r.W, r.gw, r.gx, nullptr);
        case 4: return mulut_ft_interval_stage_forward(0, r.interval, r.w, r.modes, r.is_last, r.u, r.x, r.B, r.C, r.H, r.W, r.out, r.inside, nullptr);
        case 5: return mulut_ft_interval_stage_backward(0, r.interval, r.w, r.modes, r.is_last, r.u, r.x, r.gout, r.inside, r.B, r.C, r.H, r.W, r.gw, r.gx, nullptr);
        case 6: return mulut_ft_wide_stage_forward(0, r.interval, r.w, r.modes, r.is_last, r.u, r.x, r.B, r.C, r.H, r.W, r.out, r.inside, nullptr);
        default: return mulut_ft_wide_stage_backward(0, r.interval, r.w, r.modes, r.is_last, r.u, r.x, r.gout, r.inside, r.B, r.C, r.H, r.W, r.gw, r.gx, nullptr);
    }
}
static bool ft_takes(int ep, int interval) { return ep < 4 ? interval == 4 : ep < 6 ? interval != 4 : true; }

static float *const kTab[MULUT_MAX_MODES + 1] = {(float *)0x30000000, (float *)0x31000000, (float *)0x32000000, (float *)0x33000000, (float *)0x34000000,
                                                 (float *)0x35000000, (float *)0x36000000, (float *)0x37000000, (float *)0x38000000};
static float *const kTabHole[MULUT_MAX_MODES + 1] = {(float *)0x30000000, nullptr, (float *)0x32000000, (float *)0x33000000, (float *)0x34000000,
                                                     (float *)0x35000000, (float *)0x36000000, (float *)0x37000000, (float *)0x38000000};
static FtReq ft_good(int interval, int u, const char *modes, int H, int W) {
    return FtReq{interval, u, u > 1, 1, 1, H, W, kTab, modes, (const float *)kIn, (float *)kOut, (unsigned short *)0x40000000,
                 (const float *)0x50000000, kTab, (float *)0x60000000};
}

struct Defect { const char *name; void (*apply)(FtReq &); };
static const Defect kDefects[] = {
    {"weights NULL", [](FtReq &r) { r.w = nullptr; }},
    {"modes NULL", [](FtReq &r) { r.modes = nullptr; }},
    {"x NULL", [](FtReq &r) { r.x = nullptr; }},
    {"out NULL", [](FtReq &r) { r.out = nullptr; }},
    {"grad_out NULL", [](FtReq &r) { r.gout = nullptr; }},
    {"grad_x NULL", [](FtReq &r) { r.gx = nullptr; }},
    {"grad_wq NULL", [](FtReq &r) { r.gw = nullptr; }},
    {"inside NULL", [](FtReq &r) { r.inside = nullptr; }},
    {"weights[1] NULL", [](FtReq &r) { r.w = kTabHole; }},
    {"grad_wq[1] NULL", [](FtReq &r) { r.gw = kTabHole; }},
    {"H 0", [](FtReq &r) { r.H = 0; }},
    {"B -1", [](FtReq &r) { r.B = -1; }},
    {"interval 3", [](FtReq &r) { r.interval = 3; }},
    {"interval 7", [](FtReq &r) { r.interval = 7; }},
    {"u 0", [](FtReq &r) { r.u = 0; }},
    {"u 5", [](FtReq &r) { r.u = 5; }},
    {"modes empty", [](FtReq &r) { r.modes = ""; }},
    {"modes of nine", [](FtReq &r) { r.modes = "sdysdysdy"; }},
    {"modes sxy", [](FtReq &r) { r.modes = "sxy"; }},
    {"modes sey", [](FtReq &r) { r.modes = "sey"; }},
};
constexpr int kNDefects = (int)(sizeof(kDefects) / sizeof(kDefects[0]));

static char code_char(int rc) { return rc == 0 ? '.' : rc < 0 && rc > -10 ? (char)('0' - rc) : '?'; }

static void finetune() {
    printf("# fine-tune stages\n");
    const float *w2[2] = {kTab[0], kTab[1]};
    float *o2[2] = {kTab[2], kTab[3]};
    done(mulut_ft_quantize(0, w2, o2, 2, 625 * 16, nullptr), false, "ft_quantize");
    done(mulut_ft_quantize_backward(0, w2, o2, 2, 83521, nullptr), false, "ft_quantize_backward");
    done(mulut_ft_quantize(0, w2, nullptr, 2, 625, nullptr), false, "ft_quantize, no output");
    done(mulut_ft_quantize(0, w2, o2, 9, 625, nullptr), false, "ft_quantize, nine tables");
    o2[1] = nullptr;
    done(mulut_ft_quantize_backward(0, w2, o2, 2, 625, nullptr), false, "ft_quantize_backward, grad[1] NULL");
    for (const char *modes : {"sdy", "sey"})
        for (int W : {8, 200})
            for (int interval : {4, 5, 6})
                for (int u = 1; u <= 4; ++u)
                    for (int ep = 0; ep < 8; ++ep) {
                        if (!ft_takes(ep, interval)) continue;
                        const FtReq r = ft_good(interval, u, modes, 8, W);
                        done(ft_call(ep, r), false, "ft %s iv%d u%d %s 8x%d", kFtNames[ep], interval, u, modes, W);
                    }
    // which code a bad call gets: every single defect, then every pair (in the order of the list, the later one winning a clash)
    printf("# fine-tune refusals (. = accepted, digit n = code -n), per entry point and interval: the defects");
    for (int i = 0; i < kNDefects; ++i) printf("%s %d %s", i ? "," : "", i, kDefects[i].name);
    printf(" alone, then the pairs 0+1, 0+2, ... %d+%d\n", kNDefects - 2, kNDefects - 1);
    for (int ep = 0; ep < 8; ++ep)
        for (int interval : {4, 5, 6}) {
            if (!ft_takes(ep, interval)) continue;
            std::string line;
            for (int i = 0; i < kNDefects; ++i) {
                FtReq r = ft_good(interval, 2, "sdy", 8, 8);
                kDefects[i].apply(r);
                line += code_char(ft_call(ep, r));
            }
            line += ' ';
            for (int i = 0; i < kNDefects; ++i)
                for (int j = i + 1; j < kNDefects; ++j) {
                    FtReq r = ft_good(interval, 2, "sdy", 8, 8);
                    kDefects[i].apply(r);
                    kDefects[j].apply(r);
                    line += code_char(ft_call(ep, r));
                }
            fake_hip_flush();
            fake_hip_events().clear();      // (a defect that the entry point has no argument for leaves a good call)
            printf("refuse %s iv%d: %s\n", kFtNames[ep], interval, line.c_str());
        }
}

int main(int argc, char **argv) {
    const bool skip_destroy = argc > 1 && !strcmp(argv[1], "--skip-destroy");
    g_rows.resize((size_t)83521 * 16);
    uint32_t s = 12345u;
    for (auto &v : g_rows) {
        s = s * 1664525u + 1013904223u;
        v = (int8_t)(s >> 24);
    }
    printf("version %d\n", mulut_version());
    if (skip_destroy) {     // a context with tables, work lists, a workspace and events that nobody destroys
        mulut_ctx *c = model(2, "sdy", 4, 4);
        mulut_set_stage_timing(c, 1);
        pipeline(c, 1, 40, 52, 3, MULUT_LAYOUT_HWC);
        return 0;
    }
    inference();
    finetune();
    return 0;
}
