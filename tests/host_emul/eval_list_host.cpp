// eval_list_host.cpp -- the host halves of mulut_eval_plan_* / mulut_eval_finish (mulut_amd/csrc/mulut_eval.hip) and of mulut_ft_val_pack
// (mulut_amd/csrc/mulut_ft_data.hip) on the CPU against fake_hip.cpp: every refusal in its documented order, each decided without
// touching the device and leaving *plan NULL, the launch configurations of a 1-item, a 2-item and a 328-item plan, and create /
// destroy pairs that LeakSanitizer watches.  tests/test_val_cpu.py builds it under AddressSanitizer and UndefinedBehaviorSanitizer
// and runs it as a program; it prints one line per call and exits with the number of lines that are not what this file expects.
// The kernels never run, so the device pointers are made-up addresses that nothing follows.
#include <cmath>
#include <cstdio>
#include <string>
#include <vector>

#include "../../include/mulut.h"

std::vector<std::string> &fake_hip_events();
void fake_hip_flush();

static const void *const kGt = (const void *)0x10000000, *const kOut = (const void *)0x20000000;
static double *const kSums = (double *)0x30000000;
static const float *const kPred = (const float *)0x40000000;
static unsigned char *const kBytes = (unsigned char *)0x50000001;
static mulut_eval_plan *const kStale = (mulut_eval_plan *)0x66;
static int g_wrong = 0;

// one call: its return code and its events (a refusal has none)
static void expect(const char *what, int rc, int want_rc, const std::string &want_event, bool extra = true) {
    fake_hip_flush();
    std::vector<std::string> &ev = fake_hip_events();
    std::string got;
    for (auto &s : ev) got += (got.empty() ? "" : " | ") + s;
    ev.clear();
    const bool ok = rc == want_rc && got == want_event && extra;
    printf("%s -> %d [%s]%s\n", what, rc, got.c_str(), ok ? "" : "   UNEXPECTED");
    g_wrong += !ok;
}

static mulut_eval_item item(long long gt_off, long long out_off, int H, int W, long long gt_pool, long long out_pool) {
    mulut_eval_item it = {gt_off, out_off, H, W, gt_pool, out_pool};
    return it;
}

// create with a plan pointer that holds garbage before the call: a refusal must leave NULL there
static void refuse(const char *what, int device, const mulut_eval_item *items, int n, int shave, int want_rc) {
    mulut_eval_plan *p = kStale;
    const int rc = mulut_eval_plan_create(device, items, n, shave, &p);
    expect(what, rc, want_rc, "", p == nullptr);
}

int main() {
    static_assert(sizeof(mulut_eval_item) == 40, "mulut_eval_item is 40 bytes");
    const long long PB = 1 << 20;
    const mulut_eval_item good = item(0, 0, 16, 16, PB, PB);
    // ---- mulut_eval_plan_create: NULL pointers, n < 1, shave < 0
    expect("null plan", mulut_eval_plan_create(0, &good, 1, 4, nullptr), MULUT_EINVAL, "");
    refuse("null items", 0, nullptr, 1, 4, MULUT_EINVAL);
    refuse("n 0", 0, &good, 0, 4, MULUT_EINVAL);
    refuse("n -1", 0, &good, -1, 4, MULUT_EINVAL);
    refuse("shave -1", 0, &good, 1, -1, MULUT_EINVAL);
    // ---- shapes: below the 11 x 11 window, not larger than 2 * shave
    {
        const mulut_eval_item a = item(0, 0, 10, 16, PB, PB), b = item(0, 0, 16, 10, PB, PB), c = item(0, 0, 0, 16, PB, PB), d = item(0, 0, 16, -3, PB, PB);
        refuse("H 10", 0, &a, 1, 4, MULUT_ESHAPE);
        refuse("W 10", 0, &b, 1, 4, MULUT_ESHAPE);
        refuse("H 0", 0, &c, 1, 4, MULUT_ESHAPE);
        refuse("W -3", 0, &d, 1, 4, MULUT_ESHAPE);
        refuse("16 x 16, shave 8", 0, &good, 1, 8, MULUT_ESHAPE);
        refuse("16 x 16, shave 2^30", 0, &good, 1, 1 << 30, MULUT_ESHAPE);
        // a bad argument of the first class wins over a bad shape, a bad shape LATER in the list over a bad offset EARLIER in it
        refuse("n 0, H 10", 0, &a, 0, 4, MULUT_EINVAL);
        const mulut_eval_item two[2] = {item(-1, 0, 16, 16, PB, PB), a};
        refuse("offset -1 then H 10", 0, two, 2, 4, MULUT_ESHAPE);
    }
    // ---- pools: negative offsets, an image that ends one byte past its pool, products that leave 32 bits
    {
        const long long sz = 16 * 16 * 3;
        const mulut_eval_item a = item(-1, 0, 16, 16, PB, PB), b = item(0, -1, 16, 16, PB, PB), c = item(PB - sz + 1, 0, 16, 16, PB, PB),
                              d = item(0, PB - sz + 1, 16, 16, PB, PB), e = item(0, 0, 16, 16, sz - 1, PB), f = item(0, 0, 16, 16, PB, -5),
                              g = item(0, 0, 0x7fffffff, 0x7fffffff, PB, PB), h = item(0x7fffffffffffffffLL, 0, 16, 16, PB, PB);
        refuse("gt_off -1", 0, &a, 1, 4, MULUT_EINVAL);
        refuse("out_off -1", 0, &b, 1, 4, MULUT_EINVAL);
        refuse("gt one byte past", 0, &c, 1, 4, MULUT_EINVAL);
        refuse("out one byte past", 0, &d, 1, 4, MULUT_EINVAL);
        refuse("gt pool too small", 0, &e, 1, 4, MULUT_EINVAL);
        refuse("out pool negative", 0, &f, 1, 4, MULUT_EINVAL);
        refuse("(2^31 - 1)^2 pixels", 0, &g, 1, 4, MULUT_EINVAL);
        refuse("gt_off 2^63 - 1", 0, &h, 1, 4, MULUT_EINVAL);
        // an offset outside wins over too many workgroups
        std::vector<mulut_eval_item> many(2049, item(0, 0, 1 << 15, 1 << 15, 1LL << 32, 1LL << 32));
        many[2048].gt_off = 1LL << 32;
        refuse("too many workgroups and an offset outside", 0, many.data(), 2049, 4, MULUT_EINVAL);
    }
    // ---- 2^31 workgroups in one launch: 2048 items of 2^15 x 2^15 have 2048 x 2^20 SSIM tiles (and 2^21 squared-error blocks)
    {
        std::vector<mulut_eval_item> many(2048, item(0, 0, 1 << 15, 1 << 15, 1LL << 32, 1LL << 32));
        refuse("2^31 tiles", 0, many.data(), 2048, 4, MULUT_EUNSUPPORTED);
    }
    // ---- a device the runtime does not have: the arguments are in order, the device is asked for and refused
    refuse("device 3", 3, &good, 1, 4, MULUT_ENODEVICE);
    // ---- plans: one allocation, one copy; a run is three launches; destroy frees the allocation
    {   // 11 x 11, shave 4: one block, one tile.  40 bytes of item, 8 + 8 of map, 2 doubles
        const mulut_eval_item one = item(5, 7, 11, 11, PB, PB);
        mulut_eval_plan *p = nullptr;
        expect("create 1 item", mulut_eval_plan_create(0, &one, 1, 4, &p), MULUT_OK, "malloc 72 | memcpy 56", p != nullptr);
        expect("run null plan", mulut_eval_plan_run(nullptr, kGt, kOut, kSums, nullptr), MULUT_EINVAL, "");
        expect("run null gt", mulut_eval_plan_run(p, nullptr, kOut, kSums, nullptr), MULUT_EINVAL, "");
        expect("run null out", mulut_eval_plan_run(p, kGt, nullptr, kSums, nullptr), MULUT_EINVAL, "");
        expect("run null sums", mulut_eval_plan_run(p, kGt, kOut, nullptr, nullptr), MULUT_EINVAL, "");
        expect("run 1 item", mulut_eval_plan_run(p, kGt, kOut, kSums, nullptr), MULUT_OK,
               "launch sse_list_kernel grid 1,1,1 block 256,1,1 lds 0 | launch ssim_list_kernel grid 1,1,1 block 256,1,1 lds 0 | "
               "launch eval_sum_kernel grid 1,1,1 block 64,1,1 lds 0");
        expect("destroy 1 item", mulut_eval_plan_destroy(p), MULUT_OK, "free 72");
    }
    {   // 521 x 520, shave 4: 513 x 512 interior pixels = 1026 blocks of 256, capped at 1024; 511 x 510 windows = 16 x 16 tiles.
        // 43 x 43: 35 x 35 interior = 5 blocks; 33 x 33 windows = 4 tiles
        const mulut_eval_item two[2] = {item(0, 0, 521, 520, PB, PB), item(521 * 520 * 3 + 1, 521 * 520 * 3 + 1, 43, 43, PB, PB)};
        mulut_eval_plan *p = nullptr;
        expect("create 2 items", mulut_eval_plan_create(0, two, 2, 4, &p), MULUT_OK, "malloc 20704 | memcpy 10392", p != nullptr);
        expect("run 2 items", mulut_eval_plan_run(p, kGt, kOut, kSums, (void *)0x77), MULUT_OK,
               "launch sse_list_kernel grid 1029,1,1 block 256,1,1 lds 0 | launch ssim_list_kernel grid 260,1,1 block 256,1,1 lds 0 | "
               "launch eval_sum_kernel grid 2,1,1 block 64,1,1 lds 0");
        expect("destroy 2 items", mulut_eval_plan_destroy(p), MULUT_OK, "free 20704");
    }
    {   // the five benchmark sets hold 328 images
        std::vector<mulut_eval_item> items;
        for (int i = 0; i < 328; ++i) items.push_back(item(768LL * i + 1, 768LL * i + 3, 16, 16, 768 * 328 + 8, 768 * 328 + 8));
        mulut_eval_plan *p = nullptr;
        expect("create 328 items", mulut_eval_plan_create(0, items.data(), 328, 4, &p), MULUT_OK, "malloc 23616 | memcpy 18368", p != nullptr);
        expect("run 328 items", mulut_eval_plan_run(p, kGt, kOut, kSums, nullptr), MULUT_OK,
               "launch sse_list_kernel grid 328,1,1 block 256,1,1 lds 0 | launch ssim_list_kernel grid 328,1,1 block 256,1,1 lds 0 | "
               "launch eval_sum_kernel grid 328,1,1 block 64,1,1 lds 0");
        expect("destroy 328 items", mulut_eval_plan_destroy(p), MULUT_OK, "free 23616");
    }
    expect("destroy null", mulut_eval_plan_destroy(nullptr), MULUT_EINVAL, "");
    // ---- mulut_eval_finish: host only
    {
        double ps = 0, ss = 0;
        expect("finish null psnr", mulut_eval_finish(1.0, 1.0, 16, 16, 4, nullptr, &ss), MULUT_EINVAL, "");
        expect("finish null ssim", mulut_eval_finish(1.0, 1.0, 16, 16, 4, &ps, nullptr), MULUT_EINVAL, "");
        expect("finish shave -1", mulut_eval_finish(1.0, 1.0, 16, 16, -1, &ps, &ss), MULUT_EINVAL, "");
        expect("finish H 10", mulut_eval_finish(1.0, 1.0, 10, 16, 4, &ps, &ss), MULUT_ESHAPE, "");
        expect("finish shave 8", mulut_eval_finish(1.0, 1.0, 16, 16, 8, &ps, &ss), MULUT_ESHAPE, "");
        // sse 64 over 8 x 8 pixels: rmse 1, 20 log10(255); 36 windows of SSIM 0.5 each
        expect("finish", mulut_eval_finish(64.0, 18.0, 16, 16, 4, &ps, &ss), MULUT_OK, "", ps == 20.0 * std::log10(255.0) && ss == 0.5);
        expect("finish sse 0", mulut_eval_finish(0.0, 36.0, 16, 16, 4, &ps, &ss), MULUT_OK, "", std::isinf(ps) && ps > 0 && ss == 1.0);
    }
    // ---- mulut_ft_val_pack: the refusals of the crop call, then one lane per pixel
    expect("pack null pred", mulut_ft_val_pack(0, nullptr, 4, 4, kBytes, nullptr), MULUT_EINVAL, "");
    expect("pack null out", mulut_ft_val_pack(0, kPred, 4, 4, nullptr, nullptr), MULUT_EINVAL, "");
    for (int v = 0; v >= -1; --v) {
        expect("pack H <= 0", mulut_ft_val_pack(0, kPred, v, 4, kBytes, nullptr), MULUT_EINVAL, "");
        expect("pack W <= 0", mulut_ft_val_pack(0, kPred, 4, v, kBytes, nullptr), MULUT_EINVAL, "");
    }
    expect("pack null pred, 2^31 bytes", mulut_ft_val_pack(0, nullptr, 1 << 16, 1 << 16, kBytes, nullptr), MULUT_EINVAL, "");
    expect("pack 2^31 bytes or more", mulut_ft_val_pack(0, kPred, 26755, 26755, kBytes, nullptr), MULUT_EUNSUPPORTED, "");
    expect("pack (2^31 - 1)^2 pixels", mulut_ft_val_pack(0, kPred, 0x7fffffff, 0x7fffffff, kBytes, nullptr), MULUT_EUNSUPPORTED, "");
    expect("pack device 3", mulut_ft_val_pack(3, kPred, 4, 4, kBytes, nullptr), MULUT_ENODEVICE, "");
    expect("pack 1 x 1", mulut_ft_val_pack(0, kPred, 1, 1, kBytes, nullptr), MULUT_OK, "launch ft_val_pack_kernel grid 1,1,1 block 256,1,1 lds 0");
    expect("pack 12 x 13", mulut_ft_val_pack(0, kPred, 12, 13, kBytes, (void *)0x77), MULUT_OK, "launch ft_val_pack_kernel grid 1,1,1 block 256,1,1 lds 0");
    expect("pack 1024 x 768", mulut_ft_val_pack(0, kPred, 768, 1024, kBytes, nullptr), MULUT_OK, "launch ft_val_pack_kernel grid 3072,1,1 block 256,1,1 lds 0");
    expect("pack below 2^31 bytes", mulut_ft_val_pack(0, kPred, 26754, 26754, kBytes, nullptr), MULUT_OK,
           "launch ft_val_pack_kernel grid 2796003,1,1 block 256,1,1 lds 0");
    printf("%d unexpected\n", g_wrong);
    return g_wrong;
}
