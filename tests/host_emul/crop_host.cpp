// crop_host.cpp -- the host half of mulut_ft_crop_batch (mulut_amd/csrc/mulut_ft_data.hip) on the CPU against fake_hip.cpp: every
// refusal code, each decided without a launch, and the launch configuration at the smallest call and at the benchmark's batch.
// tests/test_crop_cpu.py builds it under AddressSanitizer and UndefinedBehaviorSanitizer and runs it as a program; it prints one line
// per call and exits with the number of lines that are not what this file expects.  The kernel never runs, so the device pointers
// are made-up addresses that nothing follows.
#include <cstdio>
#include <string>
#include <vector>

#include "../../include/mulut.h"

std::vector<std::string> &fake_hip_events();
void fake_hip_flush();

static const unsigned char *const kPool = (const unsigned char *)0x10000000;
static const mulut_ft_pair *const kPairs = (const mulut_ft_pair *)0x20000000;
static const int *const kDraws = (const int *)0x30000000;
static float *const kIm = (float *)0x40000000, *const kLb = (float *)0x50000000;
static int *const kBad = (int *)0x60000000;
static int g_wrong = 0;

// one call: its return code and its only event (a refusal has none)
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

int main() {
    static_assert(sizeof(mulut_ft_pair) == 40, "mulut_ft_pair is 40 bytes");
    const long long PB = 1 << 20;
    // NULL pointers, one at a time
    expect("null pool", mulut_ft_crop_batch(0, nullptr, PB, kPairs, 3, kDraws, 8, 48, 4, kIm, kLb, kBad, nullptr), MULUT_EINVAL, "");
    expect("null pairs", mulut_ft_crop_batch(0, kPool, PB, nullptr, 3, kDraws, 8, 48, 4, kIm, kLb, kBad, nullptr), MULUT_EINVAL, "");
    expect("null draws", mulut_ft_crop_batch(0, kPool, PB, kPairs, 3, nullptr, 8, 48, 4, kIm, kLb, kBad, nullptr), MULUT_EINVAL, "");
    expect("null im", mulut_ft_crop_batch(0, kPool, PB, kPairs, 3, kDraws, 8, 48, 4, nullptr, kLb, kBad, nullptr), MULUT_EINVAL, "");
    expect("null lb", mulut_ft_crop_batch(0, kPool, PB, kPairs, 3, kDraws, 8, 48, 4, kIm, nullptr, kBad, nullptr), MULUT_EINVAL, "");
    // non-positive sizes
    for (int v = 0; v >= -1; --v) {
        expect("B <= 0", mulut_ft_crop_batch(0, kPool, PB, kPairs, 3, kDraws, v, 48, 4, kIm, kLb, kBad, nullptr), MULUT_EINVAL, "");
        expect("sz <= 0", mulut_ft_crop_batch(0, kPool, PB, kPairs, 3, kDraws, 8, v, 4, kIm, kLb, kBad, nullptr), MULUT_EINVAL, "");
        expect("n_pairs <= 0", mulut_ft_crop_batch(0, kPool, PB, kPairs, v, kDraws, 8, 48, 4, kIm, kLb, kBad, nullptr), MULUT_EINVAL, "");
        expect("pool_bytes <= 0", mulut_ft_crop_batch(0, kPool, v, kPairs, 3, kDraws, 8, 48, 4, kIm, kLb, kBad, nullptr), MULUT_EINVAL, "");
    }
    // a bad argument of the first kind wins over one of the later kinds
    expect("null pool, scale 9", mulut_ft_crop_batch(0, nullptr, PB, kPairs, 3, kDraws, 8, 48, 9, kIm, kLb, kBad, nullptr), MULUT_EINVAL, "");
    // scale outside 1..4
    for (int s : {0, 5, -1})
        expect("scale", mulut_ft_crop_batch(0, kPool, PB, kPairs, 3, kDraws, 8, 48, s, kIm, kLb, kBad, nullptr), MULUT_EUNSUPPORTED, "");
    // B * (sz * scale)^2 at or above 2^31: exactly 2^31, the first size that is, and sizes whose side, square or product leave 32 bits
    expect("2^31 floats", mulut_ft_crop_batch(0, kPool, PB, kPairs, 3, kDraws, 1 << 15, 64, 4, kIm, kLb, kBad, nullptr), MULUT_EUNSUPPORTED, "");
    expect("2^31 floats, B = 1", mulut_ft_crop_batch(0, kPool, PB, kPairs, 3, kDraws, 1, 46341, 1, kIm, kLb, kBad, nullptr), MULUT_EUNSUPPORTED, "");
    expect("sz * scale beyond int", mulut_ft_crop_batch(0, kPool, PB, kPairs, 3, kDraws, 1, 0x7fffffff, 4, kIm, kLb, kBad, nullptr), MULUT_EUNSUPPORTED, "");
    expect("B * n^2 near 2^62", mulut_ft_crop_batch(0, kPool, PB, kPairs, 3, kDraws, 0x7fffffff, 46340, 1, kIm, kLb, kBad, nullptr),
           MULUT_EUNSUPPORTED, "");
    // a device the runtime does not have: the arguments are in order, the device is asked for and refused, nothing is launched
    expect("device 3", mulut_ft_crop_batch(3, kPool, PB, kPairs, 3, kDraws, 8, 48, 4, kIm, kLb, kBad, nullptr), MULUT_ENODEVICE, "");
    // launches, one workgroup per sample and 8 tiles: one tile per plane; the benchmark's batch (256 x (2^2 + 6^2) tiles); unaligned
    // outputs, bad = NULL and a stream change nothing about the configuration; the largest call below the bound
    expect("B 1 sz 1 x1", mulut_ft_crop_batch(0, kPool, PB, kPairs, 1, kDraws, 1, 1, 1, kIm, kLb, kBad, nullptr), MULUT_OK,
           "launch ft_crop_kernel grid 1,1,1 block 256,1,1 lds 0");
    expect("B 256 sz 48 x4", mulut_ft_crop_batch(0, kPool, PB, kPairs, 900, kDraws, 256, 48, 4, kIm, kLb, kBad, nullptr), MULUT_OK,
           "launch ft_crop_kernel grid 1280,1,1 block 256,1,1 lds 0");
    expect("B 8 sz 57 x3", mulut_ft_crop_batch(0, kPool, PB, kPairs, 5, kDraws, 8, 57, 3, kIm + 1, kLb + 3, nullptr, (void *)0x77), MULUT_OK,
           "launch ft_crop_kernel grid 40,1,1 block 256,1,1 lds 0");
    expect("2^31 - 2^12 floats", mulut_ft_crop_batch(0, kPool, PB, kPairs, 3, kDraws, (1 << 19) - 1, 16, 4, kIm, kLb, kBad, nullptr), MULUT_OK,
           "launch ft_crop_kernel grid 524287,1,1 block 256,1,1 lds 0");
    printf("%d unexpected\n", g_wrong);
    return g_wrong;
}
