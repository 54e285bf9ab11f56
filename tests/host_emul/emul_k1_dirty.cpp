// CPU harness of stage_u1t_kernel's neighbourhood test and sort keys (tests/test_k1_dirty_cpu.py): mulut_core.h's host twins of the
// one-hot test (tube1_onehot, tube1_span_gt1, tube1_dirty4) and the key expression the device computes with one three-input
// bit operation.  TEST ONLY.
#include <cstdint>

#include "../../mulut_amd/csrc/mulut_core.h"

using namespace mulut;

// per half of T: tube1_span_gt1's verdict (0 / 1 in bits 0 and 16)
extern "C" uint32_t k1_span_gt1(uint32_t T) { return tube1_span_gt1(T); }
extern "C" uint32_t k1_onehot(uint32_t code_pk) { return tube1_onehot(code_pk); }

// codes [n][5][8] (f << 12 | h each) -> out[n] = tube1_dirty4 of the window as the kernel holds it: dword d of a row = columns 2 d
// (low half) and 2 d + 1
extern "C" void k1_dirty_windows(const uint16_t *codes, int n, uint8_t *out) {
    for (int i = 0; i < n; ++i) {
        uint32_t win[5][4];
        for (int q = 0; q < 5; ++q)
            for (int d = 0; d < 4; ++d) win[q][d] = (uint32_t)codes[(i * 5 + q) * 8 + 2 * d] | ((uint32_t)codes[(i * 5 + q) * 8 + 2 * d + 1] << 16);
        out[i] = (uint8_t)tube1_dirty4(win);
    }
}

// a three-input bit operation by its truth table, bit by bit: result bit = table bit (4 a + 2 b + c) -- the first operand counts 0xF0,
// the second 0xCC, the third 0xAA
static uint32_t bitop3_ref(uint32_t a, uint32_t b, uint32_t c, uint32_t table) {
    uint32_t r = 0;
    for (int i = 0; i < 32; ++i) r |= ((table >> ((((a >> i) & 1u) << 2) | (((b >> i) & 1u) << 1) | ((c >> i) & 1u))) & 1u) << i;
    return r;
}
// every 16-bit half value (in both halves, the other half its complement) x the four strides of slot size `slot`: the key expression
// against table 0xEA on (code, mask, stride).  Returns the number of mismatches; *checked = keys compared.
extern "C" long k1_key_check(int slot, long *checked) {
    const int strides[4] = {kTubeSA, kTubeSB, kTubeSC, kTubeSD};
    long bad = 0;
    *checked = 0;
    for (int s = 0; s < 4; ++s)
        for (uint32_t v = 0; v < 65536u; ++v) {
            const uint32_t code = v | ((~v & 0xFFFFu) << 16), stride = (uint32_t)(strides[s] * slot);
            const uint32_t want = bitop3_ref(code, 0xF000F000u, pk_dup(stride), 0xEAu);
            bad += tube1_key(code, stride) != want;
            bad += (want & 0x0FFF0FFFu) != pk_dup(stride) || (want >> 28) != ((code >> 28) & 15u) || ((want >> 12) & 15u) != ((code >> 12) & 15u);
            ++*checked;
        }
    return bad;
}
