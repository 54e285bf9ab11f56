// CPU harness of stage_tube2_kernel's one-set form (tests/test_tube2_oneset_cpu.py): the rotation-closed placement of mulut_core.h
// (tube4r_*) and the arithmetic of one accumulator set against the two-set form and against plain integers.  TEST ONLY.
#include <cmath>
#include <cstdint>

#include "../../mulut_amd/csrc/mulut_core.h"

using namespace mulut;

extern "C" int oneset_row_elem(int r, int sy, int sx) { return row_elem(r, sy, sx, 4); }
// place of block position p (and of row element p in a slot): out = plane, dword, half
extern "C" void oneset_place(int p, int *out) {
    out[0] = tube4r_plane(p);
    out[1] = tube4r_dword(p);
    out[2] = tube4r_half(p);
}
extern "C" int oneset_pos(int plane, int dword, int half) { return tube4r_pos(plane, dword, half); }
// rotation r, row plane: out = accumulator plane, halves swapped
extern "C" void oneset_rot(int r, int plane, int *out) {
    out[0] = tube4r_acc_plane(r, plane);
    out[1] = tube4r_swap(r, plane);
}

// the kernel's staging step: a slot of the plain band (16 fields e[]) -> its eight dwords in the rotation-closed order (LO plane, HI plane)
extern "C" void oneset_from_plain(const uint16_t *e, uint32_t *out) {
    uint32_t lo[4], hi[4], rlo[4], rhi[4];
    for (int k = 0; k < 4; ++k) {
        lo[k] = (uint32_t)e[4 * k] | ((uint32_t)e[4 * k + 2] << 16);
        hi[k] = (uint32_t)e[4 * k + 1] | ((uint32_t)e[4 * k + 3] << 16);
    }
    tube4r_from_plain(lo, hi, rlo, rhi);
    for (int k = 0; k < 4; ++k) {
        out[k] = rlo[k];
        out[4 + k] = rhi[k];
    }
}

static uint32_t mac(int half, bool swap, uint32_t x, uint32_t wpk, uint32_t acc) {
    if (swap) return half ? pk_mad_w_swap<1>(x, wpk, acc) : pk_mad_w_swap<0>(x, wpk, acc);
    return half ? pk_mad_w<1>(x, wpk, acc) : pk_mad_w<0>(x, wpk, acc);
}
static uint32_t field2(int e, const uint32_t (&lo)[4], const uint32_t (&hi)[4]) {      // the kernel's tube_field on the plain layout
    const uint32_t word = (e & 1) ? hi[e >> 2] : lo[e >> 2];
    return (e & 2) ? (word >> 16) : (word & 0xFFFFu);
}

// n cases of 12 passes (pass = pattern * 4 + rotation) of a final stage with M modes.  rows[case][pass][j][e]: the 16-bit field of
// element e of path row j (value + 128, times the pattern's multiplicity), w[case][pass][j]: the weights (sum 16).  Out, 16 bytes per
// case in block order: two = two accumulator sets on the plain layout (the kernel's blocks A / B and its signed epilogue), one = one set
// on the rotation-closed layout, ref = integer sums and the integer round-half-even.
extern "C" void oneset_run(const uint16_t *rows, const uint8_t *w, long n, int M, uint8_t *two, uint8_t *one, uint8_t *ref) {
    const uint32_t nb = pk_dup((uint32_t)(65536 - 128 * kQ * 4 * M));
    const DivMagic dm = make_div_magic((uint32_t)stage_divisor(M, true));
    const float inv_d = 1.0f / (float)dm.d;
    for (long c = 0; c < n; ++c) {
        const uint16_t *R = rows + c * 12 * 5 * 16;
        const uint8_t *W = w + c * 12 * 5;
        uint32_t lo02[4], hi02[4], lo13[4] = {0, 0, 0, 0}, hi13[4] = {0, 0, 0, 0}, acc[2][4];
        for (int k = 0; k < 4; ++k) lo02[k] = hi02[k] = acc[0][k] = acc[1][k] = nb;
        int sum[16];
        for (int p = 0; p < 16; ++p) sum[p] = -128 * kQ * 4 * M;
        for (int pat = 0; pat < 3; ++pat)
            for (int rc = 0; rc < 2; ++rc)            // a pair: rotation rc with the low halves of the packed weights, rc + 2 with the high ones
                for (int half = 0; half < 2; ++half) {
                    const int r = rc + 2 * half, pass = pat * 4 + r;
                    for (int j = 0; j < 5; ++j) {
                        const uint16_t *e = R + (pass * 5 + j) * 16;
                        const uint32_t wpk = (uint32_t)W[(pat * 4 + rc) * 5 + j] | ((uint32_t)W[(pat * 4 + rc + 2) * 5 + j] << 16);
                        // two sets, plain layout
                        uint32_t rlo[4], rhi[4];
                        for (int k = 0; k < 4; ++k) {
                            rlo[k] = (uint32_t)e[4 * k] | ((uint32_t)e[4 * k + 2] << 16);
                            rhi[k] = (uint32_t)e[4 * k + 1] | ((uint32_t)e[4 * k + 3] << 16);
                        }
                        uint32_t(&lo)[4] = rc ? lo13 : lo02;
                        uint32_t(&hi)[4] = rc ? hi13 : hi02;
                        if (half) swar_fma_x4_rev<1>(lo, hi, rlo, rhi, wpk);
                        else swar_fma_x4<0>(lo, hi, rlo, rhi, wpk);
                        // one set, rotation-closed layout
                        for (int plane = 0; plane < 2; ++plane)
                            for (int k = 0; k < 4; ++k) {
                                const uint32_t x = (uint32_t)e[tube4r_pos(plane, k, 0)] | ((uint32_t)e[tube4r_pos(plane, k, 1)] << 16);
                                uint32_t &a = acc[tube4r_acc_plane(r, plane)][k];
                                a = mac(half, tube4r_swap(r, plane) != 0, x, wpk, a);
                            }
                        for (int p = 0; p < 16; ++p) sum[p] += (int)W[pass * 5 + j] * (int)e[row_elem(r, p >> 2, p & 3, 4)];
                    }
                }
        for (int p = 0; p < 16; ++p) {
            const int sy = p >> 2, sx = p & 3;
            const uint32_t s = field2(4 * sy + sx, lo02, hi02) + field2((3 - sx) * 4 + sy, lo13, hi13);
            two[c * 16 + p] = (uint8_t)rhe_clip_u8_f32((int)(int16_t)(uint16_t)s, inv_d);
            const uint32_t word = acc[tube4r_plane(p)][tube4r_dword(p)];
            const uint16_t f = (uint16_t)(tube4r_half(p) ? word >> 16 : word & 0xFFFFu);
            one[c * 16 + p] = (uint8_t)rhe_clip_u8_f32((int)(int16_t)f, inv_d);
            ref[c * 16 + p] = (uint8_t)rhe_clip_u8(sum[p], dm);
        }
    }
}
