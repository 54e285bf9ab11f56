// CPU harness of stage_up_fix2_kernel's body for lists of up to four modes (tests/test_fix2_cpu.py): the packed row sums, the
// placement of a pass in the group's two accumulator sets, the finishing map and the entry decode of mulut_core.h (fix2_*, Recip30),
// run the way the kernel runs them -- sixteen lanes, one pass each, sixteen shared dwords.  TEST ONLY.
#include <cstdint>
#include <cstring>

#include "../../mulut_amd/csrc/mulut_core.h"

using namespace mulut;

static int clampi(int v, int lo, int hi) { return v < lo ? lo : v > hi ? hi : v; }

// One sample (y, x) of a single-channel H x W image through a final stage of M <= 4 modes: tab[m] = the device table of mode m
// (value + 128 bytes, 16 per row), di / dj = the modes' pattern offsets [M][3].  out = the 16 bytes of its 4 x 4 block in block order;
// info[0] = the largest 16-bit field any of the sixteen shared dwords held on the way (a set takes two rotations of every mode:
// at most 2 M x 4080), info[1] / info[2] = the smallest / largest sum of two fields the finishing lanes formed (at most 4 M x 4080).
extern "C" void fix2_sample(const uint8_t *img, int H, int W, int y, int x, int M, const uint8_t *const *tab, const int *di, const int *dj,
                            uint8_t *out, int *info) {
    uint32_t lds[16];
    std::memset(lds, 0, sizeof lds);
    const int va = img[y * W + x];
    uint32_t peak = 0;
    for (int ln = 0; ln < 4 * M; ++ln) {        // lane ln: mode ln >> 2, rotation ln & 3
        const int m = ln >> 2, r = ln & 3;
        int v[3];
        for (int k = 0; k < 3; ++k) {
            int dy, dx;
            sample_offset(r, di[3 * m + k], dj[3 * m + k], dy, dx);
            v[k] = img[clampi(y + dy, 0, H - 1) * W + clampi(x + dx, 0, W - 1)];
        }
        int idx[5], w[5];
        simplex4(va, v[0], v[1], v[2], idx, w);
        uint32_t F[4] = {0, 0, 0, 0}, Hs[4] = {0, 0, 0, 0}, X[8];
        for (int j = 0; j < 5; ++j) {
            uint32_t row[4];
            std::memcpy(row, tab[m] + 16 * (size_t)idx[j], 16);
            fix2_mac_row(F, Hs, row, (uint32_t)w[j]);
        }
        fix2_pass_sums(F, Hs, X);
        for (int j = 0; j < 8; ++j) {
            uint32_t &d = lds[fix2_slot(r, j)];
            d += fix2_rotr(X[j], fix2_swap(r));         // the kernel's ds_add_u32: a 32-bit add, halves not separated
            if ((d & 0xFFFFu) > peak) peak = d & 0xFFFFu;
            if ((d >> 16) > peak) peak = d >> 16;
        }
    }
    const int unbias = 128 * kQ * 4 * M;
    const DivMagic dm = make_div_magic((uint32_t)stage_divisor(M, true));
    uint16_t half[32];
    std::memcpy(half, lds, sizeof lds);          // little-endian, as the kernel's 16-bit LDS reads see the dwords
    info[0] = (int)peak;
    info[1] = 1 << 30;
    info[2] = 0;
    for (int p = 0; p < 16; ++p) {
        const int s = (int)half[fix2_field_half(0, p)] + (int)half[fix2_field_half(1, fix2_partner(p))];
        out[p] = (uint8_t)rhe_clip_u8(s - unbias, dm);
        if (s < info[1]) info[1] = s;
        if (s > info[2]) info[2] = s;
    }
}

// Entry decode against / and %: every id < 2^30 that starts or ends a row of width W, and the last id of image k - 1 and the
// first of image k for every image of a 2^30-sample launch.  Returns the number of ids that decode wrongly (0 = none) and, in
// info, [0] whether the multiply-high form was taken, [1] the number of ids checked (low 32 bits), [2] the same, high bits.
static bool decode_ok(uint32_t id, uint32_t W, uint32_t H, const Recip30 &rw, const Recip30 &rwh, bool fast) {
    int x, y, n;
    fix2_decode(id, W, H, rw, rwh, fast, x, y, n);
    return (uint32_t)x == id % W && (uint32_t)y == (id / W) % H && (uint32_t)n == id / (W * H);
}
extern "C" long fix2_decode_check(uint32_t W, uint32_t H, uint32_t *info) {
    const Recip30 rw = make_recip30(W), rwh = make_recip30(W * H);
    const bool fast = rw.exact != 0 && rwh.exact != 0;
    const uint32_t top = (1u << 30) - 1;
    long bad = 0;
    uint64_t checked = 0;
    for (uint64_t s = 0; s <= top; s += W) {           // s starts a row, s + W - 1 ends it
        bad += !decode_ok((uint32_t)s, W, H, rw, rwh, fast);
        const uint64_t e = s + W - 1;
        ++checked;
        if (e != s && e <= top) {
            bad += !decode_ok((uint32_t)e, W, H, rw, rwh, fast);
            ++checked;
        }
    }
    const uint64_t wh = (uint64_t)W * H;
    for (uint64_t k = 1; k * wh <= top; ++k) {
        bad += !decode_ok((uint32_t)(k * wh - 1), W, H, rw, rwh, fast);
        bad += !decode_ok((uint32_t)(k * wh), W, H, rw, rwh, fast);
        checked += 2;
    }
    bad += !decode_ok(top, W, H, rw, rwh, fast);
    info[0] = fast ? 1u : 0u;
    info[1] = (uint32_t)checked;
    info[2] = (uint32_t)(checked >> 32);
    return bad;
}
// the reciprocal alone: magic, shift, exact of a divisor
extern "C" void fix2_recip(uint32_t d, uint32_t *out) {
    const Recip30 r = make_recip30(d);
    out[0] = r.magic;
    out[1] = r.shift;
    out[2] = r.exact;
}
