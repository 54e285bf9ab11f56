// CPU unit-test harness for mulut_amd/csrc/mulut_interval.h -- TEST ONLY, never a product path.
// It drives the per-site functions the interval-5 / 6 kernels are built from (simplex4_iv, rhe_clip_u8_iv, iv_bias_num,
// iv_div_modes, with pattern_offsets / sample_offset / row_elem of mulut_core.h) over a whole image with plain loops.
// Launch geometry, LDS tiling and the C ABI are covered by the -m gpu tests.
#include <cstddef>
#include <cstdint>

#include "../../mulut_amd/csrc/mulut_interval.h"

using namespace mulut;

static inline int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

template <int IV>
static int stage_iv(const int8_t *const *luts, const char *modes, int M, int is_last, const uint8_t *in_chw, int H, int W, int C,
                    int u, uint8_t *out_hwc) {
    const DivMagic dm = make_div_magic((uint32_t)iv_div_modes(M, is_last != 0));
    const int bias = iv_bias_num<IV>(M, is_last != 0);
    const int uu = u * u, Wo = W * u;
    for (int c = 0; c < C; ++c) {
        const uint8_t *pl = in_chw + (size_t)c * H * W;
        for (int y = 0; y < H; ++y)
            for (int x = 0; x < W; ++x) {
                int K[16] = {0};
                for (int m = 0; m < M; ++m) {
                    int di[3], dj[3];
                    if (!pattern_offsets(modes[m], di, dj)) return -1;
                    for (int r = 0; r < 4; ++r) {
                        int v[3];
                        for (int k = 0; k < 3; ++k) {
                            int dy, dx;
                            sample_offset(r, di[k], dj[k], dy, dx);
                            v[k] = pl[(size_t)clampi(y + dy, 0, H - 1) * W + clampi(x + dx, 0, W - 1)];
                        }
                        int idx[5], w[5];
                        simplex4_iv<IV>(pl[(size_t)y * W + x], v[0], v[1], v[2], idx, w);
                        for (int sy = 0; sy < u; ++sy)
                            for (int sx = 0; sx < u; ++sx) {
                                const int e = row_elem(r, sy, sx, u);
                                for (int j = 0; j < 5; ++j) K[sy * u + sx] += w[j] * (int)luts[m][(size_t)idx[j] * uu + e];
                            }
                    }
                }
                for (int sy = 0; sy < u; ++sy)
                    for (int sx = 0; sx < u; ++sx)
                        out_hwc[((size_t)(y * u + sy) * Wo + (x * u + sx)) * C + c] = (uint8_t)rhe_clip_u8_iv<IV>(K[sy * u + sx] + bias, dm);
            }
    }
    return 0;
}

extern "C" int emul_stage_interval(const int8_t *const *luts, const char *modes, int M, int is_last, const uint8_t *in_chw, int H,
                                   int W, int C, int u, int interval, uint8_t *out_hwc) {
    if (M < 1 || M > 8 || u < 1 || u > 4 || H < 1 || W < 1 || C < 1) return -2;
    if (interval == 5) return stage_iv<5>(luts, modes, M, is_last, in_chw, H, W, C, u, out_hwc);
    if (interval == 6) return stage_iv<6>(luts, modes, M, is_last, in_chw, H, W, C, u, out_hwc);
    return -2;
}

// rhe_clip_u8_iv against exact round-half-even division over every numerator a stage can reach, for M = 1..8, both stage kinds;
// returns the number of mismatches
extern "C" long emul_check_rhe_interval(int interval) {
    long bad = 0;
    for (int M = 1; M <= 8; ++M)
        for (int last = 0; last < 2; ++last) {
            const int q = 1 << interval, d = q * (last ? M : 4 * M), span = 128 * q * 4 * M;
            const DivMagic dm = make_div_magic((uint32_t)iv_div_modes(M, last != 0));
            const int bias = interval == 5 ? iv_bias_num<5>(M, last != 0) : iv_bias_num<6>(M, last != 0);
            for (int K = -span; K <= span; ++K) {
                const long long n = (long long)K + bias;
                long long qf = n >= 0 ? n / d : -((-n + d - 1) / d), rm = n - qf * d;
                if (2 * rm > d || (2 * rm == d && (qf & 1))) ++qf;
                const uint32_t want = (uint32_t)(qf < 0 ? 0 : qf > 255 ? 255 : qf);
                const uint32_t got = interval == 5 ? rhe_clip_u8_iv<5>((int)n, dm) : rhe_clip_u8_iv<6>((int)n, dm);
                bad += got != want;
            }
        }
    return bad;
}
