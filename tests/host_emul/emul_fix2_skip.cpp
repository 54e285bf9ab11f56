// CPU harness of stage_up_fix2_kernel's entry-level skip (tests/test_fix2_skip_cpu.py): the sixteen lanes of a group, lane ln holding
// pass (mode ln >> 2, rotation ln & 3), take the anchor and the pass's three neighbours with the kernel's clamps and evaluate
// mulut_core.h's fix2_pass_far.  TEST ONLY.
#include <cstdint>

#include "../../mulut_amd/csrc/mulut_core.h"

using namespace mulut;

static int clampi(int v, int lo, int hi) { return v < lo ? lo : v > hi ? hi : v; }

// Every sample of rows [oy0, oy1) of a single-channel H x W image (row r of the frame at img + r * W), M <= 4 modes with the pattern offsets
// di / dj [M][3]: far[(y - oy0) * W + x] = the group's quarter of the ballot, bit ln set iff lane ln's pass is far.  The rows a launch may
// read are oy0 - 2 .. oy1 + 1 inside the frame, as the kernels clamp them.
extern "C" void fix2_far_map(const uint8_t *img, int H, int W, int oy0, int oy1, int M, const int *di, const int *dj, uint16_t *far) {
    constexpr int kHalo = 2;      // mulut_dev.h: the reach of one stage
    const int ylo = imax(oy0 - kHalo, 0), yhi = imin(oy1 + kHalo, H) - 1;
    for (int y = oy0; y < oy1; ++y)
        for (int x = 0; x < W; ++x) {
            const int va = img[y * W + x];
            uint32_t bits = 0;
            for (int ln = 0; ln < 16; ++ln) {
                int v[3] = {va, va, va};      // a lane without a pass votes "not far"
                if (ln < 4 * M) {
                    const int m = ln >> 2, r = ln & 3;
                    for (int k = 0; k < 3; ++k) {
                        int dy, dx;
                        sample_offset(r, di[3 * m + k], dj[3 * m + k], dy, dx);
                        v[k] = img[clampi(y + dy, ylo, yhi) * W + clampi(x + dx, 0, W - 1)];
                    }
                }
                if (fix2_pass_far(va, v[0], v[1], v[2])) bits |= 1u << ln;
            }
            far[(y - oy0) * W + x] = (uint16_t)bits;
        }
}

extern "C" int fix2_reach() { return kFix2Reach; }
