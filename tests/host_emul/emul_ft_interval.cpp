// CPU unit-test harness for mulut_amd/csrc/mulut_ft_interval.h and the host-compilable part of mulut_ft.h -- TEST ONLY, never a product path.
// It runs the per-pass set-up of the interval-5 / 6 fine-tune kernels (ft_iv_pass: rows, weights, rank order, corner codes) over
// an array of key quadruples, and the order code every fine-tune kernel (interval 4 included) ranks its keys with.  Launch
// geometry, LDS images and the C ABI are covered by the -m gpu tests.
#include <cstddef>
#include <cstdint>

#include "../../mulut_amd/csrc/mulut_ft_interval.h"

using namespace mulut;

template <int IV>
static void passes_iv(const float *v, long n, int *idx, float *wt, int *ord, int *corner) {
    for (long i = 0; i < n; ++i) {
        const float q[4] = {v[4 * i], v[4 * i + 1], v[4 * i + 2], v[4 * i + 3]};
        FtIvPass p;
        ft_iv_pass<IV>(q, p);
        for (int j = 0; j < 5; ++j) {
            idx[5 * i + j] = p.idx[j];
            wt[5 * i + j] = p.wt[j];
            corner[5 * i + j] = ft_iv_corner(p, j);
        }
        for (int j = 0; j < 4; ++j) ord[4 * i + j] = (p.ord >> (2 * j)) & 3;
    }
}

// v: n x 4 key values; idx, wt, corner: n x 5; ord: n x 4 (key of rank j)
extern "C" int emul_ft_interval_passes(int interval, const float *v, long n, int *idx, float *wt, int *ord, int *corner) {
    if (interval == 5) passes_iv<5>(v, n, idx, wt, ord, corner);
    else if (interval == 6) passes_iv<6>(v, n, idx, wt, ord, corner);
    else return -2;
    return 0;
}

// ft_order_code of n quadruples of LSBs (f: n x 4, each >= 0): code[i] = the keys by rank, two bits each
extern "C" void emul_ft_order_code(const float *f, long n, int *code) {
    for (long i = 0; i < n; ++i) code[i] = ft_order_code(f[4 * i], f[4 * i + 1], f[4 * i + 2], f[4 * i + 3]);
}
