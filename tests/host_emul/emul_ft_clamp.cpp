// CPU unit-test harness for ft_pass_setup() of mulut_amd/csrc/mulut_ft.h, the per-pass set-up of every interval-4 fine-tune kernel
// -- TEST ONLY, never a product path.  It runs the set-up the kernels run (clamped = 1) and, beside it, the set-up as it was before
// the MSB of a key was clamped into 0 .. L - 2, restated HERE and nowhere in the library (clamped = 0): the test holds the two
// equal for every key value the ABI allows, and the clamped one inside the table and the tube band for every other value.
#include <cstddef>
#include <cstdint>

#include "../../mulut_amd/csrc/mulut_ft.h"

using namespace mulut;

// the set-up without the clamp.  For a key outside 0..255 (int)hf leaves 0 .. 15 and the rows leave the table: such keys are
// only ever given to the clamped form
static void pass_setup_unclamped(const float *plane, int H, int W, int y, int x, int r, const int (&di)[3], const int (&dj)[3], FtPass &p) {
    int pix[4], h[4];
    float f[4];
    pix[0] = y * W + x;
    for (int k = 0; k < 3; ++k) {
        int dy, dx;
        sample_offset(r, di[k], dj[k], dy, dx);
        pix[k + 1] = imin(imax(y + dy, 0), H - 1) * W + imin(imax(x + dx, 0), W - 1);
    }
    for (int k = 0; k < 4; ++k) {
        const float v = plane[pix[k]];
        const float hf = floorf(v / 16.0f);
        h[k] = (int)hf;
        f[k] = v - 16.0f * hf;
    }
    const int ord = ft_order_code(f[0], f[1], f[2], f[3]);
    p.ord = ord;
    float fs[4];
    ft_sort_lsb(f, fs);
    const int row_stride[4] = {17 * 17 * 17, 17 * 17, 17, 1}, tube_stride[4] = {27, 18, 12, 8};
    p.idx[0] = h[0] * row_stride[0] + h[1] * row_stride[1] + h[2] * row_stride[2] + h[3];
    p.tslot[0] = h[0] * tube_stride[0] + h[1] * tube_stride[1] + h[2] * tube_stride[2] + h[3] * tube_stride[3];
    for (int j = 0; j < 4; ++j) {
        const int key = (ord >> (2 * j)) & 3;
        p.idx[j + 1] = p.idx[j] + row_stride[key];
        p.tslot[j + 1] = p.tslot[j] + tube_stride[key];
    }
    const int hx = imax(imax(h[0], h[1]), imax(h[2], h[3])), hn = imin(imin(h[0], h[1]), imin(h[2], h[3]));
    p.in_tube = hx - hn <= 1 && hn >= 0 && hx <= 15;
    ft_weights(16.0f, fs, p.wt);
}

// every site of one H x W plane under the four rotations of one pattern (di, dj: the offsets of keys b, c, d).
// idx, wt, tslot: [H * W * 4][5]; in_tube, ord: [H * W * 4]; pass (y, x, r) is entry (y * W + x) * 4 + r
extern "C" void emul_ft4_passes(const float *plane, int H, int W, const int *di, const int *dj, int clamped, int *idx, float *wt, int *tslot,
                                int *in_tube, int *ord) {
    const int pdi[3] = {di[0], di[1], di[2]}, pdj[3] = {dj[0], dj[1], dj[2]};
    for (int y = 0; y < H; ++y)
        for (int x = 0; x < W; ++x)
            for (int r = 0; r < 4; ++r) {
                FtPass p;
                if (clamped) ft_pass_setup(plane, H, W, y, x, r, pdi, pdj, p);
                else pass_setup_unclamped(plane, H, W, y, x, r, pdi, pdj, p);
                const size_t i = ((size_t)y * W + x) * 4 + r;
                for (int j = 0; j < 5; ++j) {
                    idx[5 * i + j] = p.idx[j];
                    wt[5 * i + j] = p.wt[j];
                    tslot[5 * i + j] = p.tslot[j];
                }
                in_tube[i] = p.in_tube ? 1 : 0;
                ord[i] = p.ord;
            }
}

// n key quadruples (a, b, c, d) straight into the set-up the kernels run: each as the 2 x 2 plane [a b; c d], whose site (0, 0) reads
// exactly these four keys under pattern s and rotation 0.  idx, tslot: [n][5]; ord: [n]
extern "C" void emul_ft4_quads(const float *v, long n, int *idx, int *tslot, int *ord) {
    const int di[3] = {0, 1, 1}, dj[3] = {1, 0, 1};
    for (long i = 0; i < n; ++i) {
        FtPass p;
        ft_pass_setup(v + 4 * i, 2, 2, 0, 0, 0, di, dj, p);
        for (int j = 0; j < 5; ++j) {
            idx[5 * i + j] = p.idx[j];
            tslot[5 * i + j] = p.tslot[j];
        }
        ord[i] = p.ord;
    }
}

extern "C" int emul_ft4_rows(void) { return kRows; }
extern "C" int emul_ft4_tube_slots(void) { return kTubeSlots; }
