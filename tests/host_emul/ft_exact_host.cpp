// ft_exact_host.cpp -- the host model of mulut_ft_exact_stage_backward: the arithmetic of mulut_amd/csrc/mulut_ft_exact.h (with
// mulut_ft.h and mulut_ft_interval.h) compiled by g++ -ffp-contract=off and walked one site at a time with plain int64 adds.  A CPU
// test program with its own main (tests/ft_fixed_cases.py builds it under AddressSanitizer and UndefinedBehaviorSanitizer and runs
// it), not a product path.
//
//   ft_exact_host CASE OUT      reads a case, writes the expected grad_wq[0..M) and grad_x as raw float32, prints one line:
//                               "gmax_bits S_w S_x max|table sum| max|input sum|"
// CASE: int32 { magic, interval, u, is_last, B, C, H, W, M, order, seed, has_prior }, char modes[8], then float32 tables [M][rows][u*u],
// x [B][C][H][W], grad_out [B][C][H*u][W*u], uint16 inside [B][C][H][W] and, with has_prior, what grad_wq and grad_x hold before the
// call (else zeros).  order: 0 the sites in ascending order, 1 descending, 2 shuffled by `seed` -- the bytes written must not depend on it.
// Aborts when an accumulator leaves +-2^62: the bound the scales of mulut_ft_exact.h are derived for.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../mulut_amd/csrc/mulut_ft_exact.h"

using namespace mulut;

static const int kMagic = 0x46584331;      // "1CXF"

struct Case {
    int interval, u, is_last, B, C, H, W, M, order, seed, has_prior;
    char modes[9];
    std::vector<float> tab, x, gout, gw, gx;
    std::vector<uint16_t> inside;
};

static long long g_max_w = 0, g_max_x = 0;

static void add(std::vector<long long> &acc, long long i, long long t, long long &mx) {
    if (i < 0 || i >= (long long)acc.size()) {
        fprintf(stderr, "index %lld outside the accumulators\n", i);
        abort();
    }
    acc[i] += t;
    const long long m = acc[i] < 0 ? -acc[i] : acc[i];
    if (m > (1ll << kFxAccBits)) {
        fprintf(stderr, "accumulator %lld left +-2^62: %lld\n", i, acc[i]);
        abort();
    }
    mx = m > mx ? m : mx;
}

template <int IV, int U>
static void run(Case &c) {
    constexpr int EL = U * U;
    const long long rows = IvGeom<IV>::rows, nsite = (long long)c.B * c.C * c.H * c.W, per = rows * EL;
    uint32_t gbits = 0;
    for (float v : c.gout) {
        const uint32_t b = (uint32_t)ft_bits(v) & 0x7fffffffu;
        gbits = b > gbits ? b : gbits;
    }
    const int reach = fx_list_reach(c.modes, c.M);
    const int Sw = fx_scale_w(gbits, nsite), Sx = fx_scale_x(gbits, U, c.M, reach, c.H, c.W);
    std::vector<long long> aw((size_t)(c.M * per), 0), ax((size_t)nsite, 0);
    std::vector<long long> order((size_t)nsite);
    for (long long i = 0; i < nsite; ++i) order[(size_t)i] = c.order == 1 ? nsite - 1 - i : i;
    if (c.order == 2) {
        uint64_t state = 0x9E3779B97F4A7C15ull ^ (uint64_t)c.seed;
        for (long long i = nsite - 1; i > 0; --i) {
            state = state * 6364136223846793005ull + 1442695040888963407ull;
            const long long j = (long long)((state >> 33) % (uint64_t)(i + 1));
            const long long t = order[(size_t)i];
            order[(size_t)i] = order[(size_t)j];
            order[(size_t)j] = t;
        }
    }
    const float avg = c.is_last ? (float)c.M : (float)(4 * c.M);
    if (gbits != 0u) {
        for (long long s : order) {
            const int x = (int)(s % c.W), y = (int)((s / c.W) % c.H);
            const long long bc = s / ((long long)c.W * c.H);
            const float *plane = c.x.data() + bc * c.H * c.W;
            float g[EL];
            fx_site_g<U>(c.gout.data() + bc * (long long)(c.H * U) * (c.W * U), c.W, y, x, c.inside[(size_t)s], avg, g);
            for (int m = 0; m < c.M; ++m) {
                int di[3], dj[3];
                if (!pattern_offsets(c.modes[m], di, dj)) abort();
                const float *tab = c.tab.data() + m * per;
                for (int r = 0; r < 4; ++r) {
                    FxPass p;
                    fx_pass<IV>(plane, c.H, c.W, y, x, r, di, dj, p);
                    float dk[4];
                    fx_key_grads<IV, U>(tab, p, r, g, dk);
                    for (int j = 0; j < 5; ++j)
                        for (int eo = 0; eo < EL; ++eo) {
                            const long long t = fx_quant(fx_table_term(p.wt[j], (float)IvGeom<IV>::q, g[eo]), Sw);
                            add(aw, m * per + (long long)p.idx[j] * EL + row_elem(r, eo / U, eo % U, U), t, g_max_w);
                        }
                    for (int k = 0; k < 4; ++k) {
                        int dy = 0, dx = 0;
                        if (k) sample_offset(r, di[k - 1], dj[k - 1], dy, dx);
                        add(ax, bc * c.H * c.W + imin(imax(y + dy, 0), c.H - 1) * c.W + imin(imax(x + dx, 0), c.W - 1), fx_quant(dk[k], Sx), g_max_x);
                    }
                }
            }
        }
    }
    for (size_t i = 0; i < aw.size(); ++i)
        if (aw[i]) c.gw[i] = c.gw[i] + fx_result(aw[i], Sw);
    for (size_t i = 0; i < ax.size(); ++i)
        if (ax[i]) c.gx[i] = c.gx[i] + fx_result(ax[i], Sx);
    printf("%u %d %d %lld %lld\n", gbits, Sw, Sx, g_max_w, g_max_x);
}

template <int IV>
static void run_u(Case &c) {
    switch (c.u) {
        case 1: run<IV, 1>(c); break;
        case 2: run<IV, 2>(c); break;
        case 3: run<IV, 3>(c); break;
        default: run<IV, 4>(c); break;
    }
}

template <class T>
static void get(FILE *f, std::vector<T> &v, size_t n) {
    v.resize(n);
    if (n && fread(v.data(), sizeof(T), n, f) != n) {
        fprintf(stderr, "case file too short\n");
        exit(2);
    }
}

int main(int argc, char **argv) {
    if (argc != 3) {
        fprintf(stderr, "usage: %s CASE OUT\n", argv[0]);
        return 2;
    }
    FILE *f = fopen(argv[1], "rb");
    if (!f) return 2;
    std::vector<int> h;
    get(f, h, 12);
    Case c;
    if (h[0] != kMagic) return 2;
    c.interval = h[1], c.u = h[2], c.is_last = h[3], c.B = h[4], c.C = h[5], c.H = h[6], c.W = h[7], c.M = h[8], c.order = h[9], c.seed = h[10],
    c.has_prior = h[11];
    memset(c.modes, 0, sizeof(c.modes));
    if (fread(c.modes, 1, 8, f) != 8) return 2;
    if (c.interval < 4 || c.interval > 6 || c.u < 1 || c.u > 4 || c.M < 1 || c.M > 8 || (int)strlen(c.modes) != c.M || c.B < 1 || c.C < 1 || c.H < 1 ||
        c.W < 1)
        return 2;
    const size_t per = (size_t)interval_rows(c.interval) * c.u * c.u, nsite = (size_t)c.B * c.C * c.H * c.W;
    get(f, c.tab, c.M * per);
    get(f, c.x, nsite);
    get(f, c.gout, nsite * c.u * c.u);
    get(f, c.inside, nsite);
    if (c.has_prior) {
        get(f, c.gw, c.M * per);
        get(f, c.gx, nsite);
    } else {
        c.gw.assign(c.M * per, 0.0f);
        c.gx.assign(nsite, 0.0f);
    }
    fclose(f);
    if (c.interval == 4) run_u<4>(c);
    else if (c.interval == 5) run_u<5>(c);
    else run_u<6>(c);
    FILE *o = fopen(argv[2], "wb");
    if (!o) return 2;
    const bool ok = fwrite(c.gw.data(), 4, c.gw.size(), o) == c.gw.size() && fwrite(c.gx.data(), 4, c.gx.size(), o) == c.gx.size();
    return fclose(o) == 0 && ok ? 0 : 2;
}
