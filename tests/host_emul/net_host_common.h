// net_host_common.h -- what net_host.cpp and net_train_host.cpp share: the line-per-check bookkeeping over fake_hip.cpp's event trace and
// a unit's random weights.  Test code only: not part of the library's sources.
#ifndef NET_HOST_COMMON_H_
#define NET_HOST_COMMON_H_

#include <cmath>
#include <cstdio>
#include <string>
#include <vector>

#include "../../include/mulut.h"
#include "../../mulut_amd/csrc/mulut_net.h"

std::vector<std::string> &fake_hip_events();
void fake_hip_flush();

static int g_wrong = 0;

static void expect(const char *what, long long rc, long long want_rc, const std::string &want_event) {
    fake_hip_flush();
    std::vector<std::string> &ev = fake_hip_events();
    std::string got;
    for (auto &s : ev) got += (got.empty() ? "" : " | ") + s;
    ev.clear();
    const bool ok = rc == want_rc && got == want_event;
    printf("%s -> %lld [%s]%s\n", what, rc, got.c_str(), ok ? "" : "   UNEXPECTED");
    g_wrong += !ok;
}

static void check(const char *what, bool ok) {
    printf("%s%s\n", what, ok ? " ok" : "   UNEXPECTED");
    g_wrong += !ok;
}

struct Weights {
    int nf, u;
    std::vector<float> w[6], b[6];
    const float *wp[6], *bp[6];
};

static unsigned g_seed;      // each program's main sets it first
static float rnd() {         // in [-1, 1)
    g_seed = g_seed * 1664525u + 1013904223u;
    return (float)((g_seed >> 8) & 0xffff) / 32768.0f - 1.0f;
}

// trained: weights of 1.5 / sqrt(fan-in) and biases of 0.2 times rnd(), the magnitudes of a network that computes something; else rnd() itself
static void make(Weights &m, int nf, int u, bool trained) {
    m.nf = nf;
    m.u = u;
    for (int l = 0; l < 6; ++l) {
        const int in = mulut::net_layer_in(nf, l + 1), out = mulut::net_layer_out(nf, u, l + 1);
        m.w[l].resize((size_t)in * out);
        m.b[l].resize((size_t)out);
        const float s = trained ? 1.5f / std::sqrt((float)in) : 1.0f;
        for (auto &v : m.w[l]) v = rnd() * s;
        for (auto &v : m.b[l]) v = rnd() * (trained ? 0.2f : 1.0f);
        m.wp[l] = m.w[l].data();
        m.bp[l] = m.b[l].data();
    }
}

#endif
