// abi_tables_host.cpp -- drives mulut_read_table_image beside mulut_set_lut (include/mulut.h) on the CPU against fake_hip.cpp and
// prints, per ABI call, its return code and what it asked of the runtime, in the format of abi_host.cpp.
// tests/test_host_tables_cpu.py builds it with the host half of every file of the library under AddressSanitizer,
// UndefinedBehaviorSanitizer and LeakSanitizer (tools/host_abi.py --driver abi_tables_host), compares the output with
// tests/golden/host_tables_trace.txt and asserts the accessor's contract on the trace itself.
#include <algorithm>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/mulut.h"

std::vector<std::string> &fake_hip_events();
void fake_hip_flush();

static std::vector<int8_t> g_rows;      // 83521 x 16 seeded int8 values: every host table is cut from it

// prints "<call> -> rc" and the events of the call, runs of one repeated line folded; consecutive frees are sorted among themselves
// (the order in which the members of a context die is not behaviour)
static long long done(long long rc, const char *fmt, ...) {
    fake_hip_flush();
    char buf[256];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    std::vector<std::string> &ev = fake_hip_events();
    for (size_t i = 0; i < ev.size();) {
        size_t j = i;
        while (j < ev.size() && ev[j].compare(0, 5, "free ") == 0) ++j;
        std::sort(ev.begin() + (long)i, ev.begin() + (long)j);
        i = j > i ? j : i + 1;
    }
    printf("%s -> %lld\n", buf, rc);
    for (size_t i = 0; i < ev.size();) {
        size_t j = i;
        while (j < ev.size() && ev[j] == ev[i]) ++j;
        if (j - i > 1) printf("  %s x%zu\n", ev[i].c_str(), j - i);
        else printf("  %s\n", ev[i].c_str());
        i = j;
    }
    ev.clear();
    return rc;
}

static int rows_of(int interval) { return interval == 4 ? 83521 : interval == 5 ? 6561 : 625; }

static mulut_ctx *create(const char *name) {
    mulut_ctx *c = nullptr;
    done(mulut_create(0, &c), "create %s", name);
    return c;
}
static void host(mulut_ctx *c, int iv, int s, char m, int v, const char *slot) {
    done(mulut_set_lut(c, s, m, g_rows.data(), rows_of(iv), v), "set_lut iv%d s%d %c v%d %s", iv, s, m, v, slot);
}
static void images(mulut_ctx *c, int s, char m) {
    static std::vector<uint8_t> buf(64);
    for (int which = 0; which < 3; ++which)
        done(mulut_read_table_image(c, s, m, which, buf.data(), (long long)buf.size(), nullptr), "read_table_image s%d %c image %d, 64 bytes", s, m, which);
}

int main() {
    g_rows.resize((size_t)83521 * 16);
    uint32_t seed = 12345u;
    for (auto &v : g_rows) {
        seed = seed * 1664525u + 1013904223u;
        v = (int8_t)(seed >> 24);
    }
    printf("version %d\n", mulut_version());
    // every shape set into an empty slot, read back (sizes; 64 bytes each), rewritten, replaced by another shape
    for (int iv : {4, 5, 6}) {
        printf("# interval %d\n", iv);
        mulut_ctx *a = create("A");
        done(mulut_configure(a, 2, "sdy", 4, iv), "configure A 2 sdy x4 iv%d", iv);
        int stage = 1;
        for (char m : {'s', 'e'})
            for (int v : {1, 4, 9, 16}) {
                images(a, stage, m);
                host(a, iv, stage, m, v, "empty");
                images(a, stage, m);
                ++stage;
            }
        host(a, iv, 4, 's', 16, "rewrite");
        images(a, 4, 's');
        host(a, iv, 4, 's', 1, "other-shape");
        images(a, 4, 's');
        printf("# interval %d: sizes, refused calls\n", iv);
        uint8_t byte;
        done(mulut_read_table_image(a, 1, 's', 0, nullptr, 0, nullptr), "read_table_image s1 s image 0, size only");
        done(mulut_read_table_image(a, 3, 'd', 0, &byte, 1, nullptr), "read_table_image s3 d image 0 of a slot never set");
        done(mulut_read_table_image(nullptr, 1, 's', 0, &byte, 1, nullptr), "refused: no context");
        done(mulut_read_table_image(a, 1, 's', 3, &byte, 1, nullptr), "refused: image 3");
        done(mulut_read_table_image(a, 1, 's', -1, &byte, 1, nullptr), "refused: image -1");
        done(mulut_read_table_image(a, 1, 's', 0, nullptr, 1, nullptr), "refused: no buffer");
        done(mulut_read_table_image(a, 1, 's', 0, &byte, -1, nullptr), "refused: negative size");
        done(mulut_read_table_image(a, 0, 's', 0, &byte, 1, nullptr), "refused: stage 0");
        done(mulut_read_table_image(a, 9, 's', 0, &byte, 1, nullptr), "refused: stage 9");
        done(mulut_read_table_image(a, 1, 'q', 0, &byte, 1, nullptr), "refused: pattern q");
        done(mulut_destroy(a), "destroy A");
    }
    return 0;
}
