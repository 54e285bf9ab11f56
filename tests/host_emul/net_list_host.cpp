// net_list_host.cpp -- the host half of mulut_net_plan_* (mulut_amd/csrc/mulut_net_list.hip) on the CPU against fake_hip.cpp: every
// refusal of create and of run, each decided without touching the device (create leaving *plan NULL), the order of the refusal
// classes where two codes can tell it, the allocation, the copy and the launches of plans of 1, 2 and 3 stages, and create / destroy
// pairs that LeakSanitizer watches.  tests/test_net_list_cpu.py builds it under AddressSanitizer and UndefinedBehaviorSanitizer and
// runs it as a program; it prints one line per call and exits with the number of lines that are not what this file expects.
//   net_list_host                              the checks
//   net_list_host tables CH STAGES SCALE HxW.. a plan over images of these sizes, packed back to back in both pools: its events, its
//                                              item table and its workgroup map as the device would read them (device memory is host
//                                              memory here), for the test to hold against its own restatement
// The kernels never run, so the pools are made-up addresses that nothing follows.
#include <cstdlib>
#include <cstring>

#include "net_host_common.h"
#include "../../mulut_amd/csrc/mulut_net_list.h"

static const void *const kIn = (const void *)0x10000001;
static void *const kOut = (void *)0x20000003;
static mulut_net_plan *const kStale = (mulut_net_plan *)0x66;

static mulut_net_item item(long long in_off, long long out_off, int h, int w, long long in_pool, long long out_pool) {
    mulut_net_item it = {in_off, out_off, h, w, in_pool, out_pool};
    return it;
}

// create with a plan pointer that holds garbage before the call: a refusal must leave NULL there and no event
static void refuse(const char *what, int device, const mulut_net_item *items, int n, int ch, int stages, int scale, int want_rc) {
    mulut_net_plan *p = kStale;
    const int rc = mulut_net_plan_create(device, items, n, ch, stages, scale, &p);
    expect(what, rc, want_rc, "");
    check("  plan is NULL", p == nullptr);
}

static mulut_net_unit *unit(int nf, int u) {
    Weights m;
    make(m, nf, u, true);
    mulut_net_unit *h = nullptr;
    if (mulut_net_unit_create(0, nf, u, m.wp, m.bp, &h) != MULUT_OK) ++g_wrong;
    fake_hip_flush();
    fake_hip_events().clear();
    return h;
}

// images packed back to back in both pools, in list order
static std::vector<mulut_net_item> packed(const std::vector<std::pair<int, int>> &hw, int ch, int scale) {
    long long in = 0, out = 0;
    for (auto &s : hw) in += (long long)s.first * s.second * ch, out += (long long)s.first * s.second * ch * scale * scale;
    std::vector<mulut_net_item> items;
    long long io = 0, oo = 0;
    for (auto &s : hw) {
        items.push_back(item(io, oo, s.first, s.second, in, out));
        io += (long long)s.first * s.second * ch;
        oo += (long long)s.first * s.second * ch * scale * scale;
    }
    return items;
}

static int tables(int argc, char **argv) {
    const int ch = atoi(argv[2]), stages = atoi(argv[3]), scale = atoi(argv[4]);
    std::vector<std::pair<int, int>> hw;
    for (int i = 5; i < argc; ++i) {
        int h = 0, w = 0;
        if (sscanf(argv[i], "%dx%d", &h, &w) != 2) return 2;
        hw.emplace_back(h, w);
    }
    const std::vector<mulut_net_item> items = packed(hw, ch, scale);
    mulut_net_plan *p = nullptr;
    const int rc = mulut_net_plan_create(0, items.data(), (int)items.size(), ch, stages, scale, &p);
    fake_hip_flush();
    printf("create %d", rc);
    for (auto &e : fake_hip_events()) printf(" | %s", e.c_str());
    printf("\n");
    if (rc != MULUT_OK) return 1;
    printf("groups %u set_bytes %zu map_at %zu planes_at %zu\n", p->groups, p->set_bytes, p->map_at, p->planes_at);
    const mulut::NetListItem *it = reinterpret_cast<const mulut::NetListItem *>(p->dev);
    for (int i = 0; i < p->n; ++i) printf("item %d: %lld %lld %lld %d %d\n", i, it[i].in_off, it[i].out_off, it[i].mid, it[i].h, it[i].w);
    const mulut::NetListGroup *map = reinterpret_cast<const mulut::NetListGroup *>(p->dev + p->map_at);
    printf("map:");
    for (unsigned g = 0; g < p->groups; ++g) printf(" %d:%d", map[g].item, map[g].site);
    printf("\n");
    return mulut_net_plan_destroy(p) == MULUT_OK ? 0 : 1;
}

int main(int argc, char **argv) {
    static_assert(sizeof(mulut_net_item) == 40, "mulut_net_item is 40 bytes");
    g_seed = 7;
    if (argc > 4 && strcmp(argv[1], "tables") == 0) return tables(argc, argv);
    const long long PB = 1 << 20;
    const mulut_net_item good = item(0, 0, 5, 7, PB, PB);
    // ---- mulut_net_plan_create, class 1: NULL pointers, n, ch, stages, scale < 1
    expect("null plan", mulut_net_plan_create(0, &good, 1, 3, 2, 4, nullptr), MULUT_EINVAL, "");
    refuse("null items", 0, nullptr, 1, 3, 2, 4, MULUT_EINVAL);
    refuse("n 0", 0, &good, 0, 3, 2, 4, MULUT_EINVAL);
    refuse("n -1", 0, &good, -1, 3, 2, 4, MULUT_EINVAL);
    refuse("ch 0", 0, &good, 1, 0, 2, 4, MULUT_EINVAL);
    refuse("stages 0", 0, &good, 1, 3, 0, 4, MULUT_EINVAL);
    refuse("scale 0", 0, &good, 1, 3, 2, 0, MULUT_EINVAL);
    refuse("scale -2", 0, &good, 1, 3, 2, -2, MULUT_EINVAL);
    // ---- class 2: an item without pixels
    {
        const mulut_net_item a = item(0, 0, 0, 7, PB, PB), b = item(0, 0, 5, -3, PB, PB);
        refuse("h 0", 0, &a, 1, 3, 2, 4, MULUT_EINVAL);
        refuse("w -3", 0, &b, 1, 3, 2, 4, MULUT_EINVAL);
        // an item without pixels LATER in the list wins over an item of 2^31 result bytes EARLIER in it (a refusal of the last class)
        const mulut_net_item two[2] = {item(0, 0, 1 << 13, 1 << 13, 1LL << 40, 1LL << 40), a};
        refuse("2^31 result bytes then h 0", 0, two, 2, 2, 2, 4, MULUT_EINVAL);
    }
    // ---- class 3: negative offsets, an image that ends one byte past its pool, products that leave 64 bits
    {
        const long long in = 5 * 7 * 3, out = in * 16;
        const mulut_net_item a = item(-1, 0, 5, 7, PB, PB), b = item(0, -1, 5, 7, PB, PB), c = item(PB - in + 1, 0, 5, 7, PB, PB),
                             d = item(0, PB - out + 1, 5, 7, PB, PB), e = item(0, 0, 5, 7, in - 1, PB), f = item(0, 0, 5, 7, PB, out - 1),
                             g = item(0, 0, 5, 7, PB, -5), h = item(0, 0, 0x7fffffff, 0x7fffffff, PB, PB),
                             i = item(0x7fffffffffffffffLL, 0, 5, 7, PB, PB), j = item(0, 0, 0x7fffffff, 0x7fffffff, 0x7fffffffffffffffLL, 0x7fffffffffffffffLL);
        refuse("in_off -1", 0, &a, 1, 3, 2, 4, MULUT_EINVAL);
        refuse("out_off -1", 0, &b, 1, 3, 2, 4, MULUT_EINVAL);
        refuse("input one byte past", 0, &c, 1, 3, 2, 4, MULUT_EINVAL);
        refuse("result one byte past", 0, &d, 1, 3, 2, 4, MULUT_EINVAL);
        refuse("in pool too small", 0, &e, 1, 3, 2, 4, MULUT_EINVAL);
        refuse("out pool too small", 0, &f, 1, 3, 2, 4, MULUT_EINVAL);
        refuse("out pool negative", 0, &g, 1, 3, 2, 4, MULUT_EINVAL);
        refuse("(2^31 - 1)^2 pixels", 0, &h, 1, 3, 2, 4, MULUT_EINVAL);
        refuse("in_off 2^63 - 1", 0, &i, 1, 3, 2, 4, MULUT_EINVAL);
        refuse("(2^31 - 1)^2 pixels x (2^31 - 1) channels x (2^31 - 1)^2 in pools of 2^63 - 1", 0, &j, 1, 0x7fffffff, 2, 0x7fffffff, MULUT_EINVAL);
        const mulut_net_item ok_in = item(PB - in, 0, 5, 7, PB, PB), ok_out = item(0, PB - out, 5, 7, PB, PB);
        mulut_net_plan *p = nullptr;
        expect("input ends with its pool", mulut_net_plan_create(0, &ok_in, 1, 3, 1, 4, &p), MULUT_OK, "malloc 40 | memcpy 40");
        expect("  destroy", mulut_net_plan_destroy(p), MULUT_OK, "free 40");
        expect("result ends with its pool", mulut_net_plan_create(0, &ok_out, 1, 3, 1, 4, &p), MULUT_OK, "malloc 40 | memcpy 40");
        expect("  destroy", mulut_net_plan_destroy(p), MULUT_OK, "free 40");
        // an offset outside LATER in the list wins over an item of 2^31 result bytes EARLIER in it
        const mulut_net_item two[2] = {item(0, 0, 1 << 13, 1 << 13, 1LL << 40, 1LL << 40), a};
        refuse("2^31 result bytes then in_off -1", 0, two, 2, 2, 2, 4, MULUT_EINVAL);
    }
    // ---- class 4: result ranges that overlap (inputs may be shared)
    {
        const long long out = 5 * 7 * 3 * 16;
        const mulut_net_item same[2] = {item(0, 0, 5, 7, PB, PB), item(0, 0, 5, 7, PB, PB)};
        const mulut_net_item by_one[3] = {item(0, 2 * out, 5, 7, PB, PB), item(0, 0, 5, 7, PB, PB), item(0, out - 1, 5, 7, PB, PB)};
        const mulut_net_item inside[2] = {item(0, 0, 11, 12, PB, PB), item(0, 100, 1, 1, PB, PB)};
        refuse("two results in one place", 0, same, 2, 3, 2, 4, MULUT_EINVAL);
        refuse("results that share one byte", 0, by_one, 3, 3, 2, 4, MULUT_EINVAL);
        refuse("a result inside another", 0, inside, 2, 3, 2, 4, MULUT_EINVAL);
        const mulut_net_item touch[3] = {item(0, 2 * out, 5, 7, PB, PB), item(0, 0, 5, 7, PB, PB), item(0, out, 5, 7, PB, PB)};
        mulut_net_plan *p = nullptr;      // one shared input, results that touch, out of order: 3 x (32 + 8) bytes of tables, one set of 3 x 105 bytes
        expect("results that touch, one input", mulut_net_plan_create(0, touch, 3, 3, 2, 4, &p), MULUT_OK, "malloc 435 | memcpy 120");
        expect("  destroy", mulut_net_plan_destroy(p), MULUT_OK, "free 435");
        // an overlap LATER in the list wins over an item of 2^31 result bytes EARLIER in it
        const mulut_net_item three[3] = {item(0, 1LL << 32, 1 << 13, 1 << 13, 1LL << 40, 1LL << 40), item(0, 0, 5, 7, 1LL << 40, 1LL << 40),
                                         item(0, 1, 5, 7, 1LL << 40, 1LL << 40)};
        refuse("2^31 result bytes then an overlap", 0, three, 3, 2, 2, 4, MULUT_EINVAL);
    }
    // ---- class 5: counts that pass 2^31
    {
        const long long P40 = 1LL << 40;
        const mulut_net_item big = item(0, 0, 1 << 13, 1 << 13, P40, P40);      // 2^26 pixels x 2 channels x 16
        refuse("an item of 2^31 result bytes", 0, &big, 1, 2, 2, 4, MULUT_EUNSUPPORTED);
        // 129 items of 2^31 - 2^16 sites: 129 x (2^24 - 2^9) workgroups pass 2^31 with the last
        std::vector<mulut_net_item> many;
        for (int i = 0; i < 129; ++i) many.push_back(item(0, (long long)i << 31, (1 << 15) - 1, 1 << 16, P40, P40));
        refuse("2^31 workgroups", 0, many.data(), 129, 1, 1, 1, MULUT_EUNSUPPORTED);
        // two items of 2^29 sites: one plane set of 2^30 bytes fits, two do not
        const mulut_net_item half[2] = {item(0, 0, 1 << 14, 1 << 15, P40, P40), item(0, 1LL << 29, 1 << 14, 1 << 15, P40, P40)};
        refuse("a workspace of 2^31 bytes", 0, half, 2, 1, 3, 1, MULUT_EUNSUPPORTED);
        // a refusal of this class wins over a device the runtime does not have
        refuse("an item of 2^31 result bytes on device 3", 3, &big, 1, 2, 2, 4, MULUT_EUNSUPPORTED);
    }
    // ---- a device the runtime does not have: the arguments are in order, the device is asked for and refused
    refuse("device 3", 3, &good, 1, 3, 2, 4, MULUT_ENODEVICE);

    // ---- plans and runs.  Units of nf 8 (one M-tile) and 33 (two)
    mulut_net_unit *u1[3] = {unit(8, 1), unit(8, 1), unit(8, 1)}, *u4[3] = {unit(8, 4), unit(8, 4), unit(8, 4)};
    mulut_net_unit *w1 = unit(33, 1), *w4 = unit(33, 4), *u2 = unit(8, 2);
    {   // 5 x 7 x 3 = 105 sites: one workgroup.  32 bytes of item, 8 of map; no planes for one stage
        mulut_net_plan *p = nullptr;
        expect("create 1 stage", mulut_net_plan_create(0, &good, 1, 3, 1, 4, &p), MULUT_OK, "malloc 40 | memcpy 40");
        const mulut_net_unit *const s1[3] = {u4[0], u4[1], u4[2]};
        expect("run 1 stage", mulut_net_plan_run(p, s1, "sdy", kIn, kOut, nullptr), MULUT_OK, "launch net_list_kernel<1, 4> grid 1,1,1 block 256,1,1 lds 0");
        expect("run 1 stage again, one mode, a stream", mulut_net_plan_run(p, s1, "y", kIn, kOut, (void *)0x77), MULUT_OK,
               "launch net_list_kernel<1, 4> grid 1,1,1 block 256,1,1 lds 0");
        // ---- mulut_net_plan_run's refusals: none touches the device
        const mulut_net_unit *const hole[3] = {u4[0], nullptr, u4[2]}, *const mixed[2] = {u4[0], w4}, *const low[1] = {u2};
        const mulut_net_unit *const nine[9] = {u4[0], u4[0], u4[0], u4[0], u4[0], u4[0], u4[0], u4[0], u4[0]};
        expect("run null plan", mulut_net_plan_run(nullptr, s1, "sdy", kIn, kOut, nullptr), MULUT_EINVAL, "");
        expect("run null units", mulut_net_plan_run(p, nullptr, "sdy", kIn, kOut, nullptr), MULUT_EINVAL, "");
        expect("run null modes", mulut_net_plan_run(p, s1, nullptr, kIn, kOut, nullptr), MULUT_EINVAL, "");
        expect("run null in", mulut_net_plan_run(p, s1, "sdy", nullptr, kOut, nullptr), MULUT_EINVAL, "");
        expect("run null out", mulut_net_plan_run(p, s1, "sdy", kIn, nullptr, nullptr), MULUT_EINVAL, "");
        expect("run no mode", mulut_net_plan_run(p, s1, "", kIn, kOut, nullptr), MULUT_EINVAL, "");
        expect("run a null handle", mulut_net_plan_run(p, hole, "sdy", kIn, kOut, nullptr), MULUT_EINVAL, "");
        expect("run an unknown letter", mulut_net_plan_run(p, s1, "sqy", kIn, kOut, nullptr), MULUT_EINVAL, "");
        expect("run nine modes", mulut_net_plan_run(p, nine, "sdysdysdy", kIn, kOut, nullptr), MULUT_EUNSUPPORTED, "");
        expect("run units of two widths", mulut_net_plan_run(p, mixed, "sd", kIn, kOut, nullptr), MULUT_ESHAPE, "");
        expect("run a last stage of upscale 2 under a plan of scale 4", mulut_net_plan_run(p, low, "s", kIn, kOut, nullptr), MULUT_ESHAPE, "");
        expect("destroy 1 stage", mulut_net_plan_destroy(p), MULUT_OK, "free 40");
    }
    {   // two stages: one set of 105 bytes
        mulut_net_plan *p = nullptr;
        expect("create 2 stages", mulut_net_plan_create(0, &good, 1, 3, 2, 4, &p), MULUT_OK, "malloc 145 | memcpy 40");
        const mulut_net_unit *const s2[4] = {u1[0], u1[1], u4[0], u4[1]}, *const up_first[4] = {u4[0], u4[1], u4[0], u4[1]},
                                    *const flat_last[4] = {u1[0], u1[1], u1[0], u1[1]}, *const hole2[4] = {u1[0], u1[1], u4[0], nullptr};
        expect("run 2 stages", mulut_net_plan_run(p, s2, "sd", kIn, kOut, nullptr), MULUT_OK,
               "launch net_list_kernel<1, 1> grid 1,1,1 block 256,1,1 lds 0 | launch net_list_kernel<1, 4> grid 1,1,1 block 256,1,1 lds 0");
        expect("run a first stage of upscale 4", mulut_net_plan_run(p, up_first, "sd", kIn, kOut, nullptr), MULUT_ESHAPE, "");
        expect("run a last stage of upscale 1", mulut_net_plan_run(p, flat_last, "sd", kIn, kOut, nullptr), MULUT_ESHAPE, "");
        expect("run a null handle in stage 2", mulut_net_plan_run(p, hole2, "sd", kIn, kOut, nullptr), MULUT_EINVAL, "");
        expect("destroy 2 stages", mulut_net_plan_destroy(p), MULUT_OK, "free 145");
    }
    {   // three stages over the mixed list: 3 + 18 + 105 + 126 + 129 + 396 + 129 = 906 sites, 1 + 1 + 1 + 1 + 2 + 4 + 2 = 12 workgroups, two sets
        const std::vector<mulut_net_item> items = packed({{1, 1}, {2, 3}, {5, 7}, {6, 7}, {43, 1}, {11, 12}, {1, 43}}, 3, 4);
        mulut_net_plan *p = nullptr;
        expect("create 3 stages, 7 items", mulut_net_plan_create(0, items.data(), 7, 3, 3, 4, &p), MULUT_OK, "malloc 2132 | memcpy 320");
        const mulut_net_unit *const s3[3] = {w1, u1[0], w4};      // a stage's width is its own
        expect("run 3 stages", mulut_net_plan_run(p, s3, "o", kIn, kOut, nullptr), MULUT_OK,
               "launch net_list_kernel<2, 1> grid 12,1,1 block 256,1,1 lds 0 | launch net_list_kernel<1, 1> grid 12,1,1 block 256,1,1 lds 0 | "
               "launch net_list_kernel<2, 4> grid 12,1,1 block 256,1,1 lds 0");
        expect("destroy 3 stages", mulut_net_plan_destroy(p), MULUT_OK, "free 2132");
    }
    {   // 328 items of 6 x 8 x 3 = 144 sites: two workgroups each, 656 map entries (more than a page of them)
        const std::vector<mulut_net_item> items = packed(std::vector<std::pair<int, int>>(328, {6, 8}), 3, 4);
        mulut_net_plan *p = nullptr;
        expect("create 328 items", mulut_net_plan_create(0, items.data(), 328, 3, 2, 4, &p), MULUT_OK, "malloc 62976 | memcpy 15744");
        const mulut_net_unit *const s2[2] = {u1[0], u4[0]};
        expect("run 328 items", mulut_net_plan_run(p, s2, "h", kIn, kOut, nullptr), MULUT_OK,
               "launch net_list_kernel<1, 1> grid 656,1,1 block 256,1,1 lds 0 | launch net_list_kernel<1, 4> grid 656,1,1 block 256,1,1 lds 0");
        expect("destroy 328 items", mulut_net_plan_destroy(p), MULUT_OK, "free 62976");
    }
    expect("destroy null", mulut_net_plan_destroy(nullptr), MULUT_EINVAL, "");
    for (mulut_net_unit *h : {u1[0], u1[1], u1[2], u4[0], u4[1], u4[2], w1, w4, u2}) mulut_net_unit_destroy(h);
    fake_hip_flush();
    fake_hip_events().clear();
    printf("%d unexpected\n", g_wrong);
    return g_wrong;
}
