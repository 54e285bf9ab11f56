// mulut_net_list.hip -- the fourth launch form of the fused forward (mulut_net.hip holds table, pass and stage): a whole LIST of
// images of different sizes through the whole cascade, HWC bytes in a pool to HWC bytes in another pool, in `stages` launches.
//
// Reference: sr/1_train_model.py:87-101, the per-image body of valid_steps -- an image to planar floats (:87-91), mulut_predict in
// the 'valid' phase (:93), back to HWC, round and clip to bytes (:95-101) -- for every image of a validation set at once.
//
// The site body, the weight-stream walk, the integer sums in LDS and the epilogue are those of the stage form (net_site_body, net_q127,
// net_tap_index, net_rhe_clip of mulut_net_dev.h); the loop over modes and rotations around them is net_stage_body's, restated here
// and not shared: with the loop moved into a function that both call, net_stage_kernel and the training forward net_stage_sum_kernel
// were compiled to other instruction streams and register counts (tools/asm_compare.py), and those are the measured kernels.
// What is new is where a site's taps come from and where its block goes:
//   * a workgroup serves kNetSites consecutive sites of ONE item, a site being (channel, y, x) with the channel slowest, as in the
//     stage form over that image alone.  Workgroup g finds (item, first site) in a map the host built once; the last workgroup of
//     every item is partial and its spare lanes compute the item's last site and store nothing.
//   * the first stage reads its taps from the HWC input pool (pixel stride ch), the last writes its block into the HWC output pool,
//     and the stages between read and write the plan's own planar planes (pixel stride 1): a stage's layout is two strides and two
//     bases in its arguments, not another kernel.  Stage k (0-based) of S writes plane set k & 1 and reads set (k - 1) & 1, so two
//     sets serve any S; an item's planes lie at its first site's index in the list, the stages before the last having u = 1.
//   * addresses inside an item are 32-bit (create refuses an item of 2^31 output bytes), the item's base is 64-bit.
// Output bytes are stored one by one: with ch = 3 interleaved the u x u block of a site is u runs of u bytes at stride 3, no two of
// which share a dword with a fixed alignment (no alignment is asked of out_off), and a site's 16 K to 100 K MFMA steps per stage
// dwarf its u * u byte stores, which L2 merges into the lines the neighbouring lanes and the other two channels' workgroups fill.
// Going through LDS to build whole dwords would add LDS beyond the stage form's 40 KiB and a workgroup barrier to save stores that
// are not on the critical path.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <new>
#include <utility>
#include <vector>

#include "mulut_net_dev.h"
#include "mulut_net_list.h"

namespace mulut {

struct NetListArgs {
    const float4 *w[MULUT_MAX_MODES];
    unsigned taps[MULUT_MAX_MODES];
    const NetListItem *items;
    const NetListGroup *map;
    const unsigned char *in;      // the input pool (in_hwc) or a set of planes
    unsigned char *out;           // the output pool (out_hwc) or a set of planes
    int M, is_last, ch, in_hwc, out_hwc;
};

template <int MT, int U>
__global__ void __launch_bounds__(kNetNT) net_list_kernel(NetListArgs a) {
    __shared__ float4 lds[2 * kNetChunkVec4];
    __shared__ int sums[kNetWaves][16][kNetTileSites];
    NetStream s;
    net_stream_begin(s, a.w[0], lds);
    const NetListGroup g = a.map[blockIdx.x];
    const NetListItem it = a.items[g.item];
    const int h = s.lane >> 5, sl = s.lane & 31, wave = s.tid >> 6;
    const int H = it.h, W = it.w, total = a.ch * H * W;
    const int site = g.site + wave * kNetTileSites + sl;
    const int px = site < total ? site : total - 1;
    const int c = px / (H * W), y0 = (px % (H * W)) / W, x0 = px % W;
    const unsigned char *pin = a.in + (a.in_hwc ? it.in_off + c : it.mid + c * (H * W));
    const int is = a.in_hwc ? a.ch : 1;
    int(*acc)[kNetTileSites] = sums[wave];
#pragma unroll
    for (int q = 0; q < 8; ++q) acc[8 * h + q][sl] = 0;
    for (int m = 0; m < a.M; ++m) {      // (net_stage_body's loop, its taps apart)
        const unsigned taps = a.taps[m];
        for (int r = 0; r < 4; ++r) {
            s.cur = a.w[m];
            s.next = r < 3 ? a.w[m] : a.w[m + 1 < a.M ? m + 1 : m];
            float y[8];
            const float t0 = net_tap_value(pin[net_tap_index(H, W, r, y0, x0, taps, h) * is]);
            const float t1 = net_tap_value(pin[net_tap_index(H, W, r, y0, x0, taps, 2 + h) * is]);
            net_site_body<MT, U>(s, t0, t1, y);
#pragma unroll
            for (int q = 0; q < 8; ++q) {
                const int o = 8 * h + q;
                if (o < U * U) {
                    const int si = o / U, sj = o % U;
                    const int sy = r == 0 ? si : r == 1 ? sj : r == 2 ? U - 1 - si : U - 1 - sj;
                    const int sx = r == 0 ? sj : r == 1 ? U - 1 - si : r == 2 ? U - 1 - sj : si;
                    acc[sy * U + sx][sl] += net_q127(y[q]);
                }
            }
        }
    }
    if (site >= total) return;
    unsigned char *po = a.out + (a.out_hwc ? it.out_off + c : it.mid + c * (H * U) * (W * U));      // (planar: U = 1, run sees to it)
    const int os = a.out_hwc ? a.ch : 1;
    const int D = a.is_last ? a.M : 4 * a.M, bias = a.is_last ? 0 : 127 * D;
#pragma unroll
    for (int q = 0; q < 8; ++q) {
        const int o = 8 * h + q;
        if (o < U * U) po[((y0 * U + o / U) * (W * U) + x0 * U + o % U) * os] = (unsigned char)net_rhe_clip(acc[o][sl] + bias, D);
    }
}

}  // namespace mulut

namespace {

// a * b <= cap for non-negative a, b, cap, with no product that can overflow; *out = a * b then
bool mul_within(long long a, long long b, long long cap, long long *out) {
    if (b != 0 && a > cap / b) return false;
    *out = a * b;
    return true;
}

// h x w x ch bytes, scaled by scale^2, lie at `off` wholly inside a pool of `pool` bytes; *bytes = their count then
bool image_inside(long long off, int h, int w, int ch, int scale, long long pool, long long *bytes) {
    if (off < 0 || pool < 0) return false;
    long long n = h;
    if (!mul_within(n, w, pool, &n) || !mul_within(n, ch, pool, &n) || !mul_within(n, scale, pool, &n) || !mul_within(n, scale, pool, &n)) return false;
    *bytes = n;
    return off <= pool - n;
}

}  // namespace

extern "C" {

/* sr/1_train_model.py:87-101 for a whole list of images */
int mulut_net_plan_create(int device, const mulut_net_item *items, int n, int ch, int stages, int scale, mulut_net_plan **out_plan) {
    using namespace mulut;
    if (!out_plan) return MULUT_EINVAL;
    *out_plan = nullptr;
    if (!items || n < 1 || ch < 1 || stages < 1 || scale < 1) return MULUT_EINVAL;
    for (int i = 0; i < n; ++i)
        if (items[i].h < 1 || items[i].w < 1) return MULUT_EINVAL;
    std::vector<std::pair<long long, long long>> ranges;      // [out_off, end) of every item
    try {
        ranges.reserve((size_t)n);
    } catch (const std::bad_alloc &) {
        return MULUT_EUNSUPPORTED;
    }
    for (int i = 0; i < n; ++i) {
        long long in_bytes = 0, out_bytes = 0;
        if (!image_inside(items[i].in_off, items[i].h, items[i].w, ch, 1, items[i].in_pool_bytes, &in_bytes) ||
            !image_inside(items[i].out_off, items[i].h, items[i].w, ch, scale, items[i].out_pool_bytes, &out_bytes))
            return MULUT_EINVAL;
        ranges.emplace_back(items[i].out_off, items[i].out_off + out_bytes);
    }
    {
        std::vector<std::pair<long long, long long>> sorted(ranges);
        std::sort(sorted.begin(), sorted.end());
        for (int i = 1; i < n; ++i)
            if (sorted[i].first < sorted[i - 1].second) return MULUT_EINVAL;
    }
    long long groups = 0, sites = 0;
    for (int i = 0; i < n; ++i) {
        const long long out_bytes = ranges[i].second - ranges[i].first, item_sites = out_bytes / scale / scale;
        if (out_bytes >= (1LL << 31)) return MULUT_EUNSUPPORTED;
        groups += (item_sites + kNetSites - 1) / kNetSites;      // (below 2^24 a time: the running sums stay far inside 64 bits)
        sites += item_sites;
        if (groups >= (1LL << 31)) return MULUT_EUNSUPPORTED;
    }
    const int sets = stages == 1 ? 0 : stages == 2 ? 1 : 2;
    const size_t map_at = (size_t)n * sizeof(NetListItem), planes_at = map_at + (size_t)groups * sizeof(NetListGroup);
    if ((long long)planes_at + sets * sites >= (1LL << 31)) return MULUT_EUNSUPPORTED;
    std::vector<unsigned char> host;
    try {
        host.resize(planes_at);
    } catch (const std::bad_alloc &) {
        return MULUT_EUNSUPPORTED;
    }
    static_assert(sizeof(NetListItem) == 32 && sizeof(NetListGroup) == 8, "the map starts 8-aligned behind the items");
    NetListItem *hi = reinterpret_cast<NetListItem *>(host.data());
    NetListGroup *map = reinterpret_cast<NetListGroup *>(host.data() + map_at);
    long long mid = 0;
    for (int i = 0; i < n; ++i) {
        const long long item_sites = (long long)ch * items[i].h * items[i].w;
        hi[i] = NetListItem{items[i].in_off, items[i].out_off, mid, items[i].h, items[i].w};
        for (long long first = 0; first < item_sites; first += kNetSites) *map++ = NetListGroup{i, (int)first};
        mid += item_sites;
    }
    if (hipSetDevice(device) != hipSuccess) return MULUT_ENODEVICE;
    mulut_net_plan *p = new (std::nothrow) mulut_net_plan{device, n, ch, stages, scale, (unsigned)groups, nullptr, map_at, planes_at, (size_t)sites};
    if (!p) return MULUT_EHIP;
    if (hipMalloc(reinterpret_cast<void **>(&p->dev), planes_at + (size_t)sets * (size_t)sites) != hipSuccess) {
        delete p;
        return MULUT_EHIP;
    }
    if (hipMemcpy(p->dev, host.data(), planes_at, hipMemcpyHostToDevice) != hipSuccess) {
        (void)hipFree(p->dev);
        delete p;
        return MULUT_EHIP;
    }
    *out_plan = p;
    return MULUT_OK;
}

int mulut_net_plan_destroy(mulut_net_plan *plan) {
    if (!plan) return MULUT_EINVAL;
    int rc = MULUT_OK;
    if (hipSetDevice(plan->device) != hipSuccess) rc = MULUT_ENODEVICE;
    else if (hipFree(plan->dev) != hipSuccess) rc = MULUT_EHIP;
    delete plan;
    return rc;
}

/* sr/1_train_model.py:93-101 */
int mulut_net_plan_run(const mulut_net_plan *plan, const mulut_net_unit *const units[], const char *modes, const void *in_pool, void *out_pool,
                       void *stream) {
    using namespace mulut;
    if (!plan || !units || !modes || !in_pool || !out_pool) return MULUT_EINVAL;
    NetListArgs a;
    memset(&a, 0, sizeof(a));
    const size_t M = strnlen(modes, MULUT_MAX_MODES + 1);
    for (int k = 0; k < plan->stages; ++k) {      // every stage's refusals before the first launch
        const mulut_net_unit *const *su = units + (size_t)k * (M <= MULUT_MAX_MODES ? M : 0);
        const int rc = net_stage_units(su, modes, 0, a.w, a.taps, &a.M);
        if (rc != MULUT_OK) return rc;
        if (su[0]->u != (k + 1 < plan->stages ? 1 : plan->scale) || su[0]->device != plan->device) return MULUT_ESHAPE;
    }
    if (hipSetDevice(plan->device) != hipSuccess) return MULUT_ENODEVICE;
    a.items = reinterpret_cast<const NetListItem *>(plan->dev);
    a.map = reinterpret_cast<const NetListGroup *>(plan->dev + plan->map_at);
    a.ch = plan->ch;
    unsigned char *planes = plan->dev + plan->planes_at;
    const long long launch_sites = (long long)plan->groups * kNetSites;
    for (int k = 0; k < plan->stages; ++k) {
        const mulut_net_unit *const *su = units + (size_t)k * M;
        (void)net_stage_units(su, modes, 0, a.w, a.taps, &a.M);
        a.in_hwc = k == 0;
        a.out_hwc = a.is_last = k + 1 == plan->stages;
        a.in = a.in_hwc ? static_cast<const unsigned char *>(in_pool) : planes + (size_t)((k - 1) & 1) * plan->set_bytes;
        a.out = a.out_hwc ? static_cast<unsigned char *>(out_pool) : planes + (size_t)(k & 1) * plan->set_bytes;
        MULUT_NET_LAUNCH(net_list_kernel, su[0]->mt, su[0]->u, launch_sites, stream, a);
    }
    return hipGetLastError() == hipSuccess ? MULUT_OK : MULUT_EHIP;
}

}  // extern "C"
