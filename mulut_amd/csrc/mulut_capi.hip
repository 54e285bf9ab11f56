// mulut_capi.hip -- implementation of the C ABI declared in include/mulut.h.
// Owns: the context (device id, model shape), device copies of the tables, the ping-pong
// workspace for intermediate stage images.  All image buffers belong to the caller.
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstring>
#include <new>
#include <string>
#include <utility>
#include <vector>

#include "../../include/mulut.h"
#include "mulut_interval.h"
#include "mulut_kernels.h"

using namespace mulut;

// Where a failing HIP call leaves its text (mulut_last_hip_error): the part of the context that what it owns reports into
struct HipErr {
    std::string hip_err;
};

#define HIP_TRY(ctx, expr)                                                                  \
    do {                                                                                    \
        hipError_t e__ = (expr);                                                            \
        if (e__ != hipSuccess) {                                                            \
            if (ctx) (ctx)->hip_err = std::string(#expr) + ": " + hipGetErrorString(e__);   \
            return MULUT_EHIP;                                                              \
        }                                                                                   \
    } while (0)

// Set-up calls that overwrite or free device memory a kernel of an earlier call may still read (tables, bands, slabs, work lists,
// the workspaces) wait for the device first: the caller's streams are unknown here, and a non-blocking stream is not ordered
// against the null stream the copies run on.  Only mulut_set_lut, the releasing branch of mulut_configure, DevBuf::grow when it
// reallocates and mulut_destroy come through here -- never a compute call that allocates nothing
static int wait_for_device(HipErr *ctx) {
    HIP_TRY(ctx, hipDeviceSynchronize());
    return MULUT_OK;
}

// One device allocation and its only owner: move-only, freed when the owner dies (unchecked: nothing could act on a failure there).
// Its members are the three ways the context sizes its memory; a HIP failure in any of them is MULUT_EHIP with hip_err set.
// A new buffer of the context is a new member and nothing else.
template <class T>
struct DevBuf {
    T *p = nullptr;
    size_t cap = 0;     // elements

    DevBuf() = default;
    DevBuf(DevBuf &&o) noexcept : p(o.p), cap(o.cap) { o.p = nullptr, o.cap = 0; }
    DevBuf &operator=(DevBuf &&o) noexcept { return std::swap(p, o.p), std::swap(cap, o.cap), *this; }
    ~DevBuf() {
        if (p) (void)hipFree(p);
    }
    explicit operator bool() const { return p != nullptr; }

    // at least n elements: reallocated (contents dropped, after a wait for the device) only when it is too small
    int grow(HipErr *ctx, size_t n) {
        if (n <= cap) return MULUT_OK;
        if (p) {
            const int rc = wait_for_device(ctx);
            if (rc) return rc;
            HIP_TRY(ctx, hipFree(p));
        }
        p = nullptr;
        cap = 0;
        HIP_TRY(ctx, hipMalloc((void **)&p, n * sizeof(T)));
        cap = n;
        return MULUT_OK;
    }
    // the device copy of a host image: reallocated only when the size changes
    template <class V>
    int upload(HipErr *ctx, const std::vector<V> &img) {
        const size_t n = img.size() * sizeof(V) / sizeof(T);
        if (p && cap != n) {
            HIP_TRY(ctx, hipFree(p));
            p = nullptr;
        }
        if (!p) HIP_TRY(ctx, hipMalloc((void **)&p, n * sizeof(T)));
        cap = n;
        HIP_TRY(ctx, hipMemcpy(p, img.data(), n * sizeof(T), hipMemcpyHostToDevice));
        return MULUT_OK;
    }
    int release(HipErr *ctx) {
        if (p) HIP_TRY(ctx, hipFree(p));
        p = nullptr;
        cap = 0;
        return MULUT_OK;
    }
};

struct DevTable {
    DevBuf<uint8_t> dev;    // full table image
    DevBuf<uint8_t> tube;   // "tube" band (keys spanning <= 2 MSB steps): v_num 16: expanded to 16-bit fields, two planes of kTubeSlots x 16 B;
                            // v_num 1: one dword per slot (kTube1BandBytes)
    DevBuf<uint8_t> slab;   // v_num 16: the table as 16 anchor slab pairs (mulut_core.h), kSlabTableBytes
    int vnum = 0;

    int clear(HipErr *ctx) {
        int rc = dev.release(ctx);
        if (!rc) rc = tube.release(ctx);
        if (!rc) rc = slab.release(ctx);
        if (!rc) vnum = 0;
        return rc;
    }
};

// Buffers of the detailed-tile path of the final stage (launch_detail_slab): counters, items, sample ids, blocks
struct DetailBufs {
    DevBuf<uint32_t> ctl, items, desc, tpos, dlist;
    DevBuf<uint16_t> thist;
    DevBuf<uint4> blocks;

    void fill(DetailArgs &d) const {
        d.ctl = ctl.p; d.items = items.p; d.desc = desc.p; d.blocks = blocks.p;
        d.thist = thist.p; d.tpos = tpos.p; d.dlist = dlist.p;
    }
};

// An event of the stage timing: created on first use (mulut_set_stage_timing), destroyed with its owner
struct DevEvent {
    hipEvent_t e = nullptr;

    DevEvent() = default;
    DevEvent(DevEvent &&) = delete;
    ~DevEvent() {
        if (e) (void)hipEventDestroy(e);
    }
};

// tuning keys that choose a stage's route (plan_stage); the defaults take the routes that use every buffer any route does
struct Routing {
    int final_kernel = 0;   // tuning "final_stage_kernel": 0 auto (= 6), 1 full-table kernel, 5 tube kernel (all bands resident), 6 hybrid (tube)
    int first_kernel = 0;   // tuning "first_stage_kernel", 1-byte-row stages: 0 auto (tube kernel, detailed tiles to the window kernel), 2 window kernel (full table in
                            // LDS) on every tile, 3 tube kernel on every tile
    int tube2 = 1;          // tuning "tube_pipelined": 1 = stage_tube2_kernel (hand-scheduled LDS reads) where the mode list has one, 0 = stage_tube_kernel
    int detail_kernel = 0;  // tuning "detail_kernel": 0 = anchor slabs in LDS (when the launch qualifies), 1 = full-table gather kernel
};

struct mulut_ctx : HipErr {
    int device = 0;
    bool configured = false;
    int stages = 0, n_modes = 0, scale = 0, interval = 0;
    int tab_interval = kInterval;   // the interval the tables in tab[][] were set for (configuring another one clears them)
    char modes[MULUT_MAX_MODES + 1] = {0};
    signed char di[MULUT_MAX_MODES][3], dj[MULUT_MAX_MODES][3];
    int reach = 2;  // LR rows one stage looks beyond its output rows
    bool wide = false;  // the mode list holds a 4 x 4 pattern (e, h, o): reach 3, every stage on the halo-3 instances of the full-table kernels
    DevTable tab[MULUT_MAX_STAGES][6];  // [stage-1][pattern id s,d,y,e,h,o]
    DevBuf<uint8_t> ws[2];
    int num_cus = 256;
    Routing routing;
    int f32_ok[2] = {0, 0}; // float epilogue proven exact for the [non-final, final] divisor
    int fma_ok = 0;         // fused (biased-sum) float epilogue proven exact for the final stage
    float epi_c = 0.0f;
    DevBuf<uint32_t> verdict;      // per-tile smooth/detailed verdicts of the hybrid final stage
    DevBuf<uint32_t> fix;          // [0] = count, [16...] = entries of the fix-up list (samples recomputed from the full tables)
    DevBuf<unsigned long long> dbg;      // probe buffer (mulut_debug_read), MULUT_DEBUG_WORDS words, allocated on first use
    DetailBufs det;
    bool k1_valid = false;         // ctx->tlist holds the marks of the first-stage launch that produced the next stage's input ...
    int k1_N = 0, k1_W = 0, k1_H = 0, k1_tiles_x = 0, k1_tiles_y = 0, k1_oy0 = 0, k1_oy1 = 0;   // ... of this shape ...
    const uint8_t *k1_out = nullptr;                                      // ... written to this buffer
    int stat_from_k1 = 1;          // tuning "stat_from_first_stage": the final stage's statistic looks only at tiles the first stage marked
    int up_detail_per_1024 = 8;    // the same threshold for the routed x2 / x3 final stages (their detailed tiles go to the gather kernel; profiles/r04y_scale_bench.jsonl)
    int u1_detail_per_1024 = 24;   // a tile goes to the full-table kernel when more than this share of its (sampled) 4-pixel groups spans > 1 MSB step
    DevBuf<uint32_t> tlist;        // [16 + tile] = 1: the tube kernel left this tile to the full-table kernel
    int fma1_ok = 0;               // fused float epilogue proven exact for non-final stages
    int hybrid_oob_per_1024 = 128; // a tile is "detailed" when more than 1/8 of its (sampled) sites leave the band
    bool timing = false;
    DevEvent ev[MULUT_MAX_STAGES + 1];
    DevEvent evk[MULUT_MAX_STAGES][2];          // around each stage's dominant kernel
    bool evk_set[MULUT_MAX_STAGES] = {};
    int timed_stages = 0;
};

static int pattern_id(char m) {
    return m == 's' ? 0 : m == 'd' ? 1 : m == 'y' ? 2 : m == 'e' ? 3 : m == 'h' ? 4 : m == 'o' ? 5 : -1;
}

// Tube band of a table with u x u-value rows (img: its device image): the rows with max - min of the keys <= 2, at tube_slot().
// Slots of rows outside the tube keep the fill (value + 128 = 128 in every 16-bit field; 0 for 1-byte rows)
static std::vector<uint32_t> tube_band(int u, const int8_t *rows, const std::vector<uint8_t> &img) {
    const size_t bytes = u == 1 ? kTube1BandBytes : u == 2 ? kTube2BandBytes : u == 3 ? kTube3BandBytes : kTubeBandBytes;
    std::vector<uint32_t> tb(bytes / 4, u == 1 ? 0u : 0x00800080u);
    const int rb = row_dwords(u) * 4;
    for (int A = 0; A < kL; ++A)
        for (int B = imax(0, A - 2); B <= imin(kL - 1, A + 2); ++B)
            for (int C = imax(0, A - 2); C <= imin(kL - 1, A + 2); ++C)
                for (int D = imax(0, A - 2); D <= imin(kL - 1, A + 2); ++D) {
                    if (!tube_contains(A, B, C, D)) continue;
                    const size_t row = (size_t)A * kStrideA + B * kStrideB + C * kStrideC + D, slot = (size_t)tube_slot(A, B, C, D);
                    if (u == 1) {           // one dword per slot: the value as int16 in both halves
                        const uint32_t v = (uint32_t)(uint16_t)(int16_t)rows[row];
                        tb[slot] = v | (v << 16);
                        continue;
                    }
                    const uint8_t *e = &img[row * rb];
                    if (u == 2) {           // two dwords per slot: (e0 | e1 << 16), (e2 | e3 << 16)
                        tb[slot * 2] = (uint32_t)e[0] | ((uint32_t)e[1] << 16);
                        tb[slot * 2 + 1] = (uint32_t)e[2] | ((uint32_t)e[3] << 16);
                    } else if (u == 3) {    // 24 bytes per slot: the nine values as ten 16-bit fields e0 e1 e2 e3 e4 e4 e5 e6 e7 e8
                        uint32_t f[10];
                        for (int q = 0; q < 9; ++q) f[tube3_field(q)] = e[q];
                        f[5] = e[4];
                        for (int k = 0; k < 5; ++k) tb[slot * (kTube3SlotBytes / 4) + k] = f[2 * k] | (f[2 * k + 1] << 16);
                    } else {                // 16-bit fields in two planes: LO (lo_k = e(4k) | e(4k+2) << 16) then HI (hi_k = e(4k+1) | e(4k+3) << 16)
                        for (int k = 0; k < 4; ++k) {
                            tb[slot * 4 + k] = (uint32_t)e[4 * k] | ((uint32_t)e[4 * k + 2] << 16);
                            tb[(size_t)kTubePlaneBytes / 4 + slot * 4 + k] = (uint32_t)e[4 * k + 1] | ((uint32_t)e[4 * k + 3] << 16);
                        }
                    }
                }
    return tb;
}

// anchor slab pairs of a u == 4 table: pair A = rows (A, b, c, d) and (A + 1, b, c, d) interleaved, 32 bytes per (b, c, d)
static std::vector<uint8_t> slab_pairs(const std::vector<uint8_t> &img) {
    std::vector<uint8_t> sl((size_t)kSlabTableBytes + 1024, 128);      // the LDS copy of a pair moves whole KiB
    for (int A = 0; A < 16; ++A)
        for (int bcd = 0; bcd < kStrideA; ++bcd)
            for (int f = 0; f < 2; ++f)
                memcpy(&sl[(size_t)A * kSlabPairBytes + (size_t)bcd * 32 + (size_t)f * 16], &img[((size_t)(A + f) * kStrideA + bcd) * 16], 16);
    return sl;
}

extern "C" {

int mulut_version(void) { return MULUT_VERSION; }

const char *mulut_strerror(int err) {
    switch (err) {
        case MULUT_OK: return "ok";
        case MULUT_EINVAL: return "invalid argument";
        case MULUT_EMODE: return "Mode not implemented.";
        case MULUT_ENOLUT: return "LUT for (stage, mode) not set";
        case MULUT_ESHAPE: return "LUT shape does not match (L^4, v_num) for this stage (83521 rows at interval 4, 6561 at 5, 625 at 6)";
        case MULUT_EUNSUPPORTED: return "unsupported configuration (interval must be 4, 5 or 6, scale 1..4, sizes within the 32-bit launch fields)";
        case MULUT_EHIP: return "HIP runtime error";
        case MULUT_ENODEVICE: return "no usable HIP device (there is no CPU path)";
        case MULUT_ENOTCONFIGURED: return "mulut_configure() has not been called";
        case MULUT_EWORKSPACE: return "input rows do not cover the strip plus halo";
        default: return "unknown error";
    }
}

const char *mulut_last_hip_error(const mulut_ctx *ctx) { return ctx ? ctx->hip_err.c_str() : ""; }

int mulut_create(int device_id, mulut_ctx **out_ctx) {
    if (!out_ctx) return MULUT_EINVAL;
    *out_ctx = nullptr;
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) return MULUT_ENODEVICE;
    if (device_id < 0 || device_id >= n) return MULUT_EINVAL;
    mulut_ctx *c = new (std::nothrow) mulut_ctx();
    if (!c) return MULUT_EINVAL;
    c->device = device_id;
    if (hipSetDevice(device_id) != hipSuccess) {
        delete c;
        return MULUT_ENODEVICE;
    }
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, device_id) == hipSuccess && prop.multiProcessorCount > 0)
        c->num_cus = prop.multiProcessorCount;
    *out_ctx = c;
    return MULUT_OK;
}

int mulut_destroy(mulut_ctx *ctx) {
    if (!ctx) return MULUT_EINVAL;
    (void)hipSetDevice(ctx->device);
    (void)wait_for_device(ctx);     // kernels still queued read what the context's members free as they die
    delete ctx;
    return MULUT_OK;
}

int mulut_configure(mulut_ctx *ctx, int stages, const char *modes, int scale, int interval) {
    if (!ctx || !modes) return MULUT_EINVAL;
    const size_t M = strlen(modes);
    if (stages < 1 || stages > MULUT_MAX_STAGES || M < 1 || M > MULUT_MAX_MODES) return MULUT_EUNSUPPORTED;
    if ((interval != kInterval && interval != 5 && interval != 6) || scale < 1 || scale > 4) return MULUT_EUNSUPPORTED;
    // tiles of the s / d / y kernels always stage a 2-px halo (d / y patterns; s-only models use it too); a list with a 4 x 4
    // pattern (e, h, o) reaches 3 px per stage and runs on the wide kernels
    // (a refused call leaves the context as it was: the whole list is checked before anything of the context is written)
    int reach = 2;
    signed char di[MULUT_MAX_MODES][3], dj[MULUT_MAX_MODES][3];
    for (size_t m = 0; m < M; ++m) {
        int oi[3], oj[3];
        if (!pattern_offsets(modes[m], oi, oj)) return MULUT_EMODE;
        reach = imax(reach, pattern_reach(modes[m]));
        for (int k = 0; k < 3; ++k) {
            di[m][k] = (signed char)oi[k];
            dj[m][k] = (signed char)oj[k];
        }
    }
    if (interval != ctx->tab_interval) {
        // tables of another interval have another row count: none of them can serve this one (MULUT_ENOLUT until set again)
        HIP_TRY(ctx, hipSetDevice(ctx->device));
        const int wrc = wait_for_device(ctx);
        if (wrc) return wrc;
        for (auto &st : ctx->tab)
            for (auto &t : st) {
                const int rc = t.clear(ctx);
                if (rc) return rc;
            }
        ctx->tab_interval = interval;
    }
    memcpy(ctx->di, di, sizeof(di));
    memcpy(ctx->dj, dj, sizeof(dj));
    ctx->stages = stages;
    ctx->n_modes = (int)M;
    ctx->scale = scale;
    ctx->interval = interval;
    memcpy(ctx->modes, modes, M + 1);
    ctx->reach = reach;
    ctx->wide = reach > 2;
    for (int last = 0; last < 2; ++last) {
        const DivMagic dm = make_div_magic((uint32_t)stage_divisor((int)M, last != 0));
        const int span = 128 * kQ * 4 * (int)M;      // |q * sum| <= 128 * 16 * 4M
        ctx->f32_ok[last] = rhe_f32_valid(-span + stage_bias_num((int)M, last != 0), span + stage_bias_num((int)M, last != 0),
                                          dm, 1.0f / (float)dm.d) ? 1 : 0;
    }
    {   // final stage on value+128 rows: sums are biased by 128 per weight unit, S in [0, 255 * 16 * 4M]
        const DivMagic dm = make_div_magic((uint32_t)stage_divisor((int)M, true));
        const int unbias = 128 * kQ * 4 * (int)M - stage_bias_num((int)M, true);
        const float inv_d = 1.0f / (float)dm.d;
        ctx->epi_c = -(float)unbias * inv_d;
        ctx->fma_ok = rhe_fma_valid((uint32_t)(255 * kQ * 4 * (int)M), unbias, dm, inv_d, ctx->epi_c) ? 1 : 0;
    }
    {   // non-final stages: clip(rhe((K + 127 d) / d)) = cvt_u8(fma(K, 1/d, 127)), K in [-128 * 16 * 4M, 127 * 16 * 4M]
        const DivMagic dm = make_div_magic((uint32_t)stage_divisor((int)M, false));
        const int span = 128 * kQ * 4 * (int)M;
        ctx->fma1_ok = rhe_fma_valid_i(-span, span, stage_bias_num((int)M, false), dm, 1.0f / (float)dm.d, 127.0f) ? 1 : 0;
    }
    ctx->configured = true;
    return MULUT_OK;
}

int mulut_set_lut(mulut_ctx *ctx, int stage, char mode, const int8_t *host_rows, int64_t rows, int vnum) {
    if (!ctx || !host_rows) return MULUT_EINVAL;
    if (stage < 1 || stage > MULUT_MAX_STAGES) return MULUT_EINVAL;
    const int pid = pattern_id(mode);
    if (pid < 0) return MULUT_EMODE;
    const int iv = ctx->tab_interval;
    if (rows != interval_rows(iv)) return MULUT_ESHAPE;
    int u = 0;
    for (int k = 1; k <= 4; ++k)
        if (k * k == vnum) u = k;
    if (!u) return MULUT_ESHAPE;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    DevTable &t = ctx->tab[stage - 1][pid];
    if (t.dev) {        // a table of the same shape is rewritten in place, another one is freed; an empty slot has no reader
        const int wrc = wait_for_device(ctx);
        if (wrc) return wrc;
    }
    if (iv != kInterval) {
        // intervals 5 / 6: the plain int8 rows, padded to iv_row_bytes(u) (stage_interval_kernel and pass_kernel<5 / 6> read nothing else)
        const int rb = iv_row_bytes(u);
        std::vector<uint8_t> img((size_t)iv_table_bytes((int)rows, u), 0);
        for (int64_t i = 0; i < rows; ++i) memcpy(&img[(size_t)i * rb], host_rows + i * vnum, (size_t)vnum);
        int rc = t.dev.upload(ctx, img);
        if (!rc) rc = t.tube.release(ctx);
        if (!rc) rc = t.slab.release(ctx);
        if (rc) return rc;
        t.vnum = vnum;
        return MULUT_OK;
    }
    std::vector<uint8_t> img;
    if (u == 1) {
        img.assign(kU1TableBytes, 0);
        memcpy(img.data(), host_rows, kRows);
    } else {
        const int rb = row_dwords(u) * 4;
        img.assign((size_t)kRows * rb, 128);
        for (int64_t i = 0; i < kRows; ++i)
            for (int e = 0; e < vnum; ++e) img[(size_t)i * rb + e] = (uint8_t)((int)host_rows[i * vnum + e] + 128);
    }
    int rc = t.dev.upload(ctx, img);
    if (rc) return rc;
    t.vnum = vnum;
    // e / h / o tables: the wide kernels gather from the full table only (no tube band, no anchor slabs)
    const bool band = pattern_reach(mode) <= 2;
    rc = band ? t.tube.upload(ctx, tube_band(u, host_rows, img)) : t.tube.release(ctx);
    if (rc) return rc;
    return band && u == 4 ? t.slab.upload(ctx, slab_pairs(img)) : t.slab.release(ctx);
}

long long mulut_read_table_image(mulut_ctx *ctx, int stage, char mode, int which, void *host_out, long long cap, void *stream) {
    if (!ctx || cap < 0 || (cap > 0 && !host_out) || which < 0 || which > 2) return MULUT_EINVAL;
    if (stage < 1 || stage > MULUT_MAX_STAGES) return MULUT_EINVAL;
    const int pid = pattern_id(mode);
    if (pid < 0) return MULUT_EMODE;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const DevTable &t = ctx->tab[stage - 1][pid];
    const DevBuf<uint8_t> &img = which == 0 ? t.dev : which == 1 ? t.tube : t.slab;
    HIP_TRY(ctx, hipStreamSynchronize((hipStream_t)stream));
    const long long size = img ? (long long)img.cap : 0, n = size < cap ? size : cap;
    if (n > 0) HIP_TRY(ctx, hipMemcpy(host_out, img.p, (size_t)n, hipMemcpyDeviceToHost));
    return size;
}

// bracket the dominant kernel of a stage with events when timing is on (mulut_last_kernel_ms)
#define MAIN_KERNEL(ctx, stage, st, launch)                                                   \
    do {                                                                                      \
        if ((ctx)->timing) HIP_TRY(ctx, hipEventRecord((ctx)->evk[(stage) - 1][0].e, st));      \
        HIP_TRY(ctx, launch);                                                                 \
        if ((ctx)->timing) {                                                                  \
            HIP_TRY(ctx, hipEventRecord((ctx)->evk[(stage) - 1][1].e, st));                      \
            (ctx)->evk_set[(stage) - 1] = true;                                               \
        }                                                                                     \
    } while (0)

static int stage_u(const mulut_ctx *ctx, int stage) { return stage == ctx->stages ? ctx->scale : 1; }

// Tables of one stage in mode order, shape-checked against the stage's upscale.
static int stage_tables(const mulut_ctx *ctx, int stage, const void **lut) {
    const int vnum = stage_u(ctx, stage) * stage_u(ctx, stage);
    for (int m = 0; m < ctx->n_modes; ++m) {
        const DevTable &t = ctx->tab[stage - 1][pattern_id(ctx->modes[m])];
        if (!t.dev) return MULUT_ENOLUT;
        if (t.vnum != vnum) return MULUT_ESHAPE;
        lut[m] = t.dev.p;
    }
    return MULUT_OK;
}

int mulut_pass(mulut_ctx *ctx, int stage, char mode, int r, const uint8_t *in_chw, int H, int W, int C,
               int32_t *out_q, void *stream) {
    if (!ctx || !in_chw || !out_q || H <= 0 || W <= 0 || C <= 0 || r < 0 || r > 3) return MULUT_EINVAL;
    if (!ctx->configured) return MULUT_ENOTCONFIGURED;
    if (stage < 1 || stage > ctx->stages) return MULUT_EINVAL;
    const int pid = pattern_id(mode);
    if (pid < 0) return MULUT_EMODE;
    const DevTable &t = ctx->tab[stage - 1][pid];
    if (!t.dev) return MULUT_ENOLUT;
    const int u = stage_u(ctx, stage);
    if (t.vnum != u * u) return MULUT_ESHAPE;
    PassArgs a;
    a.in = in_chw;
    a.out = out_q;
    a.lut = t.dev.p;
    a.C = C; a.H = H; a.W = W; a.u = u; a.r = r;
    int di[3], dj[3];
    pattern_offsets(mode, di, dj);
    for (int k = 0; k < 3; ++k) {
        a.di[k] = (signed char)di[k];
        a.dj[k] = (signed char)dj[k];
    }
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, launch_pass(a, ctx->interval, (hipStream_t)stream));
    return MULUT_OK;
}

// The launch arguments hold a row stride (W * u * C for a packed output), the output's row numbers (H * u) and the tile counts of a
// launch (the smallest tiling is 32 x 8) in int fields: a call whose sizes would not fit them is refused by every entry point, before
// anything is allocated or launched.  rows: the most rows of one image that a stage of the call computes
static bool sizes_fit_int(const mulut_ctx *ctx, int N, int rows, int H, int W, int C) {
    const long long lim = 0x7fffffffLL, u = ctx->scale;
    if ((long long)W * u * C > lim || (long long)H * u > lim) return false;
    const long long tiles = (long long)((W + 31) / 32) * ((rows + 7) / 8);      // (< 2^54; then N * tiles < 2^62)
    return tiles <= lim && (long long)N * tiles <= lim;
}

static View make_view(const uint8_t *p, int layout, int rows, int W, int C, int row0) {
    View v;
    v.p = const_cast<uint8_t *>(p);
    v.row0 = row0;
    if (layout == MULUT_LAYOUT_HWC) {
        v.sX = C; v.sC = 1; v.sY = W * C;
    } else {
        v.sX = 1; v.sY = W; v.sC = (long long)rows * W;
    }
    v.sN = (long long)rows * W * C;
    return v;
}

// Routes of a stage launch (plan_stage)
enum Route {
    kRouteIvLds,    // interval 5 / 6: stage_interval_kernel with the stage's tables in LDS
    kRouteIvGlobal, // interval 5 / 6: stage_interval_kernel gathering rows from the tables in global memory
    kRouteWide1,    // a list with a 4 x 4 pattern (e, h, o), 1-byte rows: stage_u1w_kernel at halo 3 ("stage_wide1_kernel")
    kRouteWideUp,   // the same, u > 1: stage_up_kernel at halo 3 ("stage_wide_up_kernel<u>")
    kRouteU1Full,   // 1-byte rows: window kernel (full table in LDS) on every tile
    kRouteU1Tube,   // 1-byte rows: tube kernel (+ window kernel on the tiles it marks, when routed) + site fix-up
    kRouteUpTube,   // x2 / x3: tube-band kernel + site fix-up (+ gather kernel on the tiles it marks, when routed)
    kRouteGather,   // u > 1: gather kernel on every tile
    kRouteTube,     // x4: tube kernel on every tile + pixel fix-up
    kRouteHybrid,   // x4: tile statistic, tube kernel on the smooth tiles, slab path or gather kernel on the detailed ones, pixel fix-up
};

// What one stage launch runs and what it needs.  plan_stage is the one place that decides it: run_stage_one executes the plan,
// stage_fit_images splits a batch by its index width, mulut_reserve sizes the buffers from it and mulut_kernel_name names it.
struct StagePlan {
    Route route;
    bool routed;            // kRouteU1Tube / kRouteUpTube: the tiles the tube kernel calls detailed go to the window / gather kernel
    bool tube2;             // x4 tube kernel: stage_tube2_kernel (else stage_tube_kernel)
    bool slab;              // kRouteHybrid: detailed tiles on the anchor slabs (else the gather kernel)
    bool wide4;             // x4 gather kernel: stage_up_wide4 (merged 16-bit fields hold 4 modes at most)
    int out_mode;           // K2Out of the x4 kernels
    int tiles_x, tiles_y;   // grid of the stage's main kernel
    size_t fix_ids, tlist_tiles, verdict_tiles;             // work lists (0: not used)
    size_t det_tiles, det_items, det_ids, det_blocks;       // buffers of the slab path
    // Index widths of the device work lists: site ids of the 1-byte-row / x2 / x3 tube kernels 32 bits (N C H W), pixel ids of the
    // x4 fix-up list 30 bits (N H W), sample descriptors of the slab path 28 bits of byte offset into the stage input.  The width
    // that admits the fewest images, and what one image takes of it (0: no list)
    unsigned long long width, per_image;
};

static void tile_grid(const StageArgs &a, void (*tile)(int &, int &), int &tiles_x, int &tiles_y) {
    int tw, th;
    tile(tw, th);
    tiles_x = (a.W + tw - 1) / tw;
    tiles_y = (a.oy1 - a.oy0 + th - 1) / th;
}

// The launch arguments every route shares; run_stage_one adds the tables and the route's own fields
static StageArgs stage_args(const mulut_ctx *ctx, int stage, const View &in, const View &out, int N, int H, int W, int C, int oy0, int oy1) {
    StageArgs a;
    memset(&a, 0, sizeof(a));
    const bool last = stage == ctx->stages;
    a.in = in; a.out = out;
    a.dbg = ctx->dbg.p;
    // in_padded: the input lies inside a workspace buffer, at its base or anywhere behind it.  A sub-launch of a large batch reads its
    // images from the middle of one, and what follows them there is more of the buffer or its padding (ensure_workspace).
    a.in_padded = 0;
    for (int k = 0; k < 2; ++k)
        if (ctx->ws[k] && in.p >= ctx->ws[k].p && in.p < ctx->ws[k].p + ctx->ws[k].cap) a.in_padded = 1;
    a.N = N; a.C = C; a.H = H; a.W = W;
    a.oy0 = oy0; a.oy1 = oy1;
    a.M = ctx->n_modes;
    for (int m = 0; m < ctx->n_modes; ++m)
        for (int k = 0; k < 3; ++k) {
            a.di[m][k] = ctx->di[m][k];
            a.dj[m][k] = ctx->dj[m][k];
        }
    a.div = make_div_magic((uint32_t)stage_divisor(ctx->n_modes, last));
    a.bias_num = stage_bias_num(ctx->n_modes, last);
    a.inv_d = 1.0f / (float)a.div.d;
    a.use_f32 = ctx->f32_ok[last ? 1 : 0];
    a.epi_c = last ? ctx->epi_c : 127.0f;
    a.use_fma = last ? ctx->fma_ok : ctx->fma1_ok;
    if (stage_u(ctx, stage) == 1 && last && !ctx->wide) a.use_fma = 0;     // (a final stage with 1-byte rows -- scale 1 -- takes the integer epilogue)
    a.verdict_take = -1;
    return a;
}

// Route of a launch with upscale u and arguments a (tiles unset); C <= 3.  packed_ok: the output may take the packed-RGB store (a
// pixel stride of exactly 3)
static StagePlan plan_stage(const mulut_ctx *ctx, const Routing &r, int u, const StageArgs &a, int out_layout, bool packed_ok) {
    StagePlan p;
    memset(&p, 0, sizeof(p));
    const unsigned long long N = (unsigned long long)a.N, rows = (unsigned long long)(a.oy1 - a.oy0), sites = (unsigned long long)a.C * a.H * a.W;
    auto bind = [&](unsigned long long width, unsigned long long per_image) {
        if (!p.width || (width - 1) / per_image < (p.width - 1) / p.per_image) {
            p.width = width;
            p.per_image = per_image;
        }
    };
    if (ctx->interval != kInterval) {
        // interval 5 / 6: every stage on stage_interval_kernel, before any other route (they are all built for q = 16, L = 17);
        // the tables sit in LDS when the whole stage's fit kIvLdsBudget.  No work lists; the tuning keys do not apply
        tile_grid(a, stage_interval_tile, p.tiles_x, p.tiles_y);
        p.route = (long long)a.M * iv_table_bytes(interval_rows(ctx->interval), u) <= kIvLdsBudget ? kRouteIvLds : kRouteIvGlobal;
        return p;
    }
    if (ctx->wide) {
        // a list with a 4 x 4 pattern: every stage on the wide kernels, before any tube / hybrid / slab / fix-up / tile-statistic
        // path (they all stage a 2-px halo or assume the s / d / y offsets); no work lists
        p.route = u == 1 ? kRouteWide1 : kRouteWideUp;
        tile_grid(a, u == 1 ? stage_u1_tile : stage_up_tile, p.tiles_x, p.tiles_y);
        return p;
    }
    if (u == 1) {
        // (any mode list: the bands live in LDS per PATTERN, a repeated pattern is simply computed again into the int32 sum)
        tile_grid(a, stage_u1_tile, p.tiles_x, p.tiles_y);
        p.route = (r.first_kernel == 0 || r.first_kernel == 3) && N * sites < (1ull << 32) ? kRouteU1Tube : kRouteU1Full;
        if (p.route == kRouteU1Full) return p;
        p.routed = r.first_kernel == 0;
        p.fix_ids = N * a.C * rows * a.W;
        p.tlist_tiles = N * p.tiles_x * p.tiles_y;
        bind(1ull << 32, sites);
        return p;
    }
    if (u == 4 && (out_layout == MULUT_LAYOUT_CHW || (a.C == 1 && packed_ok))) p.out_mode = kOutPlanarU4;
    else if (u == 4 && out_layout == MULUT_LAYOUT_HWC && a.C == 3 && packed_ok) p.out_mode = kOutPackedRGBU4;
    else p.out_mode = kOutGeneric;
    if ((u == 2 || u == 3) && r.final_kernel != 1 && N * sites < (1ull << 32)) {
        // x2 / x3 final stage on the tube band (the 1-byte-row kernel family with 4- / 9-value rows); flagged sites recomputed from the
        // full table.  final_kernel 5: the tube kernel on every tile; otherwise routed by the 1-byte-row family's local-detail
        // statistic -- detailed 64 x 64 tiles (where most sites would end up on the fix-up list) go to the gather kernel
        tile_grid(a, stage_u1t_tile, p.tiles_x, p.tiles_y);
        p.route = kRouteUpTube;
        p.routed = r.final_kernel != 5;
        p.fix_ids = N * a.C * rows * a.W;
        if (p.routed) p.tlist_tiles = N * p.tiles_x * p.tiles_y;
        bind(1ull << 32, sites);
        return p;
    }
    // u == 4: the LDS kernels (tube bands resident) for up to 3 modes, and for longer lists that stage_tube2_kernel takes as a multiset of
    // its three patterns; final_kernel 5 = on every tile, 0 / 6 = hybrid with the per-tile statistic
    p.tube2 = u == 4 && r.tube2 && stage_tube2_supported(a);
    p.wide4 = u == 4 && a.M > 4;
    // (a launch whose pixel ids would pass the 30 bits of the fix-up list -- one image that large: run_stage splits batches -- takes the
    // gather kernel, as the 1-byte-row and x2 / x3 families fall back at 2^32 site ids)
    if (u != 4 || r.final_kernel == 1 || (a.M > 3 && !p.tube2) || N * a.H * a.W >= (1ull << 30)) {
        tile_grid(a, stage_up_tile, p.tiles_x, p.tiles_y);
        p.route = kRouteGather;
        return p;
    }
    tile_grid(a, stage_band_tile, p.tiles_x, p.tiles_y);
    p.route = r.final_kernel == 5 ? kRouteTube : kRouteHybrid;
    p.fix_ids = N * rows * a.W * 3;     // every sample of the launch may end up on the fix-up list (entries: 30-bit pixel id + channel)
    bind(1ull << 30, (unsigned long long)a.H * a.W);
    if (p.route == kRouteTube) return p;
    // per-tile choice on the device: smooth tiles -> tube kernel, detailed tiles -> anchor slabs in LDS (samples grouped by anchor
    // MSB), or the full-table gather kernel where that path does not apply
    p.verdict_tiles = N * p.tiles_x * p.tiles_y;
    StageArgs t = a;
    t.tiles_x = p.tiles_x;
    t.tiles_y = p.tiles_y;
    p.slab = r.detail_kernel == 0 && detail_slab_supported(t);
    if (p.slab) {
        p.det_tiles = p.verdict_tiles;
        p.det_items = detail_items_max(t);
        p.det_ids = detail_ids_count(t);
        p.det_blocks = detail_blocks_count(t);
        bind(1ull << 28, (unsigned long long)(a.in.sN < 0 ? -a.in.sN : a.in.sN));
    }
    return p;
}

// Device buffers a plan needs (grown, never shrunk)
static int ensure_plan(mulut_ctx *ctx, const StagePlan &p) {
    int rc = MULUT_OK;
    if (p.fix_ids) rc = ctx->fix.grow(ctx, p.fix_ids + 16);      // (header + ids)
    if (!rc && p.tlist_tiles) rc = ctx->tlist.grow(ctx, p.tlist_tiles + 16);
    if (!rc && p.verdict_tiles) rc = ctx->verdict.grow(ctx, p.verdict_tiles);
    if (rc || !p.det_tiles) return rc;
    DetailBufs &d = ctx->det;
    if (!d.ctl) {
        rc = d.ctl.grow(ctx, kDetCtlDwords);
        if (rc) return rc;
        HIP_TRY(ctx, hipMemset(d.ctl.p, 0, kDetCtlDwords * sizeof(uint32_t)));
    }
    rc = d.thist.grow(ctx, p.det_tiles * 16);
    if (!rc) rc = d.tpos.grow(ctx, p.det_tiles * 16);
    if (!rc) rc = d.dlist.grow(ctx, p.det_tiles);
    if (!rc) rc = d.items.grow(ctx, p.det_items * 2);
    if (!rc) rc = d.desc.grow(ctx, p.det_ids);
    if (!rc) rc = d.blocks.grow(ctx, p.det_blocks);
    return rc;
}

// pattern id of every mode of the list (stage_interval_kernel takes one instance of its pass body per pattern)
static void fill_patterns(const mulut_ctx *ctx, PatternArgs &p) {
    for (int m = 0; m < kMaxModes; ++m) p.pat[m] = m < ctx->n_modes ? pattern_id(ctx->modes[m]) : 0;
}

// Launch one stage: input view holds LR rows [in.row0, ...), outputs for LR rows [oy0, oy1).
// C channels are processed (<= 3); they may be a group of an image with more (then the views carry that image's strides and
// packed_ok is false: the packed-RGB store needs a pixel stride of exactly 3)
// k1_ref / k1_n0: when this launch is a sub-launch of a larger one (run_stage below), the buffer and first image of the WHOLE launch --
// what the first stage's tile marks are recorded against
static int run_stage_one(mulut_ctx *ctx, int stage, const View &in, const View &out, int out_layout, int N, int H, int W,
                         int C, int oy0, int oy1, hipStream_t st, bool packed_ok, const uint8_t *k1_ref, int k1_n0) {
    StageArgs a = stage_args(ctx, stage, in, out, N, H, W, C, oy0, oy1);
    int rc = stage_tables(ctx, stage, a.lut);
    if (rc) return rc;
    const int u = stage_u(ctx, stage);
    const StagePlan p = plan_stage(ctx, ctx->routing, u, a, out_layout, packed_ok);
    a.tiles_x = p.tiles_x;
    a.tiles_y = p.tiles_y;
    if (p.route == kRouteIvLds || p.route == kRouteIvGlobal) {
        ctx->k1_valid = false;      // (no tile marks are left for the next stage)
        const bool last = stage == ctx->stages;
        IvArgs v;
        memset(&v, 0, sizeof(v));
        fill_patterns(ctx, v);
        v.reach = ctx->reach;
        v.dm = make_div_magic((uint32_t)iv_div_modes(ctx->n_modes, last));
        v.bias_num = ctx->interval == 5 ? iv_bias_num<5>(ctx->n_modes, last) : iv_bias_num<6>(ctx->n_modes, last);
        v.table_bytes = iv_table_bytes(interval_rows(ctx->interval), u);
        MAIN_KERNEL(ctx, stage, st, launch_stage_interval(a, v, ctx->interval, u, p.route == kRouteIvLds, ctx->num_cus, st));
        return MULUT_OK;
    }
    if (p.route == kRouteWide1 || p.route == kRouteWideUp) {
        ctx->k1_valid = false;      // (no tile marks are left for the next stage)
        if (p.route == kRouteWide1) MAIN_KERNEL(ctx, stage, st, launch_stage_wide1(a, st));
        else MAIN_KERNEL(ctx, stage, st, launch_stage_wide_up(a, u, st));
        return MULUT_OK;
    }
    // marks of the first-stage launch that produced this stage's input (same buffer, same shape); consumed here, never kept
    const bool k1_marks = ctx->k1_valid && ctx->k1_out == k1_ref && k1_n0 + N <= ctx->k1_N && ctx->k1_W == W && ctx->k1_H == H && ctx->k1_oy0 <= oy0 &&
                          oy1 <= ctx->k1_oy1;      // the marks cover exactly the images and rows that launch wrote: never index past its tile grid
    ctx->k1_valid = false;
    if (p.route == kRouteU1Full || p.route == kRouteGather) {
        if (p.route == kRouteU1Full) MAIN_KERNEL(ctx, stage, st, launch_stage_u1(a, st));
        else if (p.wide4) MAIN_KERNEL(ctx, stage, st, launch_stage_up_wide4(a, st));
        else MAIN_KERNEL(ctx, stage, st, launch_stage_up(a, u, p.out_mode, st));
        return MULUT_OK;
    }
    // the tube kernels: sites (pixels at x4) they flag are recomputed from the full tables, the tiles they leave go to the full-table
    // kernels -- both through device-side lists (no host synchronisation, hipGraph-capturable)
    if ((unsigned long long)N * p.per_image >= p.width) return MULUT_EUNSUPPORTED;     // (one image beyond a width: run_stage splits batches)
    rc = ensure_plan(ctx, p);
    if (rc) return rc;
    a.fix_count = ctx->fix.p;
    a.fix_list = ctx->fix.p + 16;
    HIP_TRY(ctx, hipMemsetAsync(ctx->fix.p, 0, sizeof(uint32_t), st));
    BandArgs b;
    for (int m = 0; m < ctx->n_modes; ++m) b.band[m] = ctx->tab[stage - 1][pattern_id(ctx->modes[m])].tube.p;
    if (p.route == kRouteU1Tube || p.route == kRouteUpTube) {
        StageArgs g = a;            // the gather kernel's launch on the tiles the tube kernel leaves (its own tiling)
        tile_grid(g, stage_up_tile, g.tiles_x, g.tiles_y);
        if (p.routed) HIP_TRY(ctx, hipMemsetAsync(ctx->tlist.p, 0, (16 + p.tlist_tiles) * sizeof(uint32_t), st));
        if (p.route == kRouteU1Tube || p.routed) {
            a.tile_count = ctx->tlist.p;
            a.tile_list = ctx->tlist.p + 16;
        }
        a.verdict_take = p.routed ? 0 : -1;
        if (p.route == kRouteUpTube) {
            if (u == 2) MAIN_KERNEL(ctx, stage, st, launch_stage_u2t(a, b, (unsigned)ctx->up_detail_per_1024, ctx->num_cus, st));
            else MAIN_KERNEL(ctx, stage, st, launch_stage_u3t(a, b, (unsigned)ctx->up_detail_per_1024, ctx->num_cus, st));
            g.tile_list = a.tile_list;
            if (p.routed) HIP_TRY(ctx, launch_stage_up(g, u, kOutGeneric, st));
            return MULUT_OK;
        }
        MAIN_KERNEL(ctx, stage, st, launch_stage_u1t(a, b, (unsigned)ctx->u1_detail_per_1024, st));
        if (p.routed) HIP_TRY(ctx, launch_stage_u1w_list(a, ctx->num_cus, st));
        HIP_TRY(ctx, launch_stage_u1_fix(a, ctx->num_cus, st));
        ctx->k1_valid = p.routed;
        ctx->k1_N = N; ctx->k1_W = W; ctx->k1_tiles_x = a.tiles_x; ctx->k1_tiles_y = a.tiles_y; ctx->k1_oy0 = oy0; ctx->k1_oy1 = oy1; ctx->k1_H = H;
        ctx->k1_out = out.p;
        return MULUT_OK;
    }
    // (a launch without the slab path leaves none of an earlier launch's counters behind: mulut_last_detail_counters)
    if (!p.slab && ctx->det.ctl) HIP_TRY(ctx, hipMemsetAsync(ctx->det.ctl.p, 0, kDetCtlDwords * sizeof(uint32_t), st));
    auto tube = [&]() {
        return p.tube2 ? launch_stage_tube2(a, b, p.out_mode, ctx->num_cus, st) : launch_stage_tube(a, b, p.out_mode, ctx->num_cus, st);
    };
    if (p.route == kRouteTube) {
        MAIN_KERNEL(ctx, stage, st, tube());
        HIP_TRY(ctx, launch_stage_up_fix(a, ctx->num_cus, st));
        return MULUT_OK;
    }
    // the control words of the slab path are cleared before the statistic: it raises ctl[kDetAny] when it marks a tile
    if (p.slab) HIP_TRY(ctx, hipMemsetAsync(ctx->det.ctl.p, 0, kDetCtlDwords * sizeof(uint32_t), st));
    if (ctx->stat_from_k1 && k1_marks) {
        a.k1_hdr = ctx->tlist.p;
        a.k1_tiles_x = ctx->k1_tiles_x; a.k1_tiles_y = ctx->k1_tiles_y; a.k1_oy0 = ctx->k1_oy0; a.k1_n0 = k1_n0;
    }
    HIP_TRY(ctx, launch_tile_stat(a, ctx->verdict.p, (uint32_t)ctx->hybrid_oob_per_1024, st, p.slab ? ctx->det.thist.p : nullptr, p.slab ? ctx->det.ctl.p + kDetAny : nullptr));
    a.k1_hdr = nullptr;
    a.verdict = ctx->verdict.p;
    a.vt_x = a.tiles_x;
    a.vt_y = a.tiles_y;
    a.verdict_take = 0;
    MAIN_KERNEL(ctx, stage, st, tube());
    if (p.slab) {
        DetailArgs d;
        memset(&d, 0, sizeof(d));
        ctx->det.fill(d);
        for (int m = 0; m < 3; ++m) d.slab[m] = m < ctx->n_modes ? ctx->tab[stage - 1][pattern_id(ctx->modes[m])].slab.p : nullptr;
        HIP_TRY(ctx, launch_detail_slab(a, d, p.out_mode, ctx->num_cus, st));
    } else {
        StageArgs g = a;
        tile_grid(g, stage_up_tile, g.tiles_x, g.tiles_y);
        g.verdict_take = 1;
        if (p.wide4) HIP_TRY(ctx, launch_stage_up_wide4(g, st));
        else HIP_TRY(ctx, launch_stage_up(g, u, p.out_mode, st));
    }
    HIP_TRY(ctx, launch_stage_up_fix(a, ctx->num_cus, st));
    return MULUT_OK;
}

// Images are independent (sr/4_test_lut.py:257-259 fans them out one by one), so a launch beyond an index width of its work lists
// (StagePlan::width) runs as sub-launches of whole images that fit -- every entry point (mulut_stage, mulut_pipeline_rows,
// mulut_pipeline) comes through here, none falls to a slower kernel because of its batch size.  How many images of the launch fit
// one sub-launch (>= 1; N when nothing binds):
static int stage_fit_images(const mulut_ctx *ctx, const Routing &r, int stage, const View &in, int N, int H, int W, int C, int oy0, int oy1) {
    // (the route of one image, and the widths its lists bind)
    const StagePlan p = plan_stage(ctx, r, stage_u(ctx, stage), stage_args(ctx, stage, in, in, 1, H, W, C, oy0, oy1), MULUT_LAYOUT_CHW, false);
    const unsigned long long fit = p.width ? (p.width - 1) / p.per_image : (unsigned long long)N;
    return fit < 1 ? 1 : fit < (unsigned long long)N ? (int)fit : N;
}

static int run_stage(mulut_ctx *ctx, int stage, const View &in, const View &out, int out_layout, int N, int H, int W,
                     int C, int oy0, int oy1, hipStream_t st, bool packed_ok = true) {
    const int fit = stage_fit_images(ctx, ctx->routing, stage, in, N, H, W, C, oy0, oy1);
    if (N <= fit) return run_stage_one(ctx, stage, in, out, out_layout, N, H, W, C, oy0, oy1, st, packed_ok, in.p, 0);
    // the first stage's tile marks (if this stage reads what it wrote) serve every sub-launch: kept across the calls that consume them
    const bool k1_valid = ctx->k1_valid;
    for (int n0 = 0; n0 < N; n0 += fit) {
        View vin = in, vout = out;
        vin.p += (long long)n0 * in.sN;
        vout.p += (long long)n0 * out.sN;
        ctx->k1_valid = k1_valid;
        const int rc = run_stage_one(ctx, stage, vin, vout, out_layout, imin(fit, N - n0), H, W, C, oy0, oy1, st, packed_ok, in.p, n0);
        if (rc) return rc;
    }
    // a split first stage leaves the marks of its last sub-launch only: the next stage must look at every tile itself
    ctx->k1_valid = false;
    return MULUT_OK;
}

int mulut_halo(const mulut_ctx *ctx) { return (ctx && ctx->configured) ? ctx->reach * ctx->stages : 0; }

static int ensure_workspace(mulut_ctx *ctx, size_t bytes) {
    int rc = MULUT_OK;
    for (int k = 0; k < 2 && !rc; ++k) rc = ctx->ws[k].grow(ctx, bytes + 64);      // + padding: kernels may read whole dwords / 8 bytes at the very end (StageArgs::in_padded)
    return rc;
}

int mulut_reserve(mulut_ctx *ctx, int N, int H, int W, int C) {
    if (!ctx || N <= 0 || H <= 0 || W <= 0 || C <= 0) return MULUT_EINVAL;
    if (!ctx->configured) return MULUT_ENOTCONFIGURED;
    if (!sizes_fit_int(ctx, N, H, H, W, C)) return MULUT_EUNSUPPORTED;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    // the plans of every stage's largest launches -- all N images, and the sub-launch a batch beyond an index width runs as (run_stage)
    // -- under the default routes, which use every buffer any route does: a later call of at most this shape allocates nothing,
    // whatever the tuning.  Channels run in groups of <= 3; the input is planar, as a cascade's final stage reads the workspace
    const Routing r;
    const int Cg = imin(C, 3);
    const View in = make_view(nullptr, MULUT_LAYOUT_CHW, H, W, Cg, 0);
    StagePlan need;
    memset(&need, 0, sizeof(need));
    auto atleast = [](size_t &v, size_t x) { v = x > v ? x : v; };
    for (int s = 1; s <= ctx->stages; ++s)
        for (const int n : {N, stage_fit_images(ctx, r, s, in, N, H, W, Cg, 0, H)}) {
            const StagePlan p = plan_stage(ctx, r, stage_u(ctx, s), stage_args(ctx, s, in, in, imin(n, N), H, W, Cg, 0, H), MULUT_LAYOUT_CHW, true);
            atleast(need.fix_ids, p.fix_ids);
            atleast(need.tlist_tiles, p.tlist_tiles);
            atleast(need.verdict_tiles, p.verdict_tiles);
            atleast(need.det_tiles, p.det_tiles);
            atleast(need.det_items, p.det_items);
            atleast(need.det_ids, p.det_ids);
            atleast(need.det_blocks, p.det_blocks);
        }
    const int rc = ensure_plan(ctx, need);
    if (rc || ctx->stages < 2) return rc;
    return ensure_workspace(ctx, (size_t)N * H * W * C);
}

int mulut_stage(mulut_ctx *ctx, int stage, const uint8_t *in, int in_layout, uint8_t *out, int out_layout, int N,
                int H, int W, int C, void *stream) {
    if (!ctx || !in || !out || N <= 0 || H <= 0 || W <= 0 || C <= 0) return MULUT_EINVAL;
    if (!ctx->configured) return MULUT_ENOTCONFIGURED;
    if (stage < 1 || stage > ctx->stages) return MULUT_EINVAL;
    if (!sizes_fit_int(ctx, N, H, H, W, C)) return MULUT_EUNSUPPORTED;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const int u = stage_u(ctx, stage);
    // channels are independent planes through the same tables (sr/4_test_lut.py:14-237 is channel-count agnostic): more than three
    // run in groups of three, each group a view into the caller's buffers
    for (int c0 = 0; c0 < C; c0 += 3) {
        View vin = make_view(in, in_layout, H, W, C, 0), vout = make_view(out, out_layout, H * u, W * u, C, 0);
        vin.p += (long long)c0 * vin.sC;
        vout.p += (long long)c0 * vout.sC;
        const int rc = run_stage(ctx, stage, vin, vout, out_layout, N, H, W, imin(3, C - c0), 0, H, (hipStream_t)stream, C <= 3);
        if (rc) return rc;
    }
    return MULUT_OK;
}

int mulut_pipeline_rows(mulut_ctx *ctx, const uint8_t *in, int in_row0, int in_rows, uint8_t *out, int y0, int y1,
                        int N, int H, int W, int C, int layout, void *stream) {
    if (!ctx || !in || !out || N <= 0 || H <= 0 || W <= 0 || C <= 0) return MULUT_EINVAL;
    if (!ctx->configured) return MULUT_ENOTCONFIGURED;
    if (y0 < 0 || y1 > H || y0 >= y1 || in_row0 < 0 || in_rows <= 0 || (long long)in_row0 + in_rows > H) return MULUT_EINVAL;
    if (!sizes_fit_int(ctx, N, in_rows, H, W, C)) return MULUT_EUNSUPPORTED;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const int S = ctx->stages, reach = ctx->reach;
    // rows of each stage's output that the cascade needs
    int lo[MULUT_MAX_STAGES + 1], hi[MULUT_MAX_STAGES + 1];
    for (int s = 1; s <= S; ++s) {
        lo[s] = imax(0, y0 - reach * (S - s));
        hi[s] = imin(H, y1 + reach * (S - s));
    }
    // the caller's band must cover stage 1's reads
    if (in_row0 > imax(0, lo[1] - reach) || in_row0 + in_rows < imin(H, hi[1] + reach)) return MULUT_EWORKSPACE;
    if (S > 1) {
        size_t need = 0;
        for (int s = 1; s < S; ++s) {
            const size_t b = (size_t)N * imin(C, 3) * (hi[s] - lo[s]) * W;
            if (b > need) need = b;
        }
        int rc = ensure_workspace(ctx, need);
        if (rc) return rc;
    }
    ctx->timed_stages = 0;
    // channels are independent planes through the same tables (the reference function is channel-count agnostic): more than three
    // run as groups of three, each a view into the caller's buffers (stage timing: the last group's)
    for (int c0 = 0; c0 < C; c0 += 3) {
        const int Cg = imin(3, C - c0);
        View cur = make_view(in, layout, in_rows, W, C, in_row0);
        cur.p += (long long)c0 * cur.sC;
        if (ctx->timing) HIP_TRY(ctx, hipEventRecord(ctx->ev[0].e, (hipStream_t)stream));
        for (int s = 1; s <= S; ++s) {
            const int u = stage_u(ctx, s);
            View dst;
            int dst_layout;
            if (s == S) {
                dst = make_view(out, layout, (y1 - y0) * u, W * u, C, y0 * u);
                dst.p += (long long)c0 * dst.sC;
                dst_layout = layout;
            } else {
                dst = make_view(ctx->ws[s & 1].p, MULUT_LAYOUT_CHW, hi[s] - lo[s], W, Cg, lo[s]);
                dst_layout = MULUT_LAYOUT_CHW;
            }
            int rc = run_stage(ctx, s, cur, dst, dst_layout, N, H, W, Cg, lo[s], hi[s], (hipStream_t)stream, C <= 3);
            if (rc) return rc;
            if (ctx->timing) HIP_TRY(ctx, hipEventRecord(ctx->ev[s].e, (hipStream_t)stream));
            cur = dst;
        }
    }
    if (ctx->timing) ctx->timed_stages = S;
    return MULUT_OK;
}

int mulut_pipeline(mulut_ctx *ctx, const uint8_t *in, uint8_t *out, int N, int H, int W, int C, int layout,
                   void *stream) {
    if (!ctx || !in || !out || N <= 0 || H <= 0 || W <= 0 || C <= 0) return MULUT_EINVAL;
    if (!ctx->configured) return MULUT_ENOTCONFIGURED;
    // (batches beyond the index widths of the device work lists run as sub-launches per stage: run_stage)
    return mulut_pipeline_rows(ctx, in, 0, H, out, 0, H, N, H, W, C, layout, stream);
}

int mulut_set_stage_timing(mulut_ctx *ctx, int enable) {
    if (!ctx) return MULUT_EINVAL;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    if (enable) {
        for (auto &e : ctx->ev)
            if (!e.e) HIP_TRY(ctx, hipEventCreate(&e.e));
        for (auto &p : ctx->evk)
            for (auto &e : p)
                if (!e.e) HIP_TRY(ctx, hipEventCreate(&e.e));
    }
    for (auto &f : ctx->evk_set) f = false;
    ctx->timing = enable != 0;
    ctx->timed_stages = 0;
    return MULUT_OK;
}

int mulut_last_stage_ms(mulut_ctx *ctx, float *ms, int cap) {
    if (!ctx || !ms || cap <= 0) return MULUT_EINVAL;
    const int n = ctx->timed_stages < cap ? ctx->timed_stages : cap;
    if (n > 0) HIP_TRY(ctx, hipEventSynchronize(ctx->ev[ctx->timed_stages].e));
    for (int s = 0; s < n; ++s) HIP_TRY(ctx, hipEventElapsedTime(&ms[s], ctx->ev[s].e, ctx->ev[s + 1].e));
    return n;
}

int mulut_last_kernel_ms(mulut_ctx *ctx, float *ms, int cap) {
    if (!ctx || !ms || cap <= 0) return MULUT_EINVAL;
    const int n = ctx->timed_stages < cap ? ctx->timed_stages : cap;
    if (n > 0) HIP_TRY(ctx, hipEventSynchronize(ctx->ev[ctx->timed_stages].e));
    for (int s = 0; s < n; ++s) {
        ms[s] = 0.0f;
        if (ctx->evk_set[s]) HIP_TRY(ctx, hipEventElapsedTime(&ms[s], ctx->evk[s][0].e, ctx->evk[s][1].e));
    }
    return n;
}

int mulut_last_detail_counters(mulut_ctx *ctx, uint32_t *out, int cap, void *stream) {
    if (!ctx || !out || cap <= 0) return MULUT_EINVAL;
    if (!ctx->det.ctl || !ctx->fix) return 0;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    uint32_t ctl[kDetCtlDwords], fixn = 0;
    HIP_TRY(ctx, hipMemcpyAsync(ctl, ctx->det.ctl.p, sizeof(ctl), hipMemcpyDeviceToHost, (hipStream_t)stream));
    HIP_TRY(ctx, hipMemcpyAsync(&fixn, ctx->fix.p, sizeof(fixn), hipMemcpyDeviceToHost, (hipStream_t)stream));
    HIP_TRY(ctx, hipStreamSynchronize((hipStream_t)stream));
    int n = 0;
    for (int k = 0; k < 16 && n < cap; ++k) out[n++] = ctl[k];
    if (n < cap) out[n++] = ctl[kDetItems];
    if (n < cap) out[n++] = fixn;
    for (int k = 48; k < 56 && n < cap; ++k) out[n++] = ctl[k];      // phase clocks of the slabclk probe build (zero otherwise)
    return n;
}

int mulut_debug_read(mulut_ctx *ctx, unsigned long long *out, int cap, int reset, void *stream) {
    if (!ctx || (cap > 0 && !out) || cap < 0) return MULUT_EINVAL;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    if (!ctx->dbg) {
        const int rc = ctx->dbg.grow(ctx, MULUT_DEBUG_WORDS);
        if (rc) return rc;
        HIP_TRY(ctx, hipMemset(ctx->dbg.p, 0, MULUT_DEBUG_WORDS * sizeof(unsigned long long)));
    }
    const int n = cap < MULUT_DEBUG_WORDS ? cap : MULUT_DEBUG_WORDS;
    if (n > 0) HIP_TRY(ctx, hipMemcpyAsync(out, ctx->dbg.p, (size_t)n * sizeof(unsigned long long), hipMemcpyDeviceToHost, (hipStream_t)stream));
    if (reset) HIP_TRY(ctx, hipMemsetAsync(ctx->dbg.p, 0, MULUT_DEBUG_WORDS * sizeof(unsigned long long), (hipStream_t)stream));
    HIP_TRY(ctx, hipStreamSynchronize((hipStream_t)stream));
    return n;
}

int mulut_set_tuning(mulut_ctx *ctx, const char *key, int value) {
    if (!ctx || !key) return MULUT_EINVAL;
    if (!strcmp(key, "final_stage_kernel")) {
        if (value != 0 && value != 1 && value != 5 && value != 6) return MULUT_EINVAL;      // (2-4: generations retired in round 3)
        ctx->routing.final_kernel = value;
        return MULUT_OK;
    }
    if (!strcmp(key, "first_stage_kernel")) {
        if (value != 0 && value != 2 && value != 3) return MULUT_EINVAL;      // (1: retired in round 3)
        ctx->routing.first_kernel = value;
        return MULUT_OK;
    }
    if (!strcmp(key, "stat_from_first_stage")) {
        if (value < 0 || value > 1) return MULUT_EINVAL;
        ctx->stat_from_k1 = value;
        return MULUT_OK;
    }
    if (!strcmp(key, "tube_pipelined")) {
        if (value < 0 || value > 1) return MULUT_EINVAL;
        ctx->routing.tube2 = value;
        return MULUT_OK;
    }
    if (!strcmp(key, "detail_kernel")) {     // final-stage tiles the statistic marks detailed: 0 anchor slabs in LDS, 1 full-table gathers
        if (value < 0 || value > 1) return MULUT_EINVAL;
        ctx->routing.detail_kernel = value;
        return MULUT_OK;
    }
    if (!strcmp(key, "first_stage_detail_per_1024")) {
        if (value < 0 || value > 1024) return MULUT_EINVAL;
        ctx->u1_detail_per_1024 = value;
        return MULUT_OK;
    }
    if (!strcmp(key, "final_stage_detail_per_1024")) {
        if (value < 0 || value > 1024) return MULUT_EINVAL;
        ctx->up_detail_per_1024 = value;
        return MULUT_OK;
    }
    if (!strcmp(key, "hybrid_oob_per_1024")) {
        if (value < 0 || value > 1024) return MULUT_EINVAL;
        ctx->hybrid_oob_per_1024 = value;
        return MULUT_OK;
    }
    return MULUT_EINVAL;
}

const char *mulut_kernel_name(const mulut_ctx *ctx, int is_final) {
    if (!ctx || !ctx->configured) return "";
    // the plan of a representative launch: one whole 3-channel image, read planar (as a cascade's final stage reads the workspace),
    // written as packed RGB; the non-final stage has 1-byte rows
    const int stage = is_final ? ctx->stages : 1, u = is_final ? ctx->scale : 1;
    const View in = make_view(nullptr, MULUT_LAYOUT_CHW, 64, 64, 3, 0);
    const StageArgs ra = stage_args(ctx, stage, in, in, 1, 64, 64, 3, 0, 64);
    const StagePlan p = plan_stage(ctx, ctx->routing, u, ra, MULUT_LAYOUT_HWC, true);
    // is_final 2: the final stage's tube2 kernel alone, with the accumulator form the launch takes
    if (is_final == 2 && p.tube2 && (p.route == kRouteTube || p.route == kRouteHybrid))
        return stage_tube2_one_set(ra, p.out_mode) ? "stage_tube2_kernel<rgb,one-set>" : "stage_tube2_kernel<rgb,two-set>";
    switch (p.route) {
        case kRouteIvLds:
        case kRouteIvGlobal: return stage_interval_name(ctx->interval, u, p.route == kRouteIvLds);
        case kRouteWide1:
        case kRouteWideUp: return stage_wide_name(u);
        case kRouteU1Full: return "stage_u1w_kernel";
        case kRouteU1Tube: return p.routed ? "stage_u1t_kernel (smooth tiles) + stage_u1w_kernel (detailed tiles) + stage_u1_fix_kernel"
                                           : "stage_u1t_kernel + stage_u1_fix_kernel";
        case kRouteUpTube: return u == 2 ? "stage_u1t_kernel<2> + stage_up_fix_site_kernel<2>" : "stage_u1t_kernel<3> + stage_up_fix_site_kernel<3>";
        case kRouteGather: return p.wide4 ? "stage_up_kernel<4,generic,wide>" : stage_up_name(u, p.out_mode);
        case kRouteTube: return p.tube2 ? "stage_tube2_kernel<rgb> + stage_up_fix2_kernel" : "stage_tube_kernel<rgb> + stage_up_fix2_kernel";
        default: break;
    }
    if (p.slab)
        return p.tube2 ? "hybrid: tile_stat_kernel + stage_tube2_kernel<rgb> (smooth tiles; hand-scheduled LDS pipeline, one 16x4 tile per wave) + stage_slab_kernel (detailed tiles, anchor slabs in LDS)"
                       : "hybrid: tile_stat_kernel + stage_tube_kernel<rgb> (smooth tiles) + stage_slab_kernel (detailed tiles, anchor slabs in LDS)";
    if (p.wide4) return "hybrid: tile_stat_kernel + stage_tube2_kernel<rgb> (smooth tiles) + stage_up_kernel<4,generic,wide> (detailed tiles)";
    return p.tube2 ? "hybrid: tile_stat_kernel + stage_tube2_kernel<rgb> (smooth tiles) + stage_up_kernel<4,rgb> (detailed tiles)"
                   : "hybrid: tile_stat_kernel + stage_tube_kernel<rgb> (smooth tiles) + stage_up_kernel<4,rgb> (detailed tiles)";
}

}  // extern "C"
