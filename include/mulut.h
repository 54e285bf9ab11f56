/*
 * mulut.h -- C ABI of libmulut_hip.so: MuLUT LUT inference (4D LUT retrieval + 4-simplex
 * interpolation over rotated s/d/y/e/h/o patches, cascaded stages) on AMD MI355X (gfx950).
 *
 * This is the drop-in boundary for the hot path of the reference's `sr/4_test_lut.py`.  The
 * reference is pure Python and has no FFI layer; each entry point below states which reference
 * lines it replaces (paths relative to the reference repo root), and INTEGRATION.md shows the
 * ctypes binding a maintainer of the reference would add.
 *
 * Conventions
 *   - plain C, no exceptions: every call returns MULUT_OK (0) or a negative MULUT_E* code;
 *     mulut_strerror() names it.
 *   - all image buffers are CALLER-OWNED DEVICE pointers (e.g. torch tensor data_ptr()); the
 *     library owns only its context: device copies of the tables and an intermediate-stage
 *     workspace.  LUT rows passed to mulut_set_lut() are HOST pointers.
 *   - `stream` is a hipStream_t passed as void* (NULL = the null stream); all work is
 *     stream-ordered and asynchronous with respect to the host.
 *   - the set-up calls that overwrite or free device memory of the context WAIT FOR ALL WORK IN FLIGHT ON THE DEVICE first
 *     (hipDeviceSynchronize: the caller's streams are not known to them, and a non-blocking stream is not ordered against the
 *     null stream their copies run on): mulut_set_lut() on a slot that already holds a table, mulut_configure() when it
 *     moves to another interval (it frees every table), mulut_destroy(), and any call that has to enlarge the workspace or a
 *     work list (mulut_reserve(), or a compute call larger than every call before it).  Calls still queued on any stream therefore finish on the tables and buffers
 *     they were issued with.  A compute call that allocates nothing never waits.
 *   - image buffers need NO alignment: any byte address is accepted, in and out, in both layouts (4-aligned bases with
 *     W % 4 == 0 take dword loads and stores, others the byte paths -- the same result), and nothing outside
 *     [out, out + N * H*scale * W*scale * C) is written.
 *   - a call refused for its arguments (MULUT_EINVAL, MULUT_EMODE, MULUT_ESHAPE or MULUT_EUNSUPPORTED from mulut_configure,
 *     mulut_set_lut, mulut_set_tuning) leaves the context as it was.  MULUT_EHIP is no such refusal: a HIP failure part-way through
 *     mulut_set_lut or through the table release of mulut_configure may leave that table (or its band / slab) half replaced; set the
 *     tables again, or destroy the context.
 *   - one context per device; calls on one context must be serialised by the caller.
 *   - there is NO CPU fallback: without a usable HIP device mulut_create() fails.
 *
 * Image layouts
 *   MULUT_LAYOUT_CHW : planar  [N][C][H][W]   (what FourSimplexInterpFaster receives, :296)
 *   MULUT_LAYOUT_HWC : packed  [N][H][W][C]   (what PIL / the driver loop holds, :265-270,:301)
 */
#ifndef MULUT_H_
#define MULUT_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MULUT_VERSION 100 /* 0.1.0 */

enum {
    MULUT_OK = 0,
    MULUT_EINVAL = -1,      /* bad argument (NULL pointer, non-positive size, ...)             */
    MULUT_EMODE = -2,       /* mode not in {s,d,y,e,h,o}: reference raises ValueError, 4_test_lut.py:54 */
    MULUT_ENOLUT = -3,      /* table (stage,mode) not set: reference raises from np.load, :333  */
    MULUT_ESHAPE = -4,      /* table shape does not match (rows, v_num) expected for the stage */
    MULUT_EUNSUPPORTED = -5,/* interval not in {4,5,6}, scale not in 1..4, stages/modes beyond limits, image sizes beyond the
                               32-bit fields of a launch (mulut_pipeline, "Batch size") */
    MULUT_EHIP = -6,        /* a HIP runtime call failed (mulut_last_hip_error() has the text) */
    MULUT_ENODEVICE = -7,   /* no usable gfx950 device: there is no CPU path                   */
    MULUT_ENOTCONFIGURED = -8,
    MULUT_EWORKSPACE = -9   /* strip/halo bookkeeping inconsistent with the buffers given     */
};

enum { MULUT_LAYOUT_CHW = 0, MULUT_LAYOUT_HWC = 1 };

#define MULUT_MAX_STAGES 8
#define MULUT_MAX_MODES 8

typedef struct mulut_ctx mulut_ctx;

int mulut_version(void);
const char *mulut_strerror(int err);
/* text of the last failing HIP call on this context (empty string if none) */
const char *mulut_last_hip_error(const mulut_ctx *ctx);

/* Bind a context to HIP device `device_id`. */
int mulut_create(int device_id, mulut_ctx **out_ctx);
int mulut_destroy(mulut_ctx *ctx);

/* The model shape: replaces the options the reference reads from TestOptions
 * (common/option.py:21-23,17: --stages --modes --interval --scale) at sr/4_test_lut.py:279-287.
 * `modes` is a NUL-terminated string iterated character-wise exactly like `opt.modes` (:287): any mix and repeat of the
 * 3 x 3 patterns s, d, y and the 4 x 4 patterns e, h, o (sr/model.py:12, common/network.py:173-215), up to MULUT_MAX_MODES.
 * A list holding e, h or o is "wide": its keys reach 3 pixels from the anchor, and every stage of it runs on the wide kernels
 * (one table in LDS per mode for 1-byte rows, full-table gathers for u*u-byte rows); a list of s, d, y only runs as before.
 * interval is 4 (q=16, L=17, 83521 rows), 5 (q=32, L=9, 6561 rows) or 6 (q=64, L=5, 625 rows) (sr/4_test_lut.py:14-16); any other
 * value returns MULUT_EUNSUPPORTED.  Every stage of an interval-5 / 6 context runs on stage_interval_kernel (the stage's tables in
 * LDS when they fit 96 KiB, else rows gathered from global memory), whatever the mode list.  Configuring an interval other than
 * the one the context's tables were set for clears every table: pipeline calls return MULUT_ENOLUT until they are set again, and
 * graphs captured before are invalid (see the hipGraph note at mulut_set_tuning). */
int mulut_configure(mulut_ctx *ctx, int stages, const char *modes, int scale, int interval);

/* Upload one table (any of the six patterns): replaces
 *   lutDict["s{stage}_{mode}"] = np.load(path).astype(np.float32).reshape(-1, v_num)
 * (sr/4_test_lut.py:322-333).  `host_rows` is the int8 C-order content of the .npy file,
 * rows = L^4 of the configured interval (83521 at 4 -- also before any mulut_configure() --, 6561 at 5, 625 at 6; anything else
 * returns MULUT_ESHAPE), vnum = scale*scale for the last stage, 1 otherwise.  stage is 1-based.  At interval 5 / 6 the plain rows
 * are uploaded (no tube bands, slabs or 16-bit images are built). */
int mulut_set_lut(mulut_ctx *ctx, int stage, char mode, const int8_t *host_rows, int64_t rows, int vnum);

/* One of the device images a table is kept as (for tests and tools, in the spirit of mulut_last_detail_counters; the reference has
 * no counterpart -- its tables are the arrays of :322-333 and nothing else): which = 0 the full-table image, 1 the tube band, 2 the
 * anchor slab pairs.  Synchronises `stream`, copies min(cap, size) bytes to host_out and returns the image's size in bytes -- 0
 * where the slot holds no such image (no table set; no band for e / h / o tables and at intervals 5 / 6; slab pairs only for
 * vnum 16) -- or a negative MULUT_E* code.  Not on any hot path. */
long long mulut_read_table_image(mulut_ctx *ctx, int stage, char mode, int which, void *host_out, long long cap, void *stream);

/* One (table, mode, rotation) pass: replaces FourSimplexInterpFaster(weight, img_in, h, w,
 * interval, rot=4-r, upscale, mode) (sr/4_test_lut.py:14-237) TOGETHER WITH the caller's
 * np.rot90(img, r) + edge pad (:294-296).  in_chw: device uint8 planar [C][H][W], un-rotated,
 * un-padded.  out_q: device int32 planar [C][H*u][W*u] = q * (the float64 array the reference
 * returns), exact.  u = scale if `stage` is the last configured stage, else 1. */
int mulut_pass(mulut_ctx *ctx, int stage, char mode, int r, const uint8_t *in_chw, int H, int W, int C,
               int32_t *out_q, void *stream);

/* One whole stage (all modes x 4 rotations, average, +bias, round-half-even, clip): replaces one
 * iteration of the `for s in range(stages)` body (sr/4_test_lut.py:280-306).  N images.
 * Any C >= 1 (here and in mulut_pipeline / mulut_pipeline_rows): the kernels take up to three channels per
 * launch, images with more are run as groups of three (channels are independent in the reference too). */
int mulut_stage(mulut_ctx *ctx, int stage, const uint8_t *in, int in_layout, uint8_t *out, int out_layout, int N,
                int H, int W, int C, void *stream);

/* The whole cascade for N images: replaces sr/4_test_lut.py:279-306 (= sr/5_test_lut.py:271-307).
 * in: N x (H,W,C) uint8, out: N x (H*scale, W*scale, C) uint8, both in `layout`.
 * Batch size: the device work lists index one launch with fixed widths (28 bits of byte offset into the stage input on the
 * detailed-tile path of x4 final stages, 30-bit pixel ids, 32-bit site ids).  Every entry point -- this one, mulut_pipeline_rows,
 * mulut_stage -- runs a STAGE whose launch would exceed a width as sub-launches of whole images that fit (43 frames of 1080p RGB
 * per final-stage launch): same result, same kernels; no batch size falls to a slower path.  (The timing helpers then report the
 * last sub-launch of a stage.)  A SINGLE image beyond a width (the widths count the logical image, H or H_full rows, not the rows
 * of a strip) keeps its result and changes kernels:
 *   - stage input of 2^28 bytes or more (x4 final stage): its detailed tiles take the gather kernel, not the anchor slabs;
 *   - H * W >= 2^30 (x4 final stage): the whole stage runs on the gather kernel (stage_up_kernel), no tube kernel or fix-up list;
 *   - C * H * W >= 2^32, C <= 3 the channels of one group (stages with 1-byte rows, x2 / x3 final stages): the window kernel
 *     (stage_u1w_kernel) resp. the gather kernel on every tile.
 * Planes of 2^31 bytes or more, in and out, are supported in both layouts (the image and channel strides are 64-bit).
 * Refused with MULUT_EUNSUPPORTED, by this call, mulut_pipeline_rows, mulut_stage and mulut_reserve alike and before anything is
 * allocated or launched: sizes that do not fit the 32-bit signed fields of the launch arguments -- a packed output row of
 * W * scale * C bytes or H * scale output rows beyond 2^31 - 1, or more than 2^31 - 1 tiles of 32 x 8 sites in one call
 * (N * ceil(W / 32) * ceil(rows / 8), rows = H, or the rows of the band handed to mulut_pipeline_rows). */
int mulut_pipeline(mulut_ctx *ctx, const uint8_t *in, uint8_t *out, int N, int H, int W, int C, int layout,
                   void *stream);

/* Strip form for tile sharding (one strip per GPU).  The logical image is H_full x W; `in` holds
 * its rows [in_row0, in_row0 + in_rows) and `out` receives output rows for LR rows [y0, y1), i.e.
 * HR rows [y0*scale, y1*scale), stored from row 0 of `out`.  The input must cover the halo
 * [y0 - mulut_halo(ctx), y1 + mulut_halo(ctx)) clipped to the image; edge replication happens only
 * at true image borders, so strips tile bit-exactly.  The index widths of "Batch size" (mulut_pipeline) are those of the LOGICAL
 * image: sub-launches, the fall-backs of a single image beyond a width and the refusals are decided from H_full, whatever the
 * band holds -- except the 2^28 bytes of the anchor-slab path, which count the band's bytes. */
int mulut_pipeline_rows(mulut_ctx *ctx, const uint8_t *in, int in_row0, int in_rows, uint8_t *out, int y0, int y1,
                        int N, int H_full, int W, int C, int layout, void *stream);

/* LR rows of context needed above/below a strip for the configured cascade: 2 per stage (the reach of the d / y patterns
 * over the four rotations), 3 per stage for a wide mode list (e, h, o). */
int mulut_halo(const mulut_ctx *ctx);

/* Pre-size the intermediate-stage workspace and every device work list so that later pipeline calls of at most this shape
 * allocate nothing (required before capturing a pipeline call into a hipGraph).  Buffers that only a stage's sub-launches
 * use (see mulut_pipeline, "Batch size") are sized for the largest sub-launch. */
int mulut_reserve(mulut_ctx *ctx, int N, int H, int W, int C);

/* Per-stage device timing for bench.py's roofline leg: when enabled, every mulut_pipeline[_rows]
 * call brackets each stage's kernel launch with hipEvents recorded on the caller's stream;
 * mulut_last_stage_ms() waits for the last call's events and returns the elapsed milliseconds of
 * each stage (n = number of stages written, <= cap).  Off by default (events cost a few us). */
int mulut_set_stage_timing(mulut_ctx *ctx, int enable);
int mulut_last_stage_ms(mulut_ctx *ctx, float *ms, int cap);
/* The same call's milliseconds of each stage's DOMINANT kernel alone (the stage's helper launches -- tile statistic,
 * fix-up lists, the kernel that takes the detailed tiles -- are in mulut_last_stage_ms only): the launch duration
 * bench.py prices against the roofline. */
int mulut_last_kernel_ms(mulut_ctx *ctx, float *ms, int cap);
/* Work counters of the detailed-tile path of the last final-stage launch (scale 4; device -> host copy, synchronises with
 * `stream`): out[0..15] = samples (pixel x channel) per anchor MSB that went through the anchor-slab kernel,
 * out[16] = work items, out[17] = entries (samples, or border pixels with all their channels) on the fix-up list of that launch.  Returns the number of values written
 * (0 when the path has not run; out[0..16] are zero after an x4 tube or hybrid launch whose detailed tiles took the gather kernel).
 * For tests and the bench report; the reference has no counterpart. */
int mulut_last_detail_counters(mulut_ctx *ctx, uint32_t *out, int cap, void *stream);
/* Probe buffer of the context: MULUT_DEBUG_WORDS 64-bit words of device memory that only probe builds of the kernels
 * (-DMULUT_VARIANT_...prof: in-kernel clock stamps per phase) write to -- never an output buffer, and no output value is computed
 * from it.  Copies min(cap, MULUT_DEBUG_WORDS) words to `out` (synchronises with `stream`), then zeroes the buffer when
 * `reset` != 0.  Returns the number of words copied.  The shipped library leaves the buffer at zero. */
#define MULUT_DEBUG_WORDS 4096
int mulut_debug_read(mulut_ctx *ctx, unsigned long long *out, int cap, int reset, void *stream);

/* ---- LUT-aware fine-tuning (the differentiable twin; stateless, float32) -----------------------------
 * One stage of MuLUT.forward (sr/model.py:289-312) = InterpTorchBatch (:69-287) over all modes x 4 rotations
 * with the per-pass BPDA rounding (:308) and the stage's clamp/round (:309).  Modes s, d, y only: e, h, o return MULUT_EMODE
 * from the six functions below, as the reference's module raises for them (sr/model.py:121) -- their backward kernels stage a
 * 2-pixel halo of the input gradient.  A list with e, h or o goes to mulut_ft_wide_stage_forward / _backward further down.
 *   weights_q : M device pointers, the QUANTISED tables clamp(round(w*127),-127,127) as float32 [83521][u*u]
 *               (sr/model.py:74-76 -- done by the caller, which also applies that step's backward)
 *   x         : device float32 [B][C][H][W] in 0..255 (the module multiplies its input by 255, :290)
 *   out       : device float32 [B][C][H*u][W*u] in 0..255
 * backward: grad_out = dL/d out; accumulates dL/d weights_q into grad_wq[m] (atomic adds; zero them first) and
 * dL/dx into grad_x (zero it first).  u = upscale for the last stage, else 1.
 * Contracts of every call of this section (the quantiser pair, the four families of stage calls; tests/test_gpu_ft_abi.py):
 *   - stateless and stream-ordered: a call is one kernel launch on `stream`; it allocates nothing, waits for nothing and keeps no
 *     state that affects a result (what it keeps is set-up done once: see the capture note), so it reads what work queued earlier on
 *     that stream wrote and may be queued behind its producer.
 *   - "accumulates" means ADDS: after the call every element of grad_wq[m] and grad_x holds what it held before plus this call's
 *     gradient -- elements the batch does not touch are not written at all -- so gradients of several micro-batches may be summed
 *     by calling again without zeroing ("zero them first" is for the caller who wants one call's gradient).  The adds are float32
 *     atomics in no fixed order: bit-reproducible only where the sums are exact (mulut_ft_exact_stage_backward, further down, is
 *     the backward whose bits do not depend on that order).
 *   - alignment: float alignment (4 bytes) suffices for x, out, grad_out, grad_x and every table and gradient pointer, 2 bytes for
 *     `inside`; tables of one stage may lie back to back (rows * u*u floats apart).  Nothing outside x, weights_q[m], grad_out and
 *     `inside` is read, nothing outside out, `inside` (forward), grad_wq[m] and grad_x is written.
 *   - x outside 0..255 (below 0, above 255, infinite, NaN of either sign, denormal): defined, and inside the tables, forward and
 *     backward.  The MSB of every key is clamped into 0 .. L-2.  At interval 4 the keys are ranked on |LSB|, which makes the five rows
 *     of a pass the anchor row plus each key's stride once for any four floats: rows stay in [0, 83521), tube slots in [0, 1041).  At
 *     intervals 5 and 6 every row is clamped into [0, L^4) as well.  The LSB stays x - q*floor(x/q), so such a pixel gives the sites
 *     that read it a meaningless (for an infinity or NaN: NaN) output and gradient -- a NaN weight is added to the in-table rows of
 *     that pass -- and no other site anything else than it would get otherwise.  The reference raises an index error there.
 *   - hipGraph capture: run the call once outside capture first.  The first launch of a kernel that takes dynamic LDS raises that
 *     kernel's limit (hipFuncSetAttribute): the u = 4 backward at interval 4 (the other interval-4 kernels use static LDS), every
 *     backward and the LDS-resident forward at intervals 5 and 6; and the first interval-5 / 6 call asks for the device's CU count.
 *     Neither is capturable; both are remembered per device.  After that warm-up a call is a kernel launch and nothing else: it can
 *     be captured, and a replay reads x, grad_out, the tables and `inside` as they are in memory then (rewrite them in place). */
/* The module's quantisation of its float parameters and that step's backward (sr/model.py:74-76), for the M tables of a stage
 * (n floats each) in one launch:
 *   mulut_ft_quantize          : weights_q[m][i] = clamp(round(weights[m][i] * 127), -127, 127), round = half to even (torch.round)
 *   mulut_ft_quantize_backward : grad[m][i] = grad[m][i] * inside * 127 in place, inside = round(weights[m][i] * 127) within [-127, 127]
 *                                (the rounding is a BPDA identity, :59-67; the clamp passes gradient on its closed interval) */
int mulut_ft_quantize(int device, const float *const *weights, float *const *weights_q, int M, long long n, void *stream);
int mulut_ft_quantize_backward(int device, const float *const *weights, float *const *grad, int M, long long n, void *stream);
/* One step of the fine-tune optimiser (sr/3_finetune_lut.py:86: Adam with L2 weight decay added to the gradient, no amsgrad) over T
 * tensors of n[t] floats each in one launch (chunks of 32 tensors), in place on the current stream:
 *   g = grads + weight_decay * params;  exp_avg += (g - exp_avg) (1 - beta1);  exp_avg_sq = beta2 exp_avg_sq + (1 - beta2) g g;
 *   params -= lr / (1 - beta1^step) * exp_avg / (sqrt(exp_avg_sq) / sqrt(1 - beta2^step) + eps)
 * `step` is the number of this step, 1 for the first.  Everything in memory is float32; between the loads and the stores the arithmetic
 * is float64, so each stored value is the float64 result rounded once.  A NULL pointer, T < 1, n[t] < 1, step < 1 or a beta outside
 * [0, 1) returns MULUT_EINVAL before the device is touched.  Nothing outside the n[t] floats of each tensor is read or written. */
int mulut_ft_adam(int device, float *const *params, const float *const *grads, float *const *exp_avg, float *const *exp_avg_sq,
                  const long long *n, int T, long long step, double lr, double beta1, double beta2, double eps, double weight_decay,
                  void *stream);
int mulut_ft_stage_forward(int device, const float *const *weights_q, const char *modes, int is_last, int u, const float *x,
                           int B, int C, int H, int W, float *out, void *stream);
int mulut_ft_stage_backward(int device, const float *const *weights_q, const char *modes, int is_last, int u, const float *x,
                            const float *grad_out, int B, int C, int H, int W, float *const *grad_wq, float *grad_x,
                            void *stream);
/* The same pair with the clamp's mask handed from the forward to the backward: inside[(b*C + c)*H*W + y*W + x] bit sy*u+sx is set where
 * 0 <= pred/avg + bias <= 255 at that block position (:309, the closed interval on which the clamp passes gradient).  The plain backward
 * recomputes the stage forward to get it; with the mask it does not (one sixth of the final-stage backward at bs 256 x 48 x 48). */
int mulut_ft_stage_forward_mask(int device, const float *const *weights_q, const char *modes, int is_last, int u, const float *x,
                                int B, int C, int H, int W, float *out, unsigned short *inside, void *stream);
int mulut_ft_stage_backward_mask(int device, const float *const *weights_q, const char *modes, int is_last, int u, const float *x,
                                 const float *grad_out, const unsigned short *inside, int B, int C, int H, int W,
                                 float *const *grad_wq, float *grad_x, void *stream);
/* The masked pair at the sampling intervals 5 and 6: the module built with interval = 5 / 6 (sr/model.py:42-44, q = 2^interval and
 * L = 2^(8-interval) + 1 in InterpTorchBatch, :78-80; driver sr/3_finetune_lut.py:82,166).  weights_q are float32 [L^4][u*u]
 * (6,561 / 625 rows); everything else is as above.  interval other than 5 or 6 returns MULUT_EUNSUPPORTED (interval 4 is the
 * functions above), as do u outside 1..4 and more than MULUT_MAX_MODES modes; a mode outside s, d, y MULUT_EMODE; a NULL pointer
 * (the mask included) or a non-positive size MULUT_EINVAL -- all decided before the device is touched.  mulut_ft_quantize and
 * mulut_ft_quantize_backward serve these tables unchanged. */
int mulut_ft_interval_stage_forward(int device, int interval, const float *const *weights_q, const char *modes, int is_last, int u,
                                    const float *x, int B, int C, int H, int W, float *out, unsigned short *inside, void *stream);
int mulut_ft_interval_stage_backward(int device, int interval, const float *const *weights_q, const char *modes, int is_last, int u,
                                     const float *x, const float *grad_out, const unsigned short *inside, int B, int C, int H, int W,
                                     float *const *grad_wq, float *grad_x, void *stream);
/* The masked pair for ANY list over the six sampling patterns s, d, y, e, h, o, at interval 4, 5 or 6: MuLUT.forward's stage
 * (sr/model.py:69-312) with the 4 x 4 patterns the reference's module leaves out ("more sampling modes can be implemented
 * similarly", sr/model.py:119-121; their taps are the network's, common/network.py:173-215, edge pad 3).  weights_q are float32
 * [L^4][u*u], already quantised, as above.  A list with e, h or o runs the backward kernels built with a 3-pixel halo of the input
 * gradient; a list without is forwarded to what mulut_ft_stage_*_mask (interval 4) / mulut_ft_interval_stage_* (5, 6) launch, so
 * the results are theirs bit for bit.  `inside` is required in both calls (there is no recomputing form).  interval outside 4..6,
 * u outside 1..4 and more than MULUT_MAX_MODES modes return MULUT_EUNSUPPORTED; any other letter MULUT_EMODE; a NULL pointer or a
 * non-positive size MULUT_EINVAL -- decided before the device is touched, in the order of the functions above. */
int mulut_ft_wide_stage_forward(int device, int interval, const float *const *weights_q, const char *modes, int is_last, int u,
                                const float *x, int B, int C, int H, int W, float *out, unsigned short *inside, void *stream);
int mulut_ft_wide_stage_backward(int device, int interval, const float *const *weights_q, const char *modes, int is_last, int u,
                                 const float *x, const float *grad_out, const unsigned short *inside, int B, int C, int H, int W,
                                 float *const *grad_wq, float *grad_x, void *stream);
/* The BIT-REPRODUCIBLE backward of the same stage (sr/model.py:69-312, autograd's backward of it): arguments and meaning are those
 * of mulut_ft_wide_stage_backward -- any list over s, d, y, e, h, o, interval 4, 5 or 6, u = 1..4, `inside` required, the forward
 * is mulut_ft_wide_stage_forward, unchanged -- plus a workspace.  Every contribution to a gradient element is the float32 value the
 * kernels above compute (the expressions are written once, mulut_amd/csrc/mulut_ft_exact.h), converted to a 64-bit fixed-point
 * integer, round half to even, at a scale derived from max |grad_out| and the shape of the call alone; the integers are summed --
 * integer addition is associative -- and each sum is converted to float32 once and ADDED to its destination with one float add
 * ("accumulates" as above; an element whose integer sum is 0 is not written).
 *   - the result is a pure function of the argument VALUES: the same bits for any order in which the hardware runs the work, for
 *     any launch geometry, and -- grad_wq -- for any order of the samples in the batch (grad_x: the same permutation of its
 *     planes).  tests/host_emul/ft_exact_host.cpp restates it on the CPU with plain int64 adds; the GPU tests ask equality.
 *   - resolution: with gmax = max |grad_out|, one unit of a table sum is at most gmax * 2^(ceil(log2(4 B C H W)) - 60) (gmax * 2^-38
 *     at 256 x 48 x 48 sites), one unit of an input sum at most gmax * 2^(4 + ceil(log2 u*u) + ceil(log2 N) - 60), N = 16 M
 *     min((R + 1)^2, H W), R = max(2, reach of the list); a contribution below half a unit counts as 0.  No sum can leave +-2^62
 *     for tables within +-127 (the quantised tables) and a finite grad_out.  A non-finite grad_out gives unspecified results
 *     but no fault: no address depends on grad_out.
 *   - ws: device memory, 8-byte aligned, of at least mulut_ft_exact_ws_bytes(...) bytes, which the call owns until it completes:
 *     its content on entry is irrelevant, calls that share one ws must be ordered (one stream, or events).  Nothing outside x,
 *     weights_q[m], grad_out, `inside` and ws is read, nothing outside grad_wq[m], grad_x and ws is written.
 *   - a call is four kernel launches on `stream` (clear, maximum, accumulate, finish) and nothing else: it allocates nothing and waits
 *     for nothing, and is capturable after one warm-up call, as above.
 * Refusals, all before the device is touched, in the order of mulut_ft_wide_stage_backward (NULL grad_wq; then NULL weights_q,
 * modes, x, inside or a non-positive size MULUT_EINVAL; interval outside 4..6, more than MULUT_MAX_MODES modes, u outside 1..4
 * MULUT_EUNSUPPORTED; a letter outside the six MULUT_EMODE; a NULL table or gradient pointer MULUT_EINVAL); then NULL grad_out or
 * grad_x MULUT_EINVAL; more than 2^31 - 1 sites (B C H W) MULUT_EUNSUPPORTED; a NULL or misaligned ws MULUT_EINVAL; ws_bytes below
 * the query's value MULUT_EWORKSPACE.  mulut_ft_exact_ws_bytes returns the negative MULUT_E* code for arguments the call would refuse. */
long long mulut_ft_exact_ws_bytes(int interval, const char *modes, int u, int B, int C, int H, int W);
int mulut_ft_exact_stage_backward(int device, int interval, const float *const *weights_q, const char *modes, int is_last, int u,
                                  const float *x, const float *grad_out, const unsigned short *inside, int B, int C, int H, int W,
                                  float *const *grad_wq, float *grad_x, void *ws, long long ws_bytes, void *stream);
/* A fine-tune batch cut on the device from a device-resident training set: DIV2K.__getitem__ (sr/data.py:91-121, restated by
 * CropProvider.next() of mulut_amd/finetune_lut.py) for B samples in one launch.  The reference draws and cuts in DataLoader
 * workers (sr/data.py:27-49); here the host draws six integers per sample and the device does the rest.
 *   pool   : device bytes holding every image as the PNG decodes, HWC uint8 with `ch` channels (grey: ch = 1)
 *   pairs  : device table, one entry per (LR, HR) pair: byte offsets of the two images in `pool` and their sizes
 *            (hr_w need not be lr_w * scale: the HR window is read at the HR image's own width)
 *   draws  : device int32 [B][6] = pair, i, j, c, flips (bit 0 np.fliplr, bit 1 np.flipud), k (np.rot90's k, taken mod 4)
 *   im, lb : device float32 [B][1][sz][sz] and [B][1][sz*scale][sz*scale]; 16-byte aligned bases with sz (sz*scale) a
 *            multiple of 4 take 16-byte stores, anything else float stores -- the same result
 * Sample b: LR rows i..i+sz, columns j..j+sz, channel c and the same window times `scale` of the HR image; fliplr if bit 0, then
 * flipud if bit 1, then rot90 by k; value = float32(byte) / 255.0f, IEEE division (NumPy's result for all 256 bytes).
 * Refusals, before the device is touched: NULL pool, pairs, draws, im or lb, or a non-positive B, sz, n_pairs or pool_bytes
 * MULUT_EINVAL; then scale outside 1..4 MULUT_EUNSUPPORTED; then B * (sz*scale)^2 >= 2^31 MULUT_EUNSUPPORTED.
 * The draws are device memory, so each sample is checked by the kernel: pair in 0..n_pairs-1, 0 <= c < ch, i, j >= 0,
 * i + sz <= lr_h, j + sz <= lr_w, the scaled window inside hr_h x hr_w, and both images inside [0, pool_bytes).  A sample that fails
 * is written as zeros and adds one to *bad (device int the CALLER zeroes; NULL: not counted); no address is formed from it, so
 * nothing outside the pool is ever read.  Stateless and stream-ordered, like the calls above. */
typedef struct { long long lr_off, hr_off; int lr_h, lr_w, hr_h, hr_w, ch, pad; } mulut_ft_pair;   /* 40 bytes, offsets into pool */
int mulut_ft_crop_batch(int device, const unsigned char *pool, long long pool_bytes, const mulut_ft_pair *pairs, int n_pairs,
                        const int *draws, int B, int sz, int scale, float *im, float *lb, int *bad, void *stream);
/* The module's output as the bytes the validation loop scores and saves, in one launch: replaces
 *   pred = model_G(im) * 255.0;  np.round(np.clip(np.transpose(pred, [1, 2, 0]), 0, 255)).astype(np.uint8)      (sr/3_finetune_lut.py:50-54)
 *   pred    : device float32 planar [3][H][W], the module's output in 0..1
 *   out_hwc : device uint8 [H][W][3] at ANY byte address; nothing outside out_hwc[0, H*W*3) is written
 * byte = rintf(fminf(fmaxf(pred * 255.0f, 0.0f), 255.0f)): the float32 product, the clamp and round-half-to-even, the same byte as
 * the expression above for every finite input and both infinities.  What a NaN becomes is UNSPECIFIED (some byte; no fault).
 * Refusals as for mulut_ft_crop_batch, before the device is touched: NULL pred or out_hwc, or a non-positive H or W MULUT_EINVAL;
 * then H * W * 3 >= 2^31 MULUT_EUNSUPPORTED.  Stateless and stream-ordered, like the calls above. */
int mulut_ft_val_pack(int device, const float *pred, int H, int W, unsigned char *out_hwc, void *stream);

/* ---- device-side evaluation (not on the inference path) ---------------------------------------------------
 * Y-channel PSNR and SSIM of a super-resolved frame against its ground truth, exactly as the test script scores
 * them (sr/4_test_lut.py:313-315): y = _rgb2ycbcr(img)[:,:,0] (common/utils.py:42-60), PSNR with `shave` border
 * pixels removed and a float32 difference (:63-72), SSIM with the 11x11 sigma-1.5 Gaussian over 'valid' windows
 * in float64 (:75-101).  gt_hwc / out_hwc: device uint8 [H][W][3]; ws: device scratch of at least
 * mulut_eval_ws_doubles(H, W) doubles.  Synchronises `stream` and writes the two host doubles.
 * Errors: MULUT_ESHAPE (image smaller than the window or the shave), MULUT_EWORKSPACE. */
long long mulut_eval_ws_doubles(int H, int W);
int mulut_eval_y(int device, const void *gt_hwc, const void *out_hwc, int H, int W, int shave, double *ws, long long ws_doubles,
                 double *psnr, double *ssim, void *stream);
/* The same score for a LIST of pairs of different sizes in one stream-ordered call: the scoring of the fine-tune driver's validation
 * loop (sr/3_finetune_lut.py:23-65, PSNR and cal_ssim at :56-58) without a wait per image.  Ground truths lie in one device pool
 * of bytes, the outputs to score in another; an item names one pair by its byte offsets into the two pools (uint8 [H][W][3], no
 * alignment asked of either offset) and states the size of each pool, so the plan can vouch for every address it will form.
 * mulut_eval_plan_create (sr/3_finetune_lut.py:23-65): `items` is a HOST array of n entries.  Checked on the host, in this order, each
 *   class over the whole list before the next, and before the device is touched: a NULL `items` or `plan`, n < 1 or shave < 0
 *   MULUT_EINVAL; an item with H or W below 11 (the SSIM window) or not larger than 2 * shave MULUT_ESHAPE; an item with a negative
 *   offset or not wholly inside the pool size it states MULUT_EINVAL; 2^31 workgroups or more in one launch (the list's squared-error
 *   blocks, min(1024, ceil(interior / 256)) per item, or its 32 x 32 SSIM tiles) MULUT_EUNSUPPORTED.  Then one allocation and one
 *   blocking copy (not capturable): the item table, the map from workgroup to (item, block or tile) of each launch, and the
 *   workspace of one double per workgroup.  *plan is NULL after any failure.
 * mulut_eval_plan_run (sr/3_finetune_lut.py:56-58): three kernel launches on `stream` and nothing else -- it allocates nothing and
 *   waits for nothing, so it can be captured into a hipGraph, and a replay scores the pools as they are in memory then.  gt_pool and
 *   out_pool are device pointers to at least the bytes the items stated.  Leaves sums[i][0] = item i's summed squared Y error over
 *   the shaved interior and sums[i][1] = its summed SSIM map, n x 2 DEVICE doubles.  Each sum is made of the partial sums
 *   mulut_eval_y makes for that pair, added in the same order by one lane (no atomics): mulut_eval_finish of the two gives
 *   mulut_eval_y's two doubles bit for bit.  The workspace belongs to the plan: runs of ONE plan must be ordered one behind the
 *   other (one stream, or events); different plans are independent.  NULL plan, pool or sums MULUT_EINVAL.
 * mulut_eval_plan_destroy: frees the allocation (hipFree waits for work in flight on the device) and the plan.
 * mulut_eval_finish (common/utils.py:63-72,101; host only, needs no device): the two sums of one H x W pair to (PSNR, SSIM) -- the
 *   float32 mean of the squared error, sqrt, 20 log10(255 / rmse) (inf for sse = 0), and the SSIM sum over its (H-10)(W-10) windows.
 *   mulut_eval_y ends in this call.  NULL psnr or ssim, H, W <= 0 or shave < 0 MULUT_EINVAL; H or W below 11 or not above 2 * shave
 *   MULUT_ESHAPE. */
typedef struct { long long gt_off, out_off; int H, W; long long gt_pool_bytes, out_pool_bytes; } mulut_eval_item;   /* 40 bytes */
typedef struct mulut_eval_plan mulut_eval_plan;
int mulut_eval_plan_create(int device, const mulut_eval_item *items, int n, int shave, mulut_eval_plan **plan);
int mulut_eval_plan_run(const mulut_eval_plan *plan, const void *gt_pool, const void *out_pool, double *sums, void *stream);
int mulut_eval_plan_destroy(mulut_eval_plan *plan);
int mulut_eval_finish(double sse, double ssim_sum, int H, int W, int shave, double *psnr, double *ssim);

/* ---- LR images made on the device (not on the inference path) ------------------------------------------------
 * Pillow's bicubic resampling of 8-bit images, byte for byte: what sr/Test_dataset.py:24-25 does with
 *   img.resize((img.width // scale, img.height // scale), resample=Image.BICUBIC)
 * to make LR/X{scale}/ from HR/, and the same filter run the other way (bicubic upscaling, the baseline column of an SR table).
 * Pillow works in fixed point: per output position normalised double coefficients rounded to integers at 22 fractional bits,
 * an integer accumulator that starts at 1 << 21, clip(acc >> 22) to 0..255; a horizontal pass into uint8, then a vertical pass
 * over those bytes; an axis whose size does not change is skipped.  int32 accumulators are exact here.
 *
 * mulut_resample_coeffs (sr/Test_dataset.py:24-25; host only, needs no device): the tables of ONE axis, in -> out samples.
 *   kk [out][taps] int32 (zero beyond a row's n), xmin [out], n [out]: output xx = sum over t < n[xx] of kk[xx][t] * in[xmin[xx] + t];
 *   every tap lies in [0, in).  Returns taps = 2 * ceil(2 * max(in / out, 1)) + 1, or a negative code: a NULL pointer or in, out < 1
 *   MULUT_EINVAL; a ratio whose taps do not fit (support above 2^20) MULUT_EUNSUPPORTED; cap < out * taps int32s at kk MULUT_EWORKSPACE.
 * mulut_resample_plan_create (sr/Test_dataset.py:24-25): builds both axes' tables for in_h x in_w -> out_h x out_w and uploads them
 *   to `device` (one allocation, one blocking copy: not capturable).  A NULL `plan` or a size below 1 MULUT_EINVAL; a plane of 2^31
 *   bytes or more, tables of 2^28 entries or more, or a tile whose coefficient rows and input rows do not fit 64 KiB of LDS
 *   (1 KiB per horizontal tap + 256 bytes per input row under a tile of 16 output rows, 64 where the image grows downwards:
 *   shrinking an axis by more than about 12)
 *   MULUT_EUNSUPPORTED -- all before the device is touched.  *plan is NULL after any failure.
 * mulut_resample_plan_destroy: frees the tables (hipFree waits for work in flight on the device) and the plan.
 * mulut_resample_run (sr/Test_dataset.py:24-25): N images of C independent channels, `in` and `out` caller-owned device uint8 in
 *   MULUT_LAYOUT_HWC or MULUT_LAYOUT_CHW, each its own; no alignment needed; nothing outside out[0, N * out_h * out_w * C) is written.
 *   One kernel launch on `stream`; allocates nothing and waits for nothing, so it can be captured into a hipGraph.  NULL plan, in or
 *   out, N < 1, C < 1 or an unknown layout MULUT_EINVAL; a packed image of 2^31 bytes or more, or 2^31 workgroups or more in the
 *   call, MULUT_EUNSUPPORTED -- before the device is touched. */
typedef struct mulut_resample_plan mulut_resample_plan;
int mulut_resample_coeffs(int in, int out, int32_t *kk, int32_t *xmin, int32_t *n, long long cap);
int mulut_resample_plan_create(int device, int in_h, int in_w, int out_h, int out_w, mulut_resample_plan **plan);
int mulut_resample_plan_destroy(mulut_resample_plan *plan);
int mulut_resample_run(const mulut_resample_plan *plan, const uint8_t *in, int in_layout, uint8_t *out, int out_layout, int N, int C,
                       void *stream);

/* The trained network itself, fused: the per-site MLP of one `SRNet` (common/network.py:62-105, MuLUTUnit with dense=True: conv1
 * 4 -> nf, conv2..conv5 densely connected, conv6 5*nf -> u*u, tanh) on the f32-input MFMA, activations in registers, weights streamed
 * through LDS.  No context: a unit owns the device copy of its packed weights and nothing else.
 *   mulut_net_unit_create   w[l] / b[l]: HOST pointers to conv(l+1)'s weight ([out][in], the reference's Conv2d weight read flat) and
 *                           bias.  nf 1..64 and u 1..4 (padded with zero weights to the MFMA tile, which is exact); anything else
 *                           MULUT_EUNSUPPORTED.  Packs on the host, allocates and uploads once; the other calls allocate nothing.
 *   mulut_net_table         sr/2_transfer_to_lut.py:12-41,86-109: rows_dev = int8 [L^4][u*u], round_half_even(clamp(net, -1, 1) * 127)
 *                           over the grid 0, q, ..., 256 - q, 255 (each / 255), row = the base-L digits a, b, c, d with a slowest, for
 *                           interval 4, 5 or 6 (else MULUT_EUNSUPPORTED).  The grid values go to taps a, b, c, d whatever the pattern.
 *   mulut_net_pass          sr/1_train_model.py:33-35: out = int8 planar [N][C][H*u][W*u] =
 *                           rot90^-r(round(127 * net(pad(rot90^r(in / 255))))) for in = uint8 planar [N][C][H][W], pattern `mode`
 *                           (s, d, y, e, h, o) and r in 0..3; the replicate padding of K - 1 on the bottom and right of the rotated
 *                           image is index arithmetic on `in`.
 *   mulut_net_stage         sr/1_train_model.py:29-43 in the 'valid' phase: strlen(modes) units x 4 rotations summed as integers per
 *                           output sub-pixel, then clip(rhe(pred / (4 M) + 127), 0, 255) (is_last 0) or clip(rhe(pred / M), 0, 255)
 *                           (is_last 1, with :101), rhe = round half even, done in integers (equal to the reference's float32).
 *                           uint8 planar in and out.  The units must share u, the padded width (nf <= 32 or not) and the device:
 *                           MULUT_ESHAPE otherwise.
 * All three are stream-ordered, wait for nothing and allocate nothing.  Refused before any launch: a NULL pointer, r outside 0..3, an
 * unknown pattern letter, an empty mode list, N, C, H or W < 1 (MULUT_EINVAL); more than MULUT_MAX_MODES modes, or
 * N * C * H * W * u * u >= 2^31 (MULUT_EUNSUPPORTED). */
typedef struct mulut_net_unit mulut_net_unit;
int mulut_net_unit_create(int device, int nf, int u, const float *const w[6], const float *const b[6], mulut_net_unit **unit);
int mulut_net_unit_destroy(mulut_net_unit *unit);
int mulut_net_table(const mulut_net_unit *unit, int interval, int8_t *rows_dev, void *stream);
int mulut_net_pass(const mulut_net_unit *unit, char mode, int r, const uint8_t *in, int N, int C, int H, int W, int8_t *out, void *stream);
int mulut_net_stage(const mulut_net_unit *const units[], const char *modes, int is_last, const uint8_t *in, uint8_t *out, int N, int C,
                    int H, int W, void *stream);
/* The cascade for a LIST of images of different sizes, HWC bytes to HWC bytes, in `stages` stream-ordered launches
 * (mulut_net_list.hip): what the validation loop of sr/1_train_model.py:87-101 does per image -- the image to planar (:87-91),
 * mulut_predict in the 'valid' phase (:93), back to HWC, round and clip (:95-101) -- without a launch, an allocation or a layout pass
 * per image.  The inputs lie in one device pool of bytes, the results go to another; an item names one image: its input uint8
 * [h][w][ch] at byte in_off of in_pool, its result uint8 [h * scale][w * scale][ch] at byte out_off of out_pool (no alignment asked
 * of either offset), and it states the size of each pool, so the plan can vouch for every address the kernels will form.  Item i's
 * result is, byte for byte, what mulut_net_stage called stage after stage on that image alone (planar [1][ch][h][w]) gives, permuted
 * to HWC.
 * mulut_net_plan_create (sr/1_train_model.py:87-101): `items` is a HOST array of n entries; the model has `stages` stages, every one
 *   before the last of upscale 1 and the last of upscale `scale`.  Checked on the host, in this order, each class over the whole list
 *   before the next, and before the device is touched: a NULL `plan` (then nothing is written), a NULL `items`, n, ch, stages or
 *   scale < 1 MULUT_EINVAL; an item with h or w < 1 MULUT_EINVAL; an item with a negative offset, or whose input or result is not
 *   wholly inside the pool size it states MULUT_EINVAL; two items whose result ranges overlap MULUT_EINVAL (inputs may be shared); an
 *   item of 2^31 result bytes or more, 2^31 workgroups or more in one launch (ceil(ch * h * w / 128) per item), or a workspace of
 *   2^31 bytes or more MULUT_EUNSUPPORTED.  Then one allocation and one blocking copy (not capturable): the item table (32 bytes an
 *   item), the map from a workgroup to (item, first site of that item) (8 bytes a workgroup), and the plan's own planar
 *   intermediate planes, which the stages before the last write and the stages after the first read: sum of ch * h * w bytes a
 *   set, no set for one stage, one for two, two for more.  *plan is NULL after any failure.
 * mulut_net_plan_run (sr/1_train_model.py:93-101): exactly `stages` kernel launches on `stream` and nothing else -- it allocates
 *   nothing, copies nothing and waits for nothing, so it can be captured into a hipGraph, and a replay reads the input pool and the
 *   units' weights as they are in memory then.  `units` holds stages x strlen(modes) handles, stage-major (stage s, mode m at
 *   [s * M + m]); in_pool and out_pool are device pointers to at least the bytes the items stated.  Nothing of out_pool outside
 *   the items' result ranges is written.  Refused before any launch, stage by stage: a NULL plan, units, modes or pool MULUT_EINVAL;
 *   per stage the refusals of mulut_net_stage's unit list (an empty mode list, a NULL handle, an unknown pattern letter
 *   MULUT_EINVAL; more than MULUT_MAX_MODES modes MULUT_EUNSUPPORTED; units that differ in upscale, padded width or device
 *   MULUT_ESHAPE), then a stage before the last whose upscale is not 1, a last stage whose upscale is not `scale`, or units on
 *   another device than the plan's MULUT_ESHAPE.  The planes belong to the plan: runs of ONE plan must be ordered one behind the
 *   other (one stream, or events); different plans are independent.
 * mulut_net_plan_destroy: frees the allocation (hipFree waits for work in flight on the device) and the plan. */
typedef struct { long long in_off, out_off; int h, w; long long in_pool_bytes, out_pool_bytes; } mulut_net_item;   /* 40 bytes */
typedef struct mulut_net_plan mulut_net_plan;
int mulut_net_plan_create(int device, const mulut_net_item *items, int n, int ch, int stages, int scale, mulut_net_plan **plan);
int mulut_net_plan_run(const mulut_net_plan *plan, const mulut_net_unit *const units[], const char *modes, const void *in_pool,
                       void *out_pool, void *stream);
int mulut_net_plan_destroy(mulut_net_plan *plan);

/* ---- Training the network on the fused site body (mulut_net_train.hip): sr/1_train_model.py:26-45 in the 'train' phase and its
 * gradient.  Everything here is float32 on the device and stream-ordered; nothing allocates but mulut_net_unit_create_train.
 *   mulut_net_unit_create_train  a unit with BOTH streams -- the forward's and the backward's (the transposed weights in the same step
 *                           format, mulut_net.h) -- allocated and zeroed; mulut_net_unit_destroy frees it.  nf, u as above.
 *   mulut_net_unit_load_dev w_dev[l] / b_dev[l]: DEVICE pointers laid out as mulut_net_unit_create's host ones.  One small kernel on
 *                           `stream` writes the forward stream exactly as the host pack does and, for a unit of
 *                           mulut_net_unit_create_train, the backward stream in the same launch.  Works on either kind of unit.
 *   mulut_net_pack_host     the host packs themselves, no device involved: the stream mulut_net_unit_create uploads (backward 0) or
 *                           the backward stream (1) of HOST weights into `out`; returns the number of floats (MULUT_EWORKSPACE if
 *                           cap is smaller).  What the device pack is tested against.
 *   mulut_net_unit_read     copies a stream (backward 0 / 1) to `host` after a device synchronisation, for tests; returns the
 *                           number of floats, MULUT_EWORKSPACE if cap is smaller, MULUT_EINVAL for the backward stream of a unit
 *                           that has none.
 *   mulut_net_stage_sum     pred = float32 planar [N][C][H*u][W*u] = sum over modes and r of rot90^-r(round(127 * net(pad(rot90^r(x)))))
 *                           for x = float32 planar [N][C][H][W]: :30-35, before the stage's own arithmetic (:36-43).  The values
 *                           are integers; the sum is made in integers, so two calls agree bit for bit.
 *   mulut_net_backward_ws_bytes  the workspace for chunks of `sites` sites: 16 copies of a unit's gradient plus
 *                           (4 + 10 nf + u*u) floats per site, sites rounded up to 128.  `sites` = 128 gives the smallest workspace
 *                           mulut_net_stage_backward takes; the pixel count of the image lets every pass run as one chunk.
 *   mulut_net_stage_backward  g = dL/dpred (the shape of pred).  Round is the identity here (BPDA, :48-55), so this is the exact
 *                           Jacobian of the smooth sum of 127 * net at x.  gw / gb: 6 * M device pointers, [6 * m + l] = the gradient
 *                           of conv(l+1)'s weight / bias of unit m; they are WRITTEN, and bit-identical from run to run.  gx, if not
 *                           NULL, has the shape of x and is ADDED to (float atomics: zero it first; not bit-reproducible); NULL skips
 *                           the tap gradient (a first stage).  ws: 256-byte aligned, of ws_bytes bytes; the passes run in chunks of
 *                           as many sites as fit.  The units must come from mulut_net_unit_create_train and share nf.
 * Refusals before any launch: as mulut_net_stage's, plus a unit without a backward stream, a NULL gradient pointer, a misaligned ws
 * (MULUT_EINVAL), units of different nf (MULUT_ESHAPE), ws_bytes below mulut_net_backward_ws_bytes(nf, u, 128) (MULUT_EWORKSPACE). */
int mulut_net_unit_create_train(int device, int nf, int u, mulut_net_unit **unit);
int mulut_net_unit_load_dev(mulut_net_unit *unit, const float *const w_dev[6], const float *const b_dev[6], void *stream);
long long mulut_net_pack_host(int nf, int u, const float *const w[6], const float *const b[6], int backward, float *out, long long cap);
long long mulut_net_unit_read(const mulut_net_unit *unit, int backward, float *host, long long cap);
int mulut_net_stage_sum(const mulut_net_unit *const units[], const char *modes, const float *x, int N, int C, int H, int W, float *pred,
                        void *stream);
long long mulut_net_backward_ws_bytes(int nf, int u, long long sites);
int mulut_net_stage_backward(const mulut_net_unit *const units[], const char *modes, const float *x, const float *g, int N, int C, int H,
                             int W, void *ws, long long ws_bytes, float *gx, float *const gw[], float *const gb[], void *stream);

/* ---- The same backward with a bit-reproducible gx (mulut_net_train.hip).  No atomics and no fixed point: the site kernel STORES a
 * site's tap gradient W_1^T delta_1 into a tap buffer t = float [4][ts], the site the fast index (row k: tap a, b, c, d of the
 * pattern), and a second kernel, one thread per input pixel p of plane (n, c), gathers it.  The gather's definition:
 *
 *     acc = accumulate ? gx[p] : +0.0f
 *     for k in 0..3                                   (taps a, b, c, d of the pattern)
 *       for every site s = y0 * W + x0 of the same plane, ascending, with net_tap_index(H, W, r, y0, x0, taps, k) == p:
 *         acc = acc + t[k][plane * H * W + s]         (a plain float32 add)
 *     gx[p] = acc
 *
 * net_tap_index (mulut_net_dev.h) is where tap k of the site anchored at pixel (y0, x0) lies in rotation r: replicate-padded on the
 * bottom and right of the ROTATED image, so a pixel receives from 0, 1 or, on the last row / column of the rotated frame, up to
 * (di + 1)(dj + 1) <= 16 sites per tap.  A stage is its passes in the order the backward runs them (mode in the order of `modes`, then
 * r = 0..3), the first with accumulate = 0, the others with 1.  gx is therefore WRITTEN (callers do not zero it) and is a function
 * of the inputs alone: the same bits from run to run and for every workspace size.
 *   mulut_net_backward_exact_ws_bytes  mulut_net_backward_ws_bytes(nf, u, chunk_sites) plus the tap region of a whole pass,
 *                           16 bytes x total_sites rounded up to 128: the gather needs all sites of a pass, the weight-gradient
 *                           rows still run in chunks.  Layout: the 16 partial copies of a unit's gradient (rounded up to 256
 *                           bytes), the tap region float [4][ts], then the rows [4 + 10 nf + u*u][chunk].  total_sites < 1:
 *                           MULUT_EINVAL; >= 2^31: MULUT_EUNSUPPORTED; else as mulut_net_backward_ws_bytes.
 *   mulut_net_stage_backward_exact  the arguments of mulut_net_stage_backward.  gw / gb are the bits mulut_net_stage_backward
 *                           writes; gx, if not NULL, is written by the definition above, whatever number of chunks the workspace
 *                           allows.  The same refusals, and MULUT_EWORKSPACE when ws_bytes is below
 *                           mulut_net_backward_exact_ws_bytes(nf, u, 128, N*C*H*W).
 *   mulut_net_gx_gather     the gather of one pass on its own: t = device float [4][ts], rows beyond the N*C*H*W sites never read;
 *                           gx = device float [N][C][H][W].  Refusals before any launch: a NULL pointer, r outside 0..3, an
 *                           unknown pattern letter, a size < 1, ts < N*C*H*W (MULUT_EINVAL); sizes beyond the limits of
 *                           mulut_net_stage (MULUT_EUNSUPPORTED).
 * All three are stream-ordered, wait for nothing and allocate nothing. */
long long mulut_net_backward_exact_ws_bytes(int nf, int u, long long chunk_sites, long long total_sites);
int mulut_net_stage_backward_exact(const mulut_net_unit *const units[], const char *modes, const float *x, const float *g, int N, int C,
                                   int H, int W, void *ws, long long ws_bytes, float *gx, float *const gw[], float *const gb[], void *stream);
int mulut_net_gx_gather(int device, char mode, int r, const float *t, long long ts, int N, int C, int H, int W, float *gx, int accumulate,
                        void *stream);

/* Tuning knobs (never change results).
 * "final_stage_kernel" (scale 4, <= 3 modes): 0 = auto (= 6), 1 = full-table gather kernel, 5 = tube kernel on every tile (the tube
 *   bands of all modes resident in LDS; samples with a pass outside the tube are recomputed from the full table through a device
 *   work list), 6 = hybrid: a per-tile statistic sends smooth 64x16 tiles to the tube kernel and detailed ones to the
 *   detailed-tile path.  (2-4: the band / expanded-band kernels of rounds 1-2, retired: MULUT_EINVAL.)
 *   Scales 2 and 3: 0 = the tube-band kernel of the 1-byte-row family with 4- / 9-value rows (stage_u1t_kernel<2>, <3>) on the
 *   64x64 tiles its local-detail statistic calls smooth, the gather kernel on the others (device-side tile marks; threshold
 *   "final_stage_detail_per_1024", as "first_stage_detail_per_1024" below); 5 = the tube-band kernel on every tile; 1 = the gather kernel on every tile.
 * "tube_pipelined": 1 (default) = stage_tube2_kernel where the mode list uses all of s, d, y (any order, repeats, up to 8 modes:
 *   the common "sdy" and e.g. "sdysd"; every LDS read hand-scheduled, the next pass's
 *   rows in flight under the current pass's multiply-adds, one 16x4 tile per wave, no workgroup barrier), 0 = stage_tube_kernel.
 * "detail_kernel": the detailed tiles of the hybrid: 0 (default) = anchor slabs in LDS (samples grouped by anchor MSB on the
 *   device, stage_slab_kernel; taken when the stage input is planar, < 2^28 bytes, <= 3 modes), 1 = full-table gather kernel.
 * "stat_from_first_stage": 1 (default) = when the final stage reads what a content-routing first-stage launch of the same
 *   call wrote, its per-tile statistic looks only at the tiles that launch marked detailed; 0 = at every tile.
 * "hybrid_oob_per_1024": tile threshold of the hybrid (sites out of band per 1024, default 128).
 * "first_stage_kernel" (stages with 1-byte rows): 0 = auto (tube kernel; tiles its statistic calls detailed go to the
 *   window kernel, flagged sites are recomputed through a device work list), 2 = window kernel (full table in LDS) on every
 *   tile, 3 = tube kernel on every tile.  (1: the first one-read-per-neighbour kernel, retired: MULUT_EINVAL.)
 * "first_stage_detail_per_1024": tile threshold of first_stage_kernel 0 (default 24).
 * Wide mode lists (e, h, o): every key above is accepted and stored, but does not change their route -- all their stages run on
 *   the 3-px-halo instances of the two full-table kernels (mulut_kernel_name: stage_wide1_kernel = stage_u1w_kernel at halo 3,
 *   stage_wide_up_kernel<u> = stage_up_kernel at halo 3), which have no tube, hybrid, slab or work-list variants.
 * Intervals 5 and 6: the same -- every key is accepted and stored, and their stages run on stage_interval_kernel regardless.
 * Unknown key or value: MULUT_EINVAL.
 * hipGraph capture: call mulut_reserve() for the largest (N, H, W, C) first -- the context's workspace, verdict and work-list
 * buffers are then never reallocated by smaller calls; a LARGER later call reallocates them and invalidates graphs captured
 * before it.  Configuring the context at another interval frees every table, and mulut_set_lut() with a table of another size
 * reallocates that table: graphs captured before either would replay against freed table memory and must be captured again
 * (setting a table of the same shape rewrites it in place, so a captured graph then reads the new values).  The set-up calls
 * that wait for the device (see the conventions above: mulut_set_lut, an interval change, mulut_destroy, a growing call) call
 * hipDeviceSynchronize, which is not allowed while ANY stream of the process captures in the global capture mode (the default of
 * hipStreamBeginCapture and of torch.cuda.graph): issued then, from this or another host thread, they fail with MULUT_EHIP and
 * invalidate that capture.  Make them before the capture begins or after it ends.  Run the call to be
 * captured once outside capture first: the first launch of each kernel raises that kernel's
 * dynamic-LDS limit (hipFuncSetAttribute), which is not a capturable operation.  These one-time per-device set-ups are
 * serialised inside the library: contexts may be created and first used from several host threads. */
int mulut_set_tuning(mulut_ctx *ctx, const char *key, int value);

/* Name of the kernel variant used for the final / non-final stage (for profiles).  is_final 2: as 1, but where the final stage runs
 * stage_tube2_kernel only that kernel is named, with its accumulator form: "stage_tube2_kernel<rgb,one-set>" (all four rotations in
 * one accumulator set on the rotation-closed band: up to four modes) or "stage_tube2_kernel<rgb,two-set>". */
const char *mulut_kernel_name(const mulut_ctx *ctx, int is_final);

#ifdef __cplusplus
}
#endif
#endif /* MULUT_H_ */
