"""Operation sequences for ONE context of the C ABI and a Python model of that context (test infrastructure, shared by
test_abi_sequences_cpu.py and test_gpu_abi_state.py; nothing here needs a GPU).

A `mulut_ctx` keeps state between calls (include/mulut.h, DESIGN.md "What a context keeps between calls"): what is configured,
the tables per (stage, pattern) with the interval they were set for, the tuning values, the timing switch.  `Model` restates that
state machine from the header alone and, after every operation, yields what the header promises:

  * bytes from a reference -- oracle.c_oracle for s / d / y lists at every interval, the host emulators of tests/host_emul
    (mulut_core.h / mulut_interval.h compiled by g++) for lists with e, h, o.  Never anything the library computed;
  * or the error code the header names (ENOTCONFIGURED, ENOLUT, ESHAPE, EMODE, EUNSUPPORTED, EINVAL for a retired tuning value).

build_sequences(seed) makes a constructed tour plus seeded fill-in: an Euler circuit over the complete directed graph of the
seven route FAMILIES, so every ordered pair of different families occurs as consecutive configurations of one context, cut into
a few sequences (one context each).  After every configure: one compute call on whatever tables survived (an error, or bytes when
they happen to fit), the tables set (new / same shape, other rows / other v_num: whatever the slot held decides the form), one
checked pipeline call, then seeded operations: table rewrites, a table of the wrong v_num and its ESHAPE, tuning keys, strips,
single stages (also chained through a planar intermediate, which is what the first stage's tile marks are keyed on), passes,
reserve, timing, counters, refused calls that must leave the context as it was.
"""
import ctypes
import functools
import hashlib

import numpy as np

from host_emul_lib import load_emul
from oracle import c_oracle

from mulut_amd.lut_io import lut_rows
from mulut_amd.synth import natural_frames

OK, EINVAL, EMODE, ENOLUT, ESHAPE, EUNSUPPORTED, ENOTCONFIGURED = 0, -1, -2, -3, -4, -5, -8
CHW, HWC = 0, 1

FAMILIES = ("x4_few", "x4_many", "x23", "scale1", "wide", "iv5", "iv6")

# every key mulut_set_tuning accepts, with accepted values (the header: "never change results")
TUNING = {
    "final_stage_kernel": (0, 1, 5, 6), "first_stage_kernel": (0, 2, 3), "tube_pipelined": (0, 1), "detail_kernel": (0, 1),
    "stat_from_first_stage": (0, 1), "hybrid_oob_per_1024": (0, 32, 128, 700, 1024), "first_stage_detail_per_1024": (0, 24, 300, 1024),
    "final_stage_detail_per_1024": (0, 8, 200, 1024),
}
TUNING_REFUSED = (("final_stage_kernel", 3), ("first_stage_kernel", 1), ("tube_pipelined", 2), ("no_such_key", 0))

SIZES = ((37, 45), (64, 128), (97, 76), (13, 100), (130, 66), (70, 131), (5, 9), (150, 200), (66, 64), (33, 148))


def family_of(stages, modes, scale, interval):
    if interval != 4:
        return "iv%d" % interval
    if set(modes) & set("eho"):
        return "wide"
    if scale == 1:
        return "scale1"
    if scale in (2, 3):
        return "x23"
    return "x4_few" if len(modes) <= 3 else "x4_many"


def draw_config(family, rng):
    pick = lambda xs: xs[int(rng.integers(0, len(xs)))]  # noqa: E731
    if family == "x4_few":
        cfg = (pick((1, 2, 2, 3)), pick(("sdy", "sdy", "sd", "s", "yd", "dys")), 4, 4)
    elif family == "x4_many":
        cfg = (pick((1, 2)), pick(("sdysd", "sdysdysd", "sdyyds", "ssddd", "sdysdy")), 4, 4)
    elif family == "x23":
        cfg = (pick((1, 2, 4)), pick(("sdy", "sd", "y")), pick((2, 3)), 4)
    elif family == "scale1":
        cfg = (pick((1, 2, 3)), pick(("sdy", "s", "ds")), 1, 4)
    elif family == "wide":
        cfg = (pick((1, 2)), pick(("e", "eho", "sdyeho", "sdyehoeh", "oh")), pick((1, 2, 4, 4)), 4)
    else:
        modes = pick(("sdy", "sdy", "sd", "sdyeho", "h", "sdysd"))
        cfg = (pick((1, 2, 3) if set(modes) <= set("sdy") else (1, 2)), modes, pick((1, 2, 3, 4, 4)), int(family[2]))
    assert family_of(*cfg) == family
    return cfg


# ---------------------------------------------------------------------------------------------------------------- references
_EMUL = {}


def _emul(interval):
    key = "emul" if interval == 4 else "emul_interval"
    if key not in _EMUL:
        L = load_emul(key, ["mulut_core.h"] if interval == 4 else ["mulut_core.h", "mulut_interval.h"])
        (L.emul_stage if interval == 4 else L.emul_stage_interval).restype = ctypes.c_int
        _EMUL[key] = L
    return _EMUL[key]


def _emul_stage(luts, modes, last, img_hwc, u, interval):
    """One stage on the host emulator, channel by channel (channels are independent planes; emul_stage takes at most three)."""
    L = _emul(interval)
    keep = [np.ascontiguousarray(t, dtype=np.int8) for t in luts]
    arr = (ctypes.c_void_p * len(keep))(*[t.ctypes.data for t in keep])
    H, W, C = img_hwc.shape
    out = np.empty((H * u, W * u, C), np.uint8)
    for c in range(C):
        plane = np.ascontiguousarray(img_hwc[:, :, c])
        o = np.empty((H * u, W * u, 1), np.uint8)
        if interval == 4:
            rc = L.emul_stage(arr, modes.encode(), len(modes), int(last), ctypes.c_void_p(plane.ctypes.data), H, W, 1, u,
                              ctypes.c_void_p(o.ctypes.data))
        else:
            rc = L.emul_stage_interval(arr, modes.encode(), len(modes), int(last), ctypes.c_void_p(plane.ctypes.data), H, W, 1, u,
                                       interval, ctypes.c_void_p(o.ctypes.data))
        assert rc == 0, rc
        out[:, :, c] = o[:, :, 0]
    return out


def ref_stage(luts, modes, last, img_hwc, u, interval):
    if set(modes) <= set("sdy"):
        return c_oracle.stage(luts, modes, last, img_hwc, u, interval=interval)
    return _emul_stage(luts, modes, last, img_hwc, u, interval)


def ref_pipeline(tables, stages, modes, scale, img_hwc, interval):
    """tables: {(stage, mode): rows}"""
    if set(modes) <= set("sdy"):
        return c_oracle.pipeline({"s%d_%s" % k: v for k, v in tables.items()}, stages, modes, scale, img_hwc, interval=interval)
    cur = img_hwc
    for s in range(1, stages + 1):
        cur = _emul_stage([tables[(s, m)] for m in modes], modes, s == stages, cur, scale if s == stages else 1, interval)
    return cur


# ------------------------------------------------------------------------------------------------------------------ content
def natural_noise(N, H, W, C, seed):
    """Left half photograph-like, right half uniform noise (the natural_noise helpers of the GPU tests): smooth tiles for the tube
    kernels and detailed ones for the window / slab / gather kernels in every image."""
    img = natural_frames(N, H, W, C, seed=seed)
    img[:, :, W // 2:] = np.random.default_rng(seed).integers(0, 256, (N, H, W - W // 2, C), dtype=np.uint8)
    return img


def make_table(rng, interval, vnum, smooth):
    """int8 rows [L^4, vnum], -128 included.  `smooth`: value ~ q * (first key) - 128, so a stage maps a smooth image to a smooth
    image (the next stage then has smooth tiles too); else uniform."""
    rows = lut_rows(interval)
    if not smooth:
        return rng.integers(-128, 128, (rows, vnum), dtype=np.int8)
    L, q = 2 ** (8 - interval) + 1, 2 ** interval
    a = (np.arange(rows) // L ** 3)[:, None]
    return np.clip(q * a - 128 + rng.integers(-3, 4, (rows, vnum)), -128, 127).astype(np.int8)


# -------------------------------------------------------------------------------------------------------------------- model
class Op(object):
    """One call: `name`, keyword `args` (numpy images, never device memory) and the outcome the header promises:
    kind "ok" (no value), "bytes" (value: the reference's array), "error" (value: the MULUT_E* code) or "count" (value: how many
    stage times a timing query returns)."""

    def __init__(self, name, kind, value=None, **args):
        self.name, self.kind, self.value, self.args = name, kind, value, args

    def brief(self):
        def show(v):
            return "array%s" % (v.shape,) if isinstance(v, np.ndarray) else repr(v)
        want = {"bytes": "bytes", "ok": "ok", "count": "count %r" % (self.value,)}.get(self.kind, "error %r" % (self.value,))
        return "%s(%s) -> %s" % (self.name, ", ".join("%s=%s" % (k, show(v)) for k, v in sorted(self.args.items())), want)


class Model(object):
    """The state of a context as include/mulut.h describes it."""

    def __init__(self):
        self.cfg = None            # (stages, modes, scale, interval) of the last accepted mulut_configure
        self.tab_interval = 4      # tables set before any configure are interval-4 tables
        self.tables = {}           # (stage, mode) -> int8 rows [L^4, vnum]; they survive mulut_configure at the same interval
        self.tuning = {}
        self.timing = False
        self.timed = 0             # stages of the last pipeline call since timing was switched on
        self.forms = []            # (slot, form) of every accepted set_lut

    # -- set-up calls
    def configure(self, stages, modes, scale, interval):
        if not (1 <= stages <= 8 and 1 <= len(modes) <= 8) or interval not in (4, 5, 6) or not 1 <= scale <= 4:
            return EUNSUPPORTED
        if not set(modes) <= set("sdyeho"):
            return EMODE
        if interval != self.tab_interval:
            self.tables.clear()
            self.tab_interval = interval
        self.cfg = (stages, modes, scale, interval)
        return OK

    def set_lut(self, stage, mode, table):
        if mode not in "sdyeho":
            return EMODE
        if table.shape[0] != lut_rows(self.tab_interval) or table.shape[1] not in (1, 4, 9, 16):
            return ESHAPE
        old = self.tables.get((stage, mode))
        self.forms.append(((stage, mode), "new" if old is None else "rewrite" if old.shape == table.shape else "vnum"))
        self.tables[(stage, mode)] = table
        return OK

    def set_tuning(self, key, value):
        if key not in TUNING or (key, value) in TUNING_REFUSED:
            return EINVAL
        self.tuning[key] = value
        return OK

    # -- what a compute call on stages [first, last] meets first (mulut.h: ENOLUT for a missing table, ESHAPE for one whose
    #    v_num is not the stage's), in stage order, then mode order
    def _tables_error(self, first, last):
        stages, modes, scale, _ = self.cfg
        for s in range(first, last + 1):
            vnum = scale * scale if s == stages else 1
            for m in modes:
                t = self.tables.get((s, m))
                if t is None:
                    return ENOLUT
                if t.shape[1] != vnum:
                    return ESHAPE
        return OK

    def u(self, stage):
        return self.cfg[2] if stage == self.cfg[0] else 1

    def pipeline(self, img_nhwc):
        """(kind, value) of mulut_pipeline on N images; value in NHWC"""
        if self.cfg is None:
            return "error", ENOTCONFIGURED
        stages, modes, scale, interval = self.cfg
        rc = self._tables_error(1, stages)
        if self.timing:
            self.timed = 0 if rc else stages
        if rc:
            return "error", rc
        return "bytes", np.stack([ref_pipeline(self.tables, stages, modes, scale, im, interval) for im in img_nhwc])

    def stage(self, stage, img_nhwc):
        if self.cfg is None:
            return "error", ENOTCONFIGURED
        stages, modes, scale, interval = self.cfg
        rc = self._tables_error(stage, stage)
        if rc:
            return "error", rc
        luts = [self.tables[(stage, m)] for m in modes]
        return "bytes", np.stack([ref_stage(luts, modes, stage == stages, im, self.u(stage), interval) for im in img_nhwc])

    def pass_q(self, stage, mode, r, img_chw):
        if self.cfg is None:
            return "error", ENOTCONFIGURED
        if mode not in "sdyeho":
            return "error", EMODE
        t = self.tables.get((stage, mode))
        if t is None:
            return "error", ENOLUT
        u = self.u(stage)
        if t.shape[1] != u * u:
            return "error", ESHAPE
        return "bytes", c_oracle.pass_q(t, img_chw, r, u, mode, interval=self.cfg[3])

    @property
    def halo(self):
        stages, modes = self.cfg[:2]
        return stages * (3 if set(modes) & set("eho") else 2)


# ---------------------------------------------------------------------------------------------------------------- sequences
def euler_tour(n, rng):
    """An Euler circuit of the complete directed graph on n vertices (Hierholzer, seeded edge order): n * (n - 1) + 1 vertices,
    every ordered pair of different vertices consecutive exactly once."""
    out = {v: [int(w) for w in rng.permutation(n) if w != v] for v in range(n)}
    stack, tour = [0], []
    while stack:
        v = stack[-1]
        if out[v]:
            stack.append(out[v].pop())
        else:
            tour.append(stack.pop())
    tour.reverse()
    assert len(tour) == n * (n - 1) + 1
    return tour


class _Builder(object):
    def __init__(self, rng, coverage):
        self.rng, self.m, self.ops, self.coverage = rng, Model(), [], coverage
        self.prev_stage = None     # (stage, expected NCHW bytes) of the last planar stage output the runner still holds

    def pick(self, xs):
        return xs[int(self.rng.integers(0, len(xs)))]

    def image(self, small=False):
        H, W = self.pick(SIZES[:3] + SIZES[6:7]) if small else self.pick(SIZES)
        N, C = int(self.rng.integers(1, 3)), int(self.rng.integers(1, 6))
        if H * W >= 20000:
            N = 1
        if self.m.cfg and set(self.m.cfg[1]) & set("eho"):      # (the emulators are the slow references: a few thousand sites a second)
            H, W, N = min(H, 40), min(W, 68), 1
        return natural_noise(N, H, W, C, int(self.rng.integers(0, 1 << 30)))

    def add(self, name, kind, value=None, **args):
        self.ops.append(Op(name, kind, value, **args))
        if name == "configure":
            self.prev_stage = None

    def call(self, name, rc, **args):
        self.add(name, "ok" if rc == OK else "error", None if rc == OK else rc, **args)

    # -- operations
    def configure(self, cfg):
        self.call("configure", self.m.configure(*cfg), stages=cfg[0], modes=cfg[1], scale=cfg[2], interval=cfg[3])

    def set_lut(self, stage, mode, vnum, smooth=None):
        smooth = bool(self.rng.integers(0, 2)) if smooth is None else smooth
        table = make_table(self.rng, self.m.tab_interval, vnum, smooth)
        self.call("set_lut", self.m.set_lut(stage, mode, table), stage=stage, mode=mode, table=table)

    def pipeline(self, img=None):
        img = self.image() if img is None else img
        layout = self.pick((HWC, CHW))
        kind, value = self.m.pipeline(img)
        self.add("pipeline", kind, value, img=img, layout=layout)

    def pipeline_rows(self):
        img = self.image()
        H = img.shape[1]
        y0 = int(self.rng.integers(0, H))
        y1 = int(self.rng.integers(y0 + 1, H + 1))
        halo = self.m.halo
        r0, r1 = max(0, y0 - halo), min(H, y1 + halo)
        if self.rng.integers(0, 2) and r0 > 0:      # more rows than the halo needs are allowed
            r0 -= 1
        kind, value = self.m.pipeline(img)
        if kind == "bytes":
            s = self.m.cfg[2]
            value = np.ascontiguousarray(value[:, y0 * s:y1 * s])
        self.add("pipeline_rows", kind, value, band=np.ascontiguousarray(img[:, r0:r1]), band_row0=r0, y0=y0, y1=y1, H_full=H,
                 layout=self.pick((HWC, CHW)))

    def stage(self, stage=None, planar_out=False, from_prev=False):
        """from_prev: the stage after the one whose planar output the runner still holds, read from that very buffer (the first
        stage's tile marks are keyed on its address and shape)"""
        stages = self.m.cfg[0]
        if from_prev and (self.prev_stage is None or self.prev_stage[0] >= stages):
            from_prev = False
        if from_prev:
            stage, img = self.prev_stage[0] + 1, np.ascontiguousarray(self.prev_stage[1].transpose(0, 2, 3, 1))
        else:
            stage = int(self.rng.integers(1, stages + 1)) if stage is None else stage
            img = self.image()
        kind, value = self.m.stage(stage, img)
        out_layout = CHW if planar_out else self.pick((HWC, CHW))
        self.add("stage", kind, value, stage=stage, img=None if from_prev else img, layout=CHW if from_prev else self.pick((HWC, CHW)),
                 out_layout=out_layout, from_prev=from_prev)
        self.prev_stage = (stage, value.transpose(0, 3, 1, 2)) if kind == "bytes" and out_layout == CHW else None

    def pass_q(self, mode=None):
        stages, modes = self.m.cfg[:2] if self.m.cfg else (1, "s")
        own = [m for m in modes if m in "sdy"]
        mode = mode or (self.pick(own) if own else "s")
        img = self.image(small=True)[0].transpose(2, 0, 1)[:3]
        stage, r = int(self.rng.integers(1, stages + 1)), int(self.rng.integers(0, 4))
        kind, value = self.m.pass_q(stage, mode, r, np.ascontiguousarray(img))
        self.add("pass_q", kind, value, stage=stage, mode=mode, r=r, img=np.ascontiguousarray(img))

    def tuning(self):
        key = self.pick(sorted(TUNING))
        value = self.pick(TUNING[key])
        self.call("set_tuning", self.m.set_tuning(key, value), key=key, val=value)

    def timing(self):
        on = not self.m.timing
        self.m.timing, self.m.timed = on, 0
        self.add("set_stage_timing", "ok", enable=on)
        if on:
            self.pipeline(self.image(small=True))
        self.add("last_stage_ms", "count", self.m.timed)
        self.add("last_kernel_ms", "count", self.m.timed)

    def refused(self):
        """calls the header refuses: the context must be as it was (the checked call after them says so)"""
        stages, modes, scale, interval = self.m.cfg
        what = int(self.rng.integers(0, 6))
        if what == 0:       # a mode list with an unknown letter AFTER valid ones of another order
            bad = (modes[::-1] + "x")[:8] if len(modes) < 8 else modes[:0:-1] + "x"
            self.configure((stages, bad, scale, interval))
        elif what == 1:
            self.configure(self.pick(((stages, modes, scale, 7), (stages, modes, 5, interval), (9, modes, scale, interval),
                                      (stages, "sdysdysdy", scale, interval))))
        elif what == 2:
            self.pass_q(mode="x")
        elif what == 3:     # rows of another interval
            other = self.pick([iv for iv in (4, 5, 6) if iv != self.m.tab_interval])
            table = make_table(self.rng, other, 1, False)
            self.call("set_lut", self.m.set_lut(1, modes[0], table), stage=1, mode=modes[0], table=table)
        elif what == 4:
            key, value = self.pick(TUNING_REFUSED)
            self.call("set_tuning", self.m.set_tuning(key, value), key=key, val=value)
        else:
            table = make_table(self.rng, self.m.tab_interval, 1, False)
            self.call("set_lut", self.m.set_lut(1, "x", table), stage=1, mode="x", table=table)

    def wrong_vnum(self, slot=None):
        """a table of another v_num at a slot the configuration needs: accepted by mulut_set_lut, ESHAPE from the compute calls,
        then the right shape again"""
        stages, modes, scale, _ = self.m.cfg
        stage, mode = slot or (int(self.rng.integers(1, stages + 1)), self.pick(modes))
        need = self.m.u(stage) ** 2
        self.set_lut(stage, mode, self.pick([v for v in (1, 4, 9, 16) if v != need]))
        self.pipeline(self.image(small=True))
        self.set_lut(stage, mode, need)

    def rewrite(self, slot=None):
        stages, modes = self.m.cfg[:2]
        stage, mode = slot or (int(self.rng.integers(1, stages + 1)), self.pick(modes))
        self.set_lut(stage, mode, self.m.u(stage) ** 2)

    # -- one configuration of the tour
    def segment(self, cfg, fill):
        m = self.m
        self.configure(cfg)
        stages, modes, scale, _ = cfg
        self.pipeline(self.image(small=True))       # on whatever the context holds: ENOLUT / ESHAPE, or bytes where the tables fit
        smooth = bool(self.rng.integers(0, 2))
        for s in range(1, stages + 1):
            for mode in dict.fromkeys(modes):
                t = m.tables.get((s, mode))
                if t is None or t.shape[1] != m.u(s) ** 2 or self.rng.integers(0, 3) == 0:
                    self.set_lut(s, mode, m.u(s) ** 2, smooth)
        self.pipeline()
        # the forms of set_lut this slot has not seen yet (at most two slots per configuration)
        slots = [(s, mode) for s in range(1, stages + 1) for mode in dict.fromkeys(modes)]
        todo = [(slot, form) for slot in slots for form in ("rewrite", "vnum") if (slot, form) not in self.coverage() | set(self.m.forms)]
        for slot, form in [t for t in todo if t[0][0] >= 3] + [t for t in todo if t[0][0] < 3][:3]:
            (self.rewrite if form == "rewrite" else self.wrong_vnum)(slot)
            self.pipeline(self.image(small=True))
        for _ in range(fill):
            what = int(self.rng.integers(0, 12))
            if what == 0:
                self.rewrite()
                self.pipeline()
            elif what == 1:
                self.wrong_vnum()
                self.pipeline(self.image(small=True))
            elif what in (2, 3):
                self.tuning()
                self.pipeline()
            elif what == 4:
                self.pipeline_rows()
            elif what == 5:
                self.stage()
            elif what == 6 and stages > 1:
                self.stage(stage=1, planar_out=True)
                if self.rng.integers(0, 2):
                    self.tuning()
                self.stage(from_prev=True)
            elif what == 7:
                self.pass_q()
            elif what == 8:
                img = self.image()
                N, H, W, C = img.shape
                self.add("reserve", "ok", N=N, H=H, W=W, C=C)
                self.pipeline(img)
            elif what == 9:
                self.timing()
            elif what == 10:
                self.add("last_detail_counters", "ok")
                self.pipeline(self.image(small=True))
            else:
                self.refused()
                self.pipeline(self.image(small=True))


CONTEXTS = 6


@functools.lru_cache(maxsize=None)
def sequences():
    """the default tour, built once per process"""
    return build_sequences()


def build_sequences(seed=2024, contexts=CONTEXTS, fill=4):
    """[[Op, ...], ...]: one list per context.  The tour's 43 configurations are cut into `contexts` runs that overlap in one
    configuration, so every consecutive pair of the tour is a reconfiguration of one context."""
    rng = np.random.default_rng(seed)
    tour = [FAMILIES[v] for v in euler_tour(len(FAMILIES), rng)]
    edges = len(tour) - 1
    cuts = [round(k * edges / contexts) for k in range(contexts + 1)]
    seen = set()
    seqs = []
    for k in range(contexts):
        b = _Builder(rng, lambda: seen)
        if k == 0:          # before any configure: a compute call, and a table (interval-4 rows are accepted)
            b.pipeline(b.image(small=True))
            b.set_lut(1, "s", 1)
            b.pass_q()
        for fam in tour[cuts[k]:cuts[k + 1] + 1]:
            b.segment(draw_config(fam, rng), fill)
            seen.update(b.m.forms)
        if b.m.timing:      # leave with timing off and queried once more
            b.timing()
        seqs.append(b.ops)
    return seqs


def digest(seqs):
    """sha256 over every operation's name, arguments and expected outcome"""
    h = hashlib.sha256()
    for ops in seqs:
        for op in ops:
            h.update(("%s|%s|%r|" % (op.name, op.kind, op.value if not isinstance(op.value, np.ndarray) else op.value.shape)).encode())
            if isinstance(op.value, np.ndarray):
                h.update(np.ascontiguousarray(op.value).tobytes())
            for key in sorted(op.args):
                v = op.args[key]
                h.update(key.encode())
                h.update(np.ascontiguousarray(v).tobytes() if isinstance(v, np.ndarray) else repr(v).encode())
    return h.hexdigest()


def configurations(ops):
    """[(family, index of the accepted configure, indices of the checked compute calls before the next accepted configure)]"""
    out = []
    for i, op in enumerate(ops):
        if op.name == "configure" and op.kind == "ok":
            a = op.args
            out.append((family_of(a["stages"], a["modes"], a["scale"], a["interval"]), i, []))
        elif out and op.kind == "bytes":
            out[-1][2].append(i)
    return out
