"""Builds and loads libmulut_hip.so (the C ABI of include/mulut.h) with ctypes."""
import ctypes
import os
import shutil
import subprocess

_PKG = os.path.dirname(os.path.abspath(__file__))
_CSRC = os.path.join(_PKG, "csrc")
_LIBDIR = os.path.join(_PKG, "lib")
LIB_PATH = os.path.join(_LIBDIR, "libmulut_hip.so")
SOURCES = ["mulut_kernels.hip", "mulut_k1.hip", "mulut_detail.hip", "mulut_interval.hip", "mulut_capi.hip", "mulut_ft.hip", "mulut_ft_interval.hip", "mulut_ft_exact.hip", "mulut_ft_data.hip", "mulut_eval.hip", "mulut_resample.hip", "mulut_net.hip", "mulut_net_list.hip", "mulut_net_train.hip"]
HEADERS = ["mulut_core.h", "mulut_interval.h", "mulut_ft.h", "mulut_ft_interval.h", "mulut_ft_exact.h", "mulut_kernels.h", "mulut_dev.h", "mulut_net.h", "mulut_net_dev.h", "mulut_net_list.h", "mulut_tube2_asm.inc", os.path.join("..", "..", "include", "mulut.h")]
# -Wno-inline-asm: stage_tube2_kernel names registers ABOVE the register allocator's budget in its asm clobber lists on purpose
# (tools/gen_tube2_asm.py); -Wno-pass-failed: its occupancy attribute is that budget, not an occupancy the kernel reaches
HIPCC_FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-shared", "-Wall", "-Wno-inline-asm", "-Wno-pass-failed"]


def _prototypes():
    """One entry per function of include/mulut.h, in the header's order: name -> (restype, argtypes).  The typed pointers are what
    call sites hand byref() objects and ctypes arrays to; device and opaque pointers are plain c_void_p (callers pass data_ptr())."""
    i, p, s, c, ll, d = ctypes.c_int, ctypes.c_void_p, ctypes.c_char_p, ctypes.c_char, ctypes.c_longlong, ctypes.c_double
    pp, fp, dp, i32p = ctypes.POINTER(p), ctypes.POINTER(ctypes.c_float), ctypes.POINTER(d), ctypes.POINTER(ctypes.c_int32)
    fpp = ctypes.POINTER(fp)
    return {
        # the context and the inference cascade
        "mulut_version": (i, []),
        "mulut_strerror": (s, [i]),
        "mulut_last_hip_error": (s, [p]),
        "mulut_create": (i, [i, pp]),
        "mulut_destroy": (i, [p]),
        "mulut_configure": (i, [p, i, s, i, i]),
        "mulut_set_lut": (i, [p, i, c, p, ll, i]),
        "mulut_read_table_image": (ll, [p, i, c, i, p, ll, p]),
        "mulut_pass": (i, [p, i, c, i, p, i, i, i, p, p]),
        "mulut_stage": (i, [p, i, p, i, p, i, i, i, i, i, p]),
        "mulut_pipeline": (i, [p, p, p, i, i, i, i, i, p]),
        "mulut_pipeline_rows": (i, [p, p, i, i, p, i, i, i, i, i, i, i, p]),
        "mulut_halo": (i, [p]),
        "mulut_reserve": (i, [p, i, i, i, i]),
        "mulut_set_stage_timing": (i, [p, i]),
        "mulut_last_stage_ms": (i, [p, fp, i]),
        "mulut_last_kernel_ms": (i, [p, fp, i]),
        "mulut_last_detail_counters": (i, [p, ctypes.POINTER(ctypes.c_uint32), i, p]),
        "mulut_debug_read": (i, [p, ctypes.POINTER(ctypes.c_uint64), i, i, p]),
        # LUT-aware fine-tuning
        "mulut_ft_quantize": (i, [i, p, p, i, ll, p]),
        "mulut_ft_quantize_backward": (i, [i, p, p, i, ll, p]),
        "mulut_ft_adam": (i, [i, p, p, p, p, p, i, ll, d, d, d, d, d, p]),
        "mulut_ft_stage_forward": (i, [i, p, s, i, i, p, i, i, i, i, p, p]),
        "mulut_ft_stage_backward": (i, [i, p, s, i, i, p, p, i, i, i, i, p, p, p]),
        "mulut_ft_stage_forward_mask": (i, [i, p, s, i, i, p, i, i, i, i, p, p, p]),
        "mulut_ft_stage_backward_mask": (i, [i, p, s, i, i, p, p, p, i, i, i, i, p, p, p]),
        "mulut_ft_interval_stage_forward": (i, [i, i, p, s, i, i, p, i, i, i, i, p, p, p]),
        "mulut_ft_interval_stage_backward": (i, [i, i, p, s, i, i, p, p, p, i, i, i, i, p, p, p]),
        "mulut_ft_wide_stage_forward": (i, [i, i, p, s, i, i, p, i, i, i, i, p, p, p]),
        "mulut_ft_wide_stage_backward": (i, [i, i, p, s, i, i, p, p, p, i, i, i, i, p, p, p]),
        "mulut_ft_exact_ws_bytes": (ll, [i, s, i, i, i, i, i]),
        "mulut_ft_exact_stage_backward": (i, [i, i, p, s, i, i, p, p, p, i, i, i, i, p, p, p, ll, p]),
        "mulut_ft_crop_batch": (i, [i, p, ll, p, i, p, i, i, i, p, p, p, p]),
        "mulut_ft_val_pack": (i, [i, p, i, i, p, p]),
        # device-side evaluation
        "mulut_eval_ws_doubles": (ll, [i, i]),
        "mulut_eval_y": (i, [i, p, p, i, i, i, p, ll, dp, dp, p]),
        "mulut_eval_plan_create": (i, [i, p, i, i, pp]),
        "mulut_eval_plan_run": (i, [p, p, p, p, p]),
        "mulut_eval_plan_destroy": (i, [p]),
        "mulut_eval_finish": (i, [d, d, i, i, i, dp, dp]),
        # LR images made on the device
        "mulut_resample_coeffs": (i, [i, i, i32p, i32p, i32p, ll]),
        "mulut_resample_plan_create": (i, [i, i, i, i, i, pp]),
        "mulut_resample_plan_destroy": (i, [p]),
        "mulut_resample_run": (i, [p, p, i, p, i, i, i, p]),
        # the trained network, fused
        "mulut_net_unit_create": (i, [i, i, i, fpp, fpp, pp]),
        "mulut_net_unit_destroy": (i, [p]),
        "mulut_net_table": (i, [p, i, p, p]),
        "mulut_net_pass": (i, [p, c, i, p, i, i, i, i, p, p]),
        "mulut_net_stage": (i, [pp, s, i, p, p, i, i, i, i, p]),
        "mulut_net_plan_create": (i, [i, p, i, i, i, i, pp]),
        "mulut_net_plan_run": (i, [p, pp, s, p, p, p]),
        "mulut_net_plan_destroy": (i, [p]),
        # training the network
        "mulut_net_unit_create_train": (i, [i, i, i, pp]),
        "mulut_net_unit_load_dev": (i, [p, pp, pp, p]),
        "mulut_net_pack_host": (ll, [i, i, fpp, fpp, i, p, ll]),
        "mulut_net_unit_read": (ll, [p, i, p, ll]),
        "mulut_net_stage_sum": (i, [pp, s, p, i, i, i, i, p, p]),
        "mulut_net_backward_ws_bytes": (ll, [i, i, ll]),
        "mulut_net_stage_backward": (i, [pp, s, p, p, i, i, i, i, p, ll, p, pp, pp, p]),
        # the same backward with a bit-reproducible gx
        "mulut_net_backward_exact_ws_bytes": (ll, [i, i, ll, ll]),
        "mulut_net_stage_backward_exact": (i, [pp, s, p, p, i, i, i, i, p, ll, p, pp, pp, p]),
        "mulut_net_gx_gather": (i, [i, c, i, p, ll, i, i, i, i, p, i, p]),
        # tuning knobs and kernel names
        "mulut_set_tuning": (i, [p, s, i]),
        "mulut_kernel_name": (s, [p, i]),
    }


PROTOTYPES = _prototypes()
EXPORTS = list(PROTOTYPES)       # every symbol include/mulut.h declares

_libs = {}


def _hipcc():
    return shutil.which("hipcc") or ("/opt/rocm/bin/hipcc" if os.path.exists("/opt/rocm/bin/hipcc") else None)


def source_hash():
    """sha256 over the kernel sources and headers: ties profiler-derived numbers (profiles/*.json) to the build they
    were measured on -- bench.py reports them only while this hash still matches."""
    import hashlib
    h = hashlib.sha256()
    for f in sorted(SOURCES + [x for x in HEADERS if not x.endswith("mulut.h")]):      # device code only: the ABI header declares, it does not compute
        with open(os.path.join(_CSRC, f), "rb") as fh:
            h.update(fh.read())
    return h.hexdigest()[:16]


def needs_build():
    if not os.path.exists(LIB_PATH):
        return True
    t = os.path.getmtime(LIB_PATH)
    return any(os.path.getmtime(os.path.join(_CSRC, f)) > t for f in SOURCES + HEADERS)


def audit_tube2_isa(asm_path=None):
    """stage_tube2_kernel keeps the rows of the pass in flight in v88..v127 ACROSS asm statements (tools/gen_tube2_asm.py); the only
    things that keep the compiler out of them are its register budget (amdgpu_waves_per_eu) and the clobber lists, and neither binds a
    short-lived temporary by contract.  So the library is not accepted on trust: this compiles mulut_kernels.hip to gfx950 assembly
    (or reads `asm_path`) and raises unless, in every stage_tube2_kernel instance, (i) no instruction outside the inline-asm blocks
    names v<TUBE2_ROW0> or above, (ii) no AGPR is used and (iii) at most 128 VGPRs are allocated (the kernel is launched with 1024
    threads at 4 waves per SIMD: 512 / 4 registers per lane).  Returns the number of kernels audited."""
    import re
    import tempfile
    hipcc = _hipcc()
    if hipcc is None:
        raise RuntimeError("hipcc not found: cannot audit stage_tube2_kernel")
    inc = open(os.path.join(_CSRC, "mulut_tube2_asm.inc")).read()
    row0 = int(re.search(r"#define TUBE2_ROW0 (\d+)", inc).group(1))
    with tempfile.TemporaryDirectory() as td:
        if asm_path is None:
            asm_path = os.path.join(td, "mulut_kernels.s")
            flags = [f for f in HIPCC_FLAGS if f not in ("-fPIC", "-shared")]
            subprocess.check_call([hipcc] + flags + ["--cuda-device-only", "-S", "-o", asm_path, os.path.join(_CSRC, "mulut_kernels.hip")],
                                  stderr=subprocess.DEVNULL)
        lines = open(asm_path).read().splitlines()
    reg = re.compile(r"\bv(\d+)\b|\bv\[(\d+):(\d+)\]")
    kernels, name, in_asm, bad = [], None, False, []
    for line in lines:
        m = re.match(r"^(_ZN5mulut18stage_tube2_kernel\w+):", line)
        if m:
            name, in_asm = m.group(1), False
            kernels.append(name)
            continue
        m = re.match(r"^\s*\.set (_ZN5mulut18stage_tube2_kernel\w+)\.(num_vgpr|num_agpr), (\d+)", line)
        if m:
            if (m.group(2) == "num_agpr" and int(m.group(3)) != 0) or (m.group(2) == "num_vgpr" and int(m.group(3)) > 128):
                bad.append((m.group(1), line.strip()))
            continue
        if name is None:
            continue
        if "s_endpgm" in line:
            name = None
        elif "#ASMSTART" in line:
            in_asm = True
        elif "#ASMEND" in line:
            in_asm = False
        elif not in_asm and not line.lstrip().startswith((";", ".")):
            for a, lo, hi in reg.findall(line.split(";")[0]):
                if (int(a) if a else int(hi)) >= row0:
                    bad.append((name, line.strip()))
    if len(kernels) != 3:          # generic, planar, rgb
        raise RuntimeError("tube2 audit: expected 3 stage_tube2_kernel instances, found %d" % len(kernels))
    if bad:
        raise RuntimeError("tube2 audit failed (the compiler touched the kernel's private registers, or the register budget changed): %r" % (bad[:5],))
    return len(kernels)


def build(force=False, verbose=False):
    """Compile the HIP extension in-tree for gfx950 (cross-compiles without a GPU).  The library is only put in place after
    audit_tube2_isa() has accepted the assembly of the same sources with the same flags."""
    if not force and not needs_build():
        return LIB_PATH
    hipcc = _hipcc()
    if hipcc is None:
        raise RuntimeError("hipcc not found: cannot build libmulut_hip.so (no CPU fallback exists)")
    os.makedirs(_LIBDIR, exist_ok=True)
    tmp = "%s.%d.tmp" % (LIB_PATH, os.getpid())     # never expose a half-written library to another rank
    cmd = [hipcc] + HIPCC_FLAGS + ["-o", tmp] + SOURCES
    if verbose:
        print(" ".join(cmd))
    try:
        subprocess.check_call(cmd, cwd=_CSRC)
        audit_tube2_isa()
        os.replace(tmp, LIB_PATH)
    finally:
        if os.path.exists(tmp):
            os.remove(tmp)
    return LIB_PATH


def check(rc, error=None):
    """The test of a return code of the C ABI (MuLUTEngine._check apart, which adds its context's HIP error text): a negative one
    raises RuntimeError with mulut_strerror's text -- or `error`, a class, with MuLUTError's "mulut error {rc}: {text}" -- and
    anything else is handed back (some calls return a count)."""
    if rc < 0:
        text = load().mulut_strerror(rc).decode()
        raise RuntimeError(text) if error is None else error("mulut error %d: %s" % (rc, text))
    return rc


def load(path=None):
    """Return the ctypes handle; builds the library first if its sources are newer.
    `path` (or $MULUT_LIB) selects another build of the same ABI, e.g. an A/B kernel variant."""
    path = path or os.environ.get("MULUT_LIB") or LIB_PATH
    if path in _libs:
        return _libs[path]
    if path == LIB_PATH and needs_build():
        if os.environ.get("MULUT_NO_BUILD") == "1":
            # profiler runs (the preloaded tool has initialised the GPU) and non-zero ranks must never compile
            if not os.path.exists(LIB_PATH):
                raise RuntimeError("libmulut_hip.so is missing and MULUT_NO_BUILD=1 forbids building it here")
        elif _hipcc() is not None:
            build()
        elif not os.path.exists(LIB_PATH):
            raise RuntimeError("libmulut_hip.so is missing and hipcc is unavailable; "
                               "run `python -c 'import __graft_entry__ as g; g.build()'`")
    L = ctypes.CDLL(path)
    for name, (restype, argtypes) in PROTOTYPES.items():
        fn = getattr(L, name)
        fn.restype, fn.argtypes = restype, argtypes
    _libs[path] = L
    return L


def stream_ptr(device=None):
    """The current torch stream of `device` as the void* every `stream` parameter of the ABI takes."""
    import torch
    return ctypes.c_void_p(torch.cuda.current_stream(device).cuda_stream)


def ptr_array(tensors):
    """The data pointers of `tensors` as a void*[]: what the `const float *const *` parameters take."""
    return (ctypes.c_void_p * len(tensors))(*[t.data_ptr() for t in tensors])
