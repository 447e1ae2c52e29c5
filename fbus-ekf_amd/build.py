#!/usr/bin/env python3
"""Builds fbus-ekf_amd/lib/libfbus_ekf.so (HIP, gfx950) in-tree with hipcc.

The library is len(units()) translation units compiled in parallel and linked into one shared object:
  fbus_ekf.hip                          handle and C ABI; it defines and launches no kernel (unit "main")
  kernels_tu.hip, once per unit         one kernel family for one (float|double, N = 18|15), both dialects (-DFBUS_TU_T/N/FAMILY):
                                        every row of FAMILIES for float, the rows marked fp64 for double, each for N = 18 and N = 15
  small_tu.hip, once per unit           the same for the small families (state I/O, hypothesis groups, sensor updates, screening, reports),
                                        built with the base flags alone, and once more for the kernels that depend on neither N nor the
                                        dialect (unit "common")
Objects live in fbus-ekf_amd/lib/obj/ (git-ignored) and are rebuilt when a source or any header under csrc/ is newer.
  python build.py [--force] [--only f32_18_correct,...] [--jobs N]
FBUS_OUT / FBUS_EXTRA_FLAGS: experiment builds (A/B of differently built kernels via FBUS_EKF_LIB).
"""
import os
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "csrc")
HEADERS = sorted(os.path.join(CSRC, h) for h in os.listdir(CSRC) if h.endswith(".hpp")) + [os.path.join(HERE, "..", "include", "fbus_ekf.h")]
OUT = os.environ.get("FBUS_OUT") or os.path.join(HERE, "lib", "libfbus_ekf.so")   # FBUS_OUT / FBUS_EXTRA_FLAGS: experiment builds
OBJDIR = os.environ.get("FBUS_OBJDIR") or os.path.join(os.path.dirname(OUT), "obj" if not os.environ.get("FBUS_OUT") else
                                                       "obj_" + os.path.splitext(os.path.basename(OUT))[0])
MAX_ILP = "-mllvm -amdgpu-sched-strategy=max-ilp"
# One row per kernel family (kernels_tu.hip and small_tu.hip list what each number holds):
#   name: (FBUS_TU_FAMILY, the family whose flags it is built with, built for fp64 records too)
# An extension family (a kernel of another family with a trailing pack) is built with the flags of the family it extends, both record
# types.  fp64 has one fused frame kernel (family "frame": frame2_kernel) and runs the windows frame by frame.
# The small families (None in the place of that family) are built from small_tu.hip with the base flags alone: no scheduler flag, no
# FBUS_*_FLAGS override.
FAMILIES = {
    "predict":    (1,  "predict", True),
    "correct":    (2,  "correct", True),
    "frame":      (3,  "frame",   True),
    "frames":     (5,  "frames",  False),
    "team":       (6,  "team",    False),
    "meas":       (7,  "meas",    True),
    "fmeas":      (8,  "fmeas",   False),
    "msplit":     (9,  "msplit",  False),
    "framest":    (10, "frames",  False),   # the windows with per-frame trajectory rows
    "fmeast":     (11, "fmeas",   False),
    "measnis":    (12, "meas",    True),    # the pixel / corner and the pose updates with the NIS output and the gate
    "correctnis": (13, "correct", True),
    "prednz":     (14, "predict", True),    # predict and the NIS updates with per-filter noise
    "measnz":     (15, "meas",    True),
    "correctnz":  (16, "correct", True),
    "measlik":    (17, "meas",    True),    # the tabled NIS updates with the log-likelihood sums
    "correctlik": (18, "correct", True),
    "framesnz":   (19, "frames",  False),   # the trajectory windows with per-filter noise (the resident windows of a tabled handle)
    "fmeasnz":    (20, "fmeas",   False),
    "state":      (21, None,      True),    # pack / unpack / snapshot / reset_cov and the two initialisations
    "group":      (22, None,      True),    # hypothesis groups
    "sensor":     (23, None,      True),    # depth, velocity and general rows
    "screen":     (24, None,      True),    # per-marker screening
    "report":     (25, None,      True),    # NEES and draws
}
COMMON = 26                           # small_tu.hip's unit that is built once: the kernels that depend on neither N nor the dialect
# Seconds one unit took to compile, N = 18 (N = 15: about 0.7 of it), in a forced build with 16 jobs (EXPERIMENTS.md): build() starts
# the longest first.  fp32, then the fp64 units that differ much from their fp32 twin; a family that is missing counts as 10.
SECONDS = {"fmeas": 53, "fmeast": 39, "meas": 39, "fmeasnz": 38, "frame": 35, "correctlik": 34, "team": 33, "correctnis": 32, "correctnz": 32,
           "framest": 30, "correct": 29, "frames": 29, "framesnz": 27, "measlik": 19, "measnis": 19, "sensor": 19, "measnz": 17, "screen": 15, "msplit": 13,
           "report": 12, "group": 11, "predict": 10, "prednz": 8, "state": 4}
SECONDS_F64 = {"meas": 54, "correctnz": 39, "measnis": 25, "measnz": 24, "measlik": 24, "frame": 12}
SECONDS_ONCE = {"main": 19, "common": 6}


def seconds_of(name):
    """the estimate behind build()'s start order, for a unit name of units()"""
    if name in SECONDS_ONCE:
        return SECONDS_ONCE[name]
    tn, n, fam = name.split("_")
    base = SECONDS_F64.get(fam, SECONDS.get(fam, 10)) if tn == "f64" else SECONDS.get(fam, 10)
    return base * (1.0 if n == "18" else 0.7)
# Per-family scheduler choice, fp32 units (measured in one run, B = 65 536, tools/ab_bench.sh, profiles/logs/r02_ab2.log): the
# max-ILP strategy of the AMDGPU machine scheduler shortens the per-call kernels, where one wave per SIMD has nothing
# but its own independent instructions to cover dependent-issue stalls (predict 13.4 -> 13.05 us, stacked correct
# 23.0 -> 21.6 us, headline +3.5 %), and lengthens the fused frame kernel (-2.8 %: more live registers, more
# v_accvgpr traffic), which therefore keeps the default strategy.  FBUS_<FAMILY>_FLAGS overrides where listed.
F32_FLAGS = {"predict": os.environ.get("FBUS_PREDICT_FLAGS", MAX_ILP), "correct": MAX_ILP, "team": MAX_ILP,
             **{fam: os.environ.get("FBUS_" + fam.upper() + "_FLAGS", "") for fam in ("frame", "frames", "meas", "fmeas", "msplit")}}
# fp64 units.  meas (correct_pixels2 / correct_corners2 <double>, 512 registers + scratch): the max-memory-clause strategy leaves them
# 28-136 bytes of scratch instead of 136-340 and is 4-11 % faster (profiles/r05_f64_sched.txt); FBUS_F64_FLAGS_<FAMILY> overrides, by
# the unit's own family name
F64_FLAGS = {"meas": "-mllvm -amdgpu-sched-strategy=max-memory-clause"}
TYPES = {"f32": "float", "f64": "double"}


def hipcc():
    for c in (os.environ.get("HIPCC"), "/opt/rocm/bin/hipcc", "hipcc"):
        if c and (os.path.isabs(c) and os.path.exists(c) or not os.path.isabs(c)):
            return c
    raise RuntimeError("hipcc not found")


def units():
    """(name, source, defines)"""
    out = [("main", os.path.join(CSRC, "fbus_ekf.hip"), []), ("common", os.path.join(CSRC, "small_tu.hip"), [f"-DFBUS_TU_FAMILY={COMMON}"])]
    for tn, t in TYPES.items():
        for n in (18, 15):
            for fam, (code, like, f64) in FAMILIES.items():
                if tn == "f64" and not f64:
                    continue
                if like is None:            # a small family: the base flags and the three defines, nothing else
                    out.append((f"{tn}_{n}_{fam}", os.path.join(CSRC, "small_tu.hip"), [f"-DFBUS_TU_T={t}", f"-DFBUS_TU_N={n}", f"-DFBUS_TU_FAMILY={code}"]))
                    continue
                # fp32: the family's flags -- the fp64 kernels sit at the 512-register limit and spill more under max-ILP
                flags = F32_FLAGS[like] if tn == "f32" else os.environ.get("FBUS_F64_FLAGS_" + fam.upper(), F64_FLAGS.get(like, ""))
                if os.environ.get("FBUS_NO_FAMILY_FLAGS"):      # the flag-free A/B baseline -- for BOTH record types (advisor, round 5)
                    flags = ""
                out.append((f"{tn}_{n}_{fam}", os.path.join(CSRC, "kernels_tu.hip"),
                            [f"-DFBUS_TU_T={t}", f"-DFBUS_TU_N={n}", f"-DFBUS_TU_FAMILY={code}"] + flags.split()))
    return out


def _base_flags():
    # -fno-slp-vectorize: the SLP pass packs the unrolled scalar FMAs into v_pk_fma_f32 and pays for it with
    # ~1.9x more instructions (v_mov / v_accvgpr shuffles to form register pairs) -- measured on the .s
    return ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fno-slp-vectorize", "-fPIC"] + os.environ.get("FBUS_EXTRA_FLAGS", "").split()


def _flags_of(defs):
    """the flag string an object was / would be compiled with: written next to the object (<obj>.flags) so that a flag change made
    through the environment (FBUS_EXTRA_FLAGS, FBUS_*_FLAGS, FBUS_NO_FAMILY_FLAGS) invalidates it -- mtimes alone do not"""
    return " ".join(_base_flags() + list(defs))


def _stale(obj, src, defs=None):
    if not os.path.exists(obj):
        return True
    if defs is not None:
        try:
            if open(obj + ".flags").read() != _flags_of(defs):
                return True
        except OSError:
            return True
    t = os.path.getmtime(obj)
    return any(os.path.exists(d) and os.path.getmtime(d) > t for d in [src, os.path.abspath(__file__)] + HEADERS)


def needs_build():
    """the shared object is older than a source (the objects are a build cache: they do not travel with the library)"""
    if not os.path.exists(OUT):
        return True
    t = os.path.getmtime(OUT)
    srcs = {src for _, src, _ in units()} | set(HEADERS) | {os.path.abspath(__file__)}
    if any(os.path.exists(d) and os.path.getmtime(d) > t for d in srcs):
        return True
    # a partial rebuild (--only) links a library that is newer than every source while other objects are still stale
    return os.path.isdir(OBJDIR) and any(_stale(os.path.join(OBJDIR, name + ".o"), src, defs) for name, src, defs in units()
                                         if os.path.exists(os.path.join(OBJDIR, name + ".o")))


def build(force=False, verbose=False, only=None, jobs=None):
    if not force and not needs_build():
        return OUT
    os.makedirs(OBJDIR, exist_ok=True)
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    flags = _base_flags()
    todo = []
    for name, src, defs in units():
        obj = os.path.join(OBJDIR, name + ".o")
        if only and not any(o in name for o in only) and os.path.exists(obj):
            continue
        if force or _stale(obj, src, defs) or (only and any(o in name for o in only)):
            todo.append((name, [hipcc()] + flags + defs + ["-c", src, "-o", obj], obj, _flags_of(defs)))
    todo.sort(key=lambda u: seconds_of(u[0]), reverse=True)     # the longest first: the tail of the build is then a short unit
    jobs = jobs or int(os.environ.get("FBUS_JOBS", "0")) or min(8, os.cpu_count() or 1)

    def run(u):
        if verbose:
            print("  hipcc", u[0], flush=True)
        r = subprocess.run(u[1], capture_output=True, text=True)
        if r.returncode != 0:
            raise RuntimeError(f"{u[0]}: {' '.join(u[1])}\n{r.stderr[-4000:]}")
        if r.stderr.strip() and verbose:
            print(r.stderr[-2000:])
        with open(u[2] + ".flags", "w") as f:
            f.write(u[3])
        return u[0]

    with ThreadPoolExecutor(max_workers=jobs) as ex:
        list(ex.map(run, todo))
    objs = [os.path.join(OBJDIR, name + ".o") for name, _, _ in units()]
    cmd = [hipcc(), "--offload-arch=gfx950", "-shared", "-fPIC", "-o", OUT] + objs
    if verbose:
        print("  link", os.path.relpath(OUT, HERE), flush=True)
    subprocess.run(cmd, check=True)
    return OUT


def build_host_asan(out=None):
    """The library with fbus_ekf.hip (handle, argument checks, staging, parameter tables, RCCL binding) under AddressSanitizer + UBSan:
    `-fsanitize=address,undefined -fno-gpu-sanitize` instruments host code only, and fbus_ekf.hip holds no kernel: every device code
    object is the normal one (GPU ASan is not available on this pool).  Linked against the already built objects of all other units.
    Load it with LD_PRELOAD of clang's ASan runtime (tests/test_sanitizers_cpu.py)."""
    build()
    out = out or os.path.join(os.path.dirname(OUT), "libfbus_ekf_asan.so")
    obj = os.path.join(OBJDIR, "main_asan.o")
    san = ["-fsanitize=address,undefined", "-fno-gpu-sanitize", "-shared-libsan"]
    subprocess.run([hipcc(), "--offload-arch=gfx950", "-O1", "-g", "-std=c++17", "-fno-slp-vectorize", "-fPIC"] + san +
                   ["-c", os.path.join(CSRC, "fbus_ekf.hip"), "-o", obj], check=True, capture_output=True)
    objs = [os.path.join(OBJDIR, name + ".o") for name, _, _ in units() if name != "main"]
    subprocess.run([hipcc(), "--offload-arch=gfx950", "-shared", "-fPIC"] + san + ["-o", out, obj] + objs, check=True, capture_output=True)
    return out


def asan_runtime():
    """clang's shared ASan runtime (what LD_PRELOAD needs for build_host_asan's library)"""
    import glob
    c = sorted(glob.glob("/opt/rocm/lib/llvm/lib/clang/*/lib/linux/libclang_rt.asan-x86_64.so"))
    return c[-1] if c else None


if __name__ == "__main__":
    only = None
    jobs = None
    for i, a in enumerate(sys.argv):
        if a == "--only":
            only = sys.argv[i + 1].split(",")
        if a == "--jobs":
            jobs = int(sys.argv[i + 1])
    if "--host-asan" in sys.argv:
        print(build_host_asan())
        sys.exit(0)
    print(build(force="--force" in sys.argv, verbose=True, only=only, jobs=jobs))
