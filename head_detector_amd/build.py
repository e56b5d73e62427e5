"""In-tree build of libvgh.so and its companions libvghview.so, libvghvis.so, libvghtex.so and libvgheval.so (hipcc, gfx950 only). `python -m head_detector_amd.build`."""
from __future__ import annotations

import os
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "csrc")
LIB = os.path.join(HERE, "libvgh.so")
SOURCES = ["conv_igemm.hip", "conv_patch.hip", "conv_rings.hip", "conv_pp.hip", "ds_b2b.hip", "conv_split.hip", "conv_f32.hip", "stem_pool.hip", "postproc.hip", "flame.hip", "net.hip", "detect.hip", "raster.hip", "letterbox.hip", "ctx.hip", "streams.hip"]
EXPERIMENT_SOURCES = ["stem_ds.hip"]  # measured losers kept for tools/: part of libvgh_exp.so (-DVGH_EXPERIMENTS) only
# libvghview.so (include/vgh_view.h): result-side image helpers, a library of its own -- never linked into libvgh.so, hidden visibility but for its vghv_* exports
LIB_VIEW = os.path.join(HERE, "libvghview.so")
VIEW_SOURCES = ["aligned.hip", "draw.hip", "mesh_render.hip"]
VIEW_HEADERS = ["vghv_internal.h"]  # shared by the view library's sources only: a dependency of libvghview.so, not of libvgh.so
# libvghvis.so (include/vgh_vis.h): head visibility buffers, a library of its own like the view library -- hidden visibility but for its vghvis_* exports
LIB_VIS = os.path.join(HERE, "libvghvis.so")
VIS_SOURCES = ["visibility.hip"]
VIS_HEADERS = []  # visibility.hip shares no header with the other two libraries
# libvghtex.so (include/vgh_tex.h): head textures (Sim3DR's render_texture), a library of its own like the other two companions -- hidden visibility but for its vghtex_* exports
LIB_TEX = os.path.join(HERE, "libvghtex.so")
TEX_SOURCES = ["texture.hip"]
TEX_HEADERS = []  # texture.hip shares no header with the other libraries
# libvgheval.so (include/vgh_eval.h): mesh benchmark metrics (Z_n, chamfer), a library of its own like the other companions -- hidden visibility but for its vghev_* exports
LIB_EVAL = os.path.join(HERE, "libvgheval.so")
EVAL_SOURCES = ["mesh_metrics.hip"]
EVAL_HEADERS = []  # mesh_metrics.hip shares no header with the other libraries
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-fno-gpu-rdc", "-Wno-unused-result", "-Wno-unused-value"]


def _hipcc() -> str:
    for c in (os.environ.get("HIPCC"), "/opt/rocm/bin/hipcc", "hipcc"):
        if c and (os.path.isabs(c) and os.path.exists(c) or not os.path.isabs(c)):
            return c
    raise RuntimeError("hipcc not found")


def _core_needs_build() -> bool:
    if not os.path.exists(LIB):
        return True
    t = os.path.getmtime(LIB)
    deps = [os.path.join(CSRC, f) for f in os.listdir(CSRC) if f not in VIEW_SOURCES + VIEW_HEADERS + VIS_SOURCES + VIS_HEADERS + TEX_SOURCES + TEX_HEADERS + EVAL_SOURCES + EVAL_HEADERS] + [os.path.join(HERE, "..", "include", "vgh.h")]
    return any(os.path.getmtime(d) > t for d in deps)


def _view_needs_build() -> bool:
    if not os.path.exists(LIB_VIEW):
        return True
    t = os.path.getmtime(LIB_VIEW)
    deps = [os.path.join(CSRC, f) for f in VIEW_SOURCES + VIEW_HEADERS] + [os.path.join(HERE, "..", "include", "vgh_view.h")]
    return any(os.path.getmtime(d) > t for d in deps)


def _vis_needs_build() -> bool:
    if not os.path.exists(LIB_VIS):
        return True
    t = os.path.getmtime(LIB_VIS)
    deps = [os.path.join(CSRC, f) for f in VIS_SOURCES + VIS_HEADERS] + [os.path.join(HERE, "..", "include", "vgh_vis.h")]
    return any(os.path.getmtime(d) > t for d in deps)


def _tex_needs_build() -> bool:
    if not os.path.exists(LIB_TEX):
        return True
    t = os.path.getmtime(LIB_TEX)
    deps = [os.path.join(CSRC, f) for f in TEX_SOURCES + TEX_HEADERS] + [os.path.join(HERE, "..", "include", "vgh_tex.h")]
    return any(os.path.getmtime(d) > t for d in deps)


def _eval_needs_build() -> bool:
    if not os.path.exists(LIB_EVAL):
        return True
    t = os.path.getmtime(LIB_EVAL)
    deps = [os.path.join(CSRC, f) for f in EVAL_SOURCES + EVAL_HEADERS] + [os.path.join(HERE, "..", "include", "vgh_eval.h")]
    return any(os.path.getmtime(d) > t for d in deps)


def needs_build() -> bool:
    return _core_needs_build() or _view_needs_build() or _vis_needs_build() or _tex_needs_build() or _eval_needs_build()


LIB_EXP = os.path.join(HERE, "libvgh_exp.so")  # -DVGH_EXPERIMENTS build (work-skipping switches, env-var knobs): tools/ only


def build_lib(force: bool = False, verbose: bool = True, experiments: bool = False, variant_defines=None) -> str:
    if variant_defines:  # A/B builds of the PRODUCT code with one compile-time knob changed (no experiment switches): libvgh_var.so
        return _build(os.path.join(HERE, "libvgh_var.so"), [f"-D{d}" for d in variant_defines], "build_var", verbose)
    if experiments:
        return _build(LIB_EXP, ["-DVGH_EXPERIMENTS"], "build_exp", verbose)
    if force or _eval_needs_build():  # float64 distances in a stated operation order: no contraction into fused multiply-adds anywhere in this library
        _build(LIB_EVAL, ["-fvisibility=hidden", "-ffp-contract=off"], "build_eval", verbose, EVAL_SOURCES)
    if force or _tex_needs_build():
        _build(LIB_TEX, ["-fvisibility=hidden"], "build_tex", verbose, TEX_SOURCES)
    if force or _vis_needs_build():
        _build(LIB_VIS, ["-fvisibility=hidden"], "build_vis", verbose, VIS_SOURCES)
    if force or _view_needs_build():
        _build(LIB_VIEW, ["-fvisibility=hidden"], "build_view", verbose, VIEW_SOURCES)
    if force or _core_needs_build():
        _build(LIB, [], "build", verbose)
    return LIB


def _build(LIB: str, extra, objdir: str, verbose: bool, sources=None) -> str:
    hipcc = _hipcc()
    objs, procs = [], []
    t0 = time.time()
    os.makedirs(os.path.join(HERE, objdir), exist_ok=True)
    for src in sources or SOURCES + (EXPERIMENT_SOURCES if "-DVGH_EXPERIMENTS" in extra else []):
        obj = os.path.join(HERE, objdir, src.replace(".hip", ".o"))
        objs.append(obj)
        cmd = [hipcc, *FLAGS, *extra, "-c", os.path.join(CSRC, src), "-o", obj]
        procs.append((src, subprocess.Popen(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)))
    failed = False
    for src, p in procs:
        out, _ = p.communicate()
        if p.returncode != 0:
            failed = True
            sys.stderr.write(f"[vgh build] {src} FAILED\n{out}\n")
        elif verbose and out.strip():
            sys.stderr.write(f"[vgh build] {src}:\n{out}\n")
    if failed:
        raise RuntimeError(f"{os.path.basename(LIB)}: compilation failed")
    cmd = [hipcc, "--offload-arch=gfx950", "-shared", "-fPIC", *objs, "-o", LIB]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    if r.returncode != 0:
        raise RuntimeError(f"{os.path.basename(LIB)}: link failed\n{r.stdout}")
    import ctypes

    try:  # catches undefined symbols (e.g. a kernel whose host stub was silently dropped) at build time, not on the GPU box
        ctypes.CDLL(LIB)
    except OSError as e:
        os.remove(LIB)
        raise RuntimeError(f"{os.path.basename(LIB)}: built but does not load: {e}")
    if verbose:
        sys.stderr.write(f"[vgh build] built {LIB} in {time.time() - t0:.1f}s\n")
    return LIB


if __name__ == "__main__":
    build_lib(force="--force" in sys.argv, experiments="--experiments" in sys.argv, variant_defines=[a[2:] for a in sys.argv[1:] if a.startswith("-D")])
