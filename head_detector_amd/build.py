"""In-tree build of libvgh.so, its companions libvghview.so, libvghvis.so, libvghtex.so, libvgheval.so, libvghmerge.so and libvghtrack.so, the application
library libvghanon.so, the video library libvghvideo.so, the downstream library libvghcrop.so and the overlay library libvghosd.so (hipcc, gfx950 only). `python -m head_detector_amd.build`."""
from __future__ import annotations

import os
import subprocess
import sys
import time
from typing import NamedTuple

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "csrc")
LIB = os.path.join(HERE, "libvgh.so")
SOURCES = ["conv_igemm.hip", "conv_patch.hip", "conv_rings.hip", "conv_pp.hip", "ds_b2b.hip", "conv_split.hip", "conv_f32.hip", "stem_pool.hip", "postproc.hip", "flame.hip", "net.hip", "detect.hip", "raster.hip", "letterbox.hip", "ctx.hip", "streams.hip"]
EXPERIMENT_SOURCES = ["stem_ds.hip"]  # measured losers kept for tools/: part of libvgh_exp.so (-DVGH_EXPERIMENTS) only


class Companion(NamedTuple):
    """A library of its own: never linked into libvgh.so or into another companion, hidden visibility but for the exports of its public header."""
    lib: str  # file name, next to this file
    sources: list
    headers: list  # private headers under csrc/
    public: str  # under include/
    flags: list  # beyond FLAGS and -fvisibility=hidden
    objdir: str


HOST_HEADERS = ["companion_host.h"]  # the host plumbing of every companion (codes, message, check macros, staging, queue-then-record): header-only
RASTER_HEADERS = HOST_HEADERS + ["tile_fold.h"]  # the tile-major triangle fold: header-only, compiled into each of the three libraries that rasterise
ANON_HEADERS = HOST_HEADERS + ["head_rows.h"]  # the head rows of the two anonymisers (RGB images, YUV planes): header-only, compiled into each of the two
# a frame's byte planes addressed in place (checks, overlap rule, pair access, copy): header-only, compiled into libvghvideo.so and libvghosd.so, the two
# libraries that write such planes; the RGB anonymiser works on one packed image and does not take it
PLANE_HEADERS = ["plane_views.h"]
COMPANIONS = [  # built in this order, before the core
    # benchmark metrics, mesh (Z_n, chamfer) and detection (COCO-style box AP): float64 in a stated operation order, so no contraction into fused
    # multiply-adds anywhere in this library
    Companion("libvgheval.so", ["mesh_metrics.hip", "detection_ap.hip"], HOST_HEADERS, "vgh_eval.h", ["-ffp-contract=off"], "build_eval"),
    # the cross-tile merge of sliced detection: float32 in a stated operation order, equal bit for bit to its NumPy restatement
    Companion("libvghmerge.so", ["slice_merge.hip"], HOST_HEADERS, "vgh_merge.h", ["-ffp-contract=off"], "build_merge"),
    # head tracking across video frames: float32 in a stated operation order, equal bit for bit to its NumPy restatement
    Companion("libvghtrack.so", ["head_track.hip"], HOST_HEADERS, "vgh_track.h", ["-ffp-contract=off"], "build_track"),
    Companion("libvghtex.so", ["texture.hip"], RASTER_HEADERS, "vgh_tex.h", [], "build_tex"),  # head textures (Sim3DR's render_texture)
    Companion("libvghvis.so", ["visibility.hip"], RASTER_HEADERS, "vgh_vis.h", [], "build_vis"),  # head visibility buffers
    Companion("libvghview.so", ["aligned.hip", "draw.hip", "mesh_render.hip"], RASTER_HEADERS, "vgh_view.h", [], "build_view"),  # result-side image helpers
]
# Libraries on the result side that compose the companions' outputs in Python (and link none of them): built like a companion, before the core
APPLICATIONS = [
    # head anonymisation (pixelate, blur, fill): integer arithmetic only, equal bit for bit to its NumPy restatement
    Companion("libvghanon.so", ["anonymize.hip"], ANON_HEADERS, "vgh_anon.h", [], "build_anon"),
]
# Libraries on the video side (frames in their own YUV planes): built like a companion, before the core
VIDEO = [
    # heads anonymised in the planes of a YUV 4:2:0 frame, and RGB packed into such planes: integer arithmetic only, equal bit for bit to its NumPy restatement
    Companion("libvghvideo.so", ["yuv_anonymize.hip", "yuv_pack.hip"], ANON_HEADERS + PLANE_HEADERS, "vgh_video.h", [], "build_video"),
]
# Libraries that hand the heads to the next network: built like a companion, before the core
DOWNSTREAM = [
    # head tensors (fixed-size normalised crops of every head): integer arithmetic, then float32 in a stated operation order, equal bit for bit to its NumPy restatement
    Companion("libvghcrop.so", ["head_tensors.hip"], HOST_HEADERS + ["head_crop_rules.h"], "vgh_crop.h", ["-ffp-contract=off"], "build_crop"),
]
# Libraries that show the result in the frame that goes on to an encoder: built like a companion, before the core
OVERLAY = [
    # on-screen display (bars, boxes, bitmap text in a frame's own YUV planes or an RGB image's bytes): integer arithmetic only, equal bit for bit to its NumPy restatement
    Companion("libvghosd.so", ["osd.hip"], HOST_HEADERS + ["osd_rules.h"] + PLANE_HEADERS, "vgh_osd.h", [], "build_osd"),
]
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-fno-gpu-rdc", "-Wno-unused-result", "-Wno-unused-value"]


def _hipcc() -> str:
    for c in (os.environ.get("HIPCC"), "/opt/rocm/bin/hipcc", "hipcc"):
        if c and (os.path.isabs(c) and os.path.exists(c) or not os.path.isabs(c)):
            return c
    raise RuntimeError("hipcc not found")


def _stale(lib: str, deps) -> bool:
    return not os.path.exists(lib) or any(os.path.getmtime(d) > os.path.getmtime(lib) for d in deps)


def _core_needs_build() -> bool:  # everything in csrc/ that no companion claims
    claimed = {f for c in COMPANIONS + APPLICATIONS + VIDEO + DOWNSTREAM + OVERLAY for f in c.sources + c.headers}
    return _stale(LIB, [os.path.join(CSRC, f) for f in os.listdir(CSRC) if f not in claimed] + [os.path.join(HERE, "..", "include", "vgh.h")])


def _needs_build(c: Companion) -> bool:
    return _stale(os.path.join(HERE, c.lib), [os.path.join(CSRC, f) for f in c.sources + c.headers] + [os.path.join(HERE, "..", "include", c.public)])


def needs_build() -> bool:
    return _core_needs_build() or any(_needs_build(c) for c in COMPANIONS + APPLICATIONS + VIDEO + DOWNSTREAM + OVERLAY)


LIB_EXP = os.path.join(HERE, "libvgh_exp.so")  # -DVGH_EXPERIMENTS build (work-skipping switches, env-var knobs): tools/ only


def build_lib(force: bool = False, verbose: bool = True, experiments: bool = False, variant_defines=None) -> str:
    if variant_defines:  # A/B builds of the PRODUCT code with one compile-time knob changed (no experiment switches): libvgh_var.so
        return _build(os.path.join(HERE, "libvgh_var.so"), [f"-D{d}" for d in variant_defines], "build_var", verbose)
    if experiments:
        return _build(LIB_EXP, ["-DVGH_EXPERIMENTS"], "build_exp", verbose)
    for c in COMPANIONS + APPLICATIONS + VIDEO + DOWNSTREAM + OVERLAY:
        if force or _needs_build(c):
            _build(os.path.join(HERE, c.lib), ["-fvisibility=hidden", *c.flags], c.objdir, verbose, c.sources)
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
