"""Head textures on a 12 MP photograph (uint8, on the device) with 1, 16 and 100 heads whose vertices are already on the device: texture.unwrap_heads into
256 x 256 atlases (bilinear) and texture.render_texture of those atlases back onto the photograph (bilinear, both occlusion modes), beside the reference's
own C++ on this machine's CPU where oracle/_ref holds it (the prebuilt library only: nothing is compiled here).

    launch    HIP events around vghtex_render_texture: the fill of depth / triangle / head, the ONE staging upload (both topologies, tile lists) and the
              kernels (fill_kernel, boxes_kernel, tiles_kernel).
    call_dev  the whole Python call (to_host=False): allocating the outputs, the per-head bounds (one reduction on the device and its 4 n floats back),
              checks, launch; for the wrap also the float32 copy of the 12 MP background.  Host clock around work that ends in a device synchronise.
    cpu       `_render_texture_core` called once per head through ctypes, single-threaded, on float32 copies made beforehand: the unwrap into n atlases,
              and the wrap with ONE depth buffer for all heads (the composition of occlusion="depth"; "order" would add a 48 MB depth fill per head).

Medians over --iters after --warmup; the head counts are measured twice, alternating, and the second round is reported.  The meshes are closed
ellipsoids of FLAME's size (5 002 vertices, 10 000 triangles), 100 .. 300 px across; the UV layout is texture.cylindrical_uv of the unit ellipsoid.

    python tools/texture_bench.py [--iters 20] [--warmup 3] [--heads 1,16,100] [--size 256] [--out profiles/texture.txt]
"""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import shade_ref as sr  # noqa: E402  (the ellipsoid generator of the tests)
import texture_ref as tr  # noqa: E402  (the reference's symbol and the atlas positions)

from head_detector_amd import _lib_tex, texture  # noqa: E402

H, W = 3000, 4000


class Timed:
    """Brackets one library call with events without changing the product's code path."""

    def __init__(self, lib, name, ev0, ev1, stream):
        self._lib, self._name, self._ev, self._stream = lib, name, (ev0, ev1), stream

    def __getattr__(self, name):
        fn = getattr(self._lib, name)
        if name != self._name:
            return fn

        def timed(*args):
            self._ev[0].record(self._stream)
            rc = fn(*args)
            self._ev[1].record(self._stream)
            return rc

        return timed


def cpu_reference():
    """``_render_texture_core`` of the prebuilt oracle/_ref library, or None."""
    path = os.path.join(ROOT, "oracle", "_ref", "libsim3dr_ref.so")
    if not os.path.exists(path):
        return None
    fn = getattr(ctypes.CDLL(path), tr.SYMBOL)
    fn.argtypes, fn.restype = [ctypes.c_void_p] * 7 + [ctypes.c_int] * 10, None
    return fn


def cpu_times(fn, image_f32, verts, tri, atlas, th, tw, textures):
    """-> (unwrap ms, wrap ms) of one pass over all heads."""
    n, V = verts.shape[:2]
    C = image_f32.shape[2]
    out = np.zeros((n, th, tw, C), np.float32)
    depth = np.full((n, th, tw), -1e8, np.float32)
    t0 = time.perf_counter()
    for i in range(n):
        fn(out[i].ctypes.data, atlas.ctypes.data, tri.ctypes.data, image_f32.ctypes.data, verts[i].ctypes.data, tri.ctypes.data, depth[i].ctypes.data, V, V, tri.shape[0], th, tw, C,
           H, W, C, 1)
    t1 = time.perf_counter()
    canvas, zb = image_f32.copy(), np.full((H, W), -1e8, np.float32)
    flipped = verts * np.float32([1, 1, -1])
    t2 = time.perf_counter()
    for i in range(n):
        fn(canvas.ctypes.data, flipped[i].ctypes.data, tri.ctypes.data, textures[i].ctypes.data, atlas.ctypes.data, tri.ctypes.data, zb.ctypes.data, V, V, tri.shape[0], H, W, C,
           th, tw, C, 1)
    t3 = time.perf_counter()
    return (t1 - t0) * 1e3, (t3 - t2) * 1e3, out, canvas


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--heads", default="1,16,100", help="head counts, comma separated")
    ap.add_argument("--size", type=int, default=256, help="side of the square atlas")
    ap.add_argument("--no-cpu", action="store_true", help="leave the reference's C++ out")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("texture_bench: needs the MI355X")
    dev = torch.device("cuda", 0)
    image = np.random.default_rng(0).integers(0, 256, (H, W, 3), dtype=np.uint8)
    image_dev = torch.from_numpy(image).to(dev)
    unit, faces = sr.ellipsoid()
    uv, keep = texture.cylindrical_uv(unit[:, [0, 2, 1]], faces)  # the ellipsoid's poles on the vertical axis
    tri = np.ascontiguousarray(faces[keep])
    th = tw = a.size
    atlas = tr.atlas_vertices(uv, th, tw)
    cases = {n: sr.ellipsoid_heads(np.random.default_rng(n), n, H, W, 100.0, 300.0, unit, spread=0.95) for n in (int(v) for v in a.heads.split(","))}
    cur = torch.cuda.current_stream(dev)
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    lib = _lib_tex.load()
    timed = Timed(lib, "vghtex_render_texture", ev[0], ev[1], cur)
    fn = None if a.no_cpu else cpu_reference()
    image_f32 = image.astype(np.float32) if fn is not None else None
    lines = []
    for rnd in range(2):
        for n, verts in cases.items():
            verts_dev = torch.from_numpy(verts).to(dev)
            jobs = {"unwrap": lambda: texture.unwrap_heads(image_dev, verts_dev, tri, uv, (th, tw), to_host=False)}
            tex = jobs["unwrap"]()
            for mode in ("order", "depth"):
                jobs[f"wrap_{mode}"] = lambda mode=mode: texture.render_texture(verts_dev, tri, tex.texture, atlas, H, W, image=image_dev, occlusion=mode, z_sign=-1.0, to_host=False)
            t_launch, t_dev = {k: [] for k in jobs}, {k: [] for k in jobs}
            res = {}
            for it in range(a.warmup + a.iters):
                for key, job in jobs.items():
                    t1 = time.perf_counter()
                    texture._lib_tex.load = lambda: timed
                    try:
                        res[key] = job()
                        torch.cuda.synchronize()
                        t2 = time.perf_counter()
                    finally:
                        texture._lib_tex.load = lambda: lib
                    if it >= a.warmup:
                        t_launch[key].append(ev[0].elapsed_time(ev[1])), t_dev[key].append((t2 - t1) * 1e3)
            med = {"heads": n, "triangles": n * tri.shape[0], "atlas": a.size, "texels_written": int(tex.written.sum()),
                   "pixels_painted": int((res["wrap_order"] != image_dev).any(dim=-1).sum())}
            for key in jobs:
                med[f"{key}_launch_ms"] = float(np.median(t_launch[key]))
                med[f"{key}_call_dev_ms"] = float(np.median(t_dev[key]))
            if fn is not None and rnd == 1:
                cpu_unwrap, cpu_wrap, cpu_tex, cpu_canvas = cpu_times(fn, image_f32, verts, tri, atlas, th, tw, tex.texture.cpu().numpy())
                med.update(cpu_unwrap_ms=cpu_unwrap, cpu_wrap_depth_ms=cpu_wrap, cpu_over_unwrap_launch=cpu_unwrap / med["unwrap_launch_ms"],
                           cpu_over_wrap_depth_launch=cpu_wrap / med["wrap_depth_launch_ms"],
                           equal_to_cpu=bool(np.array_equal(cpu_tex, tex.texture.cpu().numpy()) and np.array_equal(cpu_canvas, res["wrap_depth"].cpu().numpy())))
            if rnd == 1:
                lines.append(json.dumps(med))
                print(lines[-1], flush=True)
            del res, tex, jobs
    if a.out:
        with open(a.out, "w") as f:
            f.write(f"# tools/texture_bench.py --iters {a.iters} --warmup {a.warmup} --size {a.size}: unwrap_heads / render_texture (to_host=False) on a {H} x {W} uint8 photograph, "
                    "vertices on the device; ms are medians; launch = fill + staging upload + boxes and tiles kernels (HIP events); cpu = the reference's C++, one thread\n")
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
