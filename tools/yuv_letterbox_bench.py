"""NV12 video frames into the detector: the fused route (VGH_IMG_YUV420_RAW: every tap converted inside the batched letterbox) against the two-step route it
replaces (an RGB copy of every frame, then VGH_IMG_U8_RAW), on decoder-shaped surfaces already on the device.

    fused:     engine.forward_candidates(frames)                                   one staging upload + one letterbox launch per arena chunk, then the network
    two-step:  [f.to_rgb() for f in frames] -> engine.forward_candidates(rgb)      a full-resolution RGB copy per frame, then the same with the RGB kernel
    rgb-only:  engine.forward_candidates(rgb) on copies made beforehand            the two-step route without its conversion: what the RGB letterbox + network cost

64 seeded NV12 surfaces (pitch aligned to 256 bytes, chroma plane at pitch * height aligned to 16) at 1920 x 1080 and at 3840 x 2160.  HIP events on the caller's
stream bracket each call; the routes are alternated in one process, warm, in two rounds, and the medians of the second round are reported.  The network is the
same work in all three, so differences between the calls are differences of the letterbox stage (and, for two-step, of the conversion, bracketed on its own too).
``to_rgb()`` is torch integer ops (several passes over the frame), not a tuned conversion kernel: the bytes an IDEAL conversion pass would move are printed beside
it, computed from shapes, so that the reader can put a bandwidth-bound figure in its place.  The canvases of the routes are compared byte for byte first.

    python tools/yuv_letterbox_bench.py [--variant vgg_heads_m] [--batch 64] [--iters 20] [--warmup 3] [--out profiles/yuv_letterbox.txt]

``--deep``: 10-bit P010 surfaces (VGH_IMG_YUV420P16_RAW, 16-bit words with the sample in the top bits and random bits below) against three baselines that exist
without that format, measured the same way and written to profiles/yuv16_letterbox.txt:

    deep:      engine.forward_candidates(p010 frames)                               the deep fetch: two bytes per sample, shift and mask per tap
    nv12:      engine.forward_candidates(the same pictures narrowed to NV12 beforehand)    VGH_IMG_YUV420_RAW: what the 8-bit fetch costs on these pictures
    rgb:       engine.forward_candidates(RGB copies made beforehand)                VGH_IMG_U8_RAW
    narrow:    [f.to_8bit() for f in frames] -> engine.forward_candidates(nv12)     the route a user has without the format (torch passes, not a tuned kernel)
"""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from head_detector_amd.engine import VGHeadsEngine  # noqa: E402
from head_detector_amd.letterbox import axis_tables, geometry  # noqa: E402
from head_detector_amd.video import YUV420Frame, YUV420Frame16  # noqa: E402

SIZES = [(1080, 1920), (2160, 3840)]  # (h, w)


def touched(src, dst):
    """The source coordinates of one axis that the 8 taps of the resize touch (each once)."""
    out = set()
    for o in axis_tables(src, dst)[0]:
        out.update(min(max(int(o) - 3 + k, 0), src - 1) for k in range(8))
    return out


def bytes_moved(h, w, S):
    """Bytes per frame, from shapes: what each route's kernels must read and write at the least."""
    nh, nw, _, _, _ = geometry(h, w, S)
    rows, cols = touched(h, nh), touched(w, nw)
    canvas = S * S * 3
    luma = len(rows) * len(cols)
    chroma = 2 * len({r >> 1 for r in rows}) * len({c >> 1 for c in cols})
    return {"fused_read": luma + chroma, "fused_write": canvas, "convert_read": h * w + 2 * ((h + 1) // 2) * ((w + 1) // 2), "convert_write": 3 * h * w,
            "rgb_letterbox_read": 3 * luma, "rgb_letterbox_write": canvas}


def deep_surfaces(h, w, B, dev, seed):
    """P010 as a hardware decoder lays it out: rows of 16-bit words, pitch aligned to 256 bytes, luma height aligned to 16; every word random (10 sample bits on top
    of 6 bits of garbage)."""
    pitch, rows = (2 * w + 255) // 256 * 256, (h + 15) // 16 * 16
    gen = torch.Generator(device=dev).manual_seed(seed)
    out = []
    for _ in range(B):
        buf = torch.randint(0, 256, (pitch * rows + pitch * ((h + 1) // 2),), dtype=torch.uint8, device=dev, generator=gen)
        out.append(YUV420Frame16.from_p010(buf, h, w, pitch=pitch, uv_offset=pitch * rows))
    return out


def main_deep(a):
    dev = torch.device("cuda", 0)
    S, B = a.size, a.batch
    eng = VGHeadsEngine(a.variant, image_size=S, max_batch=B, seed=1)
    cur = torch.cuda.current_stream(dev)
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
    lines = [f"VGH_IMG_YUV420P16_RAW (P010, 10 bits) vs VGH_IMG_YUV420_RAW, VGH_IMG_U8_RAW and to_8bit() + VGH_IMG_YUV420_RAW -- tools/yuv_letterbox_bench.py --deep, "
             f"{a.variant} bf16, batch {B}, S = {S}, arena_batch {eng.arena_batch}, 1 x MI355X",
             f"HIP-event medians over {a.iters} calls (second of two alternated rounds, {a.warmup} warm-up calls each); ms per call of {B} frames",
             "call = letterbox stage + network + candidate stages (the network part is the same work in every route)", ""]
    for h, w in SIZES:
        frames = deep_surfaces(h, w, B, dev, seed=h)
        nv12 = [f.to_8bit() for f in frames]  # the same pictures, narrowed beforehand
        kept = [f.to_rgb() for f in frames]

        def timed(images, before=None):
            def fn():
                ev[0].record(cur)
                batch = before() if before else images
                ev[1].record(cur)
                eng.forward_candidates(batch)
                eng.join()  # the caller's stream waits for the engine's: the event below then closes the call
                ev[2].record(cur)
            return fn

        routes = (("deep", timed(frames)), ("nv12", timed(nv12)), ("rgb", timed(kept)), ("narrow", timed(None, lambda: [f.to_8bit() for f in frames])))

        def canvas_of(fn):
            fn()
            eng.join()
            torch.cuda.synchronize()
            return eng.raw_canvas().clone()

        same = bool(torch.equal(canvas_of(routes[0][1]), canvas_of(routes[2][1])))  # (the last arena chunk's canvas; tests/test_gpu_yuv16.py pins the equality)
        med = {}
        for name, fn in routes * 2:
            for _ in range(a.warmup):
                fn()
            eng.join()
            torch.cuda.synchronize()
            whole, stage = [], []
            for _ in range(a.iters):
                fn()
                eng.join()
                torch.cuda.synchronize()
                whole.append(ev[0].elapsed_time(ev[2]))
                stage.append(ev[0].elapsed_time(ev[1]))
            med[name] = (float(np.median(whole)), float(np.min(whole)), float(np.max(whole)))
            if name == "narrow":
                med["to_8bit"] = (float(np.median(stage)), float(np.min(stage)), float(np.max(stage)))
        by = bytes_moved(h, w, S)
        mb = lambda k, per=1: by[k] * per * B / 1e6  # noqa: E731
        surf = frames[0].y_pitch * 2 * ((h + 15) // 16 * 16 + (h + 1) // 2)
        lines += [f"{w} x {h} P010 ({B} frames, {B * surf / 1e6:.0f} MB of surfaces); canvas of the deep route identical to the RGB route's: {same}",
                  *(f"  {name:<34s} median {med[key][0]:8.3f}   min {med[key][1]:8.3f}   max {med[key][2]:8.3f}" for name, key in
                    (("deep call (format 4)", "deep"), ("nv12 call (format 3, narrowed before)", "nv12"), ("rgb call (format 2, converted before)", "rgb"),
                     ("narrow call (to_8bit() + format 3)", "narrow"), ("  of which to_8bit() x " + str(B), "to_8bit"))),
                  f"  deep - nv12: {med['deep'][0] - med['nv12'][0]:+.3f} ms (the 16-bit fetch against the 8-bit fetch);  deep - rgb: {med['deep'][0] - med['rgb'][0]:+.3f} ms;  "
                  f"narrow - deep: {med['narrow'][0] - med['deep'][0]:+.3f} ms",
                  f"  bytes from shapes, per call: the deep letterbox must read at least {mb('fused_read', 2):.1f} MB (2 bytes per touched sample) + write {mb('fused_write'):.1f} MB;  "
                  f"the 8-bit letterbox reads {mb('fused_read'):.1f} MB;  an ideal narrowing pass reads {mb('convert_read', 2):.1f} MB + writes {mb('convert_read'):.1f} MB", ""]
        del frames, nv12, kept, routes
        torch.cuda.empty_cache()
    text = "\n".join(lines)
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)
    eng.close()


def surfaces(h, w, B, dev, seed):
    pitch, rows = (w + 255) // 256 * 256, (h + 15) // 16 * 16
    gen = torch.Generator(device=dev).manual_seed(seed)
    out = []
    for _ in range(B):
        buf = torch.randint(0, 256, (pitch * rows + pitch * ((h + 1) // 2),), dtype=torch.uint8, device=dev, generator=gen)
        out.append(YUV420Frame.from_nv12(buf, h, w, pitch=pitch, uv_offset=pitch * rows))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--variant", default="vgg_heads_m")
    ap.add_argument("--size", type=int, default=640)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--deep", action="store_true", help="10-bit P010 surfaces (VGH_IMG_YUV420P16_RAW) against the 8-bit, the RGB and the to_8bit() routes")
    ap.add_argument("--out", default=None, help="default: profiles/yuv_letterbox.txt, with --deep profiles/yuv16_letterbox.txt")
    a = ap.parse_args()
    if a.out is None:
        a.out = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "yuv16_letterbox.txt" if a.deep else "yuv_letterbox.txt")
    if not torch.cuda.is_available():
        raise SystemExit("yuv_letterbox_bench: needs the MI355X")
    if a.deep:
        return main_deep(a)
    dev = torch.device("cuda", 0)
    S, B = a.size, a.batch
    eng = VGHeadsEngine(a.variant, image_size=S, max_batch=B, seed=1)
    cur = torch.cuda.current_stream(dev)
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
    lines = [f"VGH_IMG_YUV420_RAW vs to_rgb() + VGH_IMG_U8_RAW -- tools/yuv_letterbox_bench.py, {a.variant} bf16, batch {B}, S = {S}, arena_batch {eng.arena_batch}, 1 x MI355X",
             f"HIP-event medians over {a.iters} calls (second of two alternated rounds, {a.warmup} warm-up calls each); ms per call of {B} frames",
             "call = letterbox stage + network + candidate stages (the network part is the same work in every route)", ""]
    for h, w in SIZES:
        frames = surfaces(h, w, B, dev, seed=h)
        kept = [f.to_rgb() for f in frames]

        def fused():
            ev[0].record(cur)
            eng.forward_candidates(frames)
            eng.join()  # the caller's stream waits for the engine's: the event below then closes the call
            ev[2].record(cur)

        def two_step():
            ev[0].record(cur)
            rgb = [f.to_rgb() for f in frames]
            ev[1].record(cur)
            eng.forward_candidates(rgb)
            eng.join()  # the caller's stream waits for the engine's: the event below then closes the call
            ev[2].record(cur)

        def rgb_only():
            ev[0].record(cur)
            eng.forward_candidates(kept)
            eng.join()  # the caller's stream waits for the engine's: the event below then closes the call
            ev[2].record(cur)

        def canvas_of(fn):
            fn()
            eng.join()
            torch.cuda.synchronize()
            return eng.raw_canvas().clone()

        same = bool(torch.equal(canvas_of(fused), canvas_of(two_step)))  # (the last arena chunk's canvas; tests/test_gpu_yuv.py pins the equality)
        med = {}
        for name, fn in (("fused", fused), ("two_step", two_step), ("rgb_only", rgb_only)) * 2:
            for _ in range(a.warmup):
                fn()
            eng.join()
            torch.cuda.synchronize()
            whole, stage = [], []
            for _ in range(a.iters):
                fn()
                eng.join()
                torch.cuda.synchronize()
                whole.append(ev[0].elapsed_time(ev[2]))
                if name == "two_step":
                    stage.append(ev[0].elapsed_time(ev[1]))
            med[name] = (float(np.median(whole)), float(np.min(whole)), float(np.max(whole)))
            if stage:
                med["convert"] = (float(np.median(stage)), float(np.min(stage)), float(np.max(stage)))
        by = bytes_moved(h, w, S)
        mb = lambda k: by[k] * B / 1e6  # noqa: E731
        lines += [f"{w} x {h} NV12 ({B} frames, {B * (frames[0].y_pitch * ((h + 15) // 16 * 16 + (h + 1) // 2)) / 1e6:.0f} MB of surfaces); canvases identical: {same}",
                  *(f"  {name:<28s} median {med[key][0]:8.3f}   min {med[key][1]:8.3f}   max {med[key][2]:8.3f}" for name, key in
                    (("fused call", "fused"), ("two-step call", "two_step"), ("  of which to_rgb() x " + str(B), "convert"), ("rgb-only call (no conversion)", "rgb_only"))),
                  f"  fused - rgb-only: {med['fused'][0] - med['rgb_only'][0]:+.3f} ms (the conversion inside the fetch against the RGB fetch);  two-step - fused: "
                  f"{med['two_step'][0] - med['fused'][0]:+.3f} ms",
                  f"  bytes from shapes, per call: fused letterbox reads {mb('fused_read'):.1f} MB + writes {mb('fused_write'):.1f} MB;  an ideal conversion pass reads "
                  f"{mb('convert_read'):.1f} MB + writes {mb('convert_write'):.1f} MB, the RGB letterbox then reads {mb('rgb_letterbox_read'):.1f} MB + writes "
                  f"{mb('rgb_letterbox_write'):.1f} MB", ""]
        del frames, kept
        torch.cuda.empty_cache()
    text = "\n".join(lines)
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)
    eng.close()


if __name__ == "__main__":
    main()
