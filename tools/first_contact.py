#!/usr/bin/env python3
"""First contact with the REAL assets, in one command (r06).  None of them exists in this image: the released weights (hub download,
head_detector/detector.py:25-30), the licensed FLAME pickle (flame.py:18-24), an exported .onnx (README.md:23,199), cv2.  Whatever is supplied is checked; every
check prints PASS / FAIL / SKIPPED with the number behind it, and the exit code is the number of FAILs.

    python tools/first_contact.py [--model vgg_heads_l] [--trcd vgg_heads_l.trcd] [--onnx vgg_heads_l.onnx] [--pkl generic_model.pkl] [--images a.jpg b.jpg ...] [--cv2]

  1. --trcd / --onnx : load_weights -> weight_manifest_diff (every missing / unexpected / mis-shaped tensor; an .onnx also says whether it was read by name or by graph
                       position and which Conv nodes stayed unbound) -> build_program in every precision.
  2. --pkl           : FLAMELayer from the pickle; the reference's known-answer fixture (yolo_head_training/tests/1.json, committed as tests/golden/fixture_1json.npz):
                       its 413 parameters through vgh_flame_decode against its vertices_3d (the one full known answer the reference holds; 1e-4);
                       that head, 400 px across, through render_mesh (csrc/mesh_render.hip) with the pickle's own faces against the composition of Sim3DR calls, bit for bit.
  3. --cv2           : the letterbox kernel (csrc/letterbox.hip, OpenCV's 8-bit LANCZOS4 restated) against cv2.resize + copyMakeBorder on seeded images and on --images,
                       bit for bit (detector.py:40-52); the warp of get_aligned_heads (csrc/aligned.hip, OpenCV's 8-bit bilinear warpAffine restated) against
                       cv2.getRotationMatrix2D + cv2.warpAffine, bit for bit (utils.py:93-117); PredictionResult.draw (csrc/draw.hip, OpenCV's rectangle / polylines /
                       circle restated) for "full", "bbox", "landmarks" and "points" against the reference's own loop of cv2 calls (draw_utils.py), bit for bit, with
                       the time that loop takes for the same heads.  Also REPORTS (does not require) the largest byte difference between video.YUV420Frame.to_rgb
                       (bt601, limited range) and cv2.cvtColor(..., COLOR_YUV2RGB_NV12), and between video.YUV420Frame.from_rgb and cv2.cvtColor(..., COLOR_RGB2YUV_I420):
                       those parities are unpinned.
  4. --images + weights (+ --pkl): bf16 / fp16 / int8 / fp8 against the fp16x3 parity mode on those photographs -- dense boxes IoU, scores, the kept detections'
                       parameters and vertices; int8 / fp8 calibrated on the same photographs.
  5. pycocotools     : wherever that package is installed, detection_metrics.average_precision (csrc/detection_ap.hip) against COCOeval(..., 'bbox') itself on a seeded set
                       written the way the reference's evaluate_wider.py / evaluate_fddb.py write it: precision, recall, scores and the twelve stats, bit for bit.
  6. --images + weights + --pkl: HeadDetector.detect_sliced (csrc/slice_merge.hip) on those photographs: heads found plain (one letterboxed pass) against sliced
                       (overlapping tiles + the whole image, merged on the device), with the per-status candidate counts; its border and overlap defaults are untuned.
GPU needed for 2 - 6 (the library has no CPU path)."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

FAILS = []


def report(name, ok, detail=""):
    print(f"[{'PASS' if ok else 'FAIL'}] {name}: {detail}", flush=True)
    if not ok:
        FAILS.append(name)


def skipped(name, why):
    print(f"[SKIPPED] {name}: {why}", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="vgg_heads_l")
    ap.add_argument("--trcd")
    ap.add_argument("--onnx")
    ap.add_argument("--pkl")
    ap.add_argument("--images", nargs="*", default=[])
    ap.add_argument("--cv2", action="store_true")
    ap.add_argument("--image-size", type=int, default=640)
    args = ap.parse_args()
    from head_detector_amd import arch
    from head_detector_amd import detector as det

    # ---- 1. archives ----
    sd = None
    for label, path in (("trcd", args.trcd), ("onnx", args.onnx)):
        if not path:
            skipped(f"{label} ingest", "no file given")
            continue
        try:
            got = det.load_weights(path, args.model)
        except Exception as e:  # noqa: BLE001
            report(f"{label} ingest", False, f"{type(e).__name__}: {e}")
            continue
        diff = det.weight_manifest_diff(args.model, got)
        how = dict(det.LAST_LOAD_REPORT) if label == "onnx" else {}
        report(f"{label} manifest", not any(diff.values()), f"{len(got)} tensors; missing {diff['missing'][:6]} unexpected {diff['unexpected'][:6]} shape {diff['shape'][:4]}"
               + (f"; read {how.get('how')}, unbound Conv nodes {how.get('conv_nodes_unbound', how.get('not_weights', []))[:4]}" if how else ""))
        if not any(diff.values()):
            for prec in ("bf16", "fp16", "fp16x3", "fp32"):
                try:
                    arch.build_program(args.model, got, args.image_size, prec)
                    report(f"{label} lowers ({prec})", True, "op program built")
                except Exception as e:  # noqa: BLE001
                    report(f"{label} lowers ({prec})", False, f"{type(e).__name__}: {e}")
            sd = sd or got
    import torch

    gpu = torch.cuda.is_available()
    # ---- 2. FLAME pickle + the reference's known answer ----
    flame_model = None
    if args.pkl and gpu:
        from head_detector_amd.flame import FLAMELayer

        dev = torch.device("cuda", 0)
        try:
            fl = FLAMELayer(flame_path=args.pkl, device=dev, max_heads=256)
            flame_model = fl
            g = np.load(os.path.join(ROOT, "tests", "golden", "fixture_1json.npz"))
            p = torch.from_numpy(g["params"]).float()[None].to(dev)
            out = fl.decode(p)  # vertices in model space after pose, rotation and scale (flame.py:122-177)
            v3 = torch.as_tensor(out[0] if isinstance(out, (tuple, list)) else out).float().cpu().numpy().reshape(-1, 3)
            ref = g["vertices_3d"].astype(np.float64)
            err = float(np.abs(v3[: ref.shape[0]] - ref).max()) if v3.shape[0] >= ref.shape[0] else float("inf")
            report("1.json known answer through vgh_flame_decode", err < 1e-4, f"max |vertex - fixture| = {err:.3e} m over {ref.shape[0]} vertices (bar 1e-4)")
            # the shaded mesh (csrc/mesh_render.hip) with the REAL FLAME faces: the fixture's head scaled to 400 px, against the composition of Sim3DR calls
            # (tests/shade_ref.py: the reference's own C++ where oracle/_ref has it, its CPU restatement otherwise), bit for bit
            sys.path.insert(0, os.path.join(ROOT, "tests"))
            import shade_ref as sr
            from head_detector_amd import mesh_render

            faces = np.ascontiguousarray(fl.faces, dtype=np.int32)
            span = float(np.ptp(v3[:, :2], axis=0).max())
            head = ((v3 - v3.mean(axis=0)) * (400.0 / span) * np.array([1.0, -1.0, 1.0]) + np.array([256.0, 240.0, 0.0])).astype(np.float32)
            photo = np.random.default_rng(1).integers(0, 256, (480, 512, 3), dtype=np.uint8)
            got = mesh_render.render_mesh(photo, [sr.make_head(head)], faces)
            want = sr.render_mesh(photo, [head], faces, sr.live() is not None)
            nbad = int((got != want).any(axis=2).sum())
            report("render_mesh with the FLAME faces (bit for bit)", nbad == 0 and bool((got != photo).any()),
                   f"{faces.shape[0]} triangles, {int((got != photo).any(axis=2).sum())} painted pixels, {nbad} differing; against {'the reference library' if sr.live() is not None else 'tests/shade_ref.py'}")
        except Exception as e:  # noqa: BLE001
            report("FLAME pickle", False, f"{type(e).__name__}: {e}")
    else:
        skipped("1.json known answer", "needs --pkl and a GPU")
    # ---- 3. letterbox against cv2 ----
    if args.cv2 and gpu:
        try:
            import cv2
        except ImportError:
            cv2 = None
            report("letterbox vs cv2", False, "cv2 is not importable here")
        if cv2 is not None:
            from head_detector_amd.letterbox import letterbox

            dev = torch.device("cuda", 0)
            rng = np.random.default_rng(0)
            imgs = [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for h, w in ((480, 640), (1080, 1920), (333, 517), (640, 640), (97, 1201))]
            for pth in args.images:
                im = cv2.imread(pth)
                if im is not None:
                    imgs.append(cv2.cvtColor(im, cv2.COLOR_BGR2RGB))
            worst, nbad = 0, 0
            S = args.image_size
            for im in imgs:
                got = letterbox(im, S, dev)[0].cpu().numpy()[0]
                h, w = im.shape[:2]
                sc = S / max(h, w)
                if sc != 1.0:  # detector.py:40-52
                    rs = cv2.resize(im, (int(round(w * sc)), int(round(h * sc))), interpolation=cv2.INTER_LANCZOS4)
                else:
                    rs = im
                ph, pw = S - rs.shape[0], S - rs.shape[1]
                ref = cv2.copyMakeBorder(rs, 0, ph, 0, pw, cv2.BORDER_CONSTANT, value=127)
                d = np.abs(got.astype(np.int32) - ref.astype(np.int32))
                worst = max(worst, int(d.max()))
                nbad += int((d > 0).sum())
            report("letterbox vs cv2 (bit for bit)", worst == 0, f"{len(imgs)} images, max |diff| {worst}, {nbad} differing bytes")
            # video.YUV420Frame.to_rgb (the rule of include/vgh.h, bt601 limited range) against cv2.cvtColor(COLOR_YUV2RGB_NV12): REPORTED, not required to agree --
            # cv2 rounds its coefficients to another fixed-point precision, so a difference of a few least significant bits is expected
            from head_detector_amd.video import YUV420Frame

            yworst, ybad, ytotal = 0, 0, 0
            for h, w in ((480, 640), (1080, 1920), (2, 2)):
                surf = rng.integers(0, 256, (h * 3 // 2, w), dtype=np.uint8)
                got = YUV420Frame.from_nv12(torch.from_numpy(surf), h, w, matrix="bt601").to_rgb().numpy()
                d = np.abs(got.astype(np.int32) - cv2.cvtColor(surf, cv2.COLOR_YUV2RGB_NV12).astype(np.int32))
                yworst, ybad, ytotal = max(yworst, int(d.max())), ybad + int((d > 0).sum()), ytotal + d.size
            print(f"[REPORT] YUV420Frame.to_rgb (bt601, limited) vs cv2 COLOR_YUV2RGB_NV12 (parity unpinned): max |diff| {yworst}, {ybad} of {ytotal} bytes differ", flush=True)
            # video.YUV420Frame16.to_rgb (the deep rule of include/vgh.h, 10-bit P010, bt601 limited range): cv2.cvtColor converts 8-bit 4:2:0 only, so the
            # comparison is against cv2 on the frame's to_8bit() NV12 narrowing -- REPORTED, unpinned like the 8-bit rule; the two low sample bits that the
            # narrowing rounds away add up to one more least significant bit
            from head_detector_amd.video import YUV420Frame16

            dworst, dbad, dtotal = 0, 0, 0
            for h, w in ((480, 640), (1080, 1920), (2, 2)):
                words = rng.integers(0, 65536, (h * 3 // 2, w), dtype=np.uint16)  # 10 sample bits on top of 6 bits a decoder promises nothing about
                deep = YUV420Frame16.from_p010(torch.from_numpy(words.view(np.int16)), h, w, matrix="bt601")
                narrow = deep.to_8bit()
                surf = np.concatenate([narrow.y.numpy(), np.stack([narrow.u.numpy(), narrow.v.numpy()], axis=-1).reshape(h // 2, w)])
                d = np.abs(deep.to_rgb().numpy().astype(np.int32) - cv2.cvtColor(surf, cv2.COLOR_YUV2RGB_NV12).astype(np.int32))
                dworst, dbad, dtotal = max(dworst, int(d.max())), dbad + int((d > 0).sum()), dtotal + d.size
            print(f"[REPORT] YUV420Frame16.to_rgb (P010, 10 bits, bt601, limited) vs cv2 COLOR_YUV2RGB_NV12 on its to_8bit() frame (parity unpinned): max |diff| {dworst}, "
                  f"{dbad} of {dtotal} bytes differ", flush=True)
            # YUV420Frame.from_rgb (the packer of include/vgh_video.h, bt601 limited range) against cv2.cvtColor(COLOR_RGB2YUV_I420): REPORTED as well -- cv2 has
            # its own fixed-point coefficients and takes a block's chroma its own way
            pworst, pbad, ptotal = 0, 0, 0
            for h, w in ((480, 640), (1080, 1920), (2, 2)):
                im = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
                got = np.concatenate([p.cpu().numpy().reshape(-1) for p in YUV420Frame.from_rgb(im, "i420", "bt601").planes])
                d = np.abs(got.astype(np.int32) - cv2.cvtColor(im, cv2.COLOR_RGB2YUV_I420).reshape(-1).astype(np.int32))
                pworst, pbad, ptotal = max(pworst, int(d.max())), pbad + int((d > 0).sum()), ptotal + d.size
            print(f"[REPORT] YUV420Frame.from_rgb (bt601, limited, I420) vs cv2 COLOR_RGB2YUV_I420 (parity unpinned): max |diff| {pworst}, {pbad} of {ptotal} bytes differ", flush=True)
            # the warp of get_aligned_heads (csrc/aligned.hip, OpenCV's 8-bit bilinear warpAffine restated) against cv2.getRotationMatrix2D + cv2.warpAffine
            from head_detector_amd import aligned

            worst, nbad, mworst, nwarp = 0, 0, 0.0, 0
            for im in imgs:
                h, w = im.shape[:2]
                for angle in (0.0, 90.0, 17.3, -23.7, 181.0):
                    centre = (int(rng.integers(0, w)), int(rng.integers(0, h)))
                    mworst = max(mworst, float(np.abs(aligned.get_rotation_matrix_2d(centre, angle) - cv2.getRotationMatrix2D(centre, angle, 1.0)).max()))
                    m, bounds = aligned.get_rotation_mat(im, centre, angle)
                    got = aligned.warp_crops(im, [(m, (0, 0, bounds[0], bounds[1]))])[0]
                    d = np.abs(got.astype(np.int32) - cv2.warpAffine(im, m, bounds, flags=cv2.INTER_LINEAR).astype(np.int32))
                    worst = max(worst, int(d.max()))
                    nbad += int((d > 0).sum())
                    nwarp += 1
            report("aligned-head warp vs cv2.warpAffine (bit for bit)", worst == 0 and mworst <= 1e-12,
                   f"{nwarp} warps, max |diff| {worst}, {nbad} differing bytes, rotation matrix max |diff| {mworst:.1e}")
            # PredictionResult.draw (csrc/draw.hip) against the reference's loop of cv2 calls for the same heads (draw_utils.py:15-42,87-90, detection_result.py:12-18,45-51)
            import time
            import types

            from head_detector_amd import draw
            from head_detector_amd.head_info import Bbox

            V, cols = 5023, 71
            k = np.arange(V)
            row, col = k // cols, np.where((k // cols) % 2 == 1, cols - 1 - k % cols, k % cols)
            start = rng.integers(0, V - cols - 1, 4816)
            tri = np.stack([start, start + 1, start + cols + rng.integers(-1, 2, 4816)], axis=1).astype(np.int32)
            tri[-40:] = rng.integers(0, V, (40, 3))  # a few edges as long as the head
            hidx, fidx = np.sort(rng.choice(V, 2470, replace=False)), np.sort(rng.choice(V, 2094, replace=False))
            nbad, ndraw, t_cv2, t_gpu = 0, 0, 0.0, 0.0
            for im in imgs[:4]:
                h, w = im.shape[:2]
                heads = []
                for _ in range(6):
                    size, cx, cy = rng.uniform(0.1, 0.6) * min(h, w), rng.uniform(-0.1 * w, 1.1 * w), rng.uniform(-0.1 * h, 1.1 * h)
                    xyz = np.stack([cx + size * ((col + rng.uniform(-0.4, 0.4, V)) / (cols - 1) - 0.5), cy + 1.2 * size * ((row + rng.uniform(-0.4, 0.4, V)) / (cols - 1) - 0.5),
                                    np.zeros(V)], axis=1).astype(np.float32)
                    x0, y0, x1, y1 = (int(q) for q in (xyz[:, 0].min(), xyz[:, 1].min(), xyz[:, 0].max(), xyz[:, 1].max()))
                    heads.append(types.SimpleNamespace(vertices_3d=xyz, bbox=Bbox(x0, y0, x1 - x0, y1 - y0)))
                radius = max(1, int(min(h, w) * 0.001))
                for method in ("full", "bbox", "landmarks", "points"):
                    t0 = time.perf_counter()
                    got = draw.draw_heads(im, heads, method, triangles=tri, head_indices=hidx, face_indices=fidx)
                    t1 = time.perf_counter()
                    ref = im.copy()
                    for head in heads:  # the reference's loop, call for call
                        pv = head.vertices_3d[:, :2]
                        if method in ("full", "bbox"):
                            x, y, bw, bh = head.bbox
                            cv2.rectangle(ref, (x, y), (x + bw, y + bh), (255, 0, 0), 2)
                        if method in ("full", "landmarks"):
                            for t in tri:
                                cv2.polylines(ref, [np.array([(pv[i][0], pv[i][1]) for i in t], np.int32).reshape((-1, 1, 2))], isClosed=True, color=(0, 0, 255), thickness=1)
                        for pt in np.take(pv, hidx if method != "points" else fidx, axis=0) if method != "bbox" else []:
                            cv2.circle(ref, (int(pt[0]), int(pt[1])), radius, (255, 255, 255), -1)
                    t2 = time.perf_counter()
                    nbad += int((got != ref).any(axis=2).sum())
                    ndraw += 1
                    t_gpu, t_cv2 = t_gpu + (t1 - t0), t_cv2 + (t2 - t1)
            report("draw vs the reference's cv2 loop (bit for bit)", nbad == 0, f"{ndraw} pictures of 6 heads, {nbad} differing pixels; the cv2 loop took {t_cv2:.2f} s, "
                   f"draw() with upload and download {t_gpu:.2f} s")
    else:
        skipped("letterbox, warp and draw vs cv2", "needs --cv2 and a GPU")
    # ---- 4. throughput modes against the parity mode on real photographs ----
    if gpu and sd is not None and args.images:
        from head_detector_amd.engine import VGHeadsEngine
        from head_detector_amd.letterbox import letterbox

        dev = torch.device("cuda", 0)
        S = args.image_size
        ims = []
        for pth in args.images:
            from PIL import Image

            ims.append(letterbox(np.array(Image.open(pth).convert("RGB")), S, dev)[0])
        x = torch.cat(ims).contiguous()
        B = x.shape[0]
        ref_eng = VGHeadsEngine(args.model, state_dict=sd, image_size=S, max_batch=B, precision="fp16x3")
        rb, rs_, rf = [t.clone() for t in ref_eng.model(x)]
        dense_b, dense_s = ref_eng.boxes_all[:B].clone(), ref_eng.scores_all[:B].clone()
        ref_eng.close()

        def iou(a, b):
            lt, rb2 = torch.maximum(a[..., :2], b[..., :2]), torch.minimum(a[..., 2:], b[..., 2:])
            wh = (rb2 - lt).clamp(min=0)
            inter = wh[..., 0] * wh[..., 1]
            return inter / ((a[..., 2] - a[..., 0]) * (a[..., 3] - a[..., 1]) + (b[..., 2] - b[..., 0]) * (b[..., 3] - b[..., 1]) - inter)

        for prec in ("bf16", "fp16", "int8", "fp8"):
            eng = VGHeadsEngine(args.model, state_dict=sd, image_size=S, max_batch=B, precision=prec, calib_images=x if prec in ("int8", "fp8") else None)
            eng.model(x)
            conf = dense_s > 0.5  # the anchors the parity mode would keep at the reference's default threshold
            i_min = float(iou(eng.boxes_all[:B][conf], dense_b[conf]).min()) if bool(conf.any()) else float("nan")
            s_err = float((eng.scores_all[:B] - dense_s).abs().max())
            eng.close()
            print(f"[INFO] {prec} vs fp16x3 on {B} photographs: IoU min over the {int(conf.sum())} anchors with score > 0.5 = {i_min:.5f}; max |score diff| {s_err:.2e}", flush=True)
    else:
        skipped("precision modes on photographs", "needs weights, --images and a GPU")
    # ---- 6. sliced detection on real photographs: heads found plain against sliced ----
    weights = args.trcd or args.onnx
    if gpu and sd is not None and args.images and args.pkl:
        try:
            hd = det.HeadDetector(args.model, args.image_size, weights=weights, flame_path=args.pkl, max_batch=8)
            for pth in args.images:
                plain = hd(pth)
                cut, info = hd.detect_sliced(pth, return_info=True)
                print(f"[INFO] {pth}: {len(plain.heads)} heads plain, {len(cut.heads)} sliced ({info.plan.n_tiles} tiles; candidates {info.status_counts}; "
                      f"{int((info.head_tile != 0).sum())} of the sliced heads come from a tile, not from the whole image)", flush=True)
            report("detect_sliced on photographs", True, f"{len(args.images)} photographs; border and overlap are untuned defaults")
        except Exception as e:  # noqa: BLE001
            report("detect_sliced on photographs", False, f"{type(e).__name__}: {e}")
    else:
        skipped("heads found plain vs sliced", "needs weights, --pkl, --images and a GPU")
    # ---- 5. detection AP against pycocotools itself ----
    try:
        from pycocotools.coco import COCO
        from pycocotools.cocoeval import COCOeval
    except ImportError:
        COCO = None
    if COCO is None or not gpu:
        skipped("average_precision vs pycocotools", "needs pycocotools and a GPU")
    else:
        import contextlib
        import io

        from head_detector_amd import detection_metrics as dm

        rng = np.random.default_rng(7)
        gts, dts = [], []
        for ng in (0, 1, 3, 17, 64, 65, 130, 2, 40, 9):
            side = rng.choice([6, 12, 24, 32, 48, 96, 160], ng)
            gt = np.stack([rng.integers(0, 600, ng), rng.integers(0, 400, ng), side, side], axis=1).reshape(ng, 4)
            found = gt[rng.random(ng) < 0.8]  # integer boxes, as parse_predictions makes them
            found = found + rng.integers(-2, 3, found.shape)
            false = np.stack([rng.integers(0, 600, 30), rng.integers(0, 400, 30), rng.integers(1, 90, 30), rng.integers(1, 90, 30)], axis=1)
            boxes = np.concatenate([found, false]).astype(np.float64)
            boxes[:, 2:] = np.maximum(boxes[:, 2:], 1)
            gts.append(gt.astype(np.float64))
            dts.append(np.concatenate([boxes, rng.integers(1, 100, (len(boxes), 1)) / 100.0], axis=1))
        gt_json = {"images": [{"id": i + 1} for i in range(len(gts))], "categories": [{"id": 1, "name": "object"}], "annotations": []}
        for i, gt in enumerate(gts):
            for x, y, w, h in gt.tolist():
                gt_json["annotations"].append({"id": len(gt_json["annotations"]) + 1, "image_id": i + 1, "category_id": 1, "bbox": [x, y, w, h], "area": w * h, "iscrowd": 0})
        dt_json = [{"image_id": i + 1, "category_id": 1, "bbox": row[:4], "score": row[4]} for i, dt in enumerate(dts) for row in dt.tolist()]
        try:
            with contextlib.redirect_stdout(io.StringIO()):
                coco_gt = COCO()
                coco_gt.dataset = gt_json
                coco_gt.createIndex()
                coco_eval = COCOeval(coco_gt, coco_gt.loadRes(dt_json), "bbox")
                coco_eval.evaluate()
                coco_eval.accumulate()
                coco_eval.summarize()
            got = dm.average_precision(dts, gts)
            want_p, want_r, want_s = (coco_eval.eval[k] for k in ("precision", "recall", "scores"))
            same = (np.array_equal(got.precision, want_p[:, :, 0]), np.array_equal(got.recall, want_r[:, 0]), np.array_equal(got.scores, want_s[:, :, 0]),
                    np.array_equal(got.stats, coco_eval.stats))
            report("average_precision vs pycocotools (bit for bit)", all(same), f"precision, recall, scores, stats equal: {same}; AP {got.ap:.6f} against {coco_eval.stats[0]:.6f}")
        except Exception as e:  # noqa: BLE001
            report("average_precision vs pycocotools", False, f"{type(e).__name__}: {e}")
    print(f"{len(FAILS)} FAIL(s): {FAILS}")
    return len(FAILS)


if __name__ == "__main__":
    sys.exit(main())
