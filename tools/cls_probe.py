"""Times the orientation classifier on the bench's step: 64 A4@200DPI pages (bench.make_pages, seed 2024) -> boxes (text path) ->
cls_crop + cls_forward + the oriented recognition crop, and the plain recognition crop beside it.  HIP events around each stage,
median of --reps; the per-layer launches (option time_convs) with their algorithmic FLOP / bytes.  One JSON line; needs an MI355X.

    python tools/cls_probe.py [--reps 20]"""
import argparse
import json
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
for p in (ROOT, ROOT / "ocr-system_amd"):
    sys.path.insert(0, str(p))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--pages", type=int, default=64)
    args = ap.parse_args()
    import numpy as np
    import torch
    import bench
    from lumina_ocr import arch
    from lumina_ocr.engine import Engine
    from lumina_ocr.pipeline import OcrPipeline

    eng = Engine(0)
    eng.load_det(arch.make_det_weights(1234))
    eng.load_rec(arch.make_rec_weights(4321, code_path=True))
    eng.load_cls(arch.make_cls_weights(2718, orientation_path=True))
    pipe = OcrPipeline(eng, post=arch.TEXT_PATH_POST)
    pages = bench.make_pages(torch, args.pages, 2024, torch.device("cuda", 0))
    processed, boxes, _, counts = pipe.submit_detect(pages)
    counts_h = counts.cpu().numpy()
    cap = boxes.shape[1]
    page_h = np.repeat(np.arange(len(counts_h)), counts_h)
    slot_h = np.arange(len(page_h)) - np.repeat(np.cumsum(counts_h) - counts_h, counts_h)
    quads = boxes.view(-1, 8).index_select(0, torch.from_numpy(page_h * cap + slot_h).cuda()).contiguous()
    page_idx = torch.from_numpy(page_h.astype(np.int32)).cuda()

    def stage(fn):
        times = []
        for i in range(args.reps + 3):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            out = fn()
            e1.record()
            torch.cuda.synchronize()
            if i >= 3:
                times.append(e0.elapsed_time(e1))
        return float(np.median(times)), out

    t_crop, (ccrops, cw) = stage(lambda: eng.cls_crop(processed, quads, page_idx))
    t_fwd, (label, score, flip) = stage(lambda: eng.cls_forward(ccrops, cw))
    t_ocrop, _ = stage(lambda: eng.rec_crop(processed, quads, page_idx, flip=flip))
    t_rcrop, _ = stage(lambda: eng.rec_crop(processed, quads, page_idx))
    eng.set_option("time_convs", 1)
    eng.cls_forward(ccrops, cw)
    layers = [dict(layer=n, kernel=k, ms=round(ms, 4), gflop=round(gf, 3), mb=round(mb, 2)) for n, k, ms, gf, mb in eng.conv_timing_detail()]
    eng.set_option("time_convs", 0)
    n = len(page_h)
    print(json.dumps(dict(pages=args.pages, crops=n, flagged=int(flip.sum()), reps=args.reps, cls_crop_ms=round(t_crop, 3),
                          cls_forward_ms=round(t_fwd, 3), rec_crop_oriented_ms=round(t_ocrop, 3), rec_crop_ms=round(t_rcrop, 3),
                          total_ms=round(t_crop + t_fwd + t_ocrop - t_rcrop, 3), layers=layers)))
    eng.close()


if __name__ == "__main__":
    main()
