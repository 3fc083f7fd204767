"""Times the barcode pass on the bench's step: 64 A4@200DPI pages (bench.make_pages, seed 2024; --code-pages of them carry the codes of
synth.synth_barcode_page drawn under their text) -> lumina_ocr_barcodes alone (twice: the spread between the two is the run's own
noise), in the same run on the same pages lumina_ocr_selection_marks (the yardstick: the same run list, then components), and a whole
pipeline step with barcodes off and on (twice).  HIP events around each stage, median of --reps, with the spread (min, max) of the
repeats.  With --kinds (names of arch.BARCODE_KINDS, or all) every page also gets one EAN-13 and one ITF-14 strip in its bottom margin
and the pass is timed on those pages with the default kinds and with the kinds given, each twice: the difference is what the extra
start filters and decoders cost, reported per row and column read.  One JSON line; needs an MI355X.

    python tools/barcode_probe.py [--reps 20] [--kinds all]"""
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
    ap.add_argument("--code-pages", type=int, default=16)
    ap.add_argument("--kinds", default="", help="comma list of barcode kinds (or all) to time beside the default ones")
    args = ap.parse_args()
    import numpy as np
    import torch
    import bench
    from lumina_ocr import arch, synth
    from lumina_ocr.engine import Engine
    from lumina_ocr.pipeline import OcrPipeline

    eng = Engine(0)
    eng.load_det(arch.make_det_weights(1234))
    eng.load_rec(arch.make_rec_weights(4321, code_path=True))
    pages = bench.make_pages(torch, args.pages, 2024, torch.device("cuda", 0))
    _, h, w, _ = pages.shape
    n_code, drawn = min(args.code_pages, args.pages), 0
    for i in range(n_code):
        page, gt = synth.synth_barcode_page(i, h, w, n_codes=4, text_lines=20)
        pages[i] = torch.from_numpy(page).cuda()
        drawn += len(gt)

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
        return dict(median=round(float(np.median(times)), 3), min=round(min(times), 3), max=round(max(times), 3)), out

    res = dict(pages=args.pages, height=h, width=w, code_pages=n_code, codes_drawn=drawn, reps=args.reps)
    off = OcrPipeline(eng, post=arch.TEXT_PATH_POST)
    on = OcrPipeline(eng, post=arch.TEXT_PATH_POST, barcodes=True)
    t_off, _ = stage(lambda: off.run(pages))
    t_codes, (_, _, cnt) = stage(lambda: eng.barcodes(pages))
    t_marks, _ = stage(lambda: eng.selection_marks(pages))
    t_on, _ = stage(lambda: on.run(pages))
    t_codes2, _ = stage(lambda: eng.barcodes(pages))
    t_off2, _ = stage(lambda: off.run(pages))
    t_on2, _ = stage(lambda: on.run(pages))
    cnt = cnt.cpu().numpy()
    res.update(codes_read=int(cnt.sum()), pages_with_codes=int((cnt > 0).sum()), barcodes_ms=t_codes, barcodes_again_ms=t_codes2, selection_marks_ms=t_marks,
               pipeline_off_ms=t_off, pipeline_off_again_ms=t_off2, pipeline_on_ms=t_on, pipeline_on_again_ms=t_on2,
               barcodes_over_marks=round(t_codes["median"] / t_marks["median"], 3),
               pipeline_delta_ms=round(min(t_on["median"], t_on2["median"]) - min(t_off["median"], t_off2["median"]), 2),
               off_spread_ms=round(abs(t_off["median"] - t_off2["median"]), 2))
    if args.kinds:
        mask = arch.barcode_kinds_mask(args.kinds)
        more = pages.clone()
        y = h - 70
        more[:, y - 20:, :, :] = 255                                      # a clear bottom margin for the two strips
        strip = np.full((50, w, 3), 255, np.uint8)
        synth.render_linear(strip, 100, 5, "EAN13", "4006381333931", 3, 40)
        synth.render_linear(strip, 600, 5, "ITF", "00012345678905", 3, 40, ratio=2.5)
        more[:, y:y + 50] = torch.from_numpy(strip).cuda()
        t_def, (_, _, c_def) = stage(lambda: eng.barcodes(more))
        t_k, (_, _, c_k) = stage(lambda: eng.barcodes(more, kinds=mask))
        t_def2, _ = stage(lambda: eng.barcodes(more))
        t_k2, _ = stage(lambda: eng.barcodes(more, kinds=mask))
        extra = min(t_k["median"], t_k2["median"]) - min(t_def["median"], t_def2["median"])
        res.update(kinds=args.kinds, kinds_mask=mask, strips_default_ms=t_def, strips_default_again_ms=t_def2, strips_kinds_ms=t_k, strips_kinds_again_ms=t_k2,
                   strips_codes_default=int(c_def.sum()), strips_codes_kinds=int(c_k.sum()), kinds_extra_ms=round(extra, 3),
                   kinds_extra_ns_per_row=round(extra * 1e6 / (args.pages * (h + w)), 1))
    print(json.dumps(res))
    eng.close()


if __name__ == "__main__":
    main()
