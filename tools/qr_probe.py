"""Times the QR pass on the bench's step: 64 A4@200DPI pages (bench.make_pages, seed 2024; --code-pages of them carry the four symbols
of synth.synth_qr_page drawn under their text) -> lumina_ocr_qrcodes alone (twice: the spread between the two is the run's own noise),
in the same run on the same pages lumina_ocr_selection_marks and lumina_ocr_barcodes (the yardsticks: the same run list and, for the
marks, the same components), and a whole pipeline step with QR codes off and on (twice).  HIP events around each stage, median of
--reps, with the spread (min, max) of the repeats.  With --max-version above 10 also lumina_ocr_qrcodes_versions on the same pages (twice:
what stage 2 costs where it finds nothing) and on the same pages with one 25-M and one 40-H symbol at 3 px drawn on each of the
--code-pages (twice).  One JSON line; needs an MI355X.

    python tools/qr_probe.py [--reps 20] [--max-version 40]"""
import argparse
import json
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
for p in (ROOT, ROOT / "ocr-system_amd"):
    sys.path.insert(0, str(p))


def synth_qr_capacity(version: int, level: int) -> int:
    from lumina_ocr.utils import qrcodes as qr
    return qr.data_codewords(version, level) - 4


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--pages", type=int, default=64)
    ap.add_argument("--code-pages", type=int, default=16)
    ap.add_argument("--max-version", type=int, default=10)
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
        page, gt = synth.synth_qr_page(i, h, w, n_codes=4, text_lines=20)
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
    on = OcrPipeline(eng, post=arch.TEXT_PATH_POST, qrcodes=True)
    t_off, _ = stage(lambda: off.run(pages))
    t_codes, (_, _, cnt) = stage(lambda: eng.qrcodes(pages))
    t_marks, _ = stage(lambda: eng.selection_marks(pages))
    t_bars, _ = stage(lambda: eng.barcodes(pages))
    t_on, _ = stage(lambda: on.run(pages))
    t_codes2, _ = stage(lambda: eng.qrcodes(pages))
    t_off2, _ = stage(lambda: off.run(pages))
    t_on2, _ = stage(lambda: on.run(pages))
    cnt = cnt.cpu().numpy()
    res.update(codes_read=int(cnt.sum()), pages_with_codes=int((cnt > 0).sum()), qrcodes_ms=t_codes, qrcodes_again_ms=t_codes2, selection_marks_ms=t_marks,
               barcodes_ms=t_bars,
               pipeline_off_ms=t_off, pipeline_off_again_ms=t_off2, pipeline_on_ms=t_on, pipeline_on_again_ms=t_on2,
               qrcodes_over_marks=round(t_codes["median"] / t_marks["median"], 3),
               pipeline_delta_ms=round(min(t_on["median"], t_on2["median"]) - min(t_off["median"], t_off2["median"]), 2),
               off_spread_ms=round(abs(t_off["median"] - t_off2["median"]), 2))
    if args.max_version > 10:
        mv = args.max_version
        t_v, (_, _, vcnt) = stage(lambda: eng.qrcodes_versions(pages, mv))
        t_base, _ = stage(lambda: eng.qrcodes(pages))
        t_v2, _ = stage(lambda: eng.qrcodes_versions(pages, mv))
        large = pages.clone()
        for i in range(n_code):
            page = np.full((h, w, 3), 255, np.uint8)
            for x, version, level in ((40, 25, 1), (520, 40, 3)):
                text = ("probe %d v%d " % (i, version) + "e-invoice/" * 300)[:synth_qr_capacity(version, level)]
                synth.draw_qr(page, x, h - 600, synth.qr_encode(text, version, level, i % 8), 3)
            large[i, h - 640:] = torch.from_numpy(page[h - 640:]).cuda()
        t_l, (_, _, lcnt) = stage(lambda: eng.qrcodes_versions(large, mv))
        t_l2, _ = stage(lambda: eng.qrcodes_versions(large, mv))
        res.update(max_version=mv, versions_small_ms=t_v, versions_small_again_ms=t_v2, qrcodes_beside_ms=t_base, versions_small_read=int(vcnt.sum().item()),
                   versions_large_ms=t_l, versions_large_again_ms=t_l2, versions_large_read=int(lcnt.sum().item()), large_drawn=2 * n_code,
                   stage2_idle_ms=round(min(t_v["median"], t_v2["median"]) - min(t_base["median"], t_codes["median"], t_codes2["median"]), 3))
    print(json.dumps(res))
    eng.close()


if __name__ == "__main__":
    main()
