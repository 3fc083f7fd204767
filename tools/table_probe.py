"""Times the rule extraction of ruled tables on the bench's step: 64 A4@200DPI pages (bench.make_pages, seed 2024; --table-pages of them
replaced by synth.synth_table_page) -> lumina_ocr_table_rules alone, lumina_ocr_grayscale and lumina_ocr_deskew on the same pages in the
same run (the two yardsticks of DESIGN.md §3), and a whole pipeline step with tables off and on.  HIP events around each stage,
median of --reps.  One JSON line; needs an MI355X.

    python tools/table_probe.py [--reps 20]"""
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
    ap.add_argument("--table-pages", type=int, default=16)
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
    for i in range(min(args.table_pages, args.pages)):
        pages[i] = torch.from_numpy(synth.synth_table_page(i, h, w, n_tables=3, spans=bool(i & 1), noise=3.0)[0]).cuda()

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

    t_rules, (hr, vr, cnt) = stage(lambda: eng.table_rules(pages))
    t_grey, _ = stage(lambda: eng.grayscale(pages))
    t_deskew, _ = stage(lambda: eng.deskew(pages))
    off = OcrPipeline(eng, post=arch.TEXT_PATH_POST)
    on = OcrPipeline(eng, post=arch.TEXT_PATH_POST, tables=True)
    t_off, _ = stage(lambda: off.run(pages))
    t_on, (dets, _) = stage(lambda: on.run(pages))
    cnt = cnt.cpu().numpy()
    print(json.dumps(dict(pages=args.pages, height=h, width=w, table_pages=min(args.table_pages, args.pages), reps=args.reps,
                          hrules=int(cnt[:, 0].sum()), vrules=int(cnt[:, 1].sum()), table_rules_ms=round(t_rules, 3), grayscale_ms=round(t_grey, 3),
                          deskew_ms=round(t_deskew, 3), rules_over_grayscale=round(t_rules / t_grey, 3), rules_over_deskew=round(t_rules / t_deskew, 3),
                          pipeline_off_ms=round(t_off, 2), pipeline_on_ms=round(t_on, 2), pipeline_delta_ms=round(t_on - t_off, 2))))
    eng.close()


if __name__ == "__main__":
    main()
