"""Times the selection-mark pass on the bench's step: 64 A4@200DPI pages (bench.make_pages, seed 2024; --mark-pages of them replaced by
synth.synth_marks_page and as many by synth.synth_radio_page) -> lumina_ocr_selection_marks alone (twice: the spread between the two is
the run's own noise), lumina_ocr_selection_marks_round, and in the same run on the same pages lumina_ocr_deskew (the yardstick of
DESIGN.md §3: it labels components too, then does Canny, Hough and a warp), the DB post-process of the pages' probability maps, and a
whole pipeline step with marks off, on (twice) and with round marks on.  HIP events around each stage, median of --reps, with the spread (min, max) of the repeats.
One JSON line; needs an MI355X.

    python tools/marks_probe.py [--reps 20]"""
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
    ap.add_argument("--mark-pages", type=int, default=16)
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
    n_mark = min(args.mark_pages, args.pages)
    for i in range(n_mark):
        pages[i] = torch.from_numpy(synth.synth_marks_page(i, h, w, n_marks=24, noise=3.0)[0]).cuda()
    n_radio = min(n_mark, args.pages - n_mark)
    for i in range(n_radio):
        pages[n_mark + i] = torch.from_numpy(synth.synth_radio_page(i, h, w, n_marks=24, noise=3.0)[0]).cuda()

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

    res = dict(pages=args.pages, height=h, width=w, mark_pages=n_mark, radio_pages=n_radio, reps=args.reps)
    t_deskew, _ = stage(lambda: eng.deskew(pages))
    prob = eng.det_forward(pages)
    t_post, _ = stage(lambda: eng.det_postprocess(prob, h, w, **arch.TEXT_PATH_POST))
    off = OcrPipeline(eng, post=arch.TEXT_PATH_POST)
    t_off, _ = stage(lambda: off.run(pages))
    t_marks, (rows, cnt) = stage(lambda: eng.selection_marks(pages))
    on = OcrPipeline(eng, post=arch.TEXT_PATH_POST, marks=True)
    t_on, _ = stage(lambda: on.run(pages))
    t_round, (_, _, _, rcnt) = stage(lambda: eng.selection_marks_round(pages))
    with_rounds = OcrPipeline(eng, post=arch.TEXT_PATH_POST, marks=True, round_marks=True)
    t_on_round, _ = stage(lambda: with_rounds.run(pages))
    t_marks2, _ = stage(lambda: eng.selection_marks(pages))       # round marks off, a second time: the run's own spread
    t_on2, _ = stage(lambda: on.run(pages))
    cnt, rcnt = cnt.cpu().numpy(), rcnt.cpu().numpy()
    res.update(marks=int(cnt.sum()), pages_with_marks=int((cnt > 0).sum()), selection_marks_ms=t_marks, deskew_ms=t_deskew,
               det_postprocess_ms=t_post, pipeline_off_ms=t_off, pipeline_on_ms=t_on,
               marks_over_deskew=round(t_marks["median"] / t_deskew["median"], 3), pipeline_delta_ms=round(t_on["median"] - t_off["median"], 2),
               round_marks=int(rcnt.sum()), selection_marks_round_ms=t_round, selection_marks_again_ms=t_marks2, pipeline_on_again_ms=t_on2,
               pipeline_on_round_ms=t_on_round, round_pass_delta_ms=round(t_round["median"] - max(t_marks["median"], t_marks2["median"]), 3),
               off_spread_ms=round(abs(t_marks["median"] - t_marks2["median"]), 3),
               round_pipeline_delta_ms=round(t_on_round["median"] - max(t_on["median"], t_on2["median"]), 2))
    print(json.dumps(res))
    eng.close()


if __name__ == "__main__":
    main()
