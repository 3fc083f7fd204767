"""Times the word boxes on the bench's step: 64 A4@200DPI pages (bench.make_pages, seed 2024) -> in one run, on the step's own crops,
lumina_ocr_ctc_decode and lumina_ocr_ctc_decode_words (HIP events around the call, so the binding's output allocations count), and a
whole pipeline step with word_boxes off and on (the kernel plus the pinned copies of the four word tensors).  Median of --reps, with
the spread (min, max) of the repeats.  One JSON line; needs an MI355X.

    python tools/words_probe.py [--reps 20]"""
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
    pages = bench.make_pages(torch, args.pages, 2024, torch.device("cuda", 0))
    _, h, w, _ = pages.shape

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

    off = OcrPipeline(eng, post=arch.TEXT_PATH_POST)
    on = OcrPipeline(eng, post=arch.TEXT_PATH_POST, word_boxes=True)
    # the step's own lines: its crops, their widths, the recogniser's output
    processed, boxes, scores, counts = off.submit_detect(pages)
    quads, _, page_idx = off._select_lines(boxes, scores, counts.cpu().numpy(), args.pages)
    crops, widths = eng.rec_crop(processed, quads, page_idx)
    idx, prob = eng.rec_forward(crops, widths)
    t_ctc, _ = stage(lambda: eng.ctc_decode(idx, prob))
    t_words, out = stage(lambda: eng.ctc_decode_words(idx, prob, quads, widths, None, on.space_id))
    t_off, _ = stage(lambda: off.run(pages))
    t_on, _ = stage(lambda: on.run(pages))
    t_off2, _ = stage(lambda: off.run(pages))   # the option off once more: the run-to-run spread the difference is read against
    word_bytes = sum(t.numel() * t.element_size() for t in out[3:])
    res = dict(pages=args.pages, height=h, width=w, reps=args.reps, crops=int(idx.shape[0]), words=int(out[6].sum().item()),
               word_copy_mb=round(word_bytes / 1e6, 2), ctc_decode_ms=t_ctc, ctc_decode_words_ms=t_words, pipeline_off_ms=t_off,
               pipeline_on_ms=t_on, pipeline_off_again_ms=t_off2,
               words_over_ctc_ms=round(t_words["median"] - t_ctc["median"], 3), pipeline_delta_ms=round(t_on["median"] - t_off["median"], 3),
               off_spread_ms=round(abs(t_off2["median"] - t_off["median"]), 3))
    print(json.dumps(res))
    eng.close()


if __name__ == "__main__":
    main()
