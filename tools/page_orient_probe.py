"""Times the page orientation on the bench's step: 64 A4@200DPI pages (bench.make_pages, seed 2024), all in one run ->
  * lumina_ocr_page_quarter against lumina_ocr_grayscale (it reads the same page bytes and writes 1/24 of them);
  * lumina_ocr_page_turn for t = 1 and t = 2 against a device-to-device copy of the same pages (both move the same bytes in and out);
  * a pipeline step with the option off, twice (option absent / page_orient=False: the second figure is the run-to-run spread);
  * a step with the option on for 64 upright pages, for --lying of them sideways and for --lying of them upside-down, next to the
    parts it is made of (quarter pass, classifier crops + forward + vote, turn, second pass), each timed alone.
The upright / sideways / upside-down pages are ruled synthetic pages (synth.synth_page(..., ruled=True)): the hand-set orientation path
of the seeded classifier is built for them.  HIP events around each stage, median of --reps with the spread (min, max).  One JSON
line; needs an MI355X.

    python tools/page_orient_probe.py [--reps 20]"""
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
    ap.add_argument("--lying", type=int, default=16)
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
    eng.load_cls(arch.make_cls_weights(2718, orientation_path=True))
    dev = torch.device("cuda", 0)
    _, h, w, _ = bench.make_pages(torch, 1, 2024, dev).shape
    n, lying = args.pages, min(args.lying, args.pages)
    portrait = [synth.synth_page(h, w, 50 + i, n_lines=40, ruled=True)[0] for i in range(4)]
    landscape = [synth.synth_page(w, h, 60 + i, n_lines=28, ruled=True)[0] for i in range(4)]
    upright = torch.from_numpy(np.stack([portrait[i % 4] for i in range(n)])).to(dev)
    side = upright.clone()
    down = upright.clone()
    for i in range(lying):
        side[i] = torch.from_numpy(np.ascontiguousarray(np.rot90(landscape[i % 4], 3))).to(dev)
        down[i] = torch.from_numpy(np.ascontiguousarray(np.rot90(portrait[i % 4], 2))).to(dev)

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

    kw = dict(post=arch.TEXT_PATH_POST)
    res = dict(pages=n, height=h, width=w, lying=lying, reps=args.reps)
    # ---- kernels against their yardsticks ----
    t_gray, _ = stage(lambda: eng.grayscale(upright))
    t_quarter, (_, flags) = stage(lambda: eng.page_quarter(side))
    dst = torch.empty_like(upright)
    t_copy, _ = stage(lambda: dst.copy_(upright))
    every = torch.arange(n, dtype=torch.int32, device=dev)
    t_turn = {t: stage(lambda t=t: eng.page_turn(upright, every, t))[0] for t in (0, 1, 2, 3)}
    res.update(grayscale_ms=t_gray, page_quarter_ms=t_quarter, quarter_over_grayscale=round(t_quarter["median"] / t_gray["median"], 3),
               sideways_found=int(flags.sum().item()), d2d_copy_ms=t_copy, page_turn_ms={str(t): v for t, v in t_turn.items()},
               turn1_over_copy=round(t_turn[1]["median"] / t_copy["median"], 3), turn2_over_copy=round(t_turn[2]["median"] / t_copy["median"], 3))
    # ---- the option off: absent and False are one code path; the second run is the spread ----
    t_absent, _ = stage(lambda: OcrPipeline(eng, **kw).run(upright))
    t_false, _ = stage(lambda: OcrPipeline(eng, page_orient=False, **kw).run(upright))
    res.update(pipeline_option_absent_ms=t_absent, pipeline_option_off_ms=t_false, off_minus_absent_ms=round(t_false["median"] - t_absent["median"], 2))
    # ---- the option on ----
    on = OcrPipeline(eng, page_orient=True, **kw)
    for name, pages in (("upright", upright), ("sideways", side), ("upside_down", down)):
        t_on, (dets, _) = stage(lambda pages=pages: on.run_oriented(pages))
        turns = np.bincount([d.turn for d in dets], minlength=4).tolist()
        res["pipeline_on_%s_ms" % name] = t_on
        res["pipeline_on_%s_turns" % name] = turns
        res["pipeline_on_%s_added_ms" % name] = round(t_on["median"] - t_absent["median"], 2)
    # ---- its parts, alone: the classifier on the step's lines, and a second pass over `lying` pages ----
    processed, boxes, scores, counts = on.submit_detect(upright)
    counts_h = counts.cpu().numpy()
    quads, _, page_idx = on._select_lines(boxes, scores, counts_h, n)

    def classify():
        crops, widths = eng.cls_crop(processed, quads, page_idx)
        return eng.page_vote(eng.cls_forward(crops, widths, on.cls_thresh)[2], page_idx, n)
    t_cls, _ = stage(classify)
    some = torch.arange(lying, dtype=torch.int32, device=dev)
    t_turn_some, turned = stage(lambda: eng.page_turn(down, some, 2))
    t_second, _ = stage(lambda: OcrPipeline(eng, **kw).run(turned))
    res.update(lines=int(counts_h.sum()), classifier_and_vote_ms=t_cls, turn_lying_pages_ms=t_turn_some, second_pass_ms=t_second)
    print(json.dumps(res))
    eng.close()


if __name__ == "__main__":
    main()
