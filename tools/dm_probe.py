"""Times the Data Matrix pass on the bench's step: 64 A4@200DPI pages (bench.make_pages, seed 2024; --code-pages of them carry the four
symbols of synth.synth_dm_page drawn under their text) -> lumina_ocr_datamatrix alone (twice: the spread between the two is the run's
own noise), in the same run on the same pages lumina_ocr_qrcodes (the yardstick: the same run list and components), and a whole
pipeline step with Data Matrix off and on (twice).  HIP events around each stage, median of --reps, with the spread (min, max) of the
repeats.  One JSON line; needs an MI355X.

With --max-size N above 52 also lumina_ocr_datamatrix_sizes at that cap: on the pages above (no large symbol: what the second stage
costs where it finds nothing) and on the same pages with one 64 x 64 and one 144 x 144 symbol at 3 px a module drawn on each of the
first --code-pages, each time interleaved call by call with lumina_ocr_datamatrix on the same pages (the yardstick).

    python tools/dm_probe.py [--reps 20] [--max-size 144]"""
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
    ap.add_argument("--max-size", type=int, default=52, help="above 52: lumina_ocr_datamatrix_sizes as well (52..144)")
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
        page, gt = synth.synth_dm_page(i, h, w, n_codes=4, text_lines=20)
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
    on = OcrPipeline(eng, post=arch.TEXT_PATH_POST, datamatrix=True)
    t_off, _ = stage(lambda: off.run(pages))
    t_dm, (_, _, cnt, _, cands) = stage(lambda: eng.datamatrix(pages, debug=True))
    t_dm, _ = stage(lambda: eng.datamatrix(pages))
    t_qr, _ = stage(lambda: eng.qrcodes(pages))
    t_on, _ = stage(lambda: on.run(pages))
    t_dm2, _ = stage(lambda: eng.datamatrix(pages))
    t_off2, _ = stage(lambda: off.run(pages))
    t_on2, _ = stage(lambda: on.run(pages))
    cnt, cands = cnt.cpu().numpy(), cands.cpu().numpy()
    res.update(codes_read=int(cnt.sum()), pages_with_codes=int((cnt > 0).sum()), candidates=int(cands.sum()), max_candidates_a_page=int(cands.max()),
               datamatrix_ms=t_dm, datamatrix_again_ms=t_dm2, qrcodes_ms=t_qr,
               pipeline_off_ms=t_off, pipeline_off_again_ms=t_off2, pipeline_on_ms=t_on, pipeline_on_again_ms=t_on2,
               datamatrix_over_qrcodes=round(t_dm["median"] / t_qr["median"], 3),
               pipeline_delta_ms=round(min(t_on["median"], t_on2["median"]) - min(t_off["median"], t_off2["median"]), 2),
               off_spread_ms=round(abs(t_off["median"] - t_off2["median"]), 2))
    if args.max_size > 52:
        from lumina_ocr.utils import datamatrix as dm

        def pair(fa, fb):
            """fa and fb call by call, interleaved -> (times of fa, times of fb, the last outputs)"""
            ta, tb, out = [], [], None
            for i in range(args.reps + 3):
                ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
                ev[0].record()
                oa = fa()
                ev[1].record()
                ob = fb()
                ev[2].record()
                torch.cuda.synchronize()
                if i >= 3:
                    ta.append(ev[0].elapsed_time(ev[1]))
                    tb.append(ev[1].elapsed_time(ev[2]))
                out = (oa, ob)
            st = lambda t: dict(median=round(float(np.median(t)), 3), min=round(min(t), 3), max=round(max(t), 3))
            return st(ta), st(tb), out

        ms = args.max_size
        t_old, t_new, (o, nw) = pair(lambda: eng.datamatrix(pages), lambda: eng.datamatrix_sizes(pages, ms))
        same = bool(torch.equal(o[0], nw[0]) and torch.equal(o[2], nw[2]))
        big = pages.clone()
        text64, text144 = "64 x 64 " * 30, "144 x 144 record " * 80
        for i in range(n_code):
            page = big[i].cpu().numpy()
            y = h // 3 + 520                               # below the four symbols of synth_dm_page; the band is cleared first
            page[y - 20:y + 144 * 3 + 20, 20:900] = 255
            synth.draw_dm(page, 40, y, synth.dm_encode(text64, dm.size_index_all(64, 64)), 3)
            synth.draw_dm(page, 400, y, synth.dm_encode(text144, dm.size_index_all(144, 144)), 3, i % 4)
            big[i] = torch.from_numpy(page).cuda()
        t_old_big, t_new_big, (o, nw) = pair(lambda: eng.datamatrix(big), lambda: eng.datamatrix_sizes(big, ms))
        rows, data, cnt2 = (t.cpu().numpy() for t in nw)
        large = [e["content"] for i in range(args.pages) for e in dm.read_datamatrix(rows[i, :cnt2[i]], data[i, :cnt2[i]]) if e["rows"] >= 64]
        res.update(max_size=ms, plain_datamatrix_ms=t_old, plain_datamatrix_sizes_ms=t_new, plain_rows_equal=same,
                   plain_sizes_over_datamatrix=round(t_new["median"] / t_old["median"], 3),
                   large_drawn=2 * n_code, large_read=len(large), large_read_right=sum(t in (text64, text144) for t in large),
                   large_datamatrix_ms=t_old_big, large_datamatrix_sizes_ms=t_new_big,
                   large_sizes_over_datamatrix=round(t_new_big["median"] / t_old_big["median"], 3),
                   large_codes_old=int(o[2].sum()), large_codes_new=int(cnt2.sum()))
    print(json.dumps(res))
    eng.close()


if __name__ == "__main__":
    main()
