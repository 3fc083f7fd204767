"""Times the Aztec pass on the bench's step: 64 A4@200DPI pages (bench.make_pages, seed 2024) -> lumina_ocr_aztec alone on the pages as
they are (no symbol) and on the same pages with one compact-2 and one full-11 symbol at 3 px a module drawn under the text of each,
and in the same run on the same pages lumina_ocr_qrcodes and lumina_ocr_datamatrix (the yardsticks: the same run list and
components).  HIP events around each stage, median of --reps, with the spread (min, max) of the repeats.  With --max-layers above 11
also lumina_ocr_aztec_layers: on the plain and on the small-symbol pages, interleaved with lumina_ocr_aztec (what the second stage
costs where nothing is pending), and on the plain pages with one 16-layer and one 32-layer symbol at 3 px a module on each of 16 of
them (what it costs where it works, and how many of the 32 it reads).  One JSON line; needs an MI355X.

    python tools/aztec_probe.py [--reps 20] [--max-layers 32]"""
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
    ap.add_argument("--max-layers", type=int, default=11, help="above 11: lumina_ocr_aztec_layers as well (11..32)")
    args = ap.parse_args()
    import numpy as np
    import torch
    import bench
    from lumina_ocr.engine import Engine
    from lumina_ocr.utils import aztec as az

    eng = Engine(0)
    plain = bench.make_pages(torch, args.pages, 2024, torch.device("cuda", 0))
    _, h, w, _ = plain.shape
    host = plain.cpu().numpy().copy()
    texts = []
    for i, page in enumerate(host):
        small, large = "PROBE %04d" % i, ("Aztec probe page %04d. " % i) * 12
        y = h - 61 * 3 - 40
        page[y - 20:, :] = 255                                           # a clear band at the foot of the page for the two symbols
        az.draw(page, 100, y, az.encode(small, True, 2), 3, i % 4)
        az.draw(page, 400, y, az.encode(large, False, 11), 3, (i + 1) % 4)
        texts.append(sorted((small, large)))
    coded = torch.from_numpy(host).cuda()

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

    res = dict(pages=args.pages, height=h, width=w, reps=args.reps)
    _, (_, _, cnt0, _, find0) = stage(lambda: eng.aztec(plain, debug=True))
    _, (codes, data, cnt1, _, find1) = stage(lambda: eng.aztec(coded, debug=True))
    t_plain, _ = stage(lambda: eng.aztec(plain))
    t_coded, _ = stage(lambda: eng.aztec(coded))
    t_qr, _ = stage(lambda: eng.qrcodes(coded))
    t_dm, _ = stage(lambda: eng.datamatrix(coded))
    t_plain2, _ = stage(lambda: eng.aztec(plain))
    codes, data, cnt1 = codes.cpu().numpy(), data.cpu().numpy(), cnt1.cpu().numpy()
    read = sum(sorted(e["content"] for e in az.read_aztec(codes[i, :cnt1[i]], data[i, :cnt1[i]])) == texts[i] for i in range(args.pages))
    res.update(finders_plain=int(find0.sum()), codes_plain=int(cnt0.sum()), finders_coded=int(find1.sum()), codes_coded=int(cnt1.sum()), pages_read_in_full=int(read),
               aztec_plain_ms=t_plain, aztec_plain_again_ms=t_plain2, aztec_coded_ms=t_coded, qrcodes_ms=t_qr, datamatrix_ms=t_dm,
               aztec_over_qrcodes=round(t_plain["median"] / t_qr["median"], 3))
    if args.max_layers > 11:
        ml = args.max_layers
        t_a1, _ = stage(lambda: eng.aztec(plain))
        t_l1, (_, _, lcnt0) = stage(lambda: eng.aztec_layers(plain, ml))
        t_a2, _ = stage(lambda: eng.aztec(coded))
        t_l2, (lcodes, ldata, lcnt1) = stage(lambda: eng.aztec_layers(coded, ml))
        t_a3, _ = stage(lambda: eng.aztec(plain))
        t_l3, _ = stage(lambda: eng.aztec_layers(plain, ml))
        same = bool(torch.equal(lcodes, torch.from_numpy(codes).cuda())) and np.array_equal(ldata.cpu().numpy()[:, :, :320], data)
        big_host, big_texts = plain.cpu().numpy().copy(), {}
        for i in range(0, args.pages, max(1, args.pages // 16)):
            page = big_host[i]
            page[h - 151 * 3 - 60:, :] = 255
            y = h - 151 * 3 - 30
            big_texts[i] = sorted((("Layers probe %04d, sixteen. " % i) * 12, ("Layers probe %04d, thirty-two. " % i) * 30))
            az.draw(page, 80, y, az.encode(big_texts[i][0], False, min(16, ml)), 3, i % 4)
            az.draw(page, 500, y, az.encode(big_texts[i][1], False, ml), 3, (i + 1) % 4)
        big = torch.from_numpy(big_host).cuda()
        t_big, (bcodes, bdata, bcnt) = stage(lambda: eng.aztec_layers(big, ml))
        t_big_old, _ = stage(lambda: eng.aztec(big))
        bcodes, bdata, bcnt = bcodes.cpu().numpy(), bdata.cpu().numpy(), bcnt.cpu().numpy()
        got = {i: [e["content"] for e in az.read_aztec(bcodes[i, :bcnt[i]], bdata[i, :bcnt[i]], max_layers=ml)] for i in big_texts}
        res.update(max_layers=ml, layers_plain_ms=t_l1, aztec_plain_beside_ms=t_a1, layers_plain_again_ms=t_l3, aztec_plain_beside_again_ms=t_a3,
                   layers_coded_ms=t_l2, aztec_coded_beside_ms=t_a2, layers_codes_plain=int(lcnt0.sum()), layers_small_rows_equal=same,
                   large_pages=len(big_texts), large_symbols=2 * len(big_texts), large_symbols_read=int(sum(sum(t in got[i] for t in big_texts[i]) for i in big_texts)),
                   layers_large_ms=t_big, aztec_large_pages_ms=t_big_old)
    print(json.dumps(res))
    eng.close()


if __name__ == "__main__":
    main()
