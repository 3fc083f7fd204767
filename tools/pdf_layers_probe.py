"""Times layered scanned-PDF pages as the provider's LUMINA_OCR_PDF_LAYERS path handles them: 64 A4 pages at 200 dpi (1654 x 2339;
--distinct different synth pages, repeated).

  strips   every page as 8 Flate strips (RGB, PNG predictor Sub): the strips' decode (one lumina_ocr_flate_image_decode per strip
           height) and lumina_ocr_page_compose, timed separately; beside them the same pages stored as one Flate image each through
           the one-image path (one decode call).  strips.decode + strips.compose - single.decode is what layering costs.
  mixed    a mixed raster page: a 100-dpi DCT background (827 x 1170) under a 300-dpi Group 4 stencil (2481 x 3508): decode of both
           and the composition onto the 2481 x 3508 canvas.
  compose  the kernel alone, timed with events: the bytes the definition moves (W H (3 + 3 layers touching)), the bytes that are
           distinct (the output and every source once: a background shown at 3 x 3 is read nine times, mostly from cache), and both
           over the time, against the 6.3 TB/s an element-wise kernel reaches on an MI355X.  Masks travel as RGB: a 1-bit stencil is
           24 bits a sample here, which is what the `mixed` figure pays.

Wall-clock per call with a synchronise after it, median of --reps with min and max; every composed page is checked against the source
bitmap first.  One JSON line; needs an MI355X.

    python tools/pdf_layers_probe.py [--reps 20] [--pages 64] [--parts strips,mixed]"""
import argparse
import io
import json
import sys
import time
import zlib
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
for p in (ROOT, ROOT / "ocr-system_amd"):
    sys.path.insert(0, str(p))

W, H = 1654, 2339
HBM_TBS = 6.3   # the guides' figure for element-wise kernels


def sub_filter(rows, bpp):
    import numpy as np
    a = rows.astype(np.int16)
    d = a.copy()
    d[:, bpp:] -= a[:, :-bpp]
    return np.concatenate([np.ones((rows.shape[0], 1), np.uint8), (d & 255).astype(np.uint8)], axis=1).tobytes()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--pages", type=int, default=64)
    ap.add_argument("--distinct", type=int, default=4)
    ap.add_argument("--parts", default="strips,mixed")
    args = ap.parse_args()
    import numpy as np
    import torch
    from PIL import Image
    from lumina_ocr import synth
    from lumina_ocr.engine import Engine

    eng = Engine(0)
    n = args.pages

    def stat(times):
        return dict(median=round(float(np.median(times)), 3), min=round(min(times), 3), max=round(max(times), 3))

    def timed(fn, reps):
        times = []
        for i in range(reps + 1):
            t0 = time.perf_counter()
            out = fn()
            torch.cuda.synchronize()
            if i:
                times.append((time.perf_counter() - t0) * 1e3)
        return stat(times), out

    def kernel_ms(fn, reps):
        times = []
        for i in range(reps + 1):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            if i:
                times.append(e0.elapsed_time(e1))
        return stat(times)

    def traffic(hw, layers, ms):
        """bytes of the definition and distinct bytes of one composition, and their rates over the kernel's median time"""
        defined = sum(3 * (min(r[3], hw[0]) - max(r[1], 0)) * (min(r[2], hw[1]) - max(r[0], 0)) * ((s is not None) + (m is not None))
                      for _, _, r, _, _, s, m in layers) + 3 * n * hw[0] * hw[1]
        distinct = 3 * n * hw[0] * hw[1] + sum(t.numel() for _, _, _, _, _, s, m in layers for t in (s, m) if t is not None)
        out = dict(defined_mb=round(defined / 1e6, 1), distinct_mb=round(distinct / 1e6, 1), defined_tb_s=round(defined / ms / 1e9, 3),
                   distinct_tb_s=round(distinct / ms / 1e9, 3))
        out["distinct_share_of_hbm"] = round(out["distinct_tb_s"] / HBM_TBS, 3)
        return out

    res = dict(pages=n, height=H, width=W, distinct=args.distinct, reps=args.reps, hbm_elementwise_tb_s=HBM_TBS)
    parts = args.parts.split(",")
    if "strips" in parts:
        src = [synth.synth_page(H, W, 100 + k, n_lines=40)[0] for k in range(args.distinct)]
        edges = [0] + [292 * k for k in range(1, 8)] + [H]            # 7 strips of 292 rows and one of 295
        bands = list(zip(edges[:-1], edges[1:]))
        strips = [[zlib.compress(sub_filter(page[r0:r1].reshape(r1 - r0, -1), 3), 6) for r0, r1 in bands] for page in src]
        whole = [zlib.compress(sub_filter(page.reshape(H, -1), 3), 6) for page in src]
        by_height = {}
        for k, (r0, r1) in enumerate(bands):
            by_height.setdefault(r1 - r0, []).append(k)

        def decode_strips():
            out = {}
            for h, ks in by_height.items():
                streams = [strips[i % len(src)][k] for i in range(n) for k in ks]
                dec, status = eng.flate_image_decode(streams, h, W, [(15, 3, 8, 0, 0)] * len(streams))
                assert status.count(0) == len(streams)
                for j, (i, k) in enumerate((i, k) for i in range(n) for k in ks):
                    out[(i, k)] = dec[j]
            return out

        t_decode, dec = timed(decode_strips, args.reps)
        layers = [(i, 0, (0, r0, W, r1), 0, (0, 0, 0), dec[(i, k)], None) for i in range(n) for k, (r0, r1) in enumerate(bands)]
        t_compose, pages = timed(lambda: eng.page_compose((H, W), n, layers), args.reps)
        assert all(np.array_equal(pages[i].cpu().numpy(), src[i]) for i in range(len(src)))
        t_single, (one, status) = timed(lambda: eng.flate_image_decode([whole[i % len(src)] for i in range(n)], H, W, [(15, 3, 8, 0, 0)] * n), args.reps)
        assert status.count(0) == n and np.array_equal(one[0].cpu().numpy(), src[0])
        k_ms = kernel_ms(lambda: eng.page_compose((H, W), n, layers), args.reps)
        res["strips"] = dict(strips_per_page=8, decode_calls=len(by_height), decode_ms=t_decode, compose_ms=t_compose, single_image_decode_ms=t_single,
                             layering_cost_ms=round(t_decode["median"] + t_compose["median"] - t_single["median"], 3),
                             compose_kernel_ms=k_ms, compose_traffic=traffic((H, W), layers, k_ms["median"]))
        del dec, layers, pages, one
    if "mixed" in parts:
        bw, bh, mw, mh = 827, 1170, 2481, 3508
        bgs, jpegs, g4s, wants = [], [], [], []
        for k in range(args.distinct):
            bg = synth.synth_page(bh, bw, 200 + k, n_lines=20)[0]
            op = io.BytesIO()
            Image.fromarray(bg).save(op, "JPEG", quality=75)
            jpegs.append(op.getvalue())
            bgs.append(np.asarray(Image.open(io.BytesIO(op.getvalue())).convert("RGB")))
            black = synth.synth_page(mh, mw, 300 + k, n_lines=40)[0].mean(axis=2) < 128
            op = io.BytesIO()
            Image.fromarray(np.where(black, 255, 0).astype(np.uint8)).convert("1").save(op, "TIFF", compression="group4", strip_size=((mw + 7) // 8) * mh)
            t = Image.open(io.BytesIO(op.getvalue()))
            g4s.append(op.getvalue()[t.tag_v2[273][0]:t.tag_v2[273][0] + t.tag_v2[279][0]])
            wants.append(black)
        fill = (26, 51, 153)

        def decode_mixed():
            b, sb = eng.jpeg_decode([jpegs[i % len(jpegs)] for i in range(n)], bh, bw)
            m, sm = eng.fax_decode([g4s[i % len(g4s)] for i in range(n)], mh, mw, [(-1, 0, 0, 0, 0)] * n)   # coded black = sample 0: painted
            assert sb.count(0) == n and sm.count(0) == n
            return b, m

        t_decode, (b, m) = timed(decode_mixed, args.reps)
        layers = [l for i in range(n) for l in ((i, 0, (0, 0, mw, mh), 0, (0, 0, 0), b[i], None), (i, 1, (0, 0, mw, mh), 0, fill, None, m[i]))]
        t_compose, pages = timed(lambda: eng.page_compose((mh, mw), n, layers), args.reps)
        got = pages[0].cpu().numpy()
        ys, xs = ((2 * np.arange(mh) + 1) * bh) // (2 * mh), ((2 * np.arange(mw) + 1) * bw) // (2 * mw)   # the sample that holds the pixel centre
        want = np.where(wants[0][:, :, None], np.asarray(fill, np.uint8), bgs[0][ys[:, None], xs[None, :]])
        assert np.array_equal(got, want), "mixed raster page differs from its definition (a device JPEG decode that differs from Pillow's would show here)"
        k_ms = kernel_ms(lambda: eng.page_compose((mh, mw), n, layers), args.reps)
        res["mixed"] = dict(background=[bw, bh], stencil=[mw, mh], decode_ms=t_decode, compose_ms=t_compose, compose_kernel_ms=k_ms,
                            compose_traffic=traffic((mh, mw), layers, k_ms["median"]), mask_bytes_as_rgb_mb=round(3 * n * mw * mh / 1e6, 1),
                            mask_bytes_packed_mb=round(n * ((mw + 7) // 8) * mh / 1e6, 1))
    print(json.dumps(res))
    eng.close()


if __name__ == "__main__":
    main()
