"""Times the lossless WebP decode (lumina_ocr_webp_decode): A4@200DPI pages (1654 x 2339; --distinct different pages of black text
rendered on white, repeated) written by Pillow (libwebp 1.6) as lossless WebP:
  * `text_default`   rendered text at Pillow's default lossless settings (mostly backward references and colour-cache hits);
  * `text_m0q0`      the same pages at method=0, quality=0 (far fewer references);
  * `noise_default`  the same pages with scanner-like noise (Gaussian, sigma 3: nearly every pixel a literal);
each as a batch of --pages pages in one call and as one page alone.  Wall-clock per call (the calls synchronise), median of --reps with
min and max after one warm-up call.  Beside each, Pillow on one host thread over the distinct files, median of --host-reps, per page
(host_batch_ms is that figure times the number of pages).  The split of the device time between the entropy walk (wp_entropy) and the
transforms comes from a kernel trace of `--trace CASE` (one warm-up call and one timed call of that case, nothing else), in a run of
its own.  Writes profiles/webp_probe.json and prints it; needs an MI355X.  No threshold: the host decode is what each figure is compared
with.

    python tools/webp_probe.py [--lossy] [--reps 20] [--pages 64] [--host-reps 3] [--cases ...] [--merge] [--trace CASE] [--out FILE]"""
import argparse
import io
import json
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
for p in (ROOT, ROOT / "ocr-system_amd"):
    sys.path.insert(0, str(p))

W, H = 1654, 2339
CASES = {"text_default": (0.0, {}), "text_m0q0": (0.0, {"method": 0, "quality": 0}), "noise_default": (3.0, {})}
# --lossy: the same pages as lossy WebP (VP8 key frames) at quality 80, clean and with the scanner-like noise, through
# lumina_ocr_webp_decode_lossy; writes profiles/webp_lossy_probe.json.  The kernel trace then splits the two walks (vp8_modes, vp8_tokens)
# from the parallel stages (vp8_recon, vp8_filter, vp8_rgb).
LOSSY_CASES = {"lossy_text_q80": (0.0, {"quality": 80}), "lossy_noise_q80": (3.0, {"quality": 80})}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--host-reps", type=int, default=3)
    ap.add_argument("--pages", type=int, default=64)
    ap.add_argument("--distinct", type=int, default=4)
    ap.add_argument("--lossy", action="store_true", help="the lossy cases through lumina_ocr_webp_decode_lossy")
    ap.add_argument("--cases", default="")
    ap.add_argument("--trace", default="")
    ap.add_argument("--merge", action="store_true", help="keep the cases the output file already holds (a case may be run with --reps of its own)")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    cases = LOSSY_CASES if args.lossy else CASES
    args.cases = args.cases or ",".join(cases)
    args.out = args.out or str(ROOT / "profiles" / ("webp_lossy_probe.json" if args.lossy else "webp_probe.json"))
    import numpy as np
    import torch
    from PIL import Image
    from PIL import ImageDraw, ImageFont
    from lumina_ocr.engine import Engine

    eng = Engine(0)
    decode = eng.webp_decode_lossy if args.lossy else eng.webp_decode
    probe = Engine.webp_probe_lossy if args.lossy else Engine.webp_probe

    def render(seed):
        """a clean rendered text page: black text on white, nothing else"""
        rng = np.random.default_rng(seed)
        words = ("lossless webp page rendered text clean scan screenshot device decode prefix code colour cache backward reference "
                 "the quick brown fox jumps over a lazy dog 0123456789").split()
        im = Image.new("RGB", (W, H), (255, 255, 255))
        d = ImageDraw.Draw(im)
        try:
            font = ImageFont.load_default(28)
        except Exception:
            font = ImageFont.load_default()
        for y in range(150, H - 150, 44):
            d.text((140, y), " ".join(rng.choice(words, 14)), fill=(0, 0, 0), font=font)
        return np.array(im)
    src = [render(100 + k) for k in range(args.distinct)]

    def write(sigma, opts):
        files = []
        for k, page in enumerate(src):
            if sigma:
                rng = np.random.default_rng(500 + k)
                page = np.clip(page.astype(np.float32) + rng.normal(0.0, sigma, page.shape), 0, 255).astype(np.uint8)
            op = io.BytesIO()
            Image.fromarray(page).save(op, "WEBP", lossless=not args.lossy, **opts)
            files.append(op.getvalue())
        return files

    def timed(fn, reps, sync=True):
        times = []
        for i in range(reps + 1):
            t0 = time.perf_counter()
            out = fn()
            if sync:
                torch.cuda.synchronize()
            if i:
                times.append((time.perf_counter() - t0) * 1e3)
        return dict(median=round(float(np.median(times)), 2), min=round(min(times), 2), max=round(max(times), 2)), out

    if args.trace:
        files = write(*cases[args.trace])
        streams = [files[i % len(files)] for i in range(args.pages)]
        out_buf = torch.empty((args.pages, H, W, 3), dtype=torch.uint8, device="cuda")
        t, (_, status) = timed(lambda: decode(streams, H, W, out=out_buf), 1)
        print(json.dumps(dict(trace=args.trace, pages=args.pages, device_ms=t, status_ok=status.count(0))))
        eng.close()
        return

    res = dict(pages=args.pages, height=H, width=W, distinct=args.distinct, host_reps=args.host_reps)
    if args.merge and Path(args.out).exists():
        res = json.loads(Path(args.out).read_text())
    for name in args.cases.split(","):
        files = write(*cases[name])
        t_host, ref = timed(lambda: [np.asarray(Image.open(io.BytesIO(s)).convert("RGB")) for s in files], args.host_reps, sync=False)
        host_page = t_host["median"] / len(files)
        entry = dict(reps=args.reps, file_kb=round(sum(len(s) for s in files) / len(files) / 1024, 1), probe_status=[probe(s)[0] for s in files],
                     host_ms_per_page=round(host_page, 2), host_ms_distinct=t_host)
        for label, n in (("batch", args.pages), ("single", 1)):
            streams = [files[i % len(files)] for i in range(n)]
            out_buf = torch.empty((n, H, W, 3), dtype=torch.uint8, device="cuda")
            t_dev, (out, status) = timed(lambda: decode(streams, H, W, out=out_buf), args.reps)
            equal = all(status[i] == 0 and np.array_equal(out[i].cpu().numpy(), ref[i]) for i in range(min(n, len(files))))
            entry[label] = dict(pages=n, device_ms=t_dev, host_batch_ms=round(host_page * n, 1), status_ok=status.count(0), equal_to_host=bool(equal),
                                device_pages_per_s=round(n / t_dev["median"] * 1e3, 2), host_pages_per_s=round(1e3 / host_page, 1))
        res[name] = entry
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(json.dumps(res) + "\n")   # (after every case: a long run leaves what it has)
    print(json.dumps(res))
    eng.close()


if __name__ == "__main__":
    main()
