"""Times the scanned-TIFF decoders: 64 A4@200DPI pages (1654 x 2339; --distinct different synth pages, repeated) per codec, as the
provider's LUMINA_OCR_DEVICE_TIFF path hands them over: the strips utils/tiff_pages.py finds in files Pillow / libtiff wrote (64 KB
strips, Pillow's default) go to lumina_ocr_strip_image_decode (LZW grey, LZW RGB with and without predictor 2, PackBits), to
lumina_ocr_fax_decode (Group 4 bilevel; the fax codings have tools/fax_probe.py) or to lumina_ocr_flate_image_decode (Deflate), the last two strip by strip in place.  Beside
each, the same files decoded by Pillow / libtiff on one host thread.  lzw_rgb_one_strip is the LZW RGB page stored as ONE strip (every
/LZWDecode PDF page, some writers' TIFFs): it decodes on a single wave and is recorded apart.  Wall-clock per call (the calls
synchronise), median of --reps with the spread.  Each codec runs in a child process of its own under a time limit, and the first one that
fails ends the probe.  One JSON line; needs an MI355X and libtiff.  No threshold: the host decode is what each figure is compared with.

    python tools/tiff_probe.py [--reps 3] [--pages 64] [--codecs g4,lzw_grey,lzw_rgb,lzw_rgb_pred2,packbits,deflate,lzw_rgb_one_strip]"""
import argparse
import io
import json
import subprocess
import sys
import time
import types
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
for p in (ROOT, ROOT / "ocr-system_amd"):
    sys.path.insert(0, str(p))

W, H = 1654, 2339
CODECS = "g4,lzw_grey,lzw_rgb,lzw_rgb_pred2,packbits,deflate,lzw_rgb_one_strip"


def one_codec(name: str, args) -> dict:
    import numpy as np
    import torch
    from PIL import Image
    from lumina_ocr import synth
    from lumina_ocr.engine import Engine
    from lumina_ocr.services.ocr_service import OCRService
    from lumina_ocr.utils import tiff_pages

    eng = Engine(0)
    src = [synth.synth_page(H, W, 100 + k, n_lines=40)[0] for k in range(args.distinct)]
    n = args.pages
    files = []
    for page in src:
        op = io.BytesIO()
        if name == "g4":
            Image.fromarray(np.where(page.mean(axis=2) < 128, 0, 255).astype(np.uint8)).convert("1").save(op, "TIFF", compression="group4")
        elif name in ("lzw_grey", "packbits"):
            Image.fromarray(page).convert("L").save(op, "TIFF", compression="tiff_lzw" if name == "lzw_grey" else "packbits")
        elif name == "deflate":
            Image.fromarray(page).save(op, "TIFF", compression="tiff_adobe_deflate")
        else:
            info = {317: 2} if name == "lzw_rgb_pred2" else {}
            if name == "lzw_rgb_one_strip":
                info[278] = H
            Image.fromarray(page).save(op, "TIFF", compression="tiff_lzw", tiffinfo=info)
        files.append(op.getvalue())
    recs = []
    for f in files:
        (rec,) = tiff_pages.read_pages(f)
        if not isinstance(rec, tiff_pages.PageImage):
            raise SystemExit("%s: the reader refused the probe's own file: %s" % (name, rec.reason))
        rec.strips = [bytes(s) for s in rec.strips]
        recs.append(rec)
    batch = [recs[i % len(recs)] for i in range(n)]
    r0 = recs[0]
    if r0.codec in ("group4", "deflate"):
        me = types.SimpleNamespace(_device=0)
        dev = lambda: OCRService._decode_tiff_strips_in_place(me, eng, batch, W, H, r0.rows_per_strip, r0.codec == "group4")
    else:
        dev = lambda: eng.strip_image_decode([r.strips for r in batch], H, W, r0.rows_per_strip, [r.strip_params() for r in batch])
    host = lambda: [np.asarray(Image.open(io.BytesIO(files[i % len(files)])).convert("RGB")) for i in range(n)]

    def timed(fn, reps):
        times = []
        for i in range(reps + 1):
            t0 = time.perf_counter()
            out = fn()
            torch.cuda.synchronize()
            if i:
                times.append((time.perf_counter() - t0) * 1e3)
        return dict(median=round(float(np.median(times)), 2), min=round(min(times), 2), max=round(max(times), 2)), out

    t_dev, (out, status) = timed(dev, args.reps)
    t_host, ref = timed(host, max(1, min(args.reps, 2)))
    equal = all(status[i] == 0 and np.array_equal(out[i].cpu().numpy(), ref[i]) for i in range(min(n, len(src))))
    eng.close()
    return dict(file_kb=round(sum(len(f) for f in files) / len(files) / 1024, 1), strips_per_page=len(r0.strips), rows_per_strip=r0.rows_per_strip,
                device_ms=t_dev, host_ms=t_host, status_ok=list(status).count(0), equal_to_host=bool(equal),
                device_pages_per_s=round(n / t_dev["median"] * 1e3, 1), host_pages_per_s=round(n / t_host["median"] * 1e3, 1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--pages", type=int, default=64)
    ap.add_argument("--distinct", type=int, default=4)
    ap.add_argument("--codecs", default=CODECS)
    ap.add_argument("--step-timeout", type=int, default=240, help="seconds each codec's child process may take")
    ap.add_argument("--child", default="", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        print(json.dumps(one_codec(args.child, args)))
        return
    res = dict(pages=args.pages, height=H, width=W, distinct=args.distinct, reps=args.reps)
    for name in args.codecs.split(","):
        if name not in CODECS.split(","):
            raise SystemExit("unknown codec " + name)
        cmd = ["timeout", "-k", "10", str(args.step_timeout), sys.executable, __file__, "--child", name, "--reps", str(args.reps),
               "--pages", str(args.pages), "--distinct", str(args.distinct)]
        r = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
        if r.returncode != 0:      # a fault, an abort or the time limit: nothing more is started on the GPU
            res[name] = dict(failed=r.returncode)
            print(json.dumps(res))
            raise SystemExit("%s ended with status %d: the probe stops here" % (name, r.returncode))
        res[name] = json.loads(r.stdout.strip().splitlines()[-1])
    print(json.dumps(res))


if __name__ == "__main__":
    main()
