"""Device PNG decode (lumina_ocr_png_decode) against Pillow's Image.open(...).convert('RGB') on one host thread.

Two seeded corpora written by Pillow at its default compression from synth.synth_page: clean text pages, and the same pages with heavy
seeded noise (standing in for scans).  Each at 1654x2339 and 2480x3508 (A4 at 200 / 300 dpi), n = 1 and n = 64 (4 distinct pages,
each repeated 16 times).  Device: host clock around a synchronise, best of 3 after a warm-up call; Pillow: one pass over the files.
Prints one JSON line per (corpus, size, n).  usage: pngdec_bench.py [--sizes 1654x2339,2480x3508] [--n 1,64]"""
import argparse
import io
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "ocr-system_amd"))
from PIL import Image  # noqa: E402

from lumina_ocr import synth  # noqa: E402
from lumina_ocr.engine import Engine  # noqa: E402


def corpus(kind, w, h, distinct=4):
    files = []
    for k in range(distinct):
        page = synth.synth_page(h, w, 100 + k, n_lines=60)[0]
        if kind == "noisy":
            rng = np.random.default_rng(500 + k)
            page = np.clip(page.astype(np.int16) + rng.normal(0, 24, page.shape).astype(np.int16), 0, 255).astype(np.uint8)
        b = io.BytesIO()
        Image.fromarray(page).save(b, "PNG")
        files.append(b.getvalue())
    return files


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="1654x2339,2480x3508")
    ap.add_argument("--n", default="1,64")
    args = ap.parse_args()
    import torch
    eng = Engine(0)
    for size in args.sizes.split(","):
        w, h = (int(v) for v in size.split("x"))
        for kind in ("clean", "noisy"):
            distinct = corpus(kind, w, h)
            for n in (int(v) for v in args.n.split(",")):
                files = [distinct[i % len(distinct)] for i in range(n)]
                out = torch.empty((n, h, w, 3), dtype=torch.uint8, device="cuda")
                _, st = eng.png_decode(files, h, w, out=out)
                torch.cuda.synchronize()
                assert st == [0] * n, st
                dev = []
                for _ in range(3):
                    t = time.perf_counter()
                    eng.png_decode(files, h, w, out=out)
                    torch.cuda.synchronize()
                    dev.append(time.perf_counter() - t)
                t = time.perf_counter()
                for f in files:
                    Image.open(io.BytesIO(f)).convert("RGB").load()
                pil = time.perf_counter() - t
                assert np.array_equal(out[0].cpu().numpy(), np.asarray(Image.open(io.BytesIO(files[0])).convert("RGB")))
                print(json.dumps({"corpus": kind, "width": w, "height": h, "n": n, "mean_png_bytes": int(np.mean([len(f) for f in distinct])),
                                  "raw_bytes": w * h * 3, "device_ms": round(min(dev) * 1e3, 2), "pillow_ms": round(pil * 1e3, 2),
                                  "device_pages_per_s": round(n / min(dev), 2), "pillow_pages_per_s": round(n / pil, 2)}), flush=True)
    eng.close()


if __name__ == "__main__":
    main()
