"""Times the progressive JPEG decode (lumina_ocr_jpeg_decode_progressive): A4@200DPI text pages (1654 x 2339; --distinct different
synth pages, repeated) written by Pillow with progressive=True at quality 90, Pillow's default scan script:
  * `batch`      --pages pages in one call;
  * `single`     one such page alone;
  * `batch_rst`  the same pages written with restart_marker_rows=1 (one restart segment per MCU row: the unit of parallel work);
  * `baseline`   the same pages as sequential files through the same entry (the existing kernels), for scale.
Beside each, the same files decoded by Pillow on one host thread.  Wall-clock per call (the calls synchronise), median of --reps with
min and max after one warm-up call.  One JSON line; needs an MI355X.  No threshold: the host decode is what each figure is compared with.

    python tools/progressive_probe.py [--reps 20] [--pages 64] [--host-reps 3]"""
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--host-reps", type=int, default=3)
    ap.add_argument("--pages", type=int, default=64)
    ap.add_argument("--distinct", type=int, default=4)
    ap.add_argument("--cases", default="batch,single,batch_rst,baseline")
    args = ap.parse_args()
    import numpy as np
    import torch
    from PIL import Image
    from lumina_ocr import synth
    from lumina_ocr.engine import Engine

    eng = Engine(0)
    src = [synth.synth_page(H, W, 100 + k, n_lines=40)[0] for k in range(args.distinct)]

    def write(**kw):
        files = []
        for page in src:
            op = io.BytesIO()
            Image.fromarray(page).save(op, "JPEG", quality=90, **kw)
            files.append(op.getvalue())
        return files

    def timed(fn, reps):
        times = []
        for i in range(reps + 1):
            t0 = time.perf_counter()
            out = fn()
            torch.cuda.synchronize()
            if i:
                times.append((time.perf_counter() - t0) * 1e3)
        return dict(median=round(float(np.median(times)), 2), min=round(min(times), 2), max=round(max(times), 2)), out

    res = dict(pages=args.pages, height=H, width=W, distinct=args.distinct, reps=args.reps, host_reps=args.host_reps)
    for name in args.cases.split(","):
        files = write(**{"batch": dict(progressive=True), "single": dict(progressive=True), "batch_rst": dict(progressive=True, restart_marker_rows=1),
                         "baseline": dict()}[name])
        n = 1 if name == "single" else args.pages
        streams = [files[i % len(files)] for i in range(n)]
        out_buf = torch.empty((n, H, W, 3), dtype=torch.uint8, device="cuda")
        t_dev, (out, status) = timed(lambda: eng.jpeg_decode_progressive(streams, H, W, out=out_buf), args.reps)
        t_host, ref = timed(lambda: [np.asarray(Image.open(io.BytesIO(s)).convert("RGB")) for s in streams], args.host_reps)
        equal = all(status[i] == 0 and np.array_equal(out[i].cpu().numpy(), ref[i]) for i in range(min(n, len(files))))
        res[name] = dict(file_kb=round(sum(len(s) for s in streams) / n / 1024, 1), scans=Engine.jpeg_probe_progressive(streams[0])[1]["scans"],
                         device_ms=t_dev, host_ms=t_host, status_ok=status.count(0), equal_to_host=bool(equal),
                         device_pages_per_s=round(n / t_dev["median"] * 1e3, 1), host_pages_per_s=round(n / t_host["median"] * 1e3, 1))
    print(json.dumps(res))
    eng.close()


if __name__ == "__main__":
    main()
