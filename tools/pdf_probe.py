"""Times the scanned-PDF decoders: 64 A4@200DPI pages (1654 x 2339; --distinct different synth pages, repeated) per filter, as the
provider's LUMINA_OCR_PDF_SCANS path hands them over: CCITT Group 4 streams to lumina_ocr_ccitt_decode, Flate streams (RGB, PNG
predictor 15, and 8-bit grey with the TIFF predictor 2) to lumina_ocr_flate_image_decode, DCT streams to lumina_ocr_jpeg_decode.  Beside
each, the same streams decoded on the host, one thread: libtiff through Pillow for Group 4 (the strip in the TIFF file it came from),
Pillow for the JPEG, Pillow's PNG decoder for the predictor-15 stream (the stream is a PNG's IDAT; wrapped in IHDR / IEND), zlib + a
numpy prefix sum for predictor 2.  Wall-clock per call (the calls synchronise), median of --reps with the spread.  One JSON line; needs
an MI355X and libtiff.  No threshold: the host decode is what each figure is compared with.

    python tools/pdf_probe.py [--reps 5] [--pages 64] [--filters g4,dct,flate_rgb,flate_grey]"""
import argparse
import io
import json
import struct
import sys
import time
import zlib
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
for p in (ROOT, ROOT / "ocr-system_amd"):
    sys.path.insert(0, str(p))

W, H = 1654, 2339


def png_wrap(idat: bytes, w: int, h: int, colour_type: int) -> bytes:
    def chunk(t, d):
        return struct.pack(">I", len(d)) + t + d + struct.pack(">I", zlib.crc32(t + d))
    return b"\x89PNG\r\n\x1a\n" + chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, 8, colour_type, 0, 0, 0)) + chunk(b"IDAT", idat) + chunk(b"IEND", b"")


def sub_filter(rows, bpp):
    import numpy as np
    a = rows.astype(np.int16)
    d = a.copy()
    d[:, bpp:] -= a[:, :-bpp]
    return np.concatenate([np.ones((rows.shape[0], 1), np.uint8), (d & 255).astype(np.uint8)], axis=1).tobytes()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--pages", type=int, default=64)
    ap.add_argument("--distinct", type=int, default=4)
    ap.add_argument("--filters", default="g4,dct,flate_grey,flate_rgb")
    args = ap.parse_args()
    import numpy as np
    import torch
    from PIL import Image
    from lumina_ocr import synth
    from lumina_ocr.engine import Engine

    eng = Engine(0)
    src = [synth.synth_page(H, W, 100 + k, n_lines=40)[0] for k in range(args.distinct)]
    n = args.pages

    def timed(fn, reps):
        times = []
        for i in range(reps + 1):
            t0 = time.perf_counter()
            out = fn()
            torch.cuda.synchronize()
            if i:
                times.append((time.perf_counter() - t0) * 1e3)
        return dict(median=round(float(np.median(times)), 2), min=round(min(times), 2), max=round(max(times), 2)), out

    res = dict(pages=n, height=H, width=W, distinct=args.distinct, reps=args.reps)
    for name in args.filters.split(","):
        if name == "g4":
            tiffs, strips = [], []
            for page in src:
                op = io.BytesIO()
                Image.fromarray(np.where(page.mean(axis=2) < 128, 255, 0).astype(np.uint8)).convert("1").save(
                    op, "TIFF", compression="group4", strip_size=((W + 7) // 8) * H)
                t = Image.open(io.BytesIO(op.getvalue()))
                tiffs.append(op.getvalue())
                strips.append(op.getvalue()[t.tag_v2[273][0]:t.tag_v2[273][0] + t.tag_v2[279][0]])
            streams = [strips[i % len(strips)] for i in range(n)]
            dev = lambda: eng.ccitt_decode(streams, H, W, [(-1, 0, 1, 0)] * n)   # BlackIsZero TIFF: a coded-black run is 255, as BlackIs1 shows it
            host = lambda: [np.asarray(Image.open(io.BytesIO(tiffs[i % len(tiffs)])).convert("RGB")) for i in range(n)]
        elif name == "dct":
            files = []
            for page in src:
                op = io.BytesIO()
                Image.fromarray(page).save(op, "JPEG", quality=85)
                files.append(op.getvalue())
            streams = [files[i % len(files)] for i in range(n)]
            dev = lambda: eng.jpeg_decode(streams, H, W)
            host = lambda: [np.asarray(Image.open(io.BytesIO(s)).convert("RGB")) for s in streams]
        elif name == "flate_rgb":
            idats = [zlib.compress(sub_filter(page.reshape(H, -1), 3), 6) for page in src]
            streams = [idats[i % len(idats)] for i in range(n)]
            pngs = [png_wrap(s, W, H, 2) for s in idats]
            dev = lambda: eng.flate_image_decode(streams, H, W, [(15, 3, 8, 0, 0)] * n)
            host = lambda: [np.asarray(Image.open(io.BytesIO(pngs[i % len(pngs)])).convert("RGB")) for i in range(n)]
        elif name == "flate_grey":
            greys = [np.ascontiguousarray(page[:, :, 1]) for page in src]
            raws = []
            for g in greys:
                d = g.astype(np.int16)
                d[:, 1:] -= g[:, :-1].astype(np.int16)
                raws.append(zlib.compress((d & 255).astype(np.uint8).tobytes(), 6))
            streams = [raws[i % len(raws)] for i in range(n)]
            dev = lambda: eng.flate_image_decode(streams, H, W, [(2, 1, 8, 0, 0)] * n)

            def host():
                out = []
                for s in streams:
                    g = np.cumsum(np.frombuffer(zlib.decompress(s), np.uint8).reshape(H, W), axis=1, dtype=np.uint8)
                    out.append(np.repeat(g[:, :, None], 3, axis=2))
                return out
        else:
            raise SystemExit("unknown filter " + name)
        t_dev, (out, status) = timed(dev, args.reps)
        t_host, ref = timed(host, max(1, min(args.reps, 2)))
        equal = all(status[i] == 0 and np.array_equal(out[i].cpu().numpy(), ref[i]) for i in range(min(n, len(src))))
        res[name] = dict(stream_kb=round(sum(len(s) for s in streams) / n / 1024, 1), device_ms=t_dev, host_ms=t_host,
                         status_ok=status.count(0), equal_to_host=bool(equal),
                         device_pages_per_s=round(n / t_dev["median"] * 1e3, 1), host_pages_per_s=round(n / t_host["median"] * 1e3, 1))
    print(json.dumps(res))
    eng.close()


if __name__ == "__main__":
    main()
