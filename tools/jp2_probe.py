"""Times the JPEG 2000 decode (lumina_ocr_jp2_decode): A4@200DPI text pages (1654 x 2339; --distinct different synth pages, repeated)
written by Pillow (OpenJPEG) with the 5/3 reversible transform:
  * `rgb_lossless`, `grey_lossless`      lossless files;
  * `rgb_layers20`, `grey_layers20`      quality_layers=[20] (rate 20: blocks stop early);
each as a batch of --pages pages in one call and as one page alone.  Wall-clock per call (the calls synchronise), median of --reps with
min and max after one warm-up call.  Beside each, Pillow on one host thread over the distinct files, median of --host-reps, per page
(host_batch_ms is that figure times the number of pages), and the host walk over the packet headers alone (tier 2: lumina_ocr_jp2_probe)
per page.  The split of the device time between tier 1 and the DWT comes from a kernel trace of `--trace CASE` (one warm-up call and one
timed call of that case, nothing else), in a run of its own.  Writes profiles/jp2_probe.json and prints it; needs an MI355X.  No
threshold: the host decode is what each figure is compared with.

--irreversible times lumina_ocr_jp2_decode_irreversible instead, on the 9/7 files an `irreversible=True` writer produces:
  * `rgb97_default`, `grey97_default`    the writer's default rate;
  * `rgb97_layers20`, `grey97_layers20`  quality_layers=[20];
and, through the same entry in the same run, the 5/3 `rgb_layers20` / `grey_layers20` files to set them beside.  It writes
profiles/jp2_irreversible_probe.json; `--trace CASE` splits tier 1, the 9/7 lifting (j2_dwt97_h / j2_dwt97_v) and the finish.

--tiles times lumina_ocr_jp2_decode_ex (both flags) on tiled files: `rgb_lossless` and `grey_layers20`, 5/3 and 9/7 (`rgb97_default`,
`grey97_layers20`), each written with tile_size=(256, 256) (`..._t256`) and (1024, 1024) (`..._t1024`) and as a one-tile file
(`..._one`), the yardstick: the three go through the same entry in the same run, their repetitions interleaved.  It writes
profiles/jp2_tiles_probe.json; `--trace CASE` (for instance rgb_lossless_t256) splits tier 1, the transforms and the rest.

    python tools/jp2_probe.py [--irreversible | --tiles] [--reps 20] [--pages 64] [--host-reps 3] [--cases ...] [--trace CASE]"""
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
CASES = {"rgb_lossless": ("RGB", {}), "grey_lossless": ("L", {}), "rgb_layers20": ("RGB", {"quality_layers": [20]}),
         "grey_layers20": ("L", {"quality_layers": [20]})}
CASES97 = {"rgb97_default": ("RGB", {"irreversible": True}), "grey97_default": ("L", {"irreversible": True}),
           "rgb97_layers20": ("RGB", {"irreversible": True, "quality_layers": [20]}),
           "grey97_layers20": ("L", {"irreversible": True, "quality_layers": [20]}),
           "rgb_layers20": CASES["rgb_layers20"], "grey_layers20": CASES["grey_layers20"]}
TILINGS = {"one": {}, "t256": {"tile_size": (256, 256)}, "t1024": {"tile_size": (1024, 1024)}}
CASES_TILES = {f"{name}_{t}": (mode, dict(opts, **topts))
               for name, (mode, opts) in (("rgb_lossless", CASES["rgb_lossless"]), ("grey_layers20", CASES["grey_layers20"]),
                                          ("rgb97_default", CASES97["rgb97_default"]), ("grey97_layers20", CASES97["grey97_layers20"]))
               for t, topts in TILINGS.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--host-reps", type=int, default=3)
    ap.add_argument("--pages", type=int, default=64)
    ap.add_argument("--distinct", type=int, default=4)
    ap.add_argument("--irreversible", action="store_true")
    ap.add_argument("--tiles", action="store_true")
    ap.add_argument("--cases", default="")
    ap.add_argument("--trace", default="")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    cases = CASES_TILES if args.tiles else CASES97 if args.irreversible else CASES
    args.cases = args.cases or ",".join(cases)
    args.out = args.out or str(ROOT / "profiles" / ("jp2_tiles_probe.json" if args.tiles else "jp2_irreversible_probe.json" if args.irreversible else "jp2_probe.json"))
    import numpy as np
    import torch
    from PIL import Image
    from lumina_ocr import synth
    from lumina_ocr.engine import Engine

    eng = Engine(0)
    decode = eng.jp2_decode_irreversible if args.irreversible else eng.jp2_decode
    probe = Engine.jp2_probe_irreversible if args.irreversible else Engine.jp2_probe
    if args.tiles:
        both = Engine.JP2_F_IRREVERSIBLE | Engine.JP2_F_TILES
        decode = lambda files, h, w, out=None: eng.jp2_decode_ex(files, h, w, both, out=out)   # noqa: E731
        probe = lambda data: Engine.jp2_probe_ex(data, both)                                    # noqa: E731
    src = [synth.synth_page(H, W, 100 + k, n_lines=40)[0] for k in range(args.distinct)]

    def write(mode, opts):
        files = []
        for page in src:
            op = io.BytesIO()
            Image.fromarray(page if mode == "RGB" else np.ascontiguousarray(page[:, :, 1])).save(op, "JPEG2000", **dict(dict(irreversible=False), **opts))
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

    res = dict(pages=args.pages, height=H, width=W, distinct=args.distinct, reps=args.reps, host_reps=args.host_reps)
    if args.tiles:
        # the tilings of one content side by side: a repetition is one call of each, in turn
        names = args.cases.split(",")
        for base in dict.fromkeys(n.rsplit("_", 1)[0] for n in names):
            group = [n for n in names if n.rsplit("_", 1)[0] == base]
            files = {n: write(*cases[n]) for n in group}
            ref = {n: [np.asarray(Image.open(io.BytesIO(s)).convert("RGB")) for s in files[n]] for n in group}
            for n in group:
                t_tier2, probes = timed(lambda: [probe(s) for s in files[n]], args.host_reps, sync=False)
                res[n] = dict(file_kb=round(sum(len(s) for s in files[n]) / len(files[n]) / 1024, 1), probe_status=[rc for rc, _ in probes],
                              tier2_host_ms_per_page=round(t_tier2["median"] / len(files[n]), 3))
            for label, npg in (("batch", args.pages), ("single", 1)):
                out_buf = torch.empty((npg, H, W, 3), dtype=torch.uint8, device="cuda")
                streams = {n: [files[n][i % len(files[n])] for i in range(npg)] for n in group}
                times = {n: [] for n in group}
                for i in range(args.reps + 1):
                    for n in group:
                        t0 = time.perf_counter()
                        out, status = decode(streams[n], H, W, out=out_buf)
                        torch.cuda.synchronize()
                        if i:
                            times[n].append((time.perf_counter() - t0) * 1e3)
                        else:
                            equal = all(status[k] == 0 and np.array_equal(out[k].cpu().numpy(), ref[n][k]) for k in range(min(npg, len(files[n]))))
                            res[n][label] = dict(pages=npg, status_ok=status.count(0), equal_to_host=bool(equal))
                for n in group:
                    t = times[n]
                    res[n][label]["device_ms"] = dict(median=round(float(np.median(t)), 2), min=round(min(t), 2), max=round(max(t), 2))
                    res[n][label]["device_pages_per_s"] = round(npg / float(np.median(t)) * 1e3, 1)
                    if base + "_one" in times:   # (the yardstick by name; absent when --cases leaves the one-tile file out)
                        res[n][label]["vs_one_tile"] = round(float(np.median(t)) / float(np.median(times[base + "_one"])), 3)
    for name in ([] if args.tiles else args.cases.split(",")):
        files = write(*cases[name])
        t_host, ref = timed(lambda: [np.asarray(Image.open(io.BytesIO(s)).convert("RGB")) for s in files], args.host_reps, sync=False)
        t_tier2, probes = timed(lambda: [probe(s) for s in files], args.host_reps, sync=False)
        host_page = t_host["median"] / len(files)
        entry = dict(file_kb=round(sum(len(s) for s in files) / len(files) / 1024, 1), probe_status=[rc for rc, _ in probes],
                     host_ms_per_page=round(host_page, 2), host_ms_distinct=t_host, tier2_host_ms_per_page=round(t_tier2["median"] / len(files), 3))
        for label, n in (("batch", args.pages), ("single", 1)):
            streams = [files[i % len(files)] for i in range(n)]
            out_buf = torch.empty((n, H, W, 3), dtype=torch.uint8, device="cuda")
            t_dev, (out, status) = timed(lambda: decode(streams, H, W, out=out_buf), args.reps)
            equal = all(status[i] == 0 and np.array_equal(out[i].cpu().numpy(), ref[i]) for i in range(min(n, len(files))))
            entry[label] = dict(pages=n, device_ms=t_dev, host_batch_ms=round(host_page * n, 1), status_ok=status.count(0), equal_to_host=bool(equal),
                                device_pages_per_s=round(n / t_dev["median"] * 1e3, 1), host_pages_per_s=round(1e3 / host_page, 1))
        res[name] = entry
    text = json.dumps(res)
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(text + "\n")
    print(text)
    eng.close()


if __name__ == "__main__":
    main()
