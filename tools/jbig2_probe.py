"""Times the JBIG2 decoder (lumina_ocr_jbig2_decode): 64 A4 text pages (one synth page, repeated) at 200 dpi (1654 x 2339) and at 300 dpi
(2481 x 3508), each as one generic region coded four ways -- template 0 with typical prediction, template 0 without, template 3, MMR --
and one page alone.  Beside each, lumina_ocr_fax_decode (Group 4) on the same bitmap in the same run: no JBIG2 decoder exists on the
host to time against, so the fax decoder is the yardstick.  An arithmetic-coded region is one serial stream decoded by one lane, so
one page alone takes about as long as the batch.  Wall-clock per call (the calls synchronise), median of --reps with the spread.  Each
case runs in a child process of its own under a time limit, and the first one that fails ends the probe.  Writes
profiles/jbig2_probe.json and prints it; needs an MI355X and libtiff.  No threshold.

The streams are made by the test-side encoder (tests/jbig2_writer.py), which is plain Python and takes seconds a page at these
sizes: --streams DIR keeps them between runs (made when missing).  The split of the device time between jb2_generic and jb2_page comes
from a kernel trace of `--trace CASE@DPI` (rocprofv3 --kernel-trace --stats -- python tools/jbig2_probe.py --trace t0@200 ...), in a
run of its own.

    python tools/jbig2_probe.py [--reps 20] [--pages 64] [--dpis 200,300] [--cases t0_tpgd,t0,t3,mmr] [--streams DIR] [--make-only] [--trace CASE@DPI]"""
import argparse
import json
import subprocess
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
for p in (ROOT, ROOT / "ocr-system_amd", ROOT / "tests"):
    sys.path.insert(0, str(p))

SIZES = {200: (1654, 2339), 300: (2481, 3508)}
CASES = {"t0_tpgd": dict(tmpl=0, tpgd=True), "t0": dict(tmpl=0), "t3": dict(tmpl=3), "mmr": dict(mmr=True)}


def ink(dpi: int):
    import numpy as np
    from lumina_ocr import synth
    w, h = SIZES[dpi]
    return (synth.synth_page(h, w, 100, n_lines=40 * dpi // 200)[0].mean(axis=2) < 128).astype(np.uint8)


def stream_for(case: str, dpi: int, cache):
    import jbig2_writer as jw
    path = None if cache is None else Path(cache) / ("%s_%d.jb2" % (case, dpi))
    if path is not None and path.exists():
        return path.read_bytes()
    bm = ink(dpi)
    data = jw.page(bm.shape[1], bm.shape[0], [dict(bitmap=bm, **CASES[case])])
    if path is not None:
        path.parent.mkdir(parents=True, exist_ok=True)
        path.write_bytes(data)
    return data


def one_case(case: str, dpi: int, args) -> dict:
    import numpy as np
    import torch
    import ccitt_cases as cc
    from lumina_ocr.engine import Engine

    eng = Engine(0)
    w, h = SIZES[dpi]
    bm = ink(dpi)
    stream = stream_for(case, dpi, args.streams)
    g4 = cc.g4_encode(bm.astype(bool))
    want = np.repeat(np.where(bm, 0, 255).astype(np.uint8)[:, :, None], 3, axis=2)

    def timed(fn, reps):
        times = []
        for i in range(reps + 1):
            t0 = time.perf_counter()
            out = fn()
            torch.cuda.synchronize()
            if i:
                times.append((time.perf_counter() - t0) * 1e3)
        return dict(median=round(float(np.median(times)), 2), min=round(min(times), 2), max=round(max(times), 2)), out

    res = dict(stream_kb=round(len(stream) / 1024, 1), group4_kb=round(len(g4) / 1024, 1))
    for n in (args.pages, 1):
        buf = torch.empty((n, h, w, 3), dtype=torch.uint8, device="cuda")
        t_jb2, (out, status) = timed(lambda: eng.jbig2_decode([stream] * n, h, w, out=buf), args.reps)
        equal = status == [0] * n and bool((out[0].cpu().numpy() == want).all()) and bool((out[n - 1].cpu().numpy() == want).all())
        t_fax, (fout, fstatus) = timed(lambda: eng.fax_decode([g4] * n, h, w, [(-1, 0, 0, 0, 0)] * n, out=buf), args.reps)
        fequal = fstatus == [0] * n and bool((fout[0].cpu().numpy() == want).all())
        res["pages_%d" % n] = dict(jbig2_ms=t_jb2, fax_group4_ms=t_fax, jbig2_pages_per_s=round(n / t_jb2["median"] * 1e3, 2),
                                   fax_pages_per_s=round(n / t_fax["median"] * 1e3, 2), equal_to_source=bool(equal), fax_equal_to_source=bool(fequal))
    eng.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--pages", type=int, default=64)
    ap.add_argument("--dpis", default="200,300")
    ap.add_argument("--cases", default=",".join(CASES))
    ap.add_argument("--streams", default=None, help="directory that keeps the encoded streams between runs")
    ap.add_argument("--make-only", action="store_true", help="encode the streams into --streams and stop (no GPU)")
    ap.add_argument("--step-timeout", type=int, default=300, help="seconds each case's child process may take")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "jbig2_probe.json"))
    ap.add_argument("--trace", default="", help="CASE@DPI: that case alone in this process, one warm-up and one timed call of each kind (for a kernel trace)")
    ap.add_argument("--child", default="", help=argparse.SUPPRESS)
    args = ap.parse_args()
    dpis = [int(d) for d in args.dpis.split(",")]
    if args.trace:
        args.child, args.reps = args.trace, 1
    if args.child:
        case, dpi = args.child.split("@")
        print(json.dumps(one_case(case, int(dpi), args)))
        return
    for name in args.cases.split(","):
        if name not in CASES:
            raise SystemExit("unknown case " + name)
    if args.make_only:
        for dpi in dpis:
            for name in args.cases.split(","):
                print(name, dpi, len(stream_for(name, dpi, args.streams)), flush=True)
        return
    res = dict(pages=args.pages, reps=args.reps, sizes={str(d): SIZES[d] for d in dpis})
    for dpi in dpis:
        for name in args.cases.split(","):
            key = "%s_%ddpi" % (name, dpi)
            cmd = ["timeout", "-k", "10", str(args.step_timeout), sys.executable, __file__, "--child", "%s@%d" % (name, dpi), "--reps", str(args.reps),
                   "--pages", str(args.pages)] + (["--streams", args.streams] if args.streams else [])
            r = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
            if r.returncode != 0:      # a fault, an abort or the time limit: nothing more is started on the GPU
                res[key] = dict(failed=r.returncode)
                print(json.dumps(res))
                raise SystemExit("%s ended with status %d: the probe stops here" % (key, r.returncode))
            res[key] = json.loads(r.stdout.strip().splitlines()[-1])
            print(key, json.dumps(res[key]), flush=True)
    Path(args.out).write_text(json.dumps(res, indent=1) + "\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
