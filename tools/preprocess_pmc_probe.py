"""Developer probe: the four byte-exact pre-processing kernels alone at the bench's sizes (64 synthetic A4 pages, 2339x1654 ->
2000x1414: Lanczos H, Lanczos V, gray sum, contrast + sharpness), for rocprofv3 --pmc passes (counters only, no tracing) and
tools/pmc_summary.py.  usage: preprocess_pmc_probe.py [reps]"""
import os, sys
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "ocr-system_amd"))
import torch
import bench
from lumina_ocr.engine import Engine

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 4
eng = Engine(0)
pages = bench.make_pages(torch, 64, 2024, torch.device("cuda", 0))
for _ in range(reps):
    small = eng.resize_lanczos(pages, 2000, 1414)
    out = eng.enhance(small, 1.2, 1.1)
torch.cuda.synchronize()
print("pages", tuple(pages.shape), "->", tuple(out.shape), "reps", reps)
eng.close()
