"""CPU: what `bench.py --dump-outputs` writes — the last step's per-page results flattened into float32 arrays that hold every
value exactly, the processed pages as a fixed seeded sample, all files together within the size limit."""
import importlib.util
import subprocess
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent


def _bench():
    spec = importlib.util.spec_from_file_location("bench_mod", ROOT / "bench.py")
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def _pages():
    from lumina_ocr.pipeline import PageDetections
    q = np.arange(24, dtype=np.int32).reshape(3, 8) * 1000
    return [PageDetections(q[:2], ["ab", "हि"], np.array([0.5, 0.25], np.float32), np.array([0.75, 1.0], np.float32), 1414, 2000),
            PageDetections(np.zeros((0, 8), np.int32), [], np.zeros(0, np.float32), np.zeros(0, np.float32), 1414, 2000),
            PageDetections(q[2:], ["x"], np.array([0.125], np.float32), np.array([0.5], np.float32), 1414, 2000)]


def test_output_arrays_flatten_the_pages_exactly(tmp_path):
    import torch
    bench = _bench()
    processed = torch.from_numpy(np.random.default_rng(7).integers(0, 256, (2, 40, 30, 3), dtype=np.uint8))
    out = bench.output_arrays(_pages(), processed)
    assert all(a.dtype == np.float32 for a in out.values())
    assert out["lines_per_page"].tolist() == [2, 0, 1]
    assert np.array_equal(out["quads"], np.arange(24).reshape(3, 8) * 1000)
    assert out["scores"].tolist() == [0.5, 0.25, 0.125] and out["det_scores"].tolist() == [0.75, 1.0, 0.5]
    assert out["text_codepoints"].tolist() == [[97, 98], [0x939, 0x93F], [120, -1]]
    idx = np.sort(np.random.default_rng(0).integers(0, processed.numel(), processed.numel()))   # the fixed seed: same bytes every run
    assert np.array_equal(out["processed_sample"], processed.numpy().ravel()[idx])
    bench.dump_outputs(tmp_path / "d", out)
    for name, a in out.items():
        assert np.array_equal(np.load(tmp_path / "d" / (name + ".npy")), a)


def test_dump_outputs_refuses_more_than_the_limit(tmp_path):
    import pytest
    bench = _bench()
    with pytest.raises(RuntimeError):
        bench.dump_outputs(tmp_path / "d", {"big": np.zeros(bench.DUMP_LIMIT // 4 + 1, np.float32)})
    assert not (tmp_path / "d").exists()


def test_dump_outputs_needs_the_real_engine():
    r = subprocess.run([sys.executable, str(ROOT / "bench.py"), "--dry-engine", "--backend", "gloo", "--dump-outputs", "x"],
                       capture_output=True, text=True, timeout=120, cwd=str(ROOT))
    assert r.returncode == 2 and "--dump-outputs" in r.stderr and not (ROOT / "x").exists()
