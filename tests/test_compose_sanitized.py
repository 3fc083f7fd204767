"""CPU, no GPU and no Python extension: the table check and the per-pixel function of lumina_ocr_page_compose (csrc/compose.h),
compiled into the stand-alone program tests/compose_main.cpp with -fsanitize=address,undefined and run as a child process over the GPU
test's tables (pdf_layer_tables.py).  The program must exit 0 (no sanitizer report), give the restatement's bytes for every accepted
table and reject every hostile one.  Skips when the compiler has no sanitizer runtime (a one-line program decides).  The test preloads
nothing and leaves the environment as it finds it."""
import shutil
import struct
import subprocess
from pathlib import Path

import numpy as np
import pytest

import pdf_layer_tables as lt
import pdf_layers_reference as lr

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "ocr-system_amd" / "csrc"
SANITIZE = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
STATIC = ["-static-libasan", "-static-libubsan"]   # the runtime inside the program: it then depends on no library's load order


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    tmp = tmp_path_factory.mktemp("compose")
    one = tmp / "one.cpp"
    one.write_text("int main() { return 0; }\n")
    flags = None
    for extra in (STATIC, []):
        r = subprocess.run([cxx, "-std=c++17"] + SANITIZE + extra + [str(one), "-o", str(tmp / "one")], capture_output=True, text=True)
        if r.returncode == 0 and subprocess.run([str(tmp / "one")], capture_output=True).returncode == 0:
            flags = SANITIZE + extra
            break
    if flags is None:
        pytest.skip("the compiler has no sanitizer runtime that starts here: " + (r.stderr.strip().splitlines() or ["(the one-line program did not run)"])[-1])
    out = tmp / "compose_main"
    r = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer"] + flags + ["-I", str(CSRC), str(ROOT / "tests" / "compose_main.cpp"),
                        "-o", str(out)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return out


def table_bytes(canvas_hw, n, layers) -> bytes:
    out = bytearray(struct.pack("<4i", n, canvas_hw[0], canvas_hw[1], len(layers)))
    for page, kind, (x0, y0, x1, y1), flip, fill, src, mask in layers:
        sh, sw = (0, 0) if src is None else src.shape[:2]
        mh, mw = (0, 0) if mask is None else mask.shape[:2]
        out += struct.pack("<14i", page, kind, x0, y0, x1, y1, flip, fill[0] | fill[1] << 8 | fill[2] << 16, sw, sh, mw, mh, src is not None, mask is not None)
        for img in (src, mask):
            if img is not None:
                out += np.ascontiguousarray(img).tobytes()
    return bytes(out)


def run(program, tmp_path, tables):
    """-> [(first output line, pages or None)] of the program over tables [(canvas_hw, n, layers)]"""
    lines = []
    for i, (hw, n, layers) in enumerate(tables):
        (tmp_path / f"t{i:03d}.bin").write_bytes(table_bytes(hw, n, layers))
        lines.append("%s %s" % (tmp_path / f"t{i:03d}.bin", tmp_path / f"o{i:03d}.bin"))
    (tmp_path / "list.txt").write_text("\n".join(lines) + "\n")
    r = subprocess.run([str(program), str(tmp_path / "list.txt")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    said = r.stdout.splitlines()
    assert len(said) == len(tables)
    out = []
    for i, ((hw, n, _), line) in enumerate(zip(tables, said)):
        pages = np.fromfile(tmp_path / f"o{i:03d}.bin", np.uint8).reshape(n, hw[0], hw[1], 3) if line == "ok" else None
        out.append((line, pages))
    return out


def test_the_gpu_tests_tables_give_the_restatements_bytes(program, tmp_path):
    cases = lt.cases()
    got = run(program, tmp_path, [(hw, n, layers) for _, hw, n, layers in cases])
    for (name, hw, n, layers), (line, pages) in zip(cases, got):
        assert line == "ok", (name, line)
        assert np.array_equal(pages, lr.compose(hw, n, layers)), name


def test_hostile_tables_are_rejected(program, tmp_path):
    host = np.zeros((4, 4, 3), np.uint8)
    tables = lt.hostile(host, host[:0])
    assert not any(lr.compose_params_ok(t, 1, 9, 20) for t in tables)
    got = run(program, tmp_path, [((9, 20), 1, t) for t in tables] + [((0, 20), 1, []), ((9, 65536), 1, [])])
    assert all(line.startswith("rejected: ") and pages is None for line, pages in got), [line for line, _ in got]
    assert len({line for line, _ in got}) >= 9   # each for its own reason
