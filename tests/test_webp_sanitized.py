"""CPU, no GPU and no Python extension: the WebP host parser (csrc/webp_parse.h) and the functions the kernels run (csrc/webp_dec.h),
compiled into the stand-alone program tests/webp_main.cpp with -fsanitize=address,undefined and run as a child process.  Over the whole
damage sweep the program must exit 0 (no sanitizer report) with the restatement's statuses and pixels; over the intact cases its host
decode must give Pillow's bytes.  Skips when the compiler has no sanitizer runtime (a one-line program decides).  The test preloads
nothing and leaves the environment as it finds it; the runtime is linked into the program where the compiler can."""
import shutil
import struct
import subprocess
from pathlib import Path

import numpy as np
import pytest

import webp_cases as wc
import webp_reference as wr

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "ocr-system_amd" / "csrc"

SANITIZE = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
STATIC = ["-static-libasan", "-static-libubsan"]   # the runtime inside the program: it then depends on no library's load order


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    tmp = tmp_path_factory.mktemp("webp_main")
    # does this compiler have a sanitizer runtime at all?  A one-line program decides, so that any failure to compile the real one is an error.
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
    out = tmp / "webp_main"
    r = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-Wall"] + flags + ["-I", str(CSRC), str(ROOT / "tests" / "webp_main.cpp"),
                        "-o", str(out)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return out


def run(program, tmp_path, files):
    """-> ([(status, [width, height, alpha, vp8x, exif, xmp])], the RGB bytes of the accepted files one after another); the child
    inherits the environment as it is"""
    pack, rgb = tmp_path / "files.pack", tmp_path / "files.rgb"
    with open(pack, "wb") as f:
        for data in files:
            f.write(struct.pack("<I", len(data)))
            f.write(data)
    r = subprocess.run([str(program), str(pack), str(rgb)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    rows = [[int(v) for v in line.split()] for line in r.stdout.splitlines()]
    assert len(rows) == len(files)
    return [(row[0], row[1:]) for row in rows], np.fromfile(rgb, np.uint8)


def _info(data):
    rc, info, _ = wr.probe(data)
    return [info[k] for k in ("width", "height", "alpha", "vp8x", "exif", "xmp")]


def test_intact_pixels(program, tmp_path):
    cases = wc.intact_cases()
    got, rgb = run(program, tmp_path, [data for _, data in cases])
    o = 0
    for (name, data), (status, info) in zip(cases, got):
        assert status == 0 and info == _info(data), (name, status, info)
        want = wc.pillow_rgb(data).reshape(-1)
        assert np.array_equal(rgb[o:o + want.size], want), name
        o += want.size
    assert o == rgb.size


def test_refused_statuses(program, tmp_path):
    cases = wc.refused_cases()
    got, _ = run(program, tmp_path, [data for _, data in cases])
    assert [st for st, _ in got] == [-2] * len(cases)
    assert [info for _, info in got] == [_info(data) for _, data in cases]


def test_damage_sweep_statuses_and_pixels(program, tmp_path):
    sweep = wc.sweep_reference()
    got, rgb = run(program, tmp_path, [data for _, _, data, _, _ in sweep])
    o = 0
    bad = []
    for (name, kind, data, rc, px), (status, info) in zip(sweep, got):
        if status != rc or info != _info(data):
            bad.append((name, status, rc))
        if status == 0 and rc == 0:
            if not np.array_equal(rgb[o:o + px.size], px.reshape(-1)):
                bad.append((name, "pixels"))
        if status == 0:
            o += info[0] * info[1] * 3
    assert not bad, (len(bad), bad[:10])
