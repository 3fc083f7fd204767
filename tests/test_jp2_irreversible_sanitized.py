"""CPU, no GPU and no Python extension: the host parser with the irreversible option (csrc/jp2_parse.h) and the 9/7 functions the
kernels run (csrc/jp2_t1.h: dequantisation, windowed lifting, colour, rounding), compiled into the stand-alone program
tests/jp2_irreversible_main.cpp with -fsanitize=address,undefined and run as a child process.  The program must exit 0 (no sanitizer
report); its statuses are the restatement's (tests/jp2_irreversible_reference.py), its host decode of the intact cases gives Pillow's
bytes at several window lengths, and its decode of a sample of the damage sweep gives the restatement's.  Skips when the compiler has
no sanitizer runtime (a one-line program decides).  The test preloads nothing and leaves the environment as it finds it."""
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

import jp2_cases as jc
import jp2_irreversible_cases as ic
import jp2_irreversible_reference as ir

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "ocr-system_amd" / "csrc"

SANITIZE = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
STATIC = ["-static-libasan", "-static-libubsan"]   # the runtime inside the program: it then depends on no library's load order


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    tmp = tmp_path_factory.mktemp("jp2_irreversible")
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
    out = tmp / "jp2_irreversible_main"
    # -ffp-contract=off as the library is built: no fused multiply-add in the float path
    r = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-ffp-contract=off"] + flags +
                       ["-I", str(CSRC), str(ROOT / "tests" / "jp2_irreversible_main.cpp"), "-o", str(out)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return out


def run(program, tmp_path, files, pixels=None):
    """-> [(status, info, irreversible)] of the program over `files` (bytes objects), written to tmp_path; pixels: the window length"""
    names = []
    for i, data in enumerate(files):
        p = tmp_path / f"f{i:05d}.jp2"
        p.write_bytes(data)
        names.append(str(p))
    lst = tmp_path / "list.txt"
    lst.write_text("\n".join(names) + "\n")
    r = subprocess.run([str(program), str(lst)] + (["--pixels", str(pixels)] if pixels else []), capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    rows = [[int(v) for v in line.split()] for line in r.stdout.splitlines()]
    assert len(rows) == len(files)
    return [(row[0], row[1:9], row[9]) for row in rows], names


@pytest.mark.parametrize("window", [2, 6, 56, 256])
def test_intact_pixels(program, tmp_path, window):
    """2 and 6: windows shorter than their halo; 56 and 256: the kernels' (j2_dwt97_v, j2_dwt97_h)"""
    cases = ic.intact()
    got, names = run(program, tmp_path, [data for _, data in cases], pixels=window)
    for (name, data), (status, info, kind), path in zip(cases, got, names):
        assert (status, kind) == (0, 1), name
        exp = jc.expected(data)
        rgb = np.fromfile(path + ".rgb", np.uint8).reshape(exp.shape)
        assert np.array_equal(rgb, exp), name


@pytest.mark.parametrize("window", [6, 56])
def test_unusual_corpus_pixels(program, tmp_path, window):
    """tests/jp2_unusual_cases.py: the whole corpus has the restatement's statuses, and the host decode of every accepted 9/7 case is
    Pillow's (the 5/3 ones: tests/test_jp2_parser_sanitized.py), before tests/test_gpu_jp2_unusual.py sends the files to the device"""
    import jp2_unusual_cases as uc
    cases = uc.accepted() + uc.refused()
    got, names = run(program, tmp_path, [c.data for c in cases], pixels=window)
    n97 = 0
    for c, (status, info, kind), path in zip(cases, got, names):
        st, _, inf = ir.probe(c.data)
        assert (status, info) == (st, inf), c.name
        assert st == (-2 if c.family == "refused" else 0), c.name
        if st == 0:
            assert kind == int(c.irreversible), c.name
        if st == 0 and c.irreversible:
            exp = jc.expected(c.data)
            assert np.array_equal(np.fromfile(path + ".rgb", np.uint8).reshape(exp.shape), exp), c.name
            n97 += 1
    assert n97 >= 5


def test_refused_and_reversible_statuses(program, tmp_path):
    cases = ic.refused()
    got, _ = run(program, tmp_path, [data for _, data, _ in cases])
    assert [st for st, _, _ in got] == [-2] * len(cases)
    plain = jc.intact()[:10]
    got, _ = run(program, tmp_path, [data for _, data in plain])
    assert [(st, kind) for st, _, kind in got] == [(0, 0)] * len(plain)   # a 5/3 file is taken as before


def test_damage_sweep_statuses(program, tmp_path):
    sweep = ic.full_sweep()
    got, _ = run(program, tmp_path, [data for _, _, data in sweep])
    bad = []
    for (bname, name, data), (status, info, _) in zip(sweep, got):
        st, _, inf = ir.probe(data)
        if (status, info) != (st, inf):
            bad.append((bname, name, status, st, info, inf))
    assert not bad, (len(bad), bad[:10])


def test_damage_sample_pixels(program, tmp_path):
    """a seeded sample of the sweep (the files tests/test_gpu_jp2_irreversible.py sends to the device among them), decoded on the host
    first by the functions the kernels run"""
    sample = ic.sweep_sample(200, seed=9700)
    got, names = run(program, tmp_path, [data for _, _, data in sample], pixels=6)
    n_ok = 0
    for (bname, name, data), (status, info, _), path in zip(sample, got, names):
        st, _, inf, rgb = ir.reference(data)
        assert (status, info) == (st, inf), (bname, name)
        if st == 0:
            assert np.array_equal(np.fromfile(path + ".rgb", np.uint8).reshape(rgb.shape), rgb), (bname, name)
            n_ok += 1
    assert n_ok >= 50
