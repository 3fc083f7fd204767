"""CPU, no GPU and no Python extension: the JPEG 2000 host parser (csrc/jp2_parse.h) and the tier-1 / lifting functions the kernels run
(csrc/jp2_t1.h), compiled into the stand-alone program tests/jp2_parse_main.cpp with -fsanitize=address,undefined and run as a child
process.  Over the whole damage sweep the program must exit 0 (no sanitizer report) with the restatement's statuses; over the intact
cases its host decode must give Pillow's bytes.  Skips when the compiler has no sanitizer runtime (a one-line program decides).  The
test preloads nothing and leaves the environment as it finds it; the runtime is linked into the program where the compiler can."""
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

import jp2_cases as jc
import jp2_reference as jr

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "ocr-system_amd" / "csrc"


SANITIZE = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
STATIC = ["-static-libasan", "-static-libubsan"]   # the runtime inside the program: it then depends on no library's load order


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    tmp = tmp_path_factory.mktemp("jp2_parse")
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
    out = tmp / "jp2_parse_main"
    r = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer"] + flags + ["-I", str(CSRC), str(ROOT / "tests" / "jp2_parse_main.cpp"),
                        "-o", str(out)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return out


def run(program, tmp_path, files, pixels=False):
    """-> [(status, info)] of the program over `files` (bytes objects), written to tmp_path; the child inherits the environment as it is"""
    names = []
    for i, data in enumerate(files):
        p = tmp_path / f"f{i:05d}.jp2"
        p.write_bytes(data)
        names.append(str(p))
    lst = tmp_path / "list.txt"
    lst.write_text("\n".join(names) + "\n")
    r = subprocess.run([str(program), str(lst)] + (["--pixels"] if pixels else []), capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    rows = [[int(v) for v in line.split()] for line in r.stdout.splitlines()]
    assert len(rows) == len(files)
    return [(row[0], row[1:]) for row in rows], names


def test_damage_sweep_statuses(program, tmp_path):
    sweep = jc.full_sweep()
    got, _ = run(program, tmp_path, [data for _, _, data in sweep])
    bad = []
    for (bname, name, data), (status, info) in zip(sweep, got):
        st, _, inf = jr.probe(data)
        if (status, info) != (st, inf):
            bad.append((bname, name, status, st, info, inf))
    assert not bad, (len(bad), bad[:10])


def test_intact_pixels(program, tmp_path):
    cases = jc.intact()
    got, names = run(program, tmp_path, [data for _, data in cases], pixels=True)
    for (name, data), (status, info), path in zip(cases, got, names):
        assert status == 0, name
        exp = jc.expected(data)
        rgb = np.fromfile(path + ".rgb", np.uint8).reshape(exp.shape)
        assert np.array_equal(rgb, exp), name


def test_refused_statuses(program, tmp_path):
    cases = jc.refused()
    got, _ = run(program, tmp_path, [data for _, data, _ in cases])
    assert [st for st, _ in got] == [-2] * len(cases)


def test_unusual_corpus_statuses(program, tmp_path):
    """every file of tests/jp2_unusual_cases.py, accepted and refused (a 9/7 one is refused here: this program has no such option)"""
    import jp2_unusual_cases as uc
    cases = uc.accepted() + uc.refused()
    got, _ = run(program, tmp_path, [c.data for c in cases])
    want = {c.name: jr.probe(c.data) for c in cases}
    assert [(c.name, st, info) for c, (st, info) in zip(cases, got)] == [(c.name, want[c.name][0], want[c.name][2]) for c in cases]
    assert [st for c, (st, _) in zip(cases, got) if not c.irreversible] == [0] * sum(not c.irreversible for c in uc.accepted()) + [-2] * 3


def test_unusual_corpus_pixels(program, tmp_path):
    """the host decode, by the functions the kernels run, of every accepted 5/3 case is Pillow's: each file goes through csrc/jp2_t1.h
    under the sanitizers before tests/test_gpu_jp2_unusual.py sends it to the device (the 9/7 ones: test_jp2_irreversible_sanitized)"""
    import jp2_unusual_cases as uc
    cases = [c for c in uc.accepted() if not c.irreversible]
    got, names = run(program, tmp_path, [c.data for c in cases], pixels=True)
    for c, (status, info), path in zip(cases, got, names):
        assert status == 0, c.name
        exp = jc.expected(c.data)
        assert np.array_equal(np.fromfile(path + ".rgb", np.uint8).reshape(exp.shape), exp), c.name


def test_gpu_damage_sample_pixels(program, tmp_path):
    """the damaged files tests/test_gpu_jp2.py sends to the device, decoded on the host first by the functions the kernels run"""
    sample = jc.sweep_sample(200, seed=2000)
    got, names = run(program, tmp_path, [data for _, _, data in sample], pixels=True)
    n_ok = 0
    for (bname, name, data), (status, info), path in zip(sample, got, names):
        st, _, inf, rgb = jc.reference(data)
        assert (status, info) == (st, inf), (bname, name)
        if st == 0:
            assert np.array_equal(np.fromfile(path + ".rgb", np.uint8).reshape(rgb.shape), rgb), (bname, name)
            n_ok += 1
    assert n_ok >= 50
