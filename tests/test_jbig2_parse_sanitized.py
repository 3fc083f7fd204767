"""CPU, no GPU and no Python extension: the JBIG2 host parser (csrc/jbig2_parse.h) and the functions the jb2_generic kernel runs
(csrc/jbig2_dec.h: the arithmetic decoder over byte contexts, the nominal and the general row walk, the SLTP decision), compiled into
the stand-alone program tests/jbig2_main.cpp with -fsanitize=address,undefined and run as a child process.  The program must exit 0
(no sanitizer report, every run ends); its statuses and info are the restatement's (tests/jbig2_reference.py) on every input, and its
bits are the restatement's wherever it decodes: on the intact cases by both row walks, and over the damage sweep of two small streams
(every single-bit flip, every truncation).  Skips when the compiler has no sanitizer runtime (a one-line program decides).  The test
preloads nothing and leaves the environment as it finds it."""
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

import jbig2_cases as jc
import jbig2_reference as jr

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "ocr-system_amd" / "csrc"

SANITIZE = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
STATIC = ["-static-libasan", "-static-libubsan"]   # the runtime inside the program: it then depends on no library's load order


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    tmp = tmp_path_factory.mktemp("jbig2")
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
    out = tmp / "jbig2_main"
    r = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer"] + flags + ["-I", str(CSRC), str(ROOT / "tests" / "jbig2_main.cpp"), "-o", str(out)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return out


def run(program, tmp_path, pages, general=False):
    """-> [(status, info, mmr, decoded, path)] of the program over `pages`: (stream, globals or None)"""
    lines, names = [], []
    for i, (stream, g) in enumerate(pages):
        p = tmp_path / f"p{i:05d}.jb2"
        p.write_bytes(stream)
        gp = "-"
        if g is not None:
            gp = str(tmp_path / f"p{i:05d}.globals")
            Path(gp).write_bytes(g)
        lines.append(f"{p} {gp}")
        names.append(str(p))
    lst = tmp_path / "list.txt"
    lst.write_text("\n".join(lines) + "\n")
    r = subprocess.run([str(program), str(lst)] + (["--general"] if general else []), capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    rows = [[int(v) for v in line.split()] for line in r.stdout.splitlines()]
    assert len(rows) == len(pages)
    return [(row[0], row[1:9], row[9], row[10], name) for row, name in zip(rows, names)]


@pytest.mark.parametrize("general", [False, True], ids=["nominal_fast_path", "general_path_everywhere"])
def test_intact_cases(program, tmp_path, general):
    cases = jc.intact()
    got = run(program, tmp_path, [(c.stream, c.globals_data) for c in cases], general)
    decoded = 0
    for c, (status, info, mmr, dec, path) in zip(cases, got):
        assert (status, info) == jr.probe(c.stream, c.globals_data)[:2] and status == 0, c.name
        assert dec == 1 - mmr, c.name
        if dec:
            assert np.array_equal(np.fromfile(path + ".bits", np.uint8).reshape(c.bits.shape), c.bits), c.name
            decoded += 1
    assert decoded >= 40


def test_refused_cases(program, tmp_path):
    cases = jc.refused()
    got = run(program, tmp_path, [(c.stream, c.globals_data) for c in cases])
    for c, (status, info, _, dec, _) in zip(cases, got):
        assert (status, dec) == (c.status, 0) and info == jr.probe(c.stream, c.globals_data)[1], c.name


def test_damage_sweep(program, tmp_path):
    """every input ends without a report; status and info are the restatement's; so are the bits of every page the program decodes
    (arithmetic regions only: the MMR lines are device code).  The acceptance counts are the README's."""
    sweep, want = jc.damage_sweep(), jc.sweep_restatement()
    got = run(program, tmp_path, [(d, None) for _, _, d in sweep])
    bad, accepted, compared = [], {}, 0
    for (name, label, d), (st, info, bits), (status, ginfo, mmr, dec, path) in zip(sweep, want, got):
        pst, pinfo, _ = jr.probe(d)
        if (status, ginfo) != (pst, pinfo):
            bad.append((name, label, status, pst))
            continue
        accepted.setdefault(name, [0, 0])
        accepted[name][0] += st == 0
        accepted[name][1] += 1
        if dec and bits is not None:
            if not np.array_equal(np.fromfile(path + ".bits", np.uint8).reshape(bits.shape), bits):
                bad.append((name, label, "bits"))
            compared += 1
    assert not bad, (len(bad), bad[:10])
    assert compared >= 200
    print("accepted of the sweep:", accepted)
