"""CPU, no GPU and no Python extension: the host parser with JP2_TAKE_TILES (csrc/jp2_parse.h) and the parity-aware lifting functions
the kernels run (csrc/jp2_t1.h), compiled into the stand-alone program tests/jp2_tiles_main.cpp with -fsanitize=address,undefined and
run as a child process.  The program must exit 0 (no sanitizer report); its statuses, info and reasons are the restatement's
(tests/jp2_tiles_reference.py) on every case, every refusal and every file of the damage sweep, and its host decode gives Pillow's
bytes on the intact cases and the restatement's on a seeded sample of the sweep.  Skips when the compiler has no sanitizer runtime (a
one-line program decides).  The test preloads nothing and leaves the environment as it finds it."""
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

import jp2_cases as jc
import jp2_irreversible_reference as ir
import jp2_reference as jr
import jp2_tiles_cases as tc
import jp2_tiles_reference as tr

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "ocr-system_amd" / "csrc"

SANITIZE = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
STATIC = ["-static-libasan", "-static-libubsan"]   # the runtime inside the program: it then depends on no library's load order
BOTH = tr.IRREVERSIBLE | tr.TILES


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    tmp = tmp_path_factory.mktemp("jp2_tiles")
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
    out = tmp / "jp2_tiles_main"
    # -ffp-contract=off as the library is built: no fused multiply-add in the float path
    r = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-ffp-contract=off"] + flags +
                       ["-I", str(CSRC), str(ROOT / "tests" / "jp2_tiles_main.cpp"), "-o", str(out)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return out


def run(program, tmp_path, files, flags=BOTH, pixels=None):
    """-> [(status, info, irreversible, tiles, reason)] of the program over `files` (bytes objects), and the paths they were written to"""
    names = []
    for i, data in enumerate(files):
        p = tmp_path / f"f{i:05d}.jp2"
        p.write_bytes(data)
        names.append(str(p))
    lst = tmp_path / "list.txt"
    lst.write_text("\n".join(names) + "\n")
    r = subprocess.run([str(program), str(lst), str(flags)] + (["--pixels", str(pixels)] if pixels else []), capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    rows = [line.split() for line in r.stdout.splitlines()]
    assert len(rows) == len(files)
    return [(int(row[0]), [int(v) for v in row[1:9]], int(row[9]), int(row[10]), "" if row[11] == "-" else row[11].replace("_", " ")) for row in rows], names


def same_reason(cxx, py):
    """the reason class: the same words, but for the messages the restatement fills in (a marker's or a box's name)"""
    return cxx == py or ("marker" in cxx and "marker" in py) or ("box" in cxx and "box" in py)


@pytest.mark.parametrize("window", [6, 256])
def test_cases_pixels(program, tmp_path, window):
    """6: windows shorter than their halo; 256: j2_dwt97_h's"""
    cases = tc.accepted()
    got, names = run(program, tmp_path, [c.data for c in cases], pixels=window)
    for c, (status, info, kind, tiles, why), path in zip(cases, got, names):
        assert (status, kind) == (0, int(c.irreversible)), (c.name, status, why)
        want = jc.expected(c.data)
        assert info[:2] == [want.shape[1], want.shape[0]], c.name
        assert np.array_equal(np.fromfile(path + ".rgb", np.uint8).reshape(want.shape), want), c.name


def test_one_tile_with_the_widest_tile_size(program, tmp_path):
    cases = tc.one_tile_widest()
    for flags in (BOTH, 0):
        got, names = run(program, tmp_path, [d for _, d in cases], flags=flags, pixels=6)
        for (name, data), (status, info, _, tiles, why), path in zip(cases, got, names):
            want = jc.expected(data)
            assert (status, tiles) == (0, 1), (name, flags, status, why)
            assert np.array_equal(np.fromfile(path + ".rgb", np.uint8).reshape(want.shape), want), (name, flags)


def test_refusals(program, tmp_path):
    cases = tc.refusals()
    got, _ = run(program, tmp_path, [data for _, data, _, _ in cases])
    for (name, data, st, word), (status, info, _, _, why) in zip(cases, got):
        pst, pwhy, pinfo = tr.probe(data)
        assert status == st == pst and word in why and why == pwhy and info == pinfo, (name, status, why)


@pytest.mark.parametrize("flags", [0, tr.IRREVERSIBLE, tr.TILES])
def test_other_flag_words(program, tmp_path, flags):
    """without JP2_TAKE_TILES the tiled cases are -2 with the reasons of the older restatements, and the older cases keep their answers;
    with it alone a 9/7 file is -2"""
    files = [c.data for c in tc.accepted()] + [d for _, d in jc.intact()[:10]]
    got, _ = run(program, tmp_path, files, flags=flags)
    ref = (lambda d: tr.probe(d, flags)) if flags & tr.TILES else ir.probe if flags else jr.probe
    for data, (status, info, _, _, why) in zip(files, got):
        st, pwhy, pinfo = ref(data)
        assert (status, info) == (st, pinfo) and same_reason(why, pwhy), (status, st, why, pwhy)
    if not flags & tr.TILES:
        assert [st for st, *_ in got[:len(tc.accepted())]] == [-2] * len(tc.accepted())


def test_damage_sweep_statuses(program, tmp_path):
    """every file of the sweep: status, info and reason class are the restatement's"""
    sweep = tc.full_sweep()
    got, _ = run(program, tmp_path, [data for _, _, data in sweep])
    bad = []
    for (bname, name, data), (status, info, _, _, why) in zip(sweep, got):
        st, pwhy, pinfo = _probe(data)
        if (status, info) != (st, pinfo) or not same_reason(why, pwhy):
            bad.append((bname, name, status, st, why, pwhy, info, pinfo))
    assert not bad, (len(bad), bad[:10])


def _probe(data):
    """the restatement's status, reason and info; from its decode where this session has one (tests/test_jp2_tiles_reference.py)"""
    held = tr._REF.get((data, BOTH))
    return held[:3] if held is not None else tr.probe(data)


def test_damage_sample_pixels(program, tmp_path):
    """a seeded sample of the sweep decoded on the host by the functions the kernels run: the restatement's bytes"""
    sweep = tc.full_sweep()
    pick = sorted(np.random.default_rng(2540).choice(len(sweep), size=400, replace=False))
    sample = [sweep[int(i)] for i in pick]
    got, names = run(program, tmp_path, [data for _, _, data in sample], pixels=6)
    n_ok = 0
    for (bname, name, data), (status, info, _, _, why), path in zip(sample, got, names):
        st, pwhy, pinfo, rgb = tr.reference(data)
        assert (status, info) == (st, pinfo) and same_reason(why, pwhy), (bname, name, status, st, why, pwhy)
        if st == 0:
            assert np.array_equal(np.fromfile(path + ".rgb", np.uint8).reshape(rgb.shape), rgb), (bname, name)
            n_ok += 1
    assert n_ok >= 100
