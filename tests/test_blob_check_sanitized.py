"""CPU, no GPU and no Python extension: the LOCW parser and the per-model tensor check every eng_load_* runs first (csrc/blob_check.h),
compiled into the stand-alone program tests/blob_main.cpp and run as a child process over the mutants of tests/blob_cases.py: once
built with -fsanitize=address,undefined (skips when a one-line program shows that the compiler has no runtime that starts here), once
built plain, so that the rule is tested where the runtime is missing.  The program must exit 0 (no sanitizer report); its status,
reason and tensor are the restatement's (tests/blob_reference.py, written from the generators' shapes) for every mutant; a refusal
names the mutated tensor; every intact blob is accepted, and the C tensor list has exactly the generator's names, dtypes and dims.
The test preloads nothing and leaves the environment as it finds it.

test_holes lists the holes of the earlier loader, each with a mutant that its conditions let through and that is refused now."""
import shutil
import subprocess
from pathlib import Path

import pytest

from lumina_ocr import arch

import blob_cases as bc
import blob_reference as br

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "ocr-system_amd" / "csrc"

SANITIZE = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
STATIC = ["-static-libasan", "-static-libubsan"]   # the runtime inside the program: it then depends on no library's load order


def compile_program(tmp, flags, opt):
    cxx = shutil.which("g++") or shutil.which("c++")
    out = tmp / "blob_main"
    r = subprocess.run([cxx, "-std=c++17", opt, "-g", "-fno-omit-frame-pointer", "-Wall"] + flags + ["-I", str(CSRC), str(ROOT / "tests" / "blob_main.cpp"), "-o", str(out)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return out


@pytest.fixture(scope="module", params=["sanitized", "plain"])
def program(request, tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    tmp = tmp_path_factory.mktemp("blob_" + request.param)
    if request.param == "plain":
        return compile_program(tmp, [], "-O2")
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
    return compile_program(tmp, flags, "-O1")


@pytest.fixture(scope="module")
def bases(tmp_path_factory):
    """name -> (kind, blob, path, per_tensor): every generator's intact blob, written once"""
    tmp = tmp_path_factory.mktemp("blob_bases")
    out = {}
    for name, kind, weights, per_tensor in bc.base_blobs():
        blob = arch.write_blob(weights)
        path = tmp / (name + ".locw")
        path.write_bytes(blob)
        out[name] = (kind, blob, path, per_tensor)
    return out


BASES = ["det", "rec", "cls", "svtr-tiny-bf16", "svtr-tiny-f16", "svtr-base-bf16", "svtr-base-f16"]
_results, _restated = {}, {}


def run_corpus(program, bases, name, tmp_path_factory):
    """-> [(mutant, (status, reason, tensor) of the program, the same of the restatement)], computed once per program and base"""
    key = (str(program), name)
    if key not in _results:
        kind, blob, path, per_tensor = bases[name]
        if name not in _restated:
            mutants = bc.corpus(kind, blob, per_tensor)
            bench = bc.Workbench(blob)
            _restated[name] = (mutants, [bench.check(kind, m) for m in mutants])
        mutants, want = _restated[name]
        recipes = tmp_path_factory.mktemp("recipes") / "recipes.bin"
        recipes.write_bytes(bc.serialise(mutants))
        r = subprocess.run([str(program), "check", kind, str(path), str(recipes)], capture_output=True, text=True)
        assert r.returncode == 0, (r.returncode, r.stderr[-4000:])
        lines = r.stdout.split("\n")[:-1]
        assert len(lines) == len(mutants)
        got = [(int(s), reason, tensor) for s, reason, tensor in (line.split("\t") for line in lines)]
        _results[key] = list(zip(mutants, got, want))
    return _results[key]


def head_pair(kind, tensor):
    head = br.CTC_HEADS.get(kind)
    return {head + ".w", head + ".b"} if head and tensor in (head + ".w", head + ".b") else {tensor}


@pytest.mark.parametrize("name", BASES)
def test_every_mutant_as_the_restatement(program, bases, name, tmp_path_factory):
    kind = bases[name][0]
    rows = run_corpus(program, bases, name, tmp_path_factory)
    bad = [(m.label, got, want) for m, got, want in rows if got != want]
    assert not bad, (len(bad), bad[:10])
    # a refusal names the mutated tensor ("" where the cut or the damage leaves no name to give); the class count is stated by the
    # head's weight and its bias together, so either may be named
    benign_missing = "svtr.config:missing"
    for m, got, _ in rows:
        if m.label in bc.ACCEPTED or (m.label == benign_missing and "tiny" in name):
            assert got == (0, "", ""), (m.label, got)
            continue
        assert got[0] == 1, (m.label, got)
        if m.label == benign_missing:
            continue   # a Base blob without its svtr.config is read as Tiny: refused, at the first tensor of another shape
        allowed = head_pair(kind, m.tensor) | ({""} if m.label.startswith("trunc") or not m.tensor else set())
        assert got[2] in allowed, (m.label, got)
    accepted = [m.label for m, got, _ in rows if got[0] == 0]
    print(name, len(rows), "mutants,", len(accepted), "accepted:", accepted)


@pytest.mark.parametrize("name", BASES)
def test_c_list_is_the_generators(program, bases, name):
    """the tensors check_blob asks for are exactly the generator's: names, storage types, dims (class count free), which are optional"""
    kind, blob, path, _ = bases[name]
    r = subprocess.run([str(program), "spec", kind, str(path)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    got = {}
    for line in r.stdout.splitlines():
        n, dt, req, dims = line.split("\t")
        assert n not in got, n
        got[n] = (int(dt), tuple(int(v) for v in dims.split()), bool(int(req)))
    variant = "base" if "base" in name else "tiny"
    assert got == br.generator_shapes(kind, variant)
    assert set(got) == set(arch.read_blob(blob))


# the holes found by reading the loader: (base, mutant label, reason).  Each of these is a well-formed container, so the parser passes
# it, and none of the conditions the loader tested before blob_check.h looked at the field it changes (the comment names what was missing)
HOLES = [
    ("det", "s1.b0.conv1.w:dim2-1", "wrong dimension"),            # make_conv never looked at dims[2]
    ("rec", "rec.b3.dw.w:dim2-1", "wrong dimension"),              # make_dw: dims[2]
    ("rec", "rec.b3.dw.b:dim0-1", "wrong dimension"),              # make_dw: bias length
    ("rec", "rec.b3.dw.w:torch-layout", "wrong dimension"),
    ("rec", "rec.b3.se1.w:rank-1", "wrong rank"),                  # make_se indexed dims[3] of any rank
    ("rec", "rec.b3.se1.w:dim1+1", "wrong dimension"),             # make_se: dims[1], dims[2]
    ("rec", "rec.b3.se2.w:dim2+1", "wrong dimension"),
    ("rec", "rec.b3.se1.b:dim0-1", "wrong dimension"),             # make_se: bias lengths
    ("rec", "rec.b3.se2.b:dim0-1", "wrong dimension"),
    ("cls", "cls.b3.se1.w:torch-layout", "wrong dimension"),
    ("rec", "ctc.fc.b:dtype", "wrong dtype"),                      # load_ctc_head: no dtype test
    ("rec", "ctc.fc.w:dtype", "wrong dtype"),
    ("rec", "ctc.fc.b:rank+1", "wrong rank"),                      # load_ctc_head: bias rank
    ("rec", "classes=65537", "class count out of range"),          # load_ctc_head: no bound on C
    ("svtr-tiny-bf16", "classes=1", "class count out of range"),
    ("rec", "lstm.l0.fw.w_ih:rank-1", "wrong rank"),               # LSTM: no rank test
    ("rec", "lstm.l0.fw.w_ih:dtype", "wrong dtype"),               # LSTM: no dtype test
    ("rec", "lstm.l0.bw.w_ih:dim0-1", "wrong dimension"),          # LSTM: bw.* unchecked -> short wcat
    ("rec", "lstm.l1.bw.w_ih:dim1-1", "wrong dimension"),
    ("rec", "lstm.l0.fw.b:dim0-1", "wrong dimension"),             # LSTM: biases
    ("rec", "lstm.l0.bw.b:dtype", "wrong dtype"),
    ("rec", "lstm.l0.fw.w_hh:dim0-1", "wrong dimension"),          # LSTM: w_hh rows -> lstm_kernel reads past the upload
    ("rec", "lstm.l1.bw.w_hh:dim0-1", "wrong dimension"),
    ("det", "fpn.p2.w:dim2-1", "wrong dimension"),                 # compose_fpn_p2 read the whole of fpn.p2.w
    ("det", "fpn.in2.b:rank+1", "wrong rank"),
    ("svtr-tiny-bf16", "svtr.config[0]=nan", "svtr.config value not a small whole number"),   # cast of any float
    ("svtr-tiny-bf16", "svtr.config[3]=1e30", "svtr.config value not a small whole number"),
    ("svtr-base-bf16", "svtr.config[9]=64.5", "svtr.config value not a small whole number"),  # local_blocks unchecked
    ("svtr-tiny-bf16", "svtr.config[9]=inf", "svtr.config value not a small whole number"),
    ("det", "stem.conv1.w:duplicate", "duplicate tensor name"),    # the last copy won
    ("det", "trailing-bytes", "trailing bytes"),                   # ignored
]


@pytest.mark.parametrize("name,label,reason", HOLES, ids=[f"{b}-{m}" for b, m, _ in HOLES])
def test_holes(program, bases, name, label, reason, tmp_path_factory):
    rows = [(m, got) for m, got, _ in run_corpus(program, bases, name, tmp_path_factory) if m.label == label]
    assert len(rows) == 1, label
    m, got = rows[0]
    assert got[0] == 1 and got[1] == reason and got[2] in head_pair(bases[name][0], m.tensor), got
