"""GPU: every output bit of the fused CTC head (ctc_fc_argmax_kernel) against a recording (tests/golden/ctc_head_recording.json) taken
on the kernel as it stood before its K loop, weight staging and epilogue were rescheduled.  Per case the SHA-256 over the raw bytes of
idx and prob of one recogniser forward; the cases are the edges of tests/test_gpu_ctc_head.py (tests/ctc_head_inputs.py) plus a launch
with more rows than the device holds resident at once:
  * the seeded CRNN head (C = 6625: 104 class tiles, the last with 33 real classes) on 1, 8 and 33 crops of ragged widths;
  * SVTR-Tiny (C = 500) in bf16 and fp16;
  * C = 3, 64, 65, 128 (one and two class tiles: the tile pipeline's prologue and drain with nothing between them);
  * classes that repeat with period 4, 32, 64 (exact ties between partner lanes, within a lane, between tiles), CRNN bf16 and SVTR fp16;
  * FC weights x 16 (the running-sum rescale underflows), CRNN bf16 and SVTR fp16;
  * 840 crops = 67 200 rows > 512 resident work-groups x 128 rows: some work-group slot takes a second row block.
The recording also holds, per case, the SHA-256 of the head's own input (the tap lstm.l1 / svtr.seq of a second forward with
keep_taps = 1).  A case that misses its hash is run again with the taps kept, and the failure message says whether the head's input
was the recorded one (then the head moved; otherwise a kernel before it did), whether the second run reproduced the recording, and
which rows, 128-row blocks and class tiles differ between the two runs.
`python tests/test_gpu_ctc_head_recording.py` rewrites the recording from the library in use (that is how it was taken)."""
import hashlib
import json
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

GOLDEN = Path(__file__).resolve().parent / "golden" / "ctc_head_recording.json"
if __name__ == "__main__":
    ROOT = Path(__file__).resolve().parent.parent
    sys.path[:0] = [str(ROOT), str(ROOT / "ocr-system_amd"), str(ROOT / "tests")]

from lumina_ocr import arch, synth

import ctc_head_inputs as ci

pytestmark = pytest.mark.gpu

RESIDENT_ROWS = 512 * 128    # 256 CUs x 2 work-groups x 128 rows
MANY_CROPS, MANY_BASE = 840, 24


def _crops(n, seed):
    rng = np.random.default_rng(seed)
    return np.stack([synth.synth_crop(rng)[0] for _ in range(n)])


def _widths(n):
    """Ragged valid widths, 33 .. 320, distinct for up to 288 crops in a row."""
    return (33 + (37 * np.arange(n)) % 288).astype(np.int32)


def _forward(engine, model, wd, crops, widths, dtype="bf16"):
    if model == "crnn":
        engine.load_rec(wd)
    else:
        engine.load_svtr(wd)
        assert engine.svtr_dtype == dtype
    fwd = engine.rec_forward if model == "crnn" else engine.svtr_forward
    idx, prob = fwd(torch.from_numpy(crops).cuda(), torch.from_numpy(widths).cuda())
    torch.cuda.synchronize()
    return idx, prob


def _sha(idx, prob):
    assert idx.dtype == torch.int32 and prob.dtype == torch.float32
    sha = hashlib.sha256()
    for t in (idx, prob):
        sha.update(t.contiguous().view(torch.uint8).cpu().numpy().tobytes())
    return sha.hexdigest()


class _Inputs:
    """The seeded weights and crops, made once for all cases."""

    def __init__(self, engine, rec_weights):
        self.rec = rec_weights
        self.svtr = {dt: arch.make_svtr_weights(variant="tiny", dtype=dt, num_classes=500) for dt in ("bf16", "f16")}
        self.crops3 = _crops(3, 77)
        self._seq0 = None
        self.engine = engine

    def wd(self, model, dtype):
        return self.rec if model == "crnn" else self.svtr[dtype]

    def seq0(self):
        """lstm.l1 of the CRNN on crops3: the head's input, which does not depend on the FC (class_edge_fc centres the bias on it)."""
        if self._seq0 is None:
            eng = self.engine
            eng.load_rec(self.rec)
            eng.set_option("keep_taps", 1)
            try:
                eng.rec_forward(torch.from_numpy(self.crops3).cuda(), torch.from_numpy(_widths(3)).cuda())
                torch.cuda.synchronize()
                self._seq0 = eng.read_tap("lstm.l1").reshape(-1, ci.K)
            finally:
                eng.set_option("keep_taps", 0)
        return self._seq0


def _seq_sha(engine, model, dtype):
    """SHA-256 of the sequence the head consumed in the last forward (keep_taps = 1), as read_tap returns it."""
    seq = engine.read_tap("lstm.l1") if model == "crnn" else engine.read_tap("svtr.seq", dtype)
    return hashlib.sha256(np.ascontiguousarray(seq).tobytes()).hexdigest()


def _run_with_taps(s, name):
    """The case once more with the taps kept -> (idx, prob, sha256 of the head's input)."""
    s.engine.set_option("keep_taps", 1)
    try:
        idx, prob = CASES[name](s)
        return idx, prob, _seq_sha(s.engine, *MODEL[name])
    finally:
        s.engine.set_option("keep_taps", 0)


def _explain(s, name, idx, prob, want):
    """What a miss looks like: the input's hash, a second run, and where the two runs differ."""
    idx2, prob2, seq_sha = _run_with_taps(s, name)
    a_i, a_p = idx.cpu().numpy().reshape(-1), prob.cpu().numpy().reshape(-1)
    b_i, b_p = idx2.cpu().numpy().reshape(-1), prob2.cpu().numpy().reshape(-1)
    bad = np.flatnonzero((a_i != b_i) | (a_p.view(np.uint32) != b_p.view(np.uint32)))
    return dict(case=name, got=_sha(idx, prob), want=want["sha256"], second_run=_sha(idx2, prob2),
                second_run_matches_recording=_sha(idx2, prob2) == want["sha256"],
                head_input_sha256=seq_sha, head_input_is_the_recorded_one=seq_sha == want["seq_sha256"],
                rows_differing_between_the_runs=int(bad.size), blocks_of_128_rows=np.unique(bad // 128)[:16].tolist(),
                rows_in_block=(bad % 128)[:16].tolist(),
                first_rows=[dict(row=int(r), idx=(int(a_i[r]), int(b_i[r])), tile=(int(a_i[r]) // 64, int(b_i[r]) // 64),
                                 prob=(float(a_p[r]), float(b_p[r]))) for r in bad[:6]])


def _case_rows(n):
    return lambda s: _forward(s.engine, "crnn", s.rec, _crops(n, 200 + n), _widths(n))


def _case_model(model, dtype):
    return lambda s: _forward(s.engine, model, s.wd(model, dtype), s.crops3, _widths(3), dtype)


def _case_classes(c):
    def run(s):
        w, b = ci.class_edge_fc(c, s.seq0())
        out = _forward(s.engine, "crnn", ci.with_fc(s.rec, "crnn", w, b), s.crops3, _widths(3))
        assert s.engine.num_classes == c
        return out
    return run


def _case_fc(make, model, dtype):
    def run(s):
        wd = s.wd(model, dtype)
        w, b = make(wd[ci.FC[model] + ".w"], wd[ci.FC[model] + ".b"])
        return _forward(s.engine, model, ci.with_fc(wd, model, w, b), s.crops3, _widths(3), dtype)
    return run


def _case_many(s):
    assert MANY_CROPS * 80 > RESIDENT_ROWS
    crops = np.tile(_crops(MANY_BASE, 311), (MANY_CROPS // MANY_BASE, 1, 1, 1))
    return _forward(s.engine, "crnn", s.rec, crops, _widths(MANY_CROPS))


CASES, MODEL = {}, {}    # name -> the forward; name -> (recogniser, storage type): which tap is the head's input


def _case(name, run, model="crnn", dtype="bf16"):
    CASES[name], MODEL[name] = run, (model, dtype)


for _n in (1, 8, 33):
    _case("crnn.rows%d" % (80 * _n), _case_rows(_n))
_case("svtr.tiny.bf16", _case_model("svtr", "bf16"), "svtr", "bf16")
_case("svtr.tiny.f16", _case_model("svtr", "f16"), "svtr", "f16")
for _c in ci.EDGE_CLASSES:
    _case("crnn.classes%d" % _c, _case_classes(_c))
for _model, _dtype in (("crnn", "bf16"), ("svtr", "f16")):
    for _p in ci.TIE_PERIODS:
        _case("%s.%s.period%d" % (_model, _dtype, _p), _case_fc(lambda w, b, p=_p: ci.periodic_fc(w, b, p), _model, _dtype), _model, _dtype)
    _case("%s.%s.saturated" % (_model, _dtype), _case_fc(ci.saturated_fc, _model, _dtype), _model, _dtype)
_case("crnn.rows%d" % (80 * MANY_CROPS), _case_many)


@pytest.fixture(scope="module")
def inputs(engine, rec_weights):
    s = _Inputs(engine, rec_weights)
    yield s
    engine.load_rec(rec_weights)         # the seeded heads back, whatever the order of the files
    engine.load_svtr(s.svtr["bf16"])


@pytest.fixture(scope="module")
def golden():
    return json.loads(GOLDEN.read_text())


def test_recording_lists_these_cases(golden):
    assert list(golden) == list(CASES)


@pytest.mark.parametrize("name", list(CASES))
def test_head_reproduces_the_recording(inputs, golden, name):
    idx, prob = CASES[name](inputs)
    want = golden[name]
    assert idx.numel() == want["rows"], name
    if _sha(idx, prob) != want["sha256"]:
        pytest.fail("the head's output is not the recorded one: %s" % json.dumps(_explain(inputs, name, idx, prob, want)))


if __name__ == "__main__":
    from lumina_ocr.engine import Engine
    eng = Engine(0)
    s = _Inputs(eng, arch.make_rec_weights(4321))
    rec = {}
    for name, run in CASES.items():
        idx, prob = run(s)
        idx2, prob2, seq_sha = _run_with_taps(s, name)
        assert _sha(idx2, prob2) == _sha(idx, prob), name    # keeping the taps changes no output
        rec[name] = {"rows": idx.numel(), "sha256": _sha(idx, prob), "seq_sha256": seq_sha}
        print(name, rec[name], flush=True)
    out = Path(sys.argv[1]) if len(sys.argv) > 1 else GOLDEN
    out.write_text(json.dumps(rec, indent=1) + "\n")
    eng.close()
