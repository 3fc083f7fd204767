"""GPU: the fused CTC head (ctc_fc_argmax_kernel: FC + arg-max + soft-max, logits never in memory) on its OWN input, in both storage
types and at its edges.  Every test runs a recogniser with keep_taps = 1, reads the sequence the head consumed (lstm.l1 of the CRNN,
svtr.seq of SVTR in the model's type), computes logits = seq @ W.T + b in float64 from the loaded weights as the loader stores them
(tests/ctc_head_inputs.py) and compares idx with np.argmax (lowest index among equals) and prob with 1 / sum(exp(l - max)):
  * on every "clear" row (top-1 / top-2 margin > 1e-4; at least 95 % of the rows) idx is EQUAL and prob within rtol 2e-4;
  * both recognisers and both types.  The launch records name the instantiation the engine chose for the model's type (a label the
    engine writes beside the launch, not a trace of it); what guards against fp16 operands being read as bf16 is the numerical
    comparison on the fp16 model;
  * M = 80 (one partly filled 128-row block), 640 (five full blocks), 2640 (a ragged last block);
  * C = 3, 64, 65, 128 (one mostly padded tile, no padded class, one real class beside 63 padded ones), edge classes winning;
  * exact ties in the partner half-wave, in the lane's other sub-tile and in later tiles: the lowest index wins;
  * logits in the hundreds: the running-sum rescale underflows, prob stays finite and reaches exactly 1.0."""
import numpy as np
import pytest
import torch

from lumina_ocr import arch, synth

import ctc_head_inputs as ci

pytestmark = pytest.mark.gpu


def _crops(n, seed):
    rng = np.random.default_rng(seed)
    return np.stack([synth.synth_crop(rng)[0] for _ in range(n)])


@pytest.fixture(scope="module")
def svtr_weights():
    """SVTR-Tiny, 500 classes, per storage type (the same seeded values; svtr.config names the type)."""
    return {dt: arch.make_svtr_weights(variant="tiny", dtype=dt, num_classes=500) for dt in ("bf16", "f16")}


@pytest.fixture(scope="module", autouse=True)
def _standard_models_afterwards(engine, rec_weights, svtr_weights):
    """The tests here load recognisers with replaced heads (3 classes, periodic, x 16) into the session's engine: put the seeded
    ones back when the module is done, so that no later test can meet a replaced head whatever the order of the files."""
    yield
    engine.load_rec(rec_weights)
    engine.load_svtr(svtr_weights["bf16"])


def _run_head(engine, model, wd, crops, dtype="bf16"):
    """-> (idx [M], prob [M], seq float32 [M, K] = the head's own input, kernel names of the run's timed launches)."""
    if model == "crnn":
        engine.load_rec(wd)
    else:
        engine.load_svtr(wd)
        assert engine.svtr_dtype == dtype
    engine.conv_timing_detail()                    # drop earlier records
    engine.set_option("keep_taps", 1)
    engine.set_option("time_convs", 1)
    try:
        fwd = engine.rec_forward if model == "crnn" else engine.svtr_forward
        idx, prob = fwd(torch.from_numpy(crops).cuda())
        torch.cuda.synchronize()
        kernels = [k for _, k, *_ in engine.conv_timing_detail()]
        seq = engine.read_tap("lstm.l1") if model == "crnn" else engine.read_tap("svtr.seq", dtype)
    finally:
        engine.set_option("keep_taps", 0)
        engine.set_option("time_convs", 0)
    return idx.cpu().numpy().reshape(-1), prob.cpu().numpy().reshape(-1), seq.reshape(-1, ci.K), kernels


def _check(got_idx, got_prob, ref, what):
    """The rules common to every case; returns nothing, asserts."""
    clear = ref["clear"]
    assert got_idx.shape == ref["idx"].shape and got_prob.dtype == np.float32
    assert clear.mean() >= ci.CLEAR_SHARE, (what, float(clear.mean()))
    assert np.isfinite(got_prob).all() and (got_prob > 0).all() and (got_prob <= 1).all(), what
    bad = np.flatnonzero(clear & (got_idx != ref["idx"]))
    assert bad.size == 0, (what, "arg-max differs on clear rows", bad[:8].tolist(), got_idx[bad[:8]].tolist(), ref["idx"][bad[:8]].tolist())
    rel = np.abs(got_prob.astype(np.float64) - ref["prob"]) / ref["prob"]
    print("%s: rows %d, clear %.4f, worst relative prob error on clear rows %.3g" % (what, len(clear), clear.mean(), rel[clear].max()))
    assert np.allclose(got_prob[clear], ref["prob"][clear], rtol=ci.PROB_RTOL, atol=0), (what, float(rel[clear].max()))


def _head_kernels(kernels):
    return sorted({k for k in kernels if k.startswith("ctc_fc_argmax_kernel<")})


@pytest.mark.parametrize("model,dtype", [("crnn", "bf16"), ("svtr", "bf16"), ("svtr", "f16")])
def test_head_on_its_own_sequence(engine, rec_weights, svtr_weights, model, dtype):
    """CRNN bf16 (C = 6625), SVTR-Tiny bf16 and fp16 (C = 500); the engine's launch record names <1> for the fp16 model, <0> otherwise."""
    wd = rec_weights if model == "crnn" else svtr_weights[dtype]
    idx, prob, seq, kernels = _run_head(engine, model, wd, _crops(3, 99), dtype)
    fc = ci.FC[model]
    assert wd[fc + ".w"].shape[0] == (6625 if model == "crnn" else 500)
    assert _head_kernels(kernels) == ["ctc_fc_argmax_kernel<%d>" % (dtype == "f16")], kernels
    _check(idx, prob, ci.reference(seq, wd[fc + ".w"], wd[fc + ".b"], dtype), "%s %s" % (model, dtype))


@pytest.mark.parametrize("n", [1, 8, 33])
def test_head_row_count_edges(engine, rec_weights, n):
    """M = 80: one partly filled 128-row block; 640: exactly five full blocks; 2640: twenty full blocks and a last one of 80 rows."""
    idx, prob, seq, _ = _run_head(engine, "crnn", rec_weights, _crops(n, 200 + n))
    assert len(idx) == 80 * n == len(seq)
    _check(idx, prob, ci.reference(seq, rec_weights["ctc.fc.w"], rec_weights["ctc.fc.b"]), "rows %d" % (80 * n))


@pytest.mark.parametrize("c", ci.EDGE_CLASSES)
def test_head_class_count_edges(engine, rec_weights, c):
    """C = 3 / 64 / 65 / 128 on the CRNN, class ids and probabilities only (no charset): the padded classes of the last tile (bias
    -1e30) never win and add nothing to the sum; class 0, class C - 1 and (C = 65) class 64 each win on some clear row.
    The bias is centred on the head's own input (ctc_head_inputs.class_edge_fc), which does not depend on the FC: hence a first
    run with the seeded head to read lstm.l1, then the run under test.  The reference and the winners are computed afterwards from
    the sequence of that second run (asserted equal to the first), so nothing the head computes enters its own reference."""
    crops = _crops(3, 41)
    _, _, seq0, _ = _run_head(engine, "crnn", rec_weights, crops)          # the head's input does not depend on the FC
    w, b = ci.class_edge_fc(c, seq0)
    idx, prob, seq, _ = _run_head(engine, "crnn", ci.with_fc(rec_weights, "crnn", w, b), crops)
    assert engine.num_classes == c and np.array_equal(seq, seq0)
    ref = ci.reference(seq, w, b)
    for k in ci.edge_winners(c):
        assert (ref["clear"] & (ref["idx"] == k)).any(), (c, k)            # the float64 reference says so
    assert idx.min() >= 0 and idx.max() < c
    _check(idx, prob, ref, "C = %d" % c)


@pytest.mark.parametrize("model,dtype", [("crnn", "bf16"), ("svtr", "f16")])
@pytest.mark.parametrize("period", ci.TIE_PERIODS)
def test_head_exact_ties_take_the_lowest_index(engine, rec_weights, svtr_weights, model, dtype, period):
    """200 classes that repeat with period P: every logit has bit-identical copies — in the partner half-wave (P = 4), in the lane's
    other 32-class sub-tile (P = 32), in later tiles (P = 64).  The winner is the copy below P, as np.argmax and the oracle take it."""
    wd = rec_weights if model == "crnn" else svtr_weights[dtype]
    fc = ci.FC[model]
    w, b = ci.periodic_fc(wd[fc + ".w"], wd[fc + ".b"], period)
    idx, prob, seq, kernels = _run_head(engine, model, ci.with_fc(wd, model, w, b), _crops(3, 77), dtype)
    assert _head_kernels(kernels) == ["ctc_fc_argmax_kernel<%d>" % (dtype == "f16")], kernels
    ref = ci.reference(seq, w, b, dtype, distinct=period)
    assert np.array_equal(ref["logits"][:, :period], ref["logits"][:, period:2 * period]) and ref["idx"].max() < period
    assert (idx[ref["clear"]] < period).all(), (period, np.unique(idx[ref["clear"]] // period).tolist())
    _check(idx, prob, ref, "%s %s period %d" % (model, dtype, period))


@pytest.mark.parametrize("model,dtype", [("crnn", "bf16"), ("svtr", "f16")])
def test_head_saturated_softmax(engine, rec_weights, svtr_weights, model, dtype):
    """FC weights x 2^4: margins in the tens to hundreds.  exp2((run_m - tm) * log2e) underflows in the running-sum rescale — already
    on the first tile, which starts from run_m = -3e38 — and prob must come out finite, in (0, 1], and exactly 1.0 wherever the
    float64 reference rounds to 1.0 in fp32."""
    wd = rec_weights if model == "crnn" else svtr_weights[dtype]
    fc = ci.FC[model]
    w, b = ci.saturated_fc(wd[fc + ".w"], wd[fc + ".b"])
    idx, prob, seq, _ = _run_head(engine, model, ci.with_fc(wd, model, w, b), _crops(3, 55), dtype)
    ref = ci.reference(seq, w, b, dtype)
    srt = np.sort(ref["logits"], axis=1)
    assert np.median(srt[:, -1] - srt[:, -2]) > 2.0 and np.abs(ref["logits"]).max() > 100.0      # the regime is the saturated one
    one = ref["prob"].astype(np.float32) == np.float32(1.0)
    assert one.sum() >= 8, int(one.sum())
    _check(idx, prob, ref, "%s %s saturated" % (model, dtype))
    assert (prob[one] == np.float32(1.0)).all(), prob[one][prob[one] != 1.0][:8]
