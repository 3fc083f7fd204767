"""CPU: the inputs of the CTC head tests (tests/ctc_head_inputs.py) do what tests/test_gpu_ctc_head.py needs of them, checked on the
oracle's own sequences (nets.rec_forward / nets.svtr_forward) — the engine's differ from these by roundings only."""
import numpy as np
import pytest

from lumina_ocr import arch, synth

import ctc_head_inputs as ci


def _crops(n, seed):
    rng = np.random.default_rng(seed)
    return np.stack([synth.synth_crop(rng)[0] for _ in range(n)])


@pytest.fixture(scope="module")
def crnn():
    """(weights, the oracle's lstm.l1 per crop seed)."""
    from oracle import nets
    wd = arch.make_rec_weights(4321)                     # conftest's rec_weights
    seqs = {seed: nets.rec_forward(wd, _crops(3, seed))[3].reshape(-1, ci.K) for seed in (99, 41, 77, 55)}
    return wd, seqs


@pytest.fixture(scope="module")
def svtr():
    """(weights per type, the oracle's svtr.seq per (type, crop seed))."""
    from oracle import nets
    wds = {dt: arch.make_svtr_weights(variant="tiny", dtype=dt, num_classes=500) for dt in ("bf16", "f16")}
    seqs = {("bf16", 99): nets.svtr_forward(wds["bf16"], _crops(3, 99))[3].reshape(-1, ci.K)}
    for seed in (99, 77, 55):
        seqs[("f16", seed)] = nets.svtr_forward(wds["f16"], _crops(3, seed))[3].reshape(-1, ci.K)
    return wds, seqs


def test_stored_weights_mirror_the_loader():
    w = np.array([[1.0, 1.0 + 2.0 ** -9, 3.0e-6, -70000.0 * 2.0 ** -1, 0.3]], np.float32)
    assert np.array_equal(ci.stored(w), arch.bf16_round(w).astype(np.float64))
    f = ci.stored(w, "f16")
    assert f[0, 0] == 1.0 and f[0, 1] == float(arch.bf16_round(w)[0, 1])                   # bf16 first, then fp16 (exact here)
    assert f[0, 2] == float(np.float16(arch.bf16_round(w)[0, 2])) and f[0, 2] != float(arch.bf16_round(w)[0, 2])   # fp16 subnormal
    assert f[0, 3] == float(np.float16(arch.bf16_round(w)[0, 3]))
    with pytest.raises(AssertionError), np.errstate(over="ignore"):
        ci.stored(np.array([[1.0e5]], np.float32), "f16")                                   # overflows fp16: not a legal test input


def test_reference_is_argmax_and_softmax_max():
    seq = np.array([[1.0, 0.0], [0.0, 1.0], [1.0, 1.0]])
    w = np.array([[2.0, 0.0], [0.0, 2.0], [2.0, 0.0]], np.float32)
    r = ci.reference(seq, w, np.zeros(3, np.float32))
    assert r["idx"].tolist() == [0, 1, 0]                                                   # the lowest index among equals
    assert np.allclose(r["prob"], [1 / (2 + np.exp(-2.0)), 1 / (1 + 2 * np.exp(-2.0)), 1 / 3.0], rtol=1e-15)
    assert r["clear"].tolist() == [False, True, False]


def test_main_cases_are_clear(crnn, svtr):
    wd, seqs = crnn
    assert ci.reference(seqs[99], wd["ctc.fc.w"], wd["ctc.fc.b"])["clear"].mean() >= ci.CLEAR_SHARE
    wds, sseq = svtr
    for dt in ("bf16", "f16"):
        r = ci.reference(sseq[(dt, 99)], wds[dt]["svtr.ctc.fc.w"], wds[dt]["svtr.ctc.fc.b"], dt)
        assert r["clear"].mean() >= ci.CLEAR_SHARE, dt
    # fp16 holds every bf16 value from 2^-14 up exactly; the loader's conversion rounds only the few seeded weights below that
    w16, wbf = ci.stored(wds["f16"]["svtr.ctc.fc.w"], "f16"), ci.stored(wds["f16"]["svtr.ctc.fc.w"], "bf16")
    changed = w16 != wbf
    assert (np.abs(wbf[changed]) < 2.0 ** -14).all() and changed.mean() < 1e-3


@pytest.mark.parametrize("c", ci.EDGE_CLASSES)
def test_class_edge_sets_make_the_edge_classes_win(crnn, c):
    wd, seqs = crnn
    w, b = ci.class_edge_fc(c, seqs[41])
    assert w.shape == (c, ci.K) and b.dtype == np.float32 and np.array_equal(w, arch.bf16_round(w))
    full = ci.with_fc(wd, "crnn", w, b)
    assert full["ctc.fc.w"].shape[0] == c and full["rec.conv1.w"] is wd["rec.conv1.w"] and wd["ctc.fc.w"].shape[0] == 6625
    r = ci.reference(seqs[41], w, b)
    assert r["clear"].mean() >= ci.CLEAR_SHARE
    assert ci.edge_winners(c) == ([0, 2] if c == 3 else [0, 64] if c == 65 else [0, c - 1])
    for k in ci.edge_winners(c):
        assert (r["clear"] & (r["idx"] == k)).sum() >= 3, (c, k)
    assert c == 3 or len(np.unique(r["idx"])) >= 8                                           # and other classes win too


@pytest.mark.parametrize("period", ci.TIE_PERIODS)
def test_periodic_sets_tie_exactly(crnn, svtr, period):
    wd, seqs = crnn
    wds, sseq = svtr
    for model, dt, src, seq in (("crnn", "bf16", wd, seqs[77]), ("svtr", "f16", wds["f16"], sseq[("f16", 77)])):
        fc = ci.FC[model]
        w, b = ci.periodic_fc(src[fc + ".w"], src[fc + ".b"], period)
        assert w.shape == (ci.TIE_CLASSES, ci.K) and b.shape == (ci.TIE_CLASSES,)
        for c in range(ci.TIE_CLASSES):
            assert np.array_equal(w[c], w[c % period]) and b[c] == b[c % period]
        r = ci.reference(seq, w, b, dt, distinct=period)
        lg = r["logits"]
        assert lg.shape == (len(seq), ci.TIE_CLASSES)
        for c in range(period, ci.TIE_CLASSES):
            assert np.array_equal(lg[:, c], lg[:, c % period])                               # exact float64 ties
        # summed class by class in one fixed order (no matrix product), the copies tie exactly as well
        direct = (seq.astype(np.float64)[:, None, :] * ci.stored(w, dt)[None, :, :]).sum(-1) + b.astype(np.float64)
        assert all(np.array_equal(direct[:, c], direct[:, c % period]) for c in range(period, ci.TIE_CLASSES))
        assert np.abs(direct - lg).max() < 1e-9
        assert r["idx"].max() < period and len(np.unique(r["idx"])) >= 2
        assert r["clear"].mean() >= ci.CLEAR_SHARE, (model, period, float(r["clear"].mean()))
    # where the copies lie in the kernel's tile: lane (r, h) holds the classes nt * 32 + (j & 3) + 8 * (j >> 2) + 4 * h of a 64-class tile
    lane = lambda c: ((c % 64) // 4) % 2                                                     # noqa: E731  (h of the class)
    assert lane(1) != lane(1 + 4) and lane(1) == lane(1 + 8)                                 # P = 4: the partner half-wave, and the same lane
    assert lane(1) == lane(1 + 32) and (1 + 32) // 64 == 0                                   # P = 32: the lane's other sub-tile
    assert (1 + 64) // 64 == 1 and ci.TIE_CLASSES > 3 * 64                                   # P = 64: later tiles, incl. the padded last one


def test_saturated_sets(crnn, svtr):
    wd, seqs = crnn
    wds, sseq = svtr
    for model, dt, src, seq in (("crnn", "bf16", wd, seqs[55]), ("svtr", "f16", wds["f16"], sseq[("f16", 55)])):
        fc = ci.FC[model]
        w, b = ci.saturated_fc(src[fc + ".w"], src[fc + ".b"])
        assert np.array_equal(w, arch.bf16_round(w)) and np.array_equal(w, np.float32(16.0) * src[fc + ".w"])   # the scale is exact
        assert np.abs(ci.stored(w, dt)).max() < 2.0 ** 7
        r = ci.reference(seq, w, b, dt)
        srt = np.sort(r["logits"], axis=1)
        assert np.median(srt[:, -1] - srt[:, -2]) > 2.0 and np.abs(r["logits"]).max() > 100.0
        assert r["clear"].mean() >= ci.CLEAR_SHARE
        one = r["prob"].astype(np.float32) == np.float32(1.0)
        assert one.sum() >= 16 and (~one).sum() >= 16, (model, int(one.sum()))               # both outcomes are in the set
        assert np.isfinite(r["prob"]).all() and (r["prob"] > 0).all() and (r["prob"] <= 1).all()
