"""GPU: lumina_ocr_ctc_decode_words through the C ABI against the restatement (tests/word_reference.py) — EQUALITY on every output;
text / len / score bitwise those of lumina_ocr_ctc_decode; rows past the count untouched; n = 0."""
import numpy as np
import pytest
import torch

import word_reference as wr

pytestmark = pytest.mark.gpu

T, MW = wr.T, wr.MAX_WORDS
SPACE = 95
SENTINEL = -7


def _call(engine, idx, prob, quads, widths, flip, space_id, n=None):
    """The C entry itself, on buffers filled with a sentinel -> host arrays"""
    n = idx.shape[0] if n is None else n
    dev = torch.device("cuda", 0)
    up = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a, dt)).to(dev)
    d_idx, d_prob, d_quads, d_widths = up(idx, np.int32), up(prob, np.float32), up(quads, np.int32), up(widths, np.int32)
    d_flip = None if flip is None else up(flip, np.int32)
    m = max(idx.shape[0], 1)
    full = lambda shape, dt: torch.full(shape, SENTINEL, dtype=dt, device=dev)
    text, length, score = full((m, T), torch.int32), full((m,), torch.int32), full((m,), torch.float32)
    wq, ws, wsc, wc = full((m, MW, 8), torch.int32), full((m, MW, 2), torch.int32), full((m, MW), torch.float32), full((m,), torch.int32)
    rc = engine.lib.lumina_ocr_ctc_decode_words(engine._h, d_idx.data_ptr(), d_prob.data_ptr(), n, d_quads.data_ptr(), d_widths.data_ptr(),
                                                0 if d_flip is None else d_flip.data_ptr(), int(space_id), text.data_ptr(), length.data_ptr(),
                                                score.data_ptr(), wq.data_ptr(), ws.data_ptr(), wsc.data_ptr(), wc.data_ptr(),
                                                torch.cuda.current_stream().cuda_stream)
    assert rc == 0, engine.lib.lumina_ocr_last_error(engine._h)
    torch.cuda.synchronize()
    return dict(text=text.cpu().numpy(), len=length.cpu().numpy(), score=score.cpu().numpy(), word_quads=wq.cpu().numpy(),
                word_spans=ws.cpu().numpy(), word_scores=wsc.cpu().numpy(), word_counts=wc.cpu().numpy())


def _assert_equal(got, ref):
    """every output equals the restatement bit for bit; rows past a line's count still hold the sentinel"""
    assert np.array_equal(got["text"], ref["text"]) and np.array_equal(got["len"], ref["len"])
    assert np.array_equal(got["score"].view(np.uint32), ref["score"].view(np.uint32))
    assert np.array_equal(got["word_counts"], ref["word_counts"])
    past = np.arange(MW)[None, :] >= ref["word_counts"][:, None]
    for k in ("word_quads", "word_spans", "word_scores"):
        g, r = got[k], ref[k]
        fill = np.broadcast_to(past.reshape(past.shape + (1,) * (g.ndim - 2)), g.shape)
        want = np.where(fill, np.array(SENTINEL, g.dtype), r)
        assert np.array_equal(g.view(np.uint32), want.view(np.uint32)), k


def _random_batch(n, seed, space_id):
    rng = np.random.default_rng(seed)
    classes = np.array([0, 0, 0, space_id if space_id >= 0 else 9, 5, 6, 7, 8, 6624], np.int32)
    idx = rng.choice(classes, size=(n, T)).astype(np.int32)
    rep = rng.random((n, T)) < 0.3                        # runs: a step repeats its left neighbour
    for t in range(1, T):
        idx[:, t] = np.where(rep[:, t], idx[:, t - 1], idx[:, t])
    idx[rng.random(n) < 0.05] = 0                         # empty lines
    prob = rng.random((n, T), dtype=np.float32)
    # quads: lying, standing (the rotation branch) and slanted, anywhere on a page (negative corners included: unclip leaves the page)
    x0, y0 = rng.integers(-20, 1500, n), rng.integers(-20, 2000, n)
    long_side, short_side = rng.integers(8, 900, n), rng.integers(6, 80, n)
    standing = rng.random(n) < 0.3
    w, h = np.where(standing, short_side, long_side), np.where(standing, long_side, short_side)
    j = rng.integers(-9, 10, (n, 8))
    quads = np.stack([x0, y0, x0 + w, y0, x0 + w, y0 + h, x0, y0 + h], 1) + j
    natural = np.array([wr.crop_width(q) for q in quads])
    widths = np.where(rng.random(n) < 0.5, natural, rng.integers(0, 321, n))   # the crop's own width, or any other valid one
    flip = (rng.random(n) < 1 / 3).astype(np.int32)
    return idx, prob, quads.astype(np.int32), widths.astype(np.int32), flip


@pytest.mark.parametrize("n", [1, 63, 64, 65, 4096])
@pytest.mark.parametrize("space_id", [SPACE, -1])
def test_random_batches_equal_the_restatement(engine, n, space_id):
    idx, prob, quads, widths, flip = _random_batch(n, 100 + n, space_id)
    ref = wr.decode_words(idx, prob, quads, widths, flip, space_id)
    got = _call(engine, idx, prob, quads, widths, flip, space_id)
    _assert_equal(got, ref)
    if n >= 63:
        assert ref["word_counts"].max() >= (1 if space_id < 0 else 4) and (ref["word_counts"] == 0).any()
        assert any(wr.crop_corners(q)[1] for q in quads) and flip.any() and not flip.all()
    # text, len and score are bitwise those of lumina_ocr_ctc_decode on the same inputs
    text, length, score = engine.ctc_decode(torch.from_numpy(idx).cuda(), torch.from_numpy(prob).cuda())
    assert np.array_equal(text.cpu().numpy(), got["text"]) and np.array_equal(length.cpu().numpy(), got["len"])
    assert np.array_equal(score.cpu().numpy().view(np.uint32), got["score"].view(np.uint32))


def test_null_flip_is_no_flip(engine):
    idx, prob, quads, widths, flip = _random_batch(65, 5, SPACE)
    got = _call(engine, idx, prob, quads, widths, None, SPACE)
    _assert_equal(got, wr.decode_words(idx, prob, quads, widths, None, SPACE))
    _assert_equal(got, wr.decode_words(idx, prob, quads, widths, np.zeros(65, np.int32), SPACE))
    flipped = _call(engine, idx, prob, quads, widths, np.ones(65, np.int32), SPACE)
    assert not np.array_equal(flipped["word_quads"], got["word_quads"]) and np.array_equal(flipped["word_spans"], got["word_spans"])


def _steps(d):
    row = np.zeros(T, np.int32)
    for t, k in d.items():
        row[t] = k
    return row


def test_known_answers(engine):
    """the hand-computed cases of tests/test_word_reference.py, on the device"""
    two = {t: 1 + t for t in range(10, 16)}
    two[16] = SPACE
    two.update({t: 40 + t for t in range(20, 31)})
    line = [0, 0, 640, 0, 640, 64, 0, 64]
    tall = [100, 50, 164, 50, 164, 690, 100, 690]
    short = [0, 0, 200, 0, 200, 64, 0, 64]
    clipped = {20: 5, 21: 6, 22: 7, 23: 8, 24: 9, 25: 9, 26: 9, 27: SPACE, 30: 5, 31: 6, 32: 7}
    forty = {}
    for k in range(40):
        forty[2 * k], forty[2 * k + 1] = 5 + (k % 3), SPACE
    cases = [(two, line, 0), (two, line, 1), (two, tall, 0), (two, tall, 1), (clipped, short, 0), (clipped, short, 1),
             ({2: SPACE, 4: 5, 5: 6, 7: SPACE, 9: SPACE, 12: 7, 14: SPACE}, line, 0), ({}, line, 0), (forty, line, 0),
             ({40: 9}, [0, 0, 320, 7, 320, 25, 0, 32], 0), (clipped, [5] * 8, 0)]
    idx = np.stack([_steps(c[0]) for c in cases])
    prob = np.tile((0.5 + np.arange(T, dtype=np.float32) / np.float32(256.0)).astype(np.float32), (len(cases), 1))
    quads = np.array([c[1] for c in cases], np.int32)
    widths = np.array([wr.crop_width(q) for q in quads], np.int32)
    flip = np.array([c[2] for c in cases], np.int32)
    got = _call(engine, idx, prob, quads, widths, flip, SPACE)
    _assert_equal(got, wr.decode_words(idx, prob, quads, widths, flip, SPACE))
    q = lambda i, k: got["word_quads"][i, k].tolist()
    assert got["word_counts"].tolist() == [2, 2, 2, 2, 2, 2, 2, 0, 40, 1, 0]
    assert q(0, 0) == [80, 0, 128, 0, 128, 64, 80, 64] and q(0, 1) == [160, 0, 248, 0, 248, 64, 160, 64]
    assert q(1, 0) == [512, 0, 560, 0, 560, 64, 512, 64] and q(1, 1) == [392, 0, 480, 0, 480, 64, 392, 64]
    assert q(2, 0) == [100, 130, 164, 130, 164, 178, 100, 178] and q(3, 0) == [100, 562, 164, 562, 164, 610, 100, 610]
    assert q(4, 0) == [160, 0, 200, 0, 200, 64, 160, 64] and q(4, 1) == [200, 0, 200, 0, 200, 64, 200, 64]
    assert q(5, 0) == [0, 0, 40, 0, 40, 64, 0, 64]
    assert got["word_spans"][6, :2].tolist() == [[1, 2], [5, 1]]
    assert all(q(8, k) == [16 * k, 0, 16 * k + 8, 0, 16 * k + 8, 64, 16 * k, 64] for k in range(40))
    assert q(9, 0) == [160, 4, 164, 4, 164, 28, 160, 28]
    # space_id = -1: one word per non-empty line
    one = _call(engine, idx, prob, quads, widths, flip, -1)
    _assert_equal(one, wr.decode_words(idx, prob, quads, widths, flip, -1))
    assert one["word_counts"].tolist() == [1, 1, 1, 1, 1, 1, 1, 0, 1, 1, 0] and one["word_quads"][0, 0].tolist() == [80, 0, 248, 0, 248, 64, 80, 64]
    assert np.array_equal(one["word_scores"][:, 0].view(np.uint32)[[0, 8]], one["score"].view(np.uint32)[[0, 8]])


def test_n_zero_is_a_no_op(engine):
    idx, prob, quads, widths, flip = _random_batch(3, 9, SPACE)
    got = _call(engine, idx, prob, quads, widths, flip, SPACE, n=0)
    assert all((v == SENTINEL).all() for v in got.values())
    assert engine.lib.lumina_ocr_ctc_decode_words(engine._h, 0, 0, 0, 0, 0, 0, SPACE, 0, 0, 0, 0, 0, 0, 0, 0) == 0   # no pointer is read
    assert engine.lib.lumina_ocr_ctc_decode_words(engine._h, 0, 0, 1, 0, 0, 0, SPACE, 0, 0, 0, 0, 0, 0, 0, 0) != 0   # a status, not a fault
    out = engine.ctc_decode_words(torch.zeros((0, T), dtype=torch.int32, device="cuda"), torch.zeros((0, T), device="cuda"),
                                  torch.zeros((0, 8), dtype=torch.int32, device="cuda"), torch.zeros((0,), dtype=torch.int32, device="cuda"))
    assert [tuple(t.shape) for t in out] == [(0, T), (0,), (0,), (0, MW, 8), (0, MW, 2), (0, MW), (0,)]


def test_the_binding_returns_what_the_entry_writes(engine):
    idx, prob, quads, widths, flip = _random_batch(130, 11, SPACE)
    ref = wr.decode_words(idx, prob, quads, widths, flip, SPACE)
    c = lambda a: torch.from_numpy(a).cuda()
    out = engine.ctc_decode_words(c(idx), c(prob), c(quads), c(widths), c(flip), SPACE)
    for t, k in zip(out, ("text", "len", "score", "word_quads", "word_spans", "word_scores", "word_counts")):
        assert np.array_equal(t.cpu().numpy().view(np.uint32), ref[k].view(np.uint32)), k   # (rows past the count: zero in both)
    with pytest.raises(ValueError):
        engine.ctc_decode_words(c(idx), c(prob), c(quads), c(widths).long(), None, SPACE)
