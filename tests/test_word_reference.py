"""CPU: the restatement of the word definition (tests/word_reference.py) against oracle.nets.ctc_greedy, against text.split(" "), and
against answers computed by hand."""
import numpy as np

from lumina_ocr import arch
from lumina_ocr.utils import layout
from oracle import nets

import word_reference as wr

T = wr.T
SPACE = 95          # class of " " in the hand-made cases (arch.ctc_charset(96)[-1])
LINE = [0, 0, 640, 0, 640, 64, 0, 64]   # a 640 x 64 line: its crop is 320 columns wide, 2 page pixels per column


def _row(steps):
    """{step: class} -> idx row, blanks elsewhere; prob row rising with the step so that every mean is told apart"""
    idx = np.zeros(T, np.int32)
    for t, k in steps.items():
        idx[t] = k
    prob = (0.5 + np.arange(T, dtype=np.float32) / np.float32(256.0)).astype(np.float32)
    return idx, prob


def _one(steps, quad=LINE, wc=None, flip=False, space_id=SPACE):
    idx, prob = _row(steps)
    wc = wr.crop_width(quad) if wc is None else wc
    out = wr.decode_words(idx[None], prob[None], np.array([quad]), np.array([wc]), np.array([int(flip)]), space_id)
    n = int(out["word_counts"][0])
    return out, [(tuple(out["word_spans"][0, k]), out["word_quads"][0, k].tolist(), out["word_scores"][0, k]) for k in range(n)], prob


def _two_words():
    steps = {t: 1 + t for t in range(10, 16)}            # six characters, one step each
    steps[16] = SPACE
    steps.update({t: 40 + t for t in range(20, 31)})     # blanks at 17..19, then eleven characters
    return steps


def _mean(prob, steps):
    s = np.float32(0)
    for t in steps:
        s = np.float32(s + prob[t])
    return np.float32(s / np.float32(len(steps)))


def test_text_len_score_equal_the_oracle_and_spans_equal_split():
    rng = np.random.default_rng(7)
    charset = arch.ctc_charset(96)
    assert charset[SPACE] == " "
    n = 300
    # few classes and many blanks / spaces: repeats, runs of spaces, empty lines all occur
    idx = rng.choice(np.array([0, 0, 0, SPACE, 5, 6, 7, 8], np.int32), size=(n, T)).astype(np.int32)
    idx[:4] = 0
    idx[4] = SPACE
    prob = rng.random((n, T), dtype=np.float32)
    quads = np.tile(np.array(LINE), (n, 1))
    widths = rng.integers(1, 321, n)
    out = wr.decode_words(idx, prob, quads, widths, rng.integers(0, 2, n), SPACE)
    ref = nets.ctc_greedy(idx, prob, charset)
    for i, (text, score) in enumerate(ref):
        got = "".join(charset[k] for k in out["text"][i, :out["len"][i]])
        assert got == text and (out["text"][i, out["len"][i]:] == -1).all()
        assert float(out["score"][i]) == score
        pieces = [w for w in text.split(" ") if w]
        spans = out["word_spans"][i, :out["word_counts"][i]]
        assert [text[a:a + c] for a, c in spans] == pieces
        assert (out["word_spans"][i, out["word_counts"][i]:] == 0).all()
    assert out["word_counts"].max() > 5 and (out["word_counts"] == 0).sum() >= 5


def test_two_words_on_a_640_line_and_where_the_proportional_split_puts_them():
    out, words, prob = _one(_two_words())
    assert out["len"][0] == 18 and len(words) == 2
    (s0, q0, c0), (s1, q1, c1) = words
    assert s0 == (0, 6) and q0 == [80, 0, 128, 0, 128, 64, 80, 64]        # columns [40, 64)
    assert s1 == (7, 11) and q1 == [160, 0, 248, 0, 248, 64, 160, 64]     # columns [80, 124)
    assert c0 == _mean(prob, range(10, 16)) and c1 == _mean(prob, range(20, 31))
    assert out["score"][0] == _mean(prob, list(range(10, 17)) + list(range(20, 31)))
    # the guess puts the same two words at [0, 213] and [249, 640]
    text = "abcdef ghijklmnopq"
    guess = layout.split_words([float(v) for v in LINE], text)
    assert [g[1][0::2] for g in guess] == [[0.0, 213.0, 213.0, 0.0], [249.0, 640.0, 640.0, 249.0]]
    assert all(g[1] != [float(v) for v in q] for g, q in zip(guess, (q0, q1)))


def test_the_same_line_flipped():
    out, words, prob = _one(_two_words(), flip=True)
    (s0, q0, c0), (s1, q1, _) = words
    # the crop was turned: crop columns [40, 64) are source columns [256, 280), [80, 124) are [196, 240)
    assert s0 == (0, 6) and q0 == [512, 0, 560, 0, 560, 64, 512, 64]
    assert s1 == (7, 11) and q1 == [392, 0, 480, 0, 480, 64, 392, 64]
    assert c0 == _mean(prob, range(10, 16))


def test_a_tall_quad_takes_the_rotation_branch():
    # a vertical line read top to bottom: 64 wide, 640 tall.  The crop's corners are TR, BR, BL, TL: its top edge runs down the right side.
    quad = [100, 50, 164, 50, 164, 690, 100, 690]
    assert wr.crop_corners(quad) == ([(164, 50), (164, 690), (100, 690), (100, 50)], 1) and wr.crop_width(quad) == 320
    out, words, _ = _one(_two_words(), quad=quad)
    (s0, q0, _), (s1, q1, _) = words
    # columns [40, 64) -> y in [50 + 80, 50 + 128]; point k stays on the side of the line's corner k (TL, TR, BR, BL)
    assert q0 == [100, 130, 164, 130, 164, 178, 100, 178]
    assert q1 == [100, 210, 164, 210, 164, 298, 100, 298]
    # the branch is 4 h^2 >= 9 w^2: a quad 64 wide turns at 96 rows
    assert wr.crop_corners([0, 0, 64, 0, 64, 95, 0, 95])[1] == 0 and wr.crop_corners([0, 0, 64, 0, 64, 96, 0, 96])[1] == 1
    # flipped as well: source columns [256, 280)
    _, fw, _ = _one(_two_words(), quad=quad, flip=True)
    assert fw[0][1] == [100, 562, 164, 562, 164, 610, 100, 610]


def test_a_slanted_quad_uses_both_edges_and_rounds_half_away_from_zero():
    # top edge (0,0) -> (320,7), bottom edge (0,32) -> (320,25): y moves by 7 c / 320 down on top, up on the bottom
    quad = [0, 0, 320, 7, 320, 25, 0, 32]
    wc = 320
    _, words, _ = _one({40: 9}, quad=quad, wc=wc)       # columns [160, 164): 7 * 160 / 320 = 3.5 -> 4 and -3.5 -> -4
    assert words[0][1] == [160, 4, 164, 4, 164, 28, 160, 28]
    assert wr.round_div(7, 160, 320) == 4 and wr.round_div(-7, 160, 320) == -4 and wr.round_div(-7, 159, 320) == -3 and wr.round_div(1, 1, 3) == 0


def test_a_clipped_line_with_characters_reported_in_the_padding():
    # 100 valid columns of a 200 x 64 line; characters at steps 20..24 start inside, end at the edge; those at 30..32 lie in the padding
    quad = [0, 0, 200, 0, 200, 64, 0, 64]
    assert wr.crop_width(quad) == 100
    steps = {20: 5, 21: 6, 22: 7, 23: 8, 24: 9, 25: 9, 26: 9, 27: SPACE, 30: 5, 31: 6, 32: 7}
    out, words, _ = _one(steps, quad=quad)
    assert [w[0] for w in words] == [(0, 5), (6, 3)]
    assert words[0][1] == [160, 0, 200, 0, 200, 64, 160, 64]     # columns [80, min(108, 100)): the run of the last character counts
    assert words[1][1] == [200, 0, 200, 0, 200, 64, 200, 64]     # [100, 100): an empty box at the edge, never past it
    # flipped: the padding is on the same side of the crop, the valid columns are mirrored
    _, fw, _ = _one(steps, quad=quad, flip=True)
    assert fw[0][1] == [0, 0, 40, 0, 40, 64, 0, 64] and fw[1][1] == [0, 0, 0, 0, 0, 64, 0, 64]
    # a degenerate quad has no crop and no words, but its text stays
    out0, w0, _ = _one(steps, quad=[5, 5, 5, 5, 5, 5, 5, 5])
    assert wr.crop_width([5] * 8) == 0 and w0 == [] and out0["len"][0] == out["len"][0] and np.array_equal(out0["text"], out["text"])


def test_leading_trailing_and_doubled_spaces():
    # " ab  c " : two kept spaces in a row need a blank between them
    steps = {2: SPACE, 4: 5, 5: 6, 7: SPACE, 8: 0, 9: SPACE, 12: 7, 14: SPACE}
    out, words, prob = _one(steps)
    assert out["len"][0] == 7
    assert [w[0] for w in words] == [(1, 2), (5, 1)]
    assert words[0][1][0::2] == [32, 48, 48, 32] and words[1][1][0::2] == [96, 104, 104, 96]
    assert words[1][2] == prob[12]
    # a repeated space class without a blank is one space
    out2, words2, _ = _one({2: 5, 3: SPACE, 4: SPACE, 5: 6})
    assert out2["len"][0] == 3 and [w[0] for w in words2] == [(0, 1), (2, 1)]
    # only spaces
    assert _one({3: SPACE, 5: SPACE})[1] == []


def test_without_a_space_class_the_line_is_one_word():
    out, words, prob = _one(_two_words(), space_id=-1)
    assert len(words) == 1 and words[0][0] == (0, 18)
    assert words[0][1] == [80, 0, 248, 0, 248, 64, 80, 64]
    assert words[0][2] == out["score"][0]


def test_an_empty_line_has_no_words():
    for sid in (SPACE, -1):
        out, words, _ = _one({}, space_id=sid)
        assert words == [] and out["len"][0] == 0 and out["score"][0] == 0.0 and (out["text"] == -1).all()


def test_forty_one_character_words():
    steps = {}
    for k in range(40):
        steps[2 * k] = 5 + (k % 3)
        steps[2 * k + 1] = SPACE
    out, words, prob = _one(steps)
    assert out["len"][0] == 80 and len(words) == wr.MAX_WORDS == 40
    for k, (span, q, c) in enumerate(words):
        assert span == (2 * k, 1) and q == [16 * k, 0, 16 * k + 8, 0, 16 * k + 8, 64, 16 * k, 64] and c == prob[2 * k]
