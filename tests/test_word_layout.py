"""CPU: build_layout_boxes(words=...) — `word` entries take the device's polygons and confidences; everything else, and the call
without `words`, is what it was."""
import numpy as np
import pytest

from lumina_ocr.pipeline import PageDetections
from lumina_ocr.utils import layout

import word_reference as wr

SPACE = 95
LINES = [([0, 0, 640, 0, 640, 64, 0, 64], "abcdef ghijklmnopq", 0.9),
         ([100, 50, 164, 50, 164, 690, 100, 690], " xy  z ", 0.8),
         ([0, 100, 200, 100, 200, 164, 0, 164], "", 0.0),
         ([0, 200, 320, 207, 320, 225, 0, 232], "solo", 0.7)]
WORDS = [[(0, 6, [80, 0, 128, 0, 128, 64, 80, 64], 0.95), (7, 11, [160, 0, 248, 0, 248, 64, 160, 64], 0.85)],
         [(1, 2, [100, 130, 164, 130, 164, 178, 100, 178], 0.75), (5, 1, [100, 210, 164, 210, 164, 298, 100, 298], 0.65)],
         [],
         [(0, 4, [160, 204, 164, 204, 164, 228, 160, 228], 0.7)]]


def _legacy(lines, page_number=1):
    """build_layout_boxes as it was before `words` existed, restated"""
    words, line_boxes = [], []
    for quad, text, score in lines:
        q = [float(v) for v in quad]
        for w, wq in layout.split_words(q, text):
            words.append({"type": "word", "content": w, "confidence": float(score), "polygon": wq, "page_number": page_number})
        line_boxes.append({"type": "line", "content": text, "polygon": q, "page_number": page_number})
    return words + line_boxes


def test_words_take_the_device_polygons_and_confidences():
    boxes = layout.build_layout_boxes(LINES, 3, words=WORDS)
    assert layout.validate_layout_boxes(boxes) == []
    got = [b for b in boxes if b["type"] == "word"]
    flat = [(LINES[i][1][a:a + c], q, s) for i, ws in enumerate(WORDS) for a, c, q, s in ws]
    assert [(b["content"], b["polygon"], b["confidence"]) for b in got] == [(t, [float(v) for v in q], float(s)) for t, q, s in flat]
    assert [b["content"] for b in got] == ["abcdef", "ghijklmnopq", "xy", "z", "solo"]
    assert all(isinstance(v, float) for b in got for v in b["polygon"]) and all(b["page_number"] == 3 for b in boxes)


def test_without_words_the_output_is_what_it_was():
    for page in (1, 4):
        assert layout.build_layout_boxes(LINES, page) == _legacy(LINES, page)
        assert layout.build_layout_boxes(LINES, page, words=None) == _legacy(LINES, page)
    assert layout.build_layout_boxes(LINES) == _legacy(LINES)
    assert layout.build_layout_boxes([]) == [] and layout.build_layout_boxes([], words=[]) == []


def test_order_type_content_and_page_number_do_not_depend_on_words():
    plain = layout.build_layout_boxes(LINES, 2)
    with_words = layout.build_layout_boxes(LINES, 2, words=WORDS)
    key = lambda bs: [(b["type"], b["content"], b["page_number"]) for b in bs]
    assert key(plain) == key(with_words)
    lines = lambda bs: [b for b in bs if b["type"] == "line"]
    assert lines(plain) == lines(with_words)
    # and the polygons are not the guess: the vertical line's words run down the page, the guess walks along its short top edge
    pw, ww = [b for b in plain if b["type"] == "word"], [b for b in with_words if b["type"] == "word"]
    assert all(a["polygon"] != b["polygon"] for a, b in zip(pw, ww))
    assert ww[2]["polygon"][1::2] == [130.0, 130.0, 178.0, 178.0] and pw[2]["polygon"][1::2] == [50.0, 50.0, 690.0, 690.0]
    assert [b["confidence"] for b in pw] == [0.9, 0.9, 0.8, 0.8, 0.7]


def test_words_must_match_the_lines():
    with pytest.raises(ValueError):
        layout.build_layout_boxes(LINES, 1, words=WORDS[:2])


def test_page_detections_hand_the_restatement_to_the_layout():
    """idx -> restatement -> PageDetections.line_words -> build_layout_boxes: spans, polygons and confidences arrive unchanged"""
    idx = np.zeros((2, wr.T), np.int32)
    for t in range(10, 16):
        idx[0, t] = 1 + t
    idx[0, 16] = SPACE
    for t in range(20, 31):
        idx[0, t] = 40 + t
    prob = np.full((2, wr.T), 0.5, np.float32)
    prob[0, 10] = 0.75
    quads = np.array([LINES[0][0], LINES[2][0]], np.int32)
    ref = wr.decode_words(idx, prob, quads, [wr.crop_width(q) for q in quads], None, SPACE)
    charset = [chr(0x30 + k) for k in range(95)] + [" "]
    texts = ["".join(charset[k] for k in ref["text"][i, :ref["len"][i]]) for i in range(2)]
    det = PageDetections(quads, texts, ref["score"], np.ones(2, np.float32), 640, 480, ref["text"], ref["len"], word_quads=ref["word_quads"],
                         word_spans=ref["word_spans"], word_scores=ref["word_scores"], word_counts=ref["word_counts"])
    lw = det.line_words()
    assert [len(x) for x in lw] == [2, 0]
    boxes = layout.build_layout_boxes(det.triples(), 1, words=lw)
    words = [b for b in boxes if b["type"] == "word"]
    assert [b["content"] for b in words] == texts[0].split(" ")
    assert words[0]["polygon"] == [80.0, 0.0, 128.0, 0.0, 128.0, 64.0, 80.0, 64.0] and words[1]["polygon"][0::2] == [160.0, 248.0, 248.0, 160.0]
    assert words[0]["confidence"] == float(ref["word_scores"][0, 0]) != words[1]["confidence"] == 0.5
    assert PageDetections(quads, texts, ref["score"], np.ones(2, np.float32)).line_words() is None
