"""Selection marks, the host half: the device's rows (lumina_ocr_selection_marks: x0, y0, x1, y1, edge, ink_in, area_in, state per
mark) -> the marks of a page as the result schema wants them (reference backend/services/ocr_service.py:313-322: state
"selected" / "unselected", confidence, polygon), and the same for the round marks (radio buttons) of
lumina_ocr_selection_marks_round: Azure's selection marks cover both.  Pure Python."""
from __future__ import annotations

from typing import Any, Dict, List, Optional, Sequence

STATES = ("unselected", "selected")


def drop_nested(rows: Sequence[Sequence[int]]) -> List[List[int]]:
    """A mark whose box lies inside another mark's box is dropped: a filled square that stands clear of its frame is a frame of its
    own to the device.  Of two marks with the same box the first stays.  The order of the rows is kept."""
    rows = [[int(v) for v in r] for r in rows]
    out = []
    for i, a in enumerate(rows):
        inside = False
        for j, b in enumerate(rows):
            if i != j and b[0] <= a[0] and b[1] <= a[1] and a[2] <= b[2] and a[3] <= b[3] and (a[:4] != b[:4] or j < i):
                inside = True
                break
        if not inside:
            out.append(a)
    return out


def _mark(row: Sequence[int], shape: str) -> Dict[str, Any]:
    x0, y0, x1, y1, edge, _, _, state = row
    w, h = x1 - x0 + 1, y1 - y0 + 1
    return dict(box=(x0, y0, x1, y1), state=STATES[1 if state else 0], confidence=float(edge) / float(2 * (w + h)),
                polygon=[float(x0), float(y0), float(x1), float(y0), float(x1), float(y1), float(x0), float(y1)], shape=shape)


def select_marks(rows: Sequence[Sequence[int]], round_rows: Optional[Sequence[Sequence[int]]] = None) -> List[Dict[str, Any]]:
    """Device rows of one page -> [dict(box=(x0, y0, x1, y1), state, confidence, polygon, shape)], nested marks dropped, in the rows' order
    (top to bottom, left to right).  confidence = the share of the box's perimeter that carries ink, edge / (2 (w + h)); polygon = the
    box corners TL, TR, BR, BL as 8 floats; shape = "square" for a checkbox row, "round" for a row of round_rows (the radio buttons,
    same row format).  With round_rows the two lists are merged in (y0, x0) order, a checkbox before a round mark at the same corner, and
    nesting is judged over the union: a centre dot that stands clear of its ring is no mark of its own."""
    tagged = [([int(v) for v in r], "square") for r in rows]
    if round_rows is not None and len(round_rows):
        tagged += [([int(v) for v in r], "round") for r in round_rows]
        tagged.sort(key=lambda t: (t[0][1], t[0][0]))       # stable: each list keeps its own order within equal corners
    kept = drop_nested([row + [i] for i, (row, _) in enumerate(tagged)])     # (a trailing index: which of the tagged rows stayed)
    return [_mark(r[:8], tagged[r[8]][1]) for r in kept]
