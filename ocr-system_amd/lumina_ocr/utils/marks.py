"""Selection marks, the host half: the device's rows (lumina_ocr_selection_marks: x0, y0, x1, y1, edge, ink_in, area_in, state per
mark) -> the marks of a page as the result schema wants them (reference backend/services/ocr_service.py:313-322: state
"selected" / "unselected", confidence, polygon).  Pure Python."""
from __future__ import annotations

from typing import Any, Dict, List, Sequence

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


def select_marks(rows: Sequence[Sequence[int]]) -> List[Dict[str, Any]]:
    """Device rows of one page -> [dict(box=(x0, y0, x1, y1), state, confidence, polygon)], nested marks dropped, in the rows' order
    (top to bottom, left to right).  confidence = the share of the box's perimeter that carries ink, edge / (2 (w + h)); polygon = the
    box corners TL, TR, BR, BL as 8 floats."""
    out = []
    for x0, y0, x1, y1, edge, _, _, state in drop_nested(rows):
        w, h = x1 - x0 + 1, y1 - y0 + 1
        out.append(dict(box=(x0, y0, x1, y1), state=STATES[1 if state else 0], confidence=float(edge) / float(2 * (w + h)),
                        polygon=[float(x0), float(y0), float(x1), float(y0), float(x1), float(y1), float(x0), float(y1)]))
    return out
