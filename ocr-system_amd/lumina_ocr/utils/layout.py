"""Engine output -> the reference's result schema (layout_boxes, markdown, html).

Schema (stored verbatim in extractions.layout_data and consumed by BoundingBoxMatcher and the UI):
  {"type": "word"|"line", "content": str, ["confidence": float,] "polygon": [x1,y1,..,x4,y4], "page_number": int}
  /root/reference/backend/services/ocr_service.py:293-311; fixture /root/reference/azure_debug_output.json:5-166.
  Units: pixels of the processed image (fixture page 2000.0 x 1090.0, :172-173), origin top-left, TL,TR,BR,BL.
A det+rec engine yields line quads; `line` entries are mandatory for matching
(/root/reference/backend/utils/bbox_matcher.py:47, :103-144) and `word` entries feed the union fallback
(:48, :155-208), so words are synthesised by splitting the line text on spaces and interpolating along the quad — or, with the
provider's LUMINA_OCR_WORD_BOXES=1, taken from the recogniser's CTC alignment (build_layout_boxes(words=...)).
"""
from __future__ import annotations

import html
from typing import Any, Dict, List, Optional, Sequence, Tuple

from . import tables as _tables
from .ocr_postprocessor import MergedLine, TextBlock, group_into_lines, sort_and_merge_lines


def _lerp(a: Sequence[float], b: Sequence[float], t: float) -> Tuple[float, float]:
    return a[0] + (b[0] - a[0]) * t, a[1] + (b[1] - a[1]) * t


def split_words(quad: Sequence[float], text: str) -> List[Tuple[str, List[float]]]:
    """Proportional split of a line quad into word quads (character counts as widths, spaces included)."""
    tl, tr, br, bl = (quad[0], quad[1]), (quad[2], quad[3]), (quad[4], quad[5]), (quad[6], quad[7])
    n = len(text)
    out: List[Tuple[str, List[float]]] = []
    if n == 0:
        return out
    pos = 0
    for word in text.split(" "):
        if word:
            t0, t1 = pos / n, (pos + len(word)) / n
            a, b = _lerp(tl, tr, t0), _lerp(tl, tr, t1)
            c, d = _lerp(bl, br, t1), _lerp(bl, br, t0)
            out.append((word, [float(round(v)) for v in (*a, *b, *c, *d)]))
        pos += len(word) + 1
    return out


def build_layout_boxes(lines: Sequence[Tuple[Sequence[int], str, float]], page_number: int = 1,
                       words: Optional[Sequence[Sequence[Tuple[int, int, Sequence[int], float]]]] = None) -> List[Dict[str, Any]]:
    """lines: (quad 8 ints, text, score) in reading order -> words first, then lines (the order of ocr_service.py:285-311).
    words: None, or for every entry of `lines` its words as the device found them in the CTC alignment (PageDetections.line_words):
    (first character in the text, character count, quad 8 ints, confidence) in text order.  A line's `word` entries then take their
    polygon and confidence from those rows and their content from that span of the text, instead of split_words' proportional guess
    and the line's score.  Without `words` the result is the one without the argument."""
    if words is not None and len(words) != len(lines):
        raise ValueError("words must hold one list per line (%d lines, %d lists)" % (len(lines), len(words)))
    word_boxes: List[Dict[str, Any]] = []
    line_boxes: List[Dict[str, Any]] = []
    for i, (quad, text, score) in enumerate(lines):
        q = [float(v) for v in quad]
        if words is None:
            for w, wq in split_words(q, text):
                word_boxes.append({"type": "word", "content": w, "confidence": float(score), "polygon": wq, "page_number": page_number})
        else:
            for first, count, wq, conf in words[i]:
                word_boxes.append({"type": "word", "content": text[int(first):int(first) + int(count)], "confidence": float(conf),
                                   "polygon": [float(v) for v in wq], "page_number": page_number})
        line_boxes.append({"type": "line", "content": text, "polygon": q, "page_number": page_number})
    return word_boxes + line_boxes


def build_paragraph_boxes(merged: Sequence[MergedLine], page_number: int = 1, gap_ratio: float = 0.7) -> List[Dict[str, Any]]:
    """`paragraph` entries of the reference schema (/root/reference/backend/services/ocr_service.py:355-367: content cut to 100
    characters + "...", role, polygon, page_number).  Azure's layout model supplies them there; a det+rec engine derives them from
    the reading-order lines: consecutive lines belong to one paragraph while the vertical gap between them (top of the next minus
    bottom of the previous) stays within gap_ratio x their mean height.  Polygon = the axis-aligned hull of the paragraph's line
    quads (TL, TR, BR, BL); role = "title" for a first paragraph whose lines are at least 1.3 x the page's median line height, else
    "text" (the reference's fallback for a paragraph without a role, :362)."""
    rows = []
    for m in merged:
        pts = [pt for b in m.blocks for pt in b.box]
        if not pts or not m.text:
            continue
        xs, ys = [p[0] for p in pts], [p[1] for p in pts]
        rows.append((m.text, min(xs), min(ys), max(xs), max(ys)))
    if not rows:
        return []
    heights = sorted(r[4] - r[2] for r in rows)
    median_h = heights[len(heights) // 2]
    groups: List[List[Tuple[str, float, float, float, float]]] = [[rows[0]]]
    for prev, cur in zip(rows, rows[1:]):
        mean_h = ((prev[4] - prev[2]) + (cur[4] - cur[2])) / 2.0
        if cur[2] - prev[4] <= gap_ratio * mean_h:
            groups[-1].append(cur)
        else:
            groups.append([cur])
    out: List[Dict[str, Any]] = []
    for gi, g in enumerate(groups):
        text = " ".join(r[0] for r in g)
        x0, y0, x1, y1 = min(r[1] for r in g), min(r[2] for r in g), max(r[3] for r in g), max(r[4] for r in g)
        g_h = sum(r[4] - r[2] for r in g) / len(g)
        out.append({"type": "paragraph", "content": text[:100] + "..." if len(text) > 100 else text,
                    "role": "title" if gi == 0 and len(groups) > 1 and g_h >= 1.3 * median_h else "text",
                    "polygon": [float(x0), float(y0), float(x1), float(y0), float(x1), float(y1), float(x0), float(y1)], "page_number": page_number})
    return out


def reading_order(dets: Sequence[Tuple[Sequence[int], str, float]]) -> Tuple[List[MergedLine], List[Tuple[Sequence[int], str, float]]]:
    """Order detections with the reference's reading-order rules; returns (merged lines, detections in reading order)."""
    blocks = [TextBlock(text=t, confidence=float(s), box=[[float(q[0]), float(q[1])], [float(q[2]), float(q[3])],
                                                           [float(q[4]), float(q[5])], [float(q[6]), float(q[7])]]) for q, t, s in dets]
    index = {id(b): d for b, d in zip(blocks, dets)}
    merged = sort_and_merge_lines(group_into_lines(blocks)) if blocks else []
    ordered = [index[id(b)] for m in merged for b in m.blocks]
    return merged, ordered


def build_table_boxes(tables: Sequence[Dict[str, Any]], page_number: int = 1, first_table_index: int = 0) -> List[Dict[str, Any]]:
    """`table` and `table_cell` entries with the reference's keys (backend/services/ocr_service.py:324-352): every table
    (utils/tables.find_tables, cells filled by fill_cells) is followed by its cells in row-major order.  table_index counts from
    first_table_index (the document's tables so far: Azure's index runs over result.tables).  row_span / column_span are Azure's
    DocumentTableCell fields; they are added only when they exceed 1."""
    out: List[Dict[str, Any]] = []
    for k, t in enumerate(tables):
        out.append({"type": "table", "table_index": first_table_index + k, "row_count": int(t["row_count"]),
                    "column_count": int(t["column_count"]), "polygon": [float(v) for v in t["polygon"]], "page_number": page_number})
        for c in t["cells"]:
            cell = {"type": "table_cell", "content": c["content"], "row_index": int(c["row_index"]), "column_index": int(c["column_index"]),
                    "polygon": [float(v) for v in c["polygon"]], "page_number": page_number}
            if c.get("row_span", 1) > 1:
                cell["row_span"] = int(c["row_span"])
            if c.get("column_span", 1) > 1:
                cell["column_span"] = int(c["column_span"])
            out.append(cell)
    return out


def table_markdown(table: Dict[str, Any]) -> str:
    """A table the way Azure's Markdown content carries one: a <table> block, one <tr> per line, rowspan / colspan where they exceed 1,
    text HTML-escaped."""
    rows = ["<table>"]
    for r in range(table["row_count"]):
        tds = []
        for c in sorted((c for c in table["cells"] if c["row_index"] == r), key=lambda c: c["column_index"]):
            attr = (' rowspan="%d"' % c["row_span"] if c.get("row_span", 1) > 1 else "") + \
                   (' colspan="%d"' % c["column_span"] if c.get("column_span", 1) > 1 else "")
            tds.append("<td%s>%s</td>" % (attr, html.escape(c["content"], quote=False)))
        rows.append("<tr>%s</tr>" % "".join(tds))
    rows.append("</table>")
    return "\n".join(rows)


def build_mark_boxes(marks: Sequence[Dict[str, Any]], page_number: int = 1) -> List[Dict[str, Any]]:
    """`selection_mark` entries with the reference's keys (backend/services/ocr_service.py:313-322): type, state ("selected" /
    "unselected"), confidence, polygon, page_number; marks as utils/marks.select_marks gives them, in their order."""
    return [{"type": "selection_mark", "state": str(m["state"]), "confidence": float(m["confidence"]),
             "polygon": [float(v) for v in m["polygon"]], "page_number": page_number} for m in marks]


def build_barcode_boxes(found: Sequence[Dict[str, Any]], page_number: int = 1) -> List[Dict[str, Any]]:
    """`barcode` entries: type, kind ("Code128" / "Code39" / "EAN13" / "UPCA" / "EAN8" / "UPCE" / "ITF" / "QRCode" / "DataMatrix" / "Aztec"), content
    (the decoded text), confidence, polygon, page_number; barcodes as utils/barcodes.read_barcodes, utils/qrcodes.read_qrcodes and
    utils/datamatrix.read_datamatrix give them, in their order.  A QR or Data Matrix symbol whose content is out of scope has content ""
    and the reason under `unsupported`; an ITF-14 has `itf14`: True; a GS1 Data Matrix has `gs1`: True."""
    return [dict({"type": "barcode", "kind": str(b["kind"]), "content": str(b["content"]), "confidence": float(b["confidence"]),
                  "polygon": [float(v) for v in b["polygon"]], "page_number": page_number},
                 **({"unsupported": str(b["unsupported"])} if "unsupported" in b else {}), **({"itf14": True} if b.get("itf14") else {}),
                 **({"gs1": True} if b.get("gs1") else {})) for b in found]


def _with_barcode_lines(merged: Sequence[MergedLine], barcodes: Sequence[Dict[str, Any]]) -> List[MergedLine]:
    """The reading-order lines with a line `:barcode: <content>` for every barcode, each in front of the first line that lies below
    the barcode's centre (barcodes at one place keep their order)."""
    out = list(merged)
    for b in barcodes:
        x0, y0, x1, y1 = b["box"]
        cy = (y0 + y1 + 1) / 2.0
        text = ":barcode: %s" % b["content"]
        block = TextBlock(text, float(b["confidence"]), [[float(x0), float(y0)], [float(x1 + 1), float(y0)], [float(x1 + 1), float(y1 + 1)], [float(x0), float(y1 + 1)]])
        at = next((i for i, m in enumerate(out) if m.y_position > cy), len(out))
        out.insert(at, MergedLine(text, float(b["confidence"]), cy, [block]))
    return out


def _block_extent(b: TextBlock) -> Tuple[float, float, float]:
    """-> (left, top, bottom) of a detection's quad"""
    return min(pt[0] for pt in b.box), min(pt[1] for pt in b.box), max(pt[1] for pt in b.box)


def _markdown_with_marks(merged: Sequence[MergedLine], tables: Sequence[Dict[str, Any]], marks: Sequence[Dict[str, Any]]) -> str:
    """page_markdown for a page with selection marks.  A mark is Azure's Markdown token :selected: / :unselected: in front of the text
    of the detection that starts nearest to the right of the mark's centre and whose vertical extent holds that centre.  A mark without
    such a detection: inside a table cell it is appended to the cell, elsewhere it is a row of its own after the text, in mark order."""
    blocks = [b for m in merged for b in m.blocks]
    tokens: Dict[int, List[str]] = {}
    loose: List[Tuple[str, float, float]] = []
    for mk in marks:
        x0, y0, x1, y1 = mk["box"]
        cx, cy = (x0 + x1) / 2.0, (y0 + y1) / 2.0
        token = ":%s:" % mk["state"]
        best = None
        for b in blocks:
            left, top, bottom = _block_extent(b)
            if left >= cx and top <= cy <= bottom and (best is None or left < best[0]):
                best = (left, b)
        if best is None:
            loose.append((token, cx, cy))
        else:
            tokens.setdefault(id(best[1]), []).append(token)

    def text_of(b: TextBlock) -> str:
        return " ".join(tokens.get(id(b), []) + ([b.text] if b.text else []))

    # the tables' cells as the Markdown shows them: their detections again, in reading order, now with the tokens
    shown = [dict(t, cells=[dict(c, parts=[]) for c in t["cells"]]) for t in tables]
    rows: List[str] = []
    written = set()
    for m in merged:
        plain: List[str] = []
        for b in m.blocks:
            x, y = _tables.quad_centre([v for pt in b.box for v in pt])
            hit = next(((i, c) for i, t in enumerate(shown) for c in [_tables.cell_at(t, x, y)] if c is not None), None)
            if hit is None:
                if text_of(b):
                    plain.append(text_of(b))
                continue
            hit[1]["parts"].append(text_of(b))
            if hit[0] not in written:
                if plain:
                    rows.append(" ".join(plain))
                    plain = []
                written.add(hit[0])
                rows.append(hit[0])          # the table's place in the flow; its block is written once every cell is known
        if plain:
            rows.append(" ".join(plain))
    orphans = []
    for token, cx, cy in loose:
        cell = next((c for t in shown for c in [_tables.cell_at(t, cx, cy)] if c is not None), None)
        if cell is None:
            orphans.append(token)
        else:
            cell["parts"].append(token)
    for t in shown:
        for c in t["cells"]:
            c["content"] = " ".join(p for p in c["parts"] if p)
    rows = [table_markdown(shown[r]) if isinstance(r, int) else r for r in rows]
    rows.extend(table_markdown(t) for i, t in enumerate(shown) if i not in written)
    return "\n".join(rows + orphans)


def page_markdown(merged: Sequence[MergedLine], tables: Optional[Sequence[Dict[str, Any]]] = None,
                  marks: Optional[Sequence[Dict[str, Any]]] = None, barcodes: Optional[Sequence[Dict[str, Any]]] = None) -> str:
    """combined_markdown is fed verbatim to the LLM step and must be non-blank for a non-empty page
    (/root/reference/backend/services/extraction_service.py:290-295, :658-662): one reading-order line per row.
    tables (utils/tables.find_tables + fill_cells): every table is written as its <table> block at the position of its first contained
    line, and the lines inside it (quad centre in a cell) leave the plain flow; what is left of a row that crosses a table stays a row
    of its own.  Lines outside tables are unchanged.
    marks (utils/marks.select_marks): see _markdown_with_marks; without marks the result is the one without the argument.
    barcodes (utils/barcodes.read_barcodes): every barcode is a line `:barcode: <content>` of its own at its place in the reading order
    (_with_barcode_lines); without barcodes the result is the one without the argument."""
    if barcodes:
        merged = _with_barcode_lines(merged, barcodes)
    if marks:
        return _markdown_with_marks(merged, tables or [], marks)
    if not tables:
        return "\n".join(m.text for m in merged if m.text)
    rows: List[str] = []
    written = set()
    for m in merged:
        plain: List[str] = []
        inside = False
        for b in m.blocks:
            x, y = _tables.quad_centre([v for pt in b.box for v in pt])
            ti = next((i for i, t in enumerate(tables) if _tables.cell_at(t, x, y) is not None), -1)
            if ti < 0:
                plain.append(b.text)
                continue
            inside = True
            if ti not in written:
                if plain:
                    rows.append(" ".join(plain))
                    plain = []
                written.add(ti)
                rows.append(table_markdown(tables[ti]))
        if not inside:
            if m.text:
                rows.append(m.text)
        elif plain:
            rows.append(" ".join(plain))
    rows.extend(table_markdown(t) for i, t in enumerate(tables) if i not in written)   # a table without a line: after the text
    return "\n".join(rows)


def html_from_markdown(markdown_text: str) -> str:
    """ocr_service.py:378-392."""
    return f"<div class='ocr-content'>\n{markdown_text}\n</div>"


def combine_markdown(pages: Sequence[Any]) -> str:
    """ocr_service.py:737-746."""
    multi = len(pages) > 1
    parts = [(f"## Page {p.page_number}\n\n{p.markdown}" if multi else p.markdown) for p in pages if p.markdown]
    return "\n\n---\n\n".join(parts)


def combine_html(pages: Sequence[Any]) -> str:
    """ocr_service.py:748-757."""
    multi = len(pages) > 1
    parts = [(f'<section data-page="{p.page_number}">\n{p.html}\n</section>' if multi else p.html) for p in pages if p.html]
    return "\n<hr>\n".join(parts)


def validate_layout_boxes(boxes: Sequence[Dict[str, Any]]) -> List[str]:
    """Schema check against the reference fixture's shape; returns a list of problems (empty == valid)."""
    problems = []
    for i, b in enumerate(boxes):
        if b.get("type") not in ("word", "line", "selection_mark", "table", "table_cell", "paragraph", "barcode"):
            problems.append(f"{i}: bad type {b.get('type')!r}")
        poly = b.get("polygon")
        if not isinstance(poly, list) or len(poly) != 8 or not all(isinstance(v, float) for v in poly):
            problems.append(f"{i}: polygon must be 8 floats")
        if not isinstance(b.get("page_number"), int) or b["page_number"] < 1:
            problems.append(f"{i}: page_number must be int >= 1")
        if b.get("type") in ("word", "line") and not isinstance(b.get("content"), str):
            problems.append(f"{i}: content must be str")
        if b.get("type") == "word" and not isinstance(b.get("confidence"), float):
            problems.append(f"{i}: word confidence must be float")
        if b.get("type") == "barcode":
            if b.get("kind") not in ("Code128", "Code39", "EAN13", "UPCA", "EAN8", "UPCE", "ITF", "QRCode", "DataMatrix", "Aztec"):
                problems.append(f"{i}: barcode kind must be Code128, Code39, EAN13, UPCA, EAN8, UPCE, ITF, QRCode, DataMatrix or Aztec")
            if not isinstance(b.get("content"), str):
                problems.append(f"{i}: barcode content must be str")
            if not isinstance(b.get("confidence"), float) or not 0.0 <= b["confidence"] <= 1.0:
                problems.append(f"{i}: barcode confidence must be a float in 0..1")
        if b.get("type") == "table":
            for k in ("table_index", "row_count", "column_count"):
                if not isinstance(b.get(k), int) or isinstance(b.get(k), bool) or b[k] < (0 if k == "table_index" else 1):
                    problems.append(f"{i}: table {k} must be int >= {0 if k == 'table_index' else 1}")
        if b.get("type") == "table_cell":
            if not isinstance(b.get("content"), str):
                problems.append(f"{i}: table_cell content must be str")
            for k in ("row_index", "column_index"):
                if not isinstance(b.get(k), int) or isinstance(b.get(k), bool) or b[k] < 0:
                    problems.append(f"{i}: table_cell {k} must be int >= 0")
            for k in ("row_span", "column_span"):
                if k in b and (not isinstance(b[k], int) or isinstance(b[k], bool) or b[k] < 2):
                    problems.append(f"{i}: table_cell {k}, when present, must be int >= 2")
        if b.get("type") == "paragraph" and not (isinstance(b.get("content"), str) and len(b["content"]) <= 103 and isinstance(b.get("role"), str)):
            problems.append(f"{i}: paragraph needs content (<= 100 characters + '...') and role")
    return problems
