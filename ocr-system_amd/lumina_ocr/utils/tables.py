"""Ruled ("lattice") tables from the rules the device finds (lumina_ocr_table_rules): the host half of the reference's `table` /
`table_cell` entries (backend/services/ocr_service.py:324-352, where Azure's layout model supplies them).  Pure Python,
integer arithmetic, no GPU.

A rule is (x0, y0, x1, y1, area), inclusive pixel bounds.  Its centre-line is yc = (y0 + y1) // 2 (horizontal) or xc = (x0 + x1) // 2
(vertical).  A horizontal and a vertical rule TOUCH when each one's centre-line lies within the other's extent widened by `snap`.
A connected component of the touch graph with at least two rules of each direction is a table; its grid lines are the rounded means of
the centre-lines that lie within `snap` of their neighbours; cells across a missing boundary merge when every merged group stays a
rectangle (row_span / column_span), else the table keeps its elementary cells.
"""
from __future__ import annotations

from typing import Any, Dict, List, Sequence, Tuple

Rule = Sequence[int]


def _group_lines(centres: List[int], snap: int) -> Tuple[List[int], List[int]]:
    """sorted centre-lines -> (grid lines, group index of each centre): neighbours at most snap apart share a group, whose grid
    line is the rounded mean (2 * sum + n) // (2 * n)."""
    lines: List[int] = []
    index: List[int] = []
    group: List[int] = []
    for c in centres:
        if group and c - group[-1] > snap:
            lines.append((2 * sum(group) + len(group)) // (2 * len(group)))
            group = []
        group.append(c)
        index.append(len(lines))
    if group:
        lines.append((2 * sum(group) + len(group)) // (2 * len(group)))
    return lines, index


def _components(hrules: List[Rule], vrules: List[Rule], snap: int) -> List[Tuple[List[int], List[int]]]:
    nh, nv = len(hrules), len(vrules)
    parent = list(range(nh + nv))

    def find(i: int) -> int:
        while parent[i] != i:
            parent[i] = parent[parent[i]]
            i = parent[i]
        return i
    for i, h in enumerate(hrules):
        yc = (h[1] + h[3]) // 2
        for j, v in enumerate(vrules):
            xc = (v[0] + v[2]) // 2
            if h[0] - snap <= xc <= h[2] + snap and v[1] - snap <= yc <= v[3] + snap:
                a, b = find(i), find(nh + j)
                if a != b:
                    parent[max(a, b)] = min(a, b)
    comps: Dict[int, Tuple[List[int], List[int]]] = {}
    for i in range(nh + nv):
        hs, vs = comps.setdefault(find(i), ([], []))
        (hs if i < nh else vs).append(i if i < nh else i - nh)
    return [c for _, c in sorted(comps.items())]


def _covered(rules: List[Tuple[int, int]], lo: int, hi: int, snap: int) -> bool:
    """does some rule (start, end) of the grid line cover the side [lo, hi] to within snap at both ends"""
    return any(s <= lo + snap and e >= hi - snap for s, e in rules)


def _table(hrules: List[Rule], vrules: List[Rule], snap: int):
    hc = sorted(((h[1] + h[3]) // 2, h[0], h[2]) for h in hrules)
    vc = sorted(((v[0] + v[2]) // 2, v[1], v[3]) for v in vrules)
    ys, hidx = _group_lines([c[0] for c in hc], snap)
    xs, vidx = _group_lines([c[0] for c in vc], snap)
    rows, cols = len(ys) - 1, len(xs) - 1
    if rows < 1 or cols < 1:
        return None
    on_y: List[List[Tuple[int, int]]] = [[] for _ in ys]
    on_x: List[List[Tuple[int, int]]] = [[] for _ in xs]
    for (_, s, e), g in zip(hc, hidx):
        on_y[g].append((s, e))
    for (_, s, e), g in zip(vc, vidx):
        on_x[g].append((s, e))
    parent = list(range(rows * cols))

    def find(i: int) -> int:
        while parent[i] != i:
            parent[i] = parent[parent[i]]
            i = parent[i]
        return i

    def union(a: int, b: int) -> None:
        a, b = find(a), find(b)
        if a != b:
            parent[max(a, b)] = min(a, b)
    for r in range(rows):
        for c in range(cols):
            if r + 1 < rows and not _covered(on_y[r + 1], xs[c], xs[c + 1], snap):
                union(r * cols + c, (r + 1) * cols + c)
            if c + 1 < cols and not _covered(on_x[c + 1], ys[r], ys[r + 1], snap):
                union(r * cols + c, r * cols + c + 1)
    groups: Dict[int, List[int]] = {}
    for i in range(rows * cols):
        groups.setdefault(find(i), []).append(i)
    spans = []
    for root in sorted(groups):
        rr = [i // cols for i in groups[root]]
        cc = [i % cols for i in groups[root]]
        r0, r1, c0, c1 = min(rr), max(rr), min(cc), max(cc)
        if (r1 - r0 + 1) * (c1 - c0 + 1) != len(groups[root]):   # an L or a ring: the table keeps its elementary cells
            spans = [(i // cols, i % cols, 1, 1) for i in range(rows * cols)]
            break
        spans.append((r0, c0, r1 - r0 + 1, c1 - c0 + 1))
    spans.sort()

    def poly(x0: int, y0: int, x1: int, y1: int) -> List[float]:
        return [float(x0), float(y0), float(x1), float(y0), float(x1), float(y1), float(x0), float(y1)]
    cells = [dict(row_index=r, column_index=c, row_span=rs, column_span=cs, content="", polygon=poly(xs[c], ys[r], xs[c + cs], ys[r + rs]))
             for r, c, rs, cs in spans]
    return dict(xs=xs, ys=ys, row_count=rows, column_count=cols, polygon=poly(xs[0], ys[0], xs[-1], ys[-1]), cells=cells)


def find_tables(hrules: Sequence[Rule], vrules: Sequence[Rule], snap: int = 8) -> List[Dict[str, Any]]:
    """Rules of one page -> its tables, ordered by (top, left): dict(xs, ys, row_count, column_count, polygon (8 floats TL, TR, BR, BL on
    the grid lines), cells=[dict(row_index, column_index, row_span, column_span, polygon, content="")]), cells in row-major order."""
    hr = [[int(v) for v in r[:4]] for r in hrules]
    vr = [[int(v) for v in r[:4]] for r in vrules]
    out = []
    for hs, vs in _components(hr, vr, int(snap)):
        if len(hs) < 2 or len(vs) < 2:
            continue
        t = _table([hr[i] for i in hs], [vr[j] for j in vs], int(snap))
        if t is not None:
            out.append(t)
    out.sort(key=lambda t: (t["ys"][0], t["xs"][0]))
    return out


def quad_centre(quad: Sequence[float]) -> Tuple[float, float]:
    return (quad[0] + quad[2] + quad[4] + quad[6]) / 4.0, (quad[1] + quad[3] + quad[5] + quad[7]) / 4.0


def cell_at(table: Dict[str, Any], x: float, y: float):
    """The cell holding the point, or None outside the table.  Intervals are half-open on the grid lines (left / top included), so
    every point of the table belongs to exactly one cell."""
    xs, ys = table["xs"], table["ys"]
    if not (xs[0] <= x < xs[-1] and ys[0] <= y < ys[-1]):
        return None
    for cell in table["cells"]:
        r, c = cell["row_index"], cell["column_index"]
        if xs[c] <= x < xs[c + cell["column_span"]] and ys[r] <= y < ys[r + cell["row_span"]]:
            return cell
    return None


def fill_cells(tables: List[Dict[str, Any]], ordered_lines: Sequence[Tuple[Sequence[float], str, float]]) -> List[int]:
    """Cell content = the detected lines whose quad centre falls in the cell, joined by one space in the order given (the reading order
    of layout.reading_order).  -> for every line the index of its table, or -1."""
    texts: Dict[int, List[str]] = {}
    where = []
    for quad, text, _ in ordered_lines:
        x, y = quad_centre([float(v) for v in quad])
        hit = -1
        for ti, t in enumerate(tables):
            cell = cell_at(t, x, y)
            if cell is not None:
                texts.setdefault(id(cell), []).append(text)
                hit = ti
                break
        where.append(hit)
    for t in tables:
        for cell in t["cells"]:
            cell["content"] = " ".join(texts.get(id(cell), []))
    return where
