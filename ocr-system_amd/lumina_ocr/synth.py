"""Seeded synthetic pages and line crops (no reference images exist offline —
backend/test_image.png is listed in /root/reference/.MISSING_LARGE_BLOBS).  Used by bench.py,
tests and tools; pure PIL/numpy, no network, no files."""
from __future__ import annotations

from typing import List, Tuple

import numpy as np
from PIL import Image, ImageDraw, ImageFont

ALPHABET = "ABCDEFGHIJKLMNOPQRSTUVWXYZabcdefghijklmnopqrstuvwxyz0123456789 .,:-/()#&@%+=?!'\"$;"  # 80 chars
A4_200DPI = (2339, 1654)  # (H, W)

_fonts = {}


def _font(size: int):
    if size not in _fonts:
        _fonts[size] = ImageFont.load_default(size=size)
    return _fonts[size]


def random_text(rng: np.random.Generator, lo: int = 4, hi: int = 24) -> str:
    n = int(rng.integers(lo, hi + 1))
    s = "".join(ALPHABET[int(i)] for i in rng.integers(0, len(ALPHABET), n)).strip()
    return s or "A"


def synth_page(h: int, w: int, seed: int, n_lines: int = 60, noise: float = 3.0, ruled: bool = False) -> Tuple[np.ndarray, List[dict]]:
    """White page with rendered text lines (10-14 pt at 200 DPI ~ 28-39 px) + Gaussian noise.
    ruled: every line is underlined by a rule size // 3 px thick, 2 px under its text, as on a filled-in form (same text otherwise).
    -> (uint8 [h,w,3], [{'text', 'box': (x0,y0,x1,y1)}])"""
    rng = np.random.default_rng(seed)
    img = Image.new("RGB", (w, h), (255, 255, 255))
    d = ImageDraw.Draw(img)
    gt = []
    scale = min(1.0, h / 2339.0 * 1.6 + 0.2)
    margin = max(4, int(0.06 * w))
    y = max(4, int(0.04 * h))
    pitch = max(14, (h - 2 * y) // max(n_lines, 1))
    for _ in range(n_lines):
        size = max(10, int(rng.integers(28, 40) * scale))
        if y + size + 4 >= h:
            break
        x = margin + int(rng.integers(0, max(1, w // 10)))
        words = []
        while True:
            words.append(random_text(rng, 3, 12))
            txt = " ".join(words)
            if d.textlength(txt, font=_font(size)) > (w - margin - x) * float(rng.uniform(0.35, 0.95)) or len(words) > 12:
                break
        while len(txt) > 1 and x + d.textlength(txt, font=_font(size)) > w - margin:
            txt = txt[:-1]
        shade = int(rng.integers(0, 41))
        d.text((x, y), txt, fill=(shade, shade, shade), font=_font(size))
        bb = d.textbbox((x, y), txt, font=_font(size))
        if ruled:
            d.rectangle((bb[0], bb[3] + 2, bb[2], bb[3] + 1 + size // 3), fill=(shade, shade, shade))
            bb = (bb[0], bb[1], bb[2], bb[3] + 1 + size // 3)
        gt.append(dict(text=txt, box=bb))
        y += max(pitch, size + 6)
    arr = np.asarray(img, np.float32)
    if noise > 0:
        arr = arr + rng.normal(0.0, noise, arr.shape).astype(np.float32)
    return np.clip(np.rint(arr), 0, 255).astype(np.uint8), gt


def synth_crop(rng: np.random.Generator) -> Tuple[np.ndarray, str]:
    """One 32x320 line crop with a rendered random string (len 4-24), right-padded with 0."""
    txt = random_text(rng)
    img = Image.new("RGB", (320, 32), (255, 255, 255))
    d = ImageDraw.Draw(img)
    size = 22
    while size > 8 and d.textlength(txt, font=_font(size)) > 312:
        size -= 1
    d.text((4, max(0, (32 - size) // 2 - 2)), txt, fill=(20, 20, 20), font=_font(size))
    arr = np.asarray(img, np.uint8).copy()
    tw = int(min(320, d.textlength(txt, font=_font(size)) + 8))
    arr[:, tw:] = 0
    return arr, txt


def synth_form_page(seed: int = 0, w: int = 2000, h: int = 1090) -> Tuple[np.ndarray, List[dict]]:
    """A 2000x1090 form-like page mimicking the layout of the reference's captured sample
    (/root/reference/azure_debug_output.json:172-173: page 2000.0 x 1090.0)."""
    rng = np.random.default_rng(seed)
    img = Image.new("RGB", (w, h), (255, 255, 255))
    d = ImageDraw.Draw(img)
    gt = []

    def put(x, y, txt, size):
        d.text((x, y), txt, fill=(15, 15, 15), font=_font(size))
        gt.append(dict(text=txt, box=d.textbbox((x, y), txt, font=_font(size))))

    put(385, 150, "SPRINGFIELD UNIVERSITY - UNDERGRADUATE ADMISSION", 40)
    rows = [("Applicant Name:", "Jordan A. Whitfield"), ("Date of Birth:", "14/03/2004"), ("Program:", "B.Sc. Computer Science"),
            ("Student ID:", "SU-2024-%05d" % int(rng.integers(0, 99999))), ("Email:", "j.whitfield@example.edu"),
            ("Phone:", "+1 555 0134"), ("Address:", "221 Maple Avenue, Springfield"), ("Guardian:", "Morgan Whitfield")]
    y = 280
    for k, v in rows:
        put(140, y, k, 32)
        put(620, y, v, 32)
        y += 88
    return np.asarray(img, np.uint8).copy(), gt


def synth_table_page(seed: int, h: int = 1100, w: int = 1500, n_tables: int = 1, thickness: int = 0, inset: int = 14, spans: bool = False,
                     noise: float = 0.0, rows: int = 0, cols: int = 0, size: int = 0) -> Tuple[np.ndarray, List[dict]]:
    """White page with n_tables ruled tables under a title line, one text per cell.
    thickness: rule thickness in pixels (0: drawn from the seed, 2-5); inset: clear distance between a rule and the text box of its
    cell; spans: the first row is one header cell across all columns and, with three or more rows, the first column's cells of rows 1
    and 2 are one cell; rows / cols / size: grid and font size (0: from the seed, 2-5 x 2-4, 26-34 px scaled like synth_page).
    -> (uint8 [h,w,3], [dict(xs, ys, thickness, row_count, column_count, cells=[dict(row_index, column_index, row_span, column_span,
    text, box)])]): xs / ys are the centre-lines of the drawn rules, (first + last pixel) // 2; cells in row-major order."""
    rng = np.random.default_rng(seed)
    img = Image.new("RGB", (w, h), (255, 255, 255))
    d = ImageDraw.Draw(img)
    scale = min(1.0, h / 2339.0 * 1.6 + 0.2)
    margin = max(8, int(0.06 * w))
    y = max(8, int(0.04 * h))
    tsize = max(10, int(30 * scale))
    d.text((margin, y), "Table %d" % seed, fill=(20, 20, 20), font=_font(tsize))
    y += tsize + 3 * inset
    gt = []
    for _ in range(n_tables):
        t = int(thickness) if thickness else int(rng.integers(2, 6))
        nr = int(rows) if rows else int(rng.integers(2, 6))
        nc = int(cols) if cols else int(rng.integers(2, 5))
        fs = int(size) if size else max(10, int(rng.integers(26, 35) * scale))
        row_h = max(72, fs + 2 * inset + t + 10)
        left = margin + int(rng.integers(0, max(1, w // 12)))
        right = w - margin - int(rng.integers(0, max(1, w // 12)))
        col_w = (right - left - t) // nc
        if y + nr * row_h + t >= h - 4 or col_w < 2 * inset + t + 3 * fs:
            break
        x0 = [left + c * col_w for c in range(nc + 1)]       # first pixel of every vertical rule
        y0 = [y + r * row_h for r in range(nr + 1)]          # first pixel of every horizontal rule
        group = {(r, c): (r, c) for r in range(nr) for c in range(nc)}   # cell -> top-left cell of its group
        span = {(r, c): (1, 1) for r in range(nr) for c in range(nc)}
        if spans:
            for c in range(nc):
                group[(0, c)] = (0, 0)
            span[(0, 0)] = (1, nc)
            if nr >= 3:
                group[(2, 0)] = (1, 0)
                span[(1, 0)] = (2, 1)
        shade = int(rng.integers(0, 41))
        ink = (shade, shade, shade)
        for k in range(nr + 1):
            for c in range(nc):
                if k in (0, nr) or group[(k - 1, c)] != group[(k, c)]:
                    d.rectangle((x0[c], y0[k], x0[c + 1] + t - 1, y0[k] + t - 1), fill=ink)
        for k in range(nc + 1):
            for r in range(nr):
                if k in (0, nc) or group[(r, k - 1)] != group[(r, k)]:
                    d.rectangle((x0[k], y0[r], x0[k] + t - 1, y0[r + 1] + t - 1), fill=ink)
        cells = []
        for r in range(nr):
            for c in range(nc):
                if group[(r, c)] != (r, c):
                    continue
                rs, cs = span[(r, c)]
                tx, ty = x0[c] + t + inset, y0[r] + t + inset
                room = x0[c + cs] - inset - tx
                txt = random_text(rng, 4, 9).replace(" ", "x")
                while len(txt) > 1 and d.textbbox((tx, ty), txt, font=_font(fs))[2] - tx > room:
                    txt = txt[:-1]
                tshade = int(rng.integers(0, 41))
                d.text((tx, ty), txt, fill=(tshade, tshade, tshade), font=_font(fs))
                cells.append(dict(row_index=r, column_index=c, row_span=rs, column_span=cs, text=txt, box=d.textbbox((tx, ty), txt, font=_font(fs))))
        gt.append(dict(xs=[(2 * v + t - 1) // 2 for v in x0], ys=[(2 * v + t - 1) // 2 for v in y0], thickness=t, row_count=nr, column_count=nc,
                       cells=cells))
        y = y0[-1] + t + 4 * inset + tsize
    arr = np.asarray(img, np.float32)
    if noise > 0:
        arr = arr + rng.normal(0.0, noise, arr.shape).astype(np.float32)
    return np.clip(np.rint(arr), 0, 255).astype(np.uint8), gt


MARK_KINDS = ("empty", "cross", "tick", "filled", "block")   # the first is unselected, the others selected


def _draw_mark(d: ImageDraw.ImageDraw, x0: int, y0: int, side: int, stroke: int, kind: str, ink) -> None:
    """A square frame of `stroke` pixels with its first pixel at (x0, y0), and what is in it: nothing, a cross, a tick, all of it
    filled, or a filled block 2 pixels clear of the frame.  Nothing leaves the square."""
    x1, y1 = x0 + side - 1, y0 + side - 1
    for k in range(stroke):
        d.rectangle((x0 + k, y0 + k, x1 - k, y1 - k), outline=ink)
    pen = max(stroke, 1 + side // 12)          # the pen that ticks a box is not thinner than a twelfth of it
    a = stroke + 1 + pen // 2                  # first and last pixel of the pen's centre-line, relative to the corner
    b = side - 1 - a
    if kind == "cross":
        d.line((x0 + a, y0 + a, x0 + b, y0 + b), fill=ink, width=pen)
        d.line((x0 + a, y0 + b, x0 + b, y0 + a), fill=ink, width=pen)
    elif kind == "tick":
        d.line((x0 + a, y0 + side // 2, x0 + side // 2, y0 + b), fill=ink, width=pen)
        d.line((x0 + side // 2, y0 + b, x0 + b, y0 + a), fill=ink, width=pen)
    elif kind == "filled":
        d.rectangle((x0, y0, x1, y1), fill=ink)
    elif kind == "block":
        d.rectangle((x0 + stroke + 2, y0 + stroke + 2, x1 - stroke - 2, y1 - stroke - 2), fill=ink)


def synth_marks_page(seed: int, h: int = 1100, w: int = 1500, n_marks: int = 12, stroke: int = 0, side: int = 0, noise: float = 0.0,
                     table: bool = True, min_side: int = 12, max_side: int = 64) -> Tuple[np.ndarray, List[dict]]:
    """White form page with checkboxes: a title line, n_marks boxes in two columns, each with a label to its right, and (table) a ruled
    2 x 2 table whose cells hold a box and a label, clear of the rules.
    side: the box side in pixels (0: drawn from the seed per box, min_side .. max_side); stroke: the frame's thickness (0: from the
    seed, 1-4), never more than side // 4, so that the frame stays out of the interior the state is read from; kind per box from the
    seed (MARK_KINDS).  -> (uint8 [h,w,3], [dict(box=(x0, y0, x1, y1) inclusive, state='selected' | 'unselected', kind, stroke,
    label, label_box, in_table)]) in drawing order: top to bottom, the left column before the right one in a row."""
    rng = np.random.default_rng(seed)
    img = Image.new("RGB", (w, h), (255, 255, 255))
    d = ImageDraw.Draw(img)
    scale = min(1.0, h / 2339.0 * 1.6 + 0.2)
    margin = max(8, int(0.06 * w))
    y = max(8, int(0.04 * h))
    tsize = max(10, int(30 * scale))
    fs = max(10, int(28 * scale))
    d.text((margin, y), "Form %d" % seed, fill=(20, 20, 20), font=_font(tsize))
    y += tsize + 40
    gt: List[dict] = []

    def put(x: int, yy: int, room: int, in_table: bool) -> int:
        """box with its corner at (x, yy) + label; -> the box side"""
        s = int(side) if side else int(rng.integers(min_side, max_side + 1))
        t = max(1, min(int(stroke) if stroke else int(rng.integers(1, 5)), s // 4))
        kind = MARK_KINDS[int(rng.integers(0, len(MARK_KINDS)))]
        shade = int(rng.integers(0, 41))
        _draw_mark(d, x, yy, s, t, kind, (shade, shade, shade))
        tx, ty = x + s + s // 2 + 8, yy + max(0, (s - fs) // 2)
        txt = random_text(rng, 4, 10).replace(" ", "x")
        while len(txt) > 1 and d.textbbox((tx, ty), txt, font=_font(fs))[2] > x + room:
            txt = txt[:-1]
        d.text((tx, ty), txt, fill=(shade, shade, shade), font=_font(fs))
        gt.append(dict(box=(x, yy, x + s - 1, yy + s - 1), state="unselected" if kind == "empty" else "selected", kind=kind, stroke=t,
                       label=txt, label_box=d.textbbox((tx, ty), txt, font=_font(fs)), in_table=in_table))
        return s

    col_w = (w - 2 * margin) // 2
    k = 0
    while k < n_marks:
        row_side = 0
        for c in range(2):
            if k < n_marks and y + max_side + 8 < h:
                row_side = max(row_side, put(margin + c * col_w + int(rng.integers(0, 24)), y, col_w - 30, False))
                k += 1
        if row_side == 0:
            break
        y += max(row_side, fs) + 26
    if table:
        t, row_h = 3, max_side + 2 * 20 + 3
        y += 20
        if y + 2 * row_h + t < h - 4:
            xs = [margin, margin + col_w, margin + 2 * col_w]
            ys = [y, y + row_h, y + 2 * row_h]
            for yy in ys:
                d.rectangle((xs[0], yy, xs[-1] + t - 1, yy + t - 1), fill=(10, 10, 10))
            for xx in xs:
                d.rectangle((xx, ys[0], xx + t - 1, ys[-1] + t - 1), fill=(10, 10, 10))
            for r in range(2):
                for c in range(2):
                    put(xs[c] + t + 20, ys[r] + t + 20, col_w - 40, True)
    arr = np.asarray(img, np.float32)
    if noise > 0:
        arr = arr + rng.normal(0.0, noise, arr.shape).astype(np.float32)
    return np.clip(np.rint(arr), 0, 255).astype(np.uint8), gt


def _draw_radio(d: ImageDraw.ImageDraw, x0: int, y0: int, diameter: int, stroke: int, dot: bool, ink) -> None:
    """A ring of `stroke` pixels whose bounding box has its first pixel at (x0, y0) and `diameter` pixels a side, and (dot) a filled
    disc in its centre of under half the diameter, clear of the ring."""
    d.ellipse((x0, y0, x0 + diameter - 1, y0 + diameter - 1), outline=ink, width=stroke)
    if dot:
        dd = max(2, diameter // 2 - 2)
        a = (diameter - dd) // 2
        d.ellipse((x0 + a, y0 + a, x0 + a + dd - 1, y0 + a + dd - 1), fill=ink)


RADIO_MAX_STROKE = 4


def synth_radio_page(seed: int, h: int = 1100, w: int = 1500, n_marks: int = 12, stroke: int = 0, diameter: int = 0, noise: float = 0.0,
                     table: bool = True, min_side: int = 12, max_side: int = 64) -> Tuple[np.ndarray, List[dict]]:
    """White form page with radio buttons, laid out as synth_marks_page lays out its boxes: a title line, n_marks marks in two columns,
    each with a label to its right at the same distance, every fourth of them a checkbox (_draw_mark) instead of a radio button, and
    (table) a ruled 2 x 2 table whose cells hold a group of four radio buttons with labels, clear of the rules.
    diameter: of the radio buttons (and side of the checkboxes) in pixels (0: from the seed per mark, min_side .. max_side); stroke: the
    ring's thickness (0: from the seed, 1 .. RADIO_MAX_STROKE), never more than diameter // 12: a radio ring is thin; a radio button is
    empty or has a centre dot, from the seed.  -> (uint8 [h,w,3], [dict(box, state, kind, stroke, label, label_box, in_table,
    shape='round' | 'square')]) in drawing order."""
    rng = np.random.default_rng(seed)
    img = Image.new("RGB", (w, h), (255, 255, 255))
    d = ImageDraw.Draw(img)
    scale = min(1.0, h / 2339.0 * 1.6 + 0.2)
    margin = max(8, int(0.06 * w))
    y = max(8, int(0.04 * h))
    tsize = max(10, int(30 * scale))
    fs = max(10, int(28 * scale))
    d.text((margin, y), "Choice %d" % seed, fill=(20, 20, 20), font=_font(tsize))
    y += tsize + 40
    gt: List[dict] = []

    def put(x: int, yy: int, room: int, in_table: bool, square: bool) -> int:
        s = int(diameter) if diameter else int(rng.integers(min_side, max_side + 1))
        want = int(stroke) if stroke else int(rng.integers(1, RADIO_MAX_STROKE + 1))
        shade = int(rng.integers(0, 41))
        if square:
            t = max(1, min(want, s // 4))
            kind = MARK_KINDS[int(rng.integers(0, len(MARK_KINDS)))]
            _draw_mark(d, x, yy, s, t, kind, (shade, shade, shade))
            state = "unselected" if kind == "empty" else "selected"
        else:
            t = max(1, min(want, s // 12))
            dot = bool(rng.integers(0, 2))
            _draw_radio(d, x, yy, s, t, dot, (shade, shade, shade))
            kind, state = ("dot", "selected") if dot else ("empty", "unselected")
        tx, ty = x + s + s // 2 + 8, yy + max(0, (s - fs) // 2)
        txt = random_text(rng, 4, 10).replace(" ", "x")
        while len(txt) > 1 and d.textbbox((tx, ty), txt, font=_font(fs))[2] > x + room:
            txt = txt[:-1]
        d.text((tx, ty), txt, fill=(shade, shade, shade), font=_font(fs))
        gt.append(dict(box=(x, yy, x + s - 1, yy + s - 1), state=state, kind=kind, stroke=t, label=txt,
                       label_box=d.textbbox((tx, ty), txt, font=_font(fs)), in_table=in_table, shape="square" if square else "round"))
        return s

    col_w = (w - 2 * margin) // 2
    k = 0
    while k < n_marks:
        row_side = 0
        for c in range(2):
            if k < n_marks and y + max_side + 8 < h:
                row_side = max(row_side, put(margin + c * col_w + int(rng.integers(0, 24)), y, col_w - 30, False, k % 4 == 3))
                k += 1
        if row_side == 0:
            break
        y += max(row_side, fs) + 26
    if table:
        t, row_h = 3, max_side + 2 * 20 + 3
        y += 20
        if y + 2 * row_h + t < h - 4:
            xs = [margin, margin + col_w, margin + 2 * col_w]
            ys = [y, y + row_h, y + 2 * row_h]
            for yy in ys:
                d.rectangle((xs[0], yy, xs[-1] + t - 1, yy + t - 1), fill=(10, 10, 10))
            for xx in xs:
                d.rectangle((xx, ys[0], xx + t - 1, ys[-1] + t - 1), fill=(10, 10, 10))
            for r in range(2):
                for c in range(2):
                    put(xs[c] + t + 20, ys[r] + t + 20, col_w - 40, True, False)
    arr = np.asarray(img, np.float32)
    if noise > 0:
        arr = arr + rng.normal(0.0, noise, arr.shape).astype(np.float32)
    return np.clip(np.rint(arr), 0, 255).astype(np.uint8), gt


ROUND_DECOY_SIZES = (16, 20, 24, 28, 34, 40, 48, 56, 64, 70)
ROUND_DECOY_WORDS = ("Of", "OK", "On", "OQDCG0oe@", "GOOD", "DOG", "Oo0", "CoCo", "e@o", "QUOTE", "O0O", "oOo")


def synth_round_decoys(seed: int, h: int = 1100, w: int = 1500, noise: float = 0.0) -> Tuple[np.ndarray, List[dict]]:
    """White page of what is round and no radio button.  One line of words per font size of ROUND_DECOY_SIZES (16-70 px), the words
    drawn from ROUND_DECOY_WORDS and from random_text with an O in front, in seeded order; and, on a free strip to the right, a solid
    filled disc, a circle touching a rule, a circle with a letter in it, and two concentric rings, at seeded diameters.
    -> (uint8 [h,w,3], [dict(kind, box)]) of the four shapes."""
    rng = np.random.default_rng(seed)
    img = Image.new("RGB", (w, h), (255, 255, 255))
    d = ImageDraw.Draw(img)
    margin = max(8, int(0.06 * w))
    strip = w - margin - 220                      # the shapes' strip starts here
    y = max(8, int(0.03 * h))
    for size in ROUND_DECOY_SIZES:
        if y + size + 8 >= h:
            break
        x = margin + int(rng.integers(0, 30))
        order = rng.permutation(len(ROUND_DECOY_WORDS))
        for i in order:
            word = ROUND_DECOY_WORDS[int(i)] if rng.integers(0, 3) else "O" + random_text(rng, 2, 5).replace(" ", "o")
            bb = d.textbbox((x, y), word, font=_font(size))
            if bb[2] >= strip - 20:
                break
            shade = int(rng.integers(0, 41))
            d.text((x, y), word, fill=(shade, shade, shade), font=_font(size))
            x = bb[2] + max(6, size // 3)
        y += size + max(10, size // 2)
    gt = []
    ink = (10, 10, 10)
    x, y = strip, max(8, int(0.04 * h))
    s = int(rng.integers(14, 61))
    d.ellipse((x, y, x + s - 1, y + s - 1), fill=ink)                                  # a solid disc
    gt.append(dict(kind="disc", box=(x, y, x + s - 1, y + s - 1)))
    y += s + 60
    s = int(rng.integers(20, 61))
    d.ellipse((x, y, x + s - 1, y + s - 1), outline=ink, width=max(1, s // 16))         # a circle standing on a rule
    d.rectangle((x - 40, y + s - 1, x + s + 80, y + s + 1), fill=ink)
    gt.append(dict(kind="on_rule", box=(x, y, x + s - 1, y + s - 1)))
    y += s + 60
    s = int(rng.integers(36, 65))
    d.ellipse((x, y, x + s - 1, y + s - 1), outline=ink, width=max(1, s // 16))         # a circle with a letter in it
    fs = (3 * s) // 4
    letter = "CRPM"[int(rng.integers(0, 4))]
    bb = d.textbbox((0, 0), letter, font=_font(fs))
    d.text((x + (s - (bb[2] + bb[0])) // 2, y + (s - (bb[3] + bb[1])) // 2), letter, fill=ink, font=_font(fs))
    gt.append(dict(kind="lettered", box=(x, y, x + s - 1, y + s - 1)))
    y += s + 60
    s = int(rng.integers(32, 65))
    d.ellipse((x, y, x + s - 1, y + s - 1), outline=ink, width=max(1, s // 20))         # two concentric rings
    a = max(3, s // 8)
    d.ellipse((x + a, y + a, x + s - 1 - a, y + s - 1 - a), outline=ink, width=max(1, s // 20))
    gt.append(dict(kind="concentric", box=(x, y, x + s - 1, y + s - 1)))
    arr = np.asarray(img, np.float32)
    if noise > 0:
        arr = arr + rng.normal(0.0, noise, arr.shape).astype(np.float32)
    return np.clip(np.rint(arr), 0, 255).astype(np.uint8), gt


# ---- barcodes (Code 128, Code 39): an encoder of our own (no barcode library exists offline); tables in utils/barcodes.py ----
def code128_symbols(text: str) -> List[int]:
    """ASCII text -> the symbol values start, data ..., check, stop with an automatic choice of code sets: runs of four or more digits
    (an even count of them) go to set C, control characters need set A, lower case needs set B; a single character of the other set
    among characters of the current one takes a SHIFT, more of them a code switch."""
    from .utils import barcodes as bc
    if not text or any(ord(c) > 127 for c in text):
        raise ValueError("Code 128 text must be non-empty ASCII")

    def digits_at(i):
        j = i
        while j < len(text) and text[j].isdigit():
            j += 1
        return j - i

    def need(c):   # the set a character needs, or None when both A and B hold it
        return "A" if ord(c) < 32 else "B" if ord(c) >= 96 else None

    def first_need(i):
        for c in text[i:]:
            if need(c):
                return need(c)
        return "B"

    n0 = digits_at(0)
    cur = "C" if n0 >= 4 or (n0 == len(text) and n0 % 2 == 0) else first_need(0)
    vals = [{"A": bc.C128_START_A, "B": bc.C128_START_B, "C": bc.C128_START_C}[cur]]
    i = 0
    while i < len(text):
        nd = digits_at(i)
        if cur == "C":
            if nd >= 2:
                vals.append(int(text[i:i + 2]))
                i += 2
                continue
            cur = first_need(i)
            vals.append(101 if cur == "A" else 100)
            continue
        if nd >= 4 and (nd % 2 == 0 or nd >= 5):
            if nd % 2:                 # an odd run: its first digit stays in the current set
                vals.append(ord(text[i]) - 32)
                i += 1
            vals.append(99)
            cur = "C"
            continue
        c = text[i]
        want = need(c)
        if want and want != cur:
            nxt = need(text[i + 1]) if i + 1 < len(text) else None
            if nxt != want and (i + 1 < len(text)):
                vals.append(98)        # SHIFT: this character alone
                vals.append(ord(c) - 32 if want == "B" else ord(c) + 64)
                i += 1
                continue
            vals.append(101 if want == "A" else 100)
            cur = want
        vals.append(ord(c) + 64 if ord(c) < 32 else ord(c) - 32)
        i += 1
    check = (vals[0] + sum(k * v for k, v in enumerate(vals[1:], 1))) % 103
    return vals + [check, bc.C128_STOP]


def code39_symbols(text: str) -> List[int]:
    """Text over Code 39's 43 characters -> the character indices * text *."""
    from .utils import barcodes as bc
    if any(c == "*" or c not in bc.CODE39_CHARS for c in text):
        raise ValueError("not a Code 39 text: %r" % text)
    return [bc.C39_STAR] + [bc.CODE39_CHARS.index(c) for c in text] + [bc.C39_STAR]


def barcode_modules(symbols, kind: str) -> List[int]:
    """Symbol values -> the element widths in modules, bar first, bars and spaces alternating."""
    from .utils import barcodes as bc
    el: List[int] = []
    if kind == "Code128":
        for v in symbols:
            el += [int(c) for c in (bc.CODE128_STOP if v == bc.C128_STOP else bc.CODE128_PATTERNS[v])]
    elif kind == "Code39":
        for k, v in enumerate(symbols):
            el += ([1] if k else []) + [int(c) for c in bc.CODE39_PATTERNS[v]]
    else:
        raise ValueError(kind)
    return el


def barcode_length(symbols, kind: str, module_px: int) -> int:
    return module_px * sum(barcode_modules(symbols, kind))


def render_barcode(page: np.ndarray, x: int, y: int, symbols, kind: str, module_px: int, height: int, reversed: bool = False,
                   vertical: bool = False, ink: int = 0) -> Tuple[int, int, int, int]:
    """Draw exact module-wide bars into page (uint8 [H,W,3], in place) from (x, y): along x and `height` rows tall, or with vertical
    along y and `height` columns wide; reversed draws the elements from the far end (a strip printed upside down).
    -> the box (x0, y0, x1, y1), inclusive."""
    return render_elements(page, x, y, [module_px * m for m in barcode_modules(symbols, kind)], height, reversed, vertical, ink)


def render_elements(page: np.ndarray, x: int, y: int, el_px, height: int, reversed: bool = False, vertical: bool = False,
                    ink: int = 0) -> Tuple[int, int, int, int]:
    """render_barcode for element widths in pixels (bar first)."""
    el = list(el_px)[::-1] if reversed else list(el_px)
    length = sum(el)
    if x < 0 or y < 0 or (y + length > page.shape[0] or x + height > page.shape[1] if vertical else x + length > page.shape[1] or y + height > page.shape[0]):
        raise ValueError("the barcode does not fit the page")
    pos = 0
    for i, m in enumerate(el):
        if i % 2 == 0:
            a, b = pos, pos + m
            if vertical:
                page[y + a:y + b, x:x + height] = ink
            else:
                page[y:y + height, x + a:x + b] = ink
        pos += m
    return (x, y, x + height - 1, y + length - 1) if vertical else (x, y, x + length - 1, y + height - 1)


# ---- EAN-13 / UPC-A, EAN-8, UPC-E and ITF: encoders from digit strings, written from the tables of utils/barcodes.py ----
def check_digit(body: str) -> int:
    """The GS1 mod-10 check digit of a digit string without it: from the right the weights are 3, 1, 3 ..."""
    return -sum(int(c) * (1 if i % 2 else 3) for i, c in enumerate(body[::-1])) % 10


def linear_elements(kind: str, digits: str, module_px: int = 2, ratio: float = 2.0) -> List[int]:
    """The digits of an "EAN13" (13; a UPC-A is 0 + its 12), "EAN8" (8), "UPCE" (8: number system, six digits, check) or "ITF" (an even
    count) -> the element widths in pixels, bar first, as they are printed; no digit is checked.  ITF's wide elements are
    round(ratio * module_px) pixels."""
    from .utils import barcodes as bc
    d = [int(c) for c in digits]
    el: List[int] = []
    if kind == "ITF":
        if len(d) % 2:
            raise ValueError("ITF takes an even number of digits")
        wide = int(ratio * module_px + 0.5)
        px = lambda v: [wide if c == "w" else module_px for c in bc.ITF_PATTERNS[v]]
        el += [module_px] * 4
        for a, b in zip(d[0::2], d[1::2]):
            el += [w for pair in zip(px(a), px(b)) for w in pair]
        return el + [wide, module_px, module_px]
    sets = {"L": bc.EAN_L, "G": bc.EAN_G, "R": bc.EAN_R, "O": bc.EAN_L, "E": bc.EAN_G}
    if kind == "EAN13" and len(d) == 13:
        left, right, parity, end = d[1:7], d[7:], bc.EAN13_PARITY[d[0]], 3
    elif kind == "EAN8" and len(d) == 8:
        left, right, parity, end = d[:4], d[4:], "LLLL", 3
    elif kind == "UPCE" and len(d) == 8 and d[0] in (0, 1):
        left, right, parity, end = d[1:7], [], bc.UPCE_PARITY[10 * d[0] + d[7]], 6
    else:
        raise ValueError("%s of %d digits" % (kind, len(d)))
    el += [1, 1, 1]
    for v, s in zip(left, parity):
        el += [int(c) for c in sets[s][v]]
    if right:
        el += [1] * 5
        for v in right:
            el += [int(c) for c in bc.EAN_R[v]]
    el += [1] * end
    return [module_px * m for m in el]


def render_linear(page: np.ndarray, x: int, y: int, kind: str, digits: str, module_px: int = 2, height: int = 24, ratio: float = 2.0,
                  reversed: bool = False, vertical: bool = False, ink: int = 0) -> Tuple[int, int, int, int]:
    """render_barcode for the digit-only kinds of linear_elements; the quiet zones are the caller's (what lies round (x, y))."""
    return render_elements(page, x, y, linear_elements(kind, digits, module_px, ratio), height, reversed, vertical, ink)


def synth_barcode_page(seed: int, h: int = 700, w: int = 1000, n_codes: int = 3, text_lines: int = 6, module_px: int = 0,
                       allow_vertical: bool = True) -> Tuple[np.ndarray, List[dict]]:
    """White page with text lines in its upper part and n_codes barcodes below them, each in a cell of its own with a clear margin:
    seeded kinds, texts, module widths (2-4 px unless given), heights, reversed and vertical ones.
    -> (uint8 [h,w,3], [dict(kind, text, symbols, box, reversed, vertical)])"""
    rng = np.random.default_rng(seed)
    top = h // 3 if text_lines else 0
    page = np.full((h, w, 3), 255, np.uint8)
    if text_lines:
        page[:top] = synth_page(top, w, seed + 1000, n_lines=text_lines, noise=0.0)[0]
    gt = []
    cell_w = w // max(n_codes, 1)
    for i in range(n_codes):
        mp = module_px or int(rng.integers(2, 5))
        kind = "Code39" if rng.integers(0, 3) == 0 else "Code128"
        vertical = bool(allow_vertical and rng.integers(0, 4) == 0)
        along = (h - top - 40) if vertical else cell_w - 20 - 12 * mp
        for n_chars in range(12, 0, -1):
            if kind == "Code39":
                text = "".join("ABCDEFGHIJKLMNOPQRSTUVWXYZ0123456789-. $/+%"[int(k)] for k in rng.integers(0, 43, n_chars))
                syms = code39_symbols(text)
            else:
                text = "".join(chr(int(k)) for k in rng.integers(32, 127, n_chars)) if rng.integers(0, 2) else "".join(
                    "0123456789"[int(k)] for k in rng.integers(0, 10, 2 * n_chars))
                syms = code128_symbols(text)
            if barcode_length(syms, kind, mp) <= along:
                break
        else:
            continue
        rev = bool(rng.integers(0, 4) == 0)
        height = min(int(rng.integers(24, 60)), cell_w - 40 if vertical else h - top - 40)
        x = i * cell_w + 10 + 6 * mp
        y = top + 10 + int(rng.integers(0, 20))
        box = render_barcode(page, x, y, syms, kind, mp, height, reversed=rev, vertical=vertical)
        gt.append(dict(kind=kind, text=text, symbols=syms, box=box, reversed=rev, vertical=vertical))
    return page, gt


def synth_barcode_decoys(h: int = 420, w: int = 900, min_rows: int = 8) -> Tuple[np.ndarray, List[dict]]:
    """White page of what looks like a barcode and is none: an evenly ruled grid of 24 vertical rules, a comb, a paragraph of |l1I
    text, a Code 128 with one bar widened by a module (the checksum breaks), a good code of fewer than min_rows rows, and a good code
    whose left quiet zone is filled with ink.  -> (uint8 [h,w,3], [dict(kind, box)])"""
    page = np.full((h, w, 3), 255, np.uint8)
    gt = []
    for k in range(24):                                           # ruled grid
        page[20:100, 20 + 9 * k:22 + 9 * k] = 0
    gt.append(dict(kind="grid", box=(20, 20, 20 + 9 * 23 + 1, 99)))
    page[20:26, 300:500] = 0                                      # comb: a spine with teeth
    for k in range(34):
        page[26:90, 300 + 6 * k:303 + 6 * k] = 0
    gt.append(dict(kind="comb", box=(300, 20, 499, 89)))
    img = Image.fromarray(page)
    d = ImageDraw.Draw(img)
    for r, line in enumerate(("|l1I|Il1|lI1|1lI|l1I|Il1|lI1", "Il1|lI1|1lI|l1I|Il1|lI1|1lI|", "1lI|l1I|Il1|lI1|1lI|l1I|Il1")):
        d.text((540, 20 + 30 * r), line, fill=(0, 0, 0), font=_font(26))
    page = np.array(img)
    gt.append(dict(kind="text", box=(540, 20, w - 1, 110)))
    syms = code128_symbols("DECOY-128")
    el = barcode_modules(syms, "Code128")
    el[8] += 1                                                    # one bar of the second symbol, a module wider
    x = 30
    for i, m in enumerate(el):
        if i % 2 == 0:
            page[150:200, x:x + 2 * m] = 0
        x += 2 * m
    gt.append(dict(kind="bad_check", box=(30, 150, x - 1, 199)))
    box = render_barcode(page, 400, 150, code128_symbols("SHORT"), "Code128", 2, min_rows - 1)
    gt.append(dict(kind="short", box=box))
    box = render_barcode(page, 60, 260, code128_symbols("NOQUIET"), "Code128", 2, 50)
    page[260:310, 20:58] = 0                                      # ink up to two pixels before the start
    gt.append(dict(kind="no_quiet", box=box))
    box = render_barcode(page, 460, 260, code39_symbols("NOQUIET"), "Code39", 2, 50)
    page[260:310, 420:458] = 0
    gt.append(dict(kind="no_quiet39", box=box))
    return page, gt


# ---- QR codes (versions 1-40; the tables are utils/qrcodes.py's, everything else is the encoder's own) ----
def qr_segment_bits(data, version: int) -> List[int]:
    """One segment a call: str of digits -> numeric, str of the 45 alphanumeric characters -> alphanumeric, other str (as UTF-8) or
    bytes -> byte; a list of those -> the segments in turn; a tuple ("bits", value, width) puts raw bits (mode indicators the host
    does not read, ECI headers).  -> the bit list without terminator or padding."""
    from .utils import qrcodes as qr
    if isinstance(data, list):
        return [b for part in data for b in qr_segment_bits(part, version)]
    put = lambda v, k: [(v >> (k - 1 - i)) & 1 for i in range(k)]
    if isinstance(data, tuple):
        return put(int(data[1]), int(data[2]))
    if isinstance(data, str) and data and all(c in "0123456789" for c in data):
        bits = put(qr.MODE_NUMERIC, 4) + put(len(data), qr.count_bits(qr.MODE_NUMERIC, version))
        for k in range(0, len(data), 3):
            g = data[k:k + 3]
            bits += put(int(g), (0, 4, 7, 10)[len(g)])
        return bits
    if isinstance(data, str) and data and all(c in qr.ALNUM for c in data):
        bits = put(qr.MODE_ALNUM, 4) + put(len(data), qr.count_bits(qr.MODE_ALNUM, version))
        for k in range(0, len(data) - 1, 2):
            bits += put(45 * qr.ALNUM.index(data[k]) + qr.ALNUM.index(data[k + 1]), 11)
        if len(data) % 2:
            bits += put(qr.ALNUM.index(data[-1]), 6)
        return bits
    raw = data.encode("utf-8") if isinstance(data, str) else bytes(data)
    bits = put(qr.MODE_BYTE, 4) + put(len(raw), qr.count_bits(qr.MODE_BYTE, version))
    for v in raw:
        bits += put(v, 8)
    return bits


def qr_data_codewords(data, version: int, level: int) -> List[int]:
    """Segments -> the data codewords of (version, level index 0..3 = L, M, Q, H): terminator (up to four zero bits), zero bits to
    the byte boundary, then 236 / 17 alternately."""
    from .utils import qrcodes as qr
    bits, cap = qr_segment_bits(data, version), 8 * qr.data_codewords(version, level)
    if len(bits) > cap:
        raise ValueError("%d bits do not fit version %d-%s (%d)" % (len(bits), version, qr.LEVELS[level], cap))
    bits += [0] * min(4, cap - len(bits))
    bits += [0] * (-len(bits) % 8)
    cw = [int("".join(map(str, bits[i:i + 8])), 2) for i in range(0, len(bits), 8)]
    pad = (236, 17)
    return cw + [pad[i % 2] for i in range(cap // 8 - len(cw))]


def qr_rs_remainder(data: List[int], ec: int) -> List[int]:
    """The ec Reed-Solomon check codewords of a block over GF(256) / 0x11D, generator (x - a^0) ... (x - a^(ec-1))."""
    from .utils import qrcodes as qr
    gen = [1]                                   # descending powers, the leading 1 first
    for i in range(ec):
        gen = [a ^ qr.gf_mul(b, qr.GF_EXP[i]) for a, b in zip(gen + [0], [0] + gen)]
    rem = [0] * ec
    for d in data:
        f = d ^ rem[0]
        rem = rem[1:] + [0]
        for k in range(ec):
            rem[k] ^= qr.gf_mul(gen[k + 1], f)
    return rem


def qr_interleave(cw: List[int], version: int, level: int) -> List[int]:
    """Data codewords -> all codewords of the symbol in placement order: the blocks' data column by column, then their check
    codewords the same way."""
    from .utils import qrcodes as qr
    nb, short, dlen, ec = qr.block_structure(version, level)
    blocks, at = [], 0
    for b in range(nb):
        n = dlen + (b >= short)
        blocks.append(cw[at:at + n])
        at += n
    checks = [qr_rs_remainder(b, ec) for b in blocks]
    out = [b[i] for i in range(dlen + 1) for b in blocks if i < len(b)]
    return out + [c[i] for i in range(ec) for c in checks]


def qr_matrix(codewords: List[int], version: int, level: int, mask: int) -> np.ndarray:
    """All codewords of a symbol -> bool [D,D] (True = dark): function patterns, the codewords in placement order, the mask, the
    format information and, from version 7, the version information."""
    from .utils import qrcodes as qr
    d = qr.dimension(version)
    m = np.zeros((d, d), bool)
    for (r, c), dark in qr.function_modules(version).items():
        m[r, c] = dark
    place = qr.placement_of(version)
    for i, (r, c) in enumerate(place):
        bit = (codewords[i >> 3] >> (7 - (i & 7))) & 1 if i < 8 * len(codewords) else 0
        m[r, c] = bool(bit) ^ qr.mask_bit(mask, r, c)
    word = qr.format_word(level, mask)
    for pos in qr.format_positions(version):
        for i, (r, c) in enumerate(pos):
            m[r, c] = bool((word >> i) & 1)
    if version >= 7:
        word = qr.version_word(version)
        for i, (a, b) in enumerate(qr.version_positions(version)):
            m[a] = m[b] = bool((word >> i) & 1)
    return m


def qr_encode(data, version: int, level: int = 1, mask: int = 0) -> np.ndarray:
    """data (see qr_segment_bits) -> the symbol's modules, bool [D,D] indexed [row, col], True = dark.  The mask is the caller's:
    no penalty rule is applied."""
    return qr_matrix(qr_interleave(qr_data_codewords(data, version, level), version, level), version, level, mask)


def draw_qr(page: np.ndarray, x: int, y: int, modules: np.ndarray, module: int, rotation: int = 0, ink: int = 0) -> Tuple[int, int, int, int]:
    """Draw a symbol into page (uint8 [H,W,3], in place) with its top-left pixel at (x, y), `module` pixels a module, turned clockwise by
    rotation quarter turns; only dark modules are drawn.  -> the box (x0, y0, x1, y1), inclusive."""
    m = np.rot90(np.asarray(modules, bool), -int(rotation) % 4)
    side = m.shape[0] * module
    if x < 0 or y < 0 or x + side > page.shape[1] or y + side > page.shape[0]:
        raise ValueError("the symbol does not fit the page")
    big = np.kron(m, np.ones((module, module), bool))
    page[y:y + side, x:x + side][big] = ink
    return x, y, x + side - 1, y + side - 1


def qr_finder(page: np.ndarray, x: int, y: int, module: int, ink: int = 0) -> None:
    """A lone finder pattern (7 x 7 modules) at (x, y)."""
    f = np.array([[max(abs(r - 3), abs(c - 3)) != 2 for c in range(7)] for r in range(7)])
    draw_qr(page, x, y, f, module, ink=ink)


def synth_qr_page(seed: int, h: int = 700, w: int = 1000, n_codes: int = 3, text_lines: int = 6, module_px: int = 0) -> Tuple[np.ndarray, List[dict]]:
    """White page with text lines in its upper part and n_codes QR symbols below them, each in a cell of its own: seeded versions,
    levels, masks, rotations, module sizes (3-6 px unless given) and contents (digits, alphanumeric or UTF-8 text).
    -> (uint8 [h,w,3], [dict(text, version, level, mask, rotation, module, box)])"""
    from .utils import qrcodes as qr
    rng = np.random.default_rng(seed)
    top = h // 3 if text_lines else 0
    page = np.full((h, w, 3), 255, np.uint8)
    if text_lines:
        page[:top] = synth_page(top, w, seed + 2000, n_lines=text_lines, noise=0.0)[0]
    gt = []
    cell_w = w // max(n_codes, 1)
    for i in range(n_codes):
        mp = module_px or int(rng.integers(3, 7))
        room = min(cell_w, h - top) - 8 * mp - 24
        vmax = min(qr.MAX_VERSION, (room // mp - 17) // 4)
        if vmax < 1:
            continue
        version, level, mask, rot = int(rng.integers(1, vmax + 1)), int(rng.integers(0, 4)), int(rng.integers(0, 8)), int(rng.integers(0, 4))
        cap = qr.data_codewords(version, level) - 3
        kind = int(rng.integers(0, 3))
        if kind == 0:
            text = "".join("0123456789"[int(k)] for k in rng.integers(0, 10, max(1, min(2 * cap, 40))))
        elif kind == 1:
            text = "".join(qr.ALNUM[int(k)] for k in rng.integers(0, 45, max(1, min(cap, 30))))
        else:
            text = ("https://lumina.example/p?id=%d&k=éü" % int(rng.integers(0, 10 ** 6)))[:max(1, cap - 4)]
        x = i * cell_w + 12 + 4 * mp
        y = top + 12 + 4 * mp + int(rng.integers(0, 8))
        box = draw_qr(page, x, y, qr_encode(text, version, level, mask), mp, rot)
        gt.append(dict(text=text, version=version, level=level, mask=mask, rotation=rot, module=mp, box=box))
    return page, gt


def synth_qr_large_page(seed: int, h: int = 1100, w: int = 800, versions=(11, 40), module_px: int = 0, text_lines: int = 6) -> Tuple[np.ndarray, List[dict]]:
    """White page with text lines in its upper part and one large QR symbol below them: a seeded version of `versions` (inclusive, as
    far as the page has room), level, mask, rotation, module size (3-4 px unless given) and a byte-mode content that fills it.  A
    page maker of its own: synth_qr_page's draws are not touched.  -> (uint8 [h,w,3], [dict(text, version, level, mask, rotation,
    module, box)])"""
    from .utils import qrcodes as qr
    rng = np.random.default_rng(seed)
    top = h // 4 if text_lines else 0
    page = np.full((h, w, 3), 255, np.uint8)
    if text_lines:
        page[:top] = synth_page(top, w, seed + 3000, n_lines=text_lines, noise=0.0)[0]
    mp = module_px or int(rng.integers(3, 5))
    room = min(w, h - top) - 8 * mp - 24
    vmax = min(int(versions[1]), (room // mp - 17) // 4)
    if vmax < int(versions[0]):
        return page, []
    version, level, mask, rot = int(rng.integers(int(versions[0]), vmax + 1)), int(rng.integers(0, 4)), int(rng.integers(0, 8)), int(rng.integers(0, 4))
    n = qr.data_codewords(version, level) - 4
    body = "https://lumina.example/e-invoice/%d?jwt=" % int(rng.integers(0, 10 ** 6))
    text = (body + "".join(ALPHABET[int(k)] for k in rng.integers(0, 62, n)))[:n]
    x, y = 12 + 4 * mp + int(rng.integers(0, 8)), top + 12 + 4 * mp + int(rng.integers(0, 8))
    box = draw_qr(page, x, y, qr_encode(text, version, level, mask), mp, rot)
    return page, [dict(text=text, version=version, level=level, mask=mask, rotation=rot, module=mp, box=box)]


def synth_qr_decoys(h: int = 330, w: int = 520) -> Tuple[np.ndarray, List[dict]]:
    """White page of what looks like a QR symbol and is none: lone finder patterns, three finders at a symbol's corners with white
    between them, a mirrored symbol, an inverted one (light on dark) and a halftone block.  -> (uint8 [h,w,3], [dict(kind, box)])"""
    page = np.full((h, w, 3), 255, np.uint8)
    gt = []
    for k, (x, y, m) in enumerate(((10, 10, 3), (60, 14, 4), (20, 60, 5))):           # lone finders of three sizes
        qr_finder(page, x, y, m)
        gt.append(dict(kind="finder", box=(x, y, x + 7 * m - 1, y + 7 * m - 1)))
    x, y, m, d = 130, 10, 4, 25                                                       # a version 2 symbol's three finders, nothing else
    for fx, fy in ((0, 0), (d - 7, 0), (0, d - 7)):
        qr_finder(page, x + fx * m, y + fy * m, m)
    gt.append(dict(kind="three_finders", box=(x, y, x + d * m - 1, y + d * m - 1)))
    sym = qr_encode("MIRRORED 123", 2, 1, 3)
    gt.append(dict(kind="mirrored", box=draw_qr(page, 260, 10, sym[:, ::-1], 4)))
    sym = qr_encode("INVERTED", 1, 0, 2)
    page[140:140 + 29 * 4, 20:20 + 29 * 4] = 0                                        # dark field, the symbol light on it
    draw_qr(page, 20 + 4 * 4, 140 + 4 * 4, sym, 4, ink=255)
    gt.append(dict(kind="inverted", box=(20, 140, 20 + 29 * 4 - 1, 140 + 29 * 4 - 1)))
    yy, xx = np.mgrid[0:120, 0:160]
    page[150:270, 200:360][((xx % 6 < 3) & (yy % 6 < 3)) | ((xx % 6 >= 3) & (yy % 6 >= 3) & ((xx // 6 + yy // 6) % 3 == 0))] = 0   # halftone block
    gt.append(dict(kind="halftone", box=(200, 150, 359, 269)))
    return page, gt


def synth_qr_crowded_page() -> Tuple[np.ndarray, dict]:
    """A 6-M symbol turned by 90 degrees (its corner finder is the top right one) and, to its right at the distance of its own finder
    spacing, a second symbol of the same module size: the corner's nearest valid partner pair takes the neighbour's finder for its +x
    partner and does not decode.  -> (uint8 [150,331,3], {box: text})"""
    page = np.full((150, 331, 3), 255, np.uint8)
    a = draw_qr(page, 10, 12, qr_encode("CROWDED CORNER 6-M", 6, 1, 4), 3, 1)
    b = draw_qr(page, 211, 12, qr_encode("NEIGHBOUR", 2, 1, 0), 3)
    return page, {a: "CROWDED CORNER 6-M", b: "NEIGHBOUR"}


# ---- Data Matrix (ECC 200; the tables are utils/datamatrix.py's, everything else is the encoder's own) ----
DM_SCHEMES = ("ascii", "c40", "text", "x12", "edifact", "base256")


def _dm_ascii(raw: bytes) -> List[int]:
    out, i = [], 0
    while i < len(raw):
        if i + 1 < len(raw) and 48 <= raw[i] <= 57 and 48 <= raw[i + 1] <= 57:
            out.append(130 + 10 * (raw[i] - 48) + raw[i + 1] - 48)
            i += 2
            continue
        out += [raw[i] + 1] if raw[i] < 128 else [235, raw[i] - 127]
        i += 1
    return out


def _dm_c40_values(ch: int, scheme: str) -> List[int]:
    """One byte -> its C40 / Text / X12 values (shifts included)."""
    from .utils import datamatrix as dm
    if scheme == "x12":
        return [dm.X12_SET.index(chr(ch))]                 # (ValueError: not an X12 character)
    if ch >= 128:
        return [1, 30] + _dm_c40_values(ch - 128, scheme)
    basic, c = (dm.C40_BASIC if scheme == "c40" else dm.TEXT_BASIC), chr(ch)
    if c in basic:
        return [3 + basic.index(c)]
    if ch < 32:
        return [0, ch]
    if c in dm.SHIFT2:
        return [1, dm.SHIFT2.index(c)]
    return [2, ch - 96] if scheme == "c40" else [2, dm.TEXT_SHIFT3.index(c)]


def dm_data_codewords(data, size: int, scheme: str = "ascii") -> List[int]:
    """data -> the data codewords of SIZES[size], padded (129, then its 253-state randomisation).  str (as UTF-8) or bytes are
    encoded in the one scheme named (DM_SCHEMES; the characters the scheme lacks are a ValueError, except that C40 and Text shift);
    a list of ints is taken as codewords as they are; a list of such parts is encoded part by part, ("scheme", part) tuples
    choosing the part's scheme.  C40 / Text / X12 end as the standard says: values that do not fill a triple go to ASCII behind an
    unlatch, the unlatch is left out when the data ends with the symbol, and one last character in one last codeword is ASCII without
    an unlatch.  EDIFACT unlatches unless its triples end with the symbol; Base 256 writes its length, or 0 ("to the end of the
    symbol") when the field fills the symbol."""
    from .utils import datamatrix as dm
    cap = dm.ALL_SIZES[size][2]
    if scheme not in DM_SCHEMES:
        raise ValueError("scheme must be one of %s" % (DM_SCHEMES,))

    def part(p, sch: str, cw: List[int]) -> None:
        if isinstance(p, tuple):
            return part(p[1], p[0], cw)
        if isinstance(p, list):
            if all(isinstance(v, int) for v in p):
                cw += p
            else:
                for q in p:
                    part(q, sch, cw)
            return
        raw = p.encode("utf-8") if isinstance(p, str) else bytes(p)
        if sch == "ascii":
            cw += _dm_ascii(raw)
        elif sch in ("c40", "text", "x12"):
            groups, k = [_dm_c40_values(b, sch) for b in raw], 0
            vals: List[int] = []
            done = 0                                       # bytes whose values lie in whole triples
            for i, g in enumerate(groups):
                vals += g
                if len(vals) % 3 == 0:
                    done, k = i + 1, len(vals)
            cw.append({"c40": dm.LATCH_C40, "text": dm.LATCH_TEXT, "x12": dm.LATCH_X12}[sch])
            for i in range(0, k, 3):
                v = 1600 * vals[i] + 40 * vals[i + 1] + vals[i + 2] + 1
                cw += [v >> 8, v & 255]
            rest = _dm_ascii(raw[done:])
            if rest and not (len(cw) + 1 == cap and len(rest) == 1):
                cw.append(dm.UNLATCH)
            elif not rest and len(cw) < cap:
                cw.append(dm.UNLATCH)
            cw += rest
        elif sch == "edifact":
            if any(not 32 <= b <= 94 for b in raw):
                raise ValueError("not an EDIFACT character")
            cw.append(dm.LATCH_EDIFACT)
            vals = [b & 63 for b in raw]
            if not (len(vals) % 4 == 0 and len(cw) + 3 * len(vals) // 4 == cap):
                vals.append(0x1F)
            bits = "".join("{:06b}".format(v) for v in vals)
            bits += "0" * (-len(bits) % 8)
            cw += [int(bits[i:i + 8], 2) for i in range(0, len(bits), 8)]
        else:
            cw.append(dm.LATCH_BASE256)
            fills = len(cw) + 1 + len(raw) == cap
            field = [0] if fills else ([len(raw)] if len(raw) < 250 else [249 + len(raw) // 250, len(raw) % 250])
            for v in field + list(raw):
                r = v + (149 * (len(cw) + 1)) % 255 + 1
                cw.append(r if r <= 255 else r - 256)

    cw: List[int] = []
    part(data, scheme, cw)
    if len(cw) > cap:
        raise ValueError("%d codewords do not fit %d x %d (%d)" % (len(cw), dm.ALL_SIZES[size][0], dm.ALL_SIZES[size][1], cap))
    if len(cw) < cap:
        cw.append(dm.PAD)
    while len(cw) < cap:
        cw.append(dm.randomised_pad(len(cw) + 1))
    return cw


def dm_rs_remainder(data: List[int], ec: int) -> List[int]:
    """The ec Reed-Solomon check codewords of a block over GF(256) / 0x12D, generator (x - a^1) ... (x - a^ec)."""
    from .utils import datamatrix as dm
    gen = dm.rs_generator(ec)
    rem = [0] * ec
    for d in data:
        f = d ^ rem[0]
        rem = rem[1:] + [0]
        for k in range(ec):
            rem[k] ^= dm.gf_mul(gen[k + 1], f)
    return rem


def dm_interleave(cw: List[int], size: int) -> List[int]:
    """Data codewords -> all codewords of the symbol in placement order: the data, then the blocks' check codewords, dealt by stream
    position: the codeword at position p is block p mod nb's next one (block b takes every nb-th data codeword from b on; behind
    144 x 144's 1558 data codewords the check codewords carry on from block 8)."""
    from .utils import datamatrix as dm
    nd, ne, nb = dm.ALL_SIZES[size][2], dm.ALL_SIZES[size][3], dm.ALL_SIZES[size][6]
    checks = [dm_rs_remainder(cw[b::nb], ne // nb) for b in range(nb)]
    taken = [0] * nb
    out = list(cw)
    for p in range(nd, nd + ne):
        out.append(checks[p % nb][taken[p % nb]])
        taken[p % nb] += 1
    return out


def dm_matrix(codewords: List[int], size: int) -> np.ndarray:
    """All codewords of a symbol -> bool [rows, cols] (True = dark): function modules, the codewords through the placement and the
    fixed 2 x 2 corner."""
    from .utils import datamatrix as dm
    m = np.zeros(dm.ALL_SIZES[size][:2], bool)
    for (r, c), dark in dm.function_modules(size).items():
        m[r, c] = dark
    for i, (r, c) in enumerate(dm.placement_of(size)):
        m[r, c] = bool((codewords[i >> 3] >> (7 - (i & 7))) & 1)
    for (r, c), dark in dm.fixed_modules(size):
        m[r, c] = dark
    return m


def dm_encode(data, size: int, scheme: str = "ascii") -> np.ndarray:
    """data (see dm_data_codewords) -> the symbol's modules, bool [rows, cols] indexed [row, col], True = dark."""
    return dm_matrix(dm_interleave(dm_data_codewords(data, size, scheme), size), size)


def dm_smallest_size(data, scheme: str = "ascii", square: bool = True, large: bool = False) -> int:
    """The first square (or any) size of the table that holds data; large=True: of ALL_SIZES, up to 144 x 144."""
    from .utils import datamatrix as dm
    for s in sorted(range(dm.NUM_SIZES_ALL if large else dm.NUM_SIZES), key=lambda s: dm.ALL_SIZES[s][2]):
        if square and dm.ALL_SIZES[s][0] != dm.ALL_SIZES[s][1]:
            continue
        try:
            dm_data_codewords(data, s, scheme)
            return s
        except ValueError as e:
            if "do not fit" not in str(e):
                raise
    raise ValueError("the data fits no size")


def draw_dm(page: np.ndarray, x: int, y: int, modules: np.ndarray, module: int, rotation: int = 0, ink: int = 0) -> Tuple[int, int, int, int]:
    """draw_qr for a matrix that need not be square: top-left pixel at (x, y), `module` pixels a module, turned clockwise by rotation
    quarter turns; only dark modules are drawn.  -> the box (x0, y0, x1, y1), inclusive."""
    m = np.rot90(np.asarray(modules, bool), -int(rotation) % 4)
    hh, ww = m.shape[0] * module, m.shape[1] * module
    if x < 0 or y < 0 or x + ww > page.shape[1] or y + hh > page.shape[0]:
        raise ValueError("the symbol does not fit the page")
    page[y:y + hh, x:x + ww][np.kron(m, np.ones((module, module), bool))] = ink
    return x, y, x + ww - 1, y + hh - 1


def synth_dm_page(seed: int, h: int = 700, w: int = 1000, n_codes: int = 3, text_lines: int = 6, module_px: int = 0) -> Tuple[np.ndarray, List[dict]]:
    """White page with text lines in its upper part and n_codes Data Matrix symbols below them, each in a cell of its own: seeded
    sizes, schemes, rotations, module sizes (3-6 px unless given) and contents.
    -> (uint8 [h,w,3], [dict(text, size, rows, cols, scheme, rotation, module, box)])"""
    from .utils import datamatrix as dm
    rng = np.random.default_rng(seed)
    top = h // 3 if text_lines else 0
    page = np.full((h, w, 3), 255, np.uint8)
    if text_lines:
        page[:top] = synth_page(top, w, seed + 3000, n_lines=text_lines, noise=0.0)[0]
    gt = []
    cell_w = w // max(n_codes, 1)
    for i in range(n_codes):
        mp = module_px or int(rng.integers(3, 7))
        room = min(cell_w, h - top) - 4 * mp - 24
        fits = [s for s in range(dm.NUM_SIZES) if max(dm.SIZES[s][:2]) * mp <= room]
        if not fits:
            continue
        size, rot = fits[int(rng.integers(0, len(fits)))], int(rng.integers(0, 4))
        cap = dm.SIZES[size][2]
        scheme = DM_SCHEMES[int(rng.integers(0, len(DM_SCHEMES)))]
        if scheme == "ascii":
            text = ("LOT%d/" % int(rng.integers(0, 10 ** 4)) + "".join("0123456789"[int(k)] for k in rng.integers(0, 10, 2 * cap)))[:max(1, cap - 1)]
        elif scheme == "base256":
            text = ("réf %d: " % int(rng.integers(0, 100)) + "données " * 30)[:max(1, (cap - 2) // 2)]
        elif scheme == "text":
            text = ("part no %d rev b, " % int(rng.integers(0, 10 ** 5)) * 12)[:max(1, cap - 3)]
        else:                                              # c40, x12, edifact: capitals, digits and two separators each set has
            sep = {"c40": (" ", ">"), "x12": ("*", ">"), "edifact": (" ", "-")}[scheme]
            text = ("INV %d%sPART%s" % (int(rng.integers(0, 10 ** 5)), sep[0], sep[1]) * 12)[:max(1, cap - 3)]
        x = i * cell_w + 12 + 2 * mp
        y = top + 12 + 2 * mp + int(rng.integers(0, 8))
        box = draw_dm(page, x, y, dm_encode(text, size, scheme), mp, rot)
        gt.append(dict(text=text, size=size, rows=dm.SIZES[size][0], cols=dm.SIZES[size][1], scheme=scheme, rotation=rot, module=mp, box=box))
    return page, gt


def synth_dm_decoys(h: int = 243, w: int = 420) -> Tuple[np.ndarray, List[dict]]:
    """White page of what looks like a Data Matrix symbol and is none: a ruled table frame, a large letter L, a QR symbol, a solid
    square, a checkbox, an L whose arm has a gap, a mirrored symbol and an inverted one.  -> (uint8 [h,w,3], [dict(kind, box)])"""
    page = np.full((h, w, 3), 255, np.uint8)
    gt = []
    x0, y0, x1, y1 = 8, 8, 127, 79                                                    # a 3 x 2 table frame, 2 px rules
    for yy in (y0, (y0 + y1) // 2, y1 - 1):
        page[yy:yy + 2, x0:x1 + 1] = 0
    for xx in (x0, x0 + 40, x0 + 80, x1 - 1):
        page[y0:y1 + 1, xx:xx + 2] = 0
    gt.append(dict(kind="table", box=(x0, y0, x1, y1)))
    page[10:70, 140:146] = 0                                                          # a letter L: no clock tracks
    page[64:70, 140:190] = 0
    gt.append(dict(kind="letter_l", box=(140, 10, 189, 69)))
    gt.append(dict(kind="qr", box=draw_qr(page, 200, 8, qr_encode("NOT A DATA MATRIX", 2, 1, 2), 3)))
    page[10:50, 290:330] = 0
    gt.append(dict(kind="solid", box=(290, 10, 329, 49)))
    page[10:46, 340:376] = 0
    page[13:43, 343:373] = 255
    gt.append(dict(kind="checkbox", box=(340, 10, 375, 45)))
    sym = dm_encode("GAP IN THE ARM", 4)
    sym[6:9, 0] = False                                                               # three modules of the upright are missing
    gt.append(dict(kind="gap", box=draw_dm(page, 10, 100, sym, 4)))
    sym = dm_encode("MIRRORED 123", 3)
    gt.append(dict(kind="mirrored", box=draw_dm(page, 110, 100, sym[:, ::-1], 4)))
    sym = dm_encode("INVERTED", 2)
    page[100:100 + 18 * 4, 200:200 + 18 * 4] = 0                                      # dark field, the symbol light on it
    draw_dm(page, 208, 108, sym, 4, ink=255)
    gt.append(dict(kind="inverted", box=(200, 100, 271, 171)))
    return page, gt
