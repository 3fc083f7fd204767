"""Restatement (test infrastructure, plain Python) of the barcode pass that lumina_ocr_barcodes runs on the device, row by row.

A row of the ink mask is a list of runs; its ELEMENTS are the run widths (bars) and the gaps between them (spaces), alternating.  Read
from bar t in a direction (+1 to the right, -1 to the left: a strip printed upside down), symbol k of a Code 128 is elements
6 k .. 6 k + 5, of a Code 39 elements 10 k .. 10 k + 8 with element 10 k + 9 the gap between characters.  A symbol of pixel width S is
matched against every pattern p of its table by d = sum |w_i M - p_i S| (M = 11 or 15 modules); the lowest d wins, ties go to the
lowest value, and d > max_dist S M / 256 rejects it.

Code 128 reads at t when symbol 0 is a start (103-105), the first stop (106: its first six elements, then a bar of 1.5 .. 2.5
modules) is symbol kstop >= 2, every symbol between is a value <= 102, and the mod-103 checksum holds.  Code 39 reads when symbol 0
is `*`, the first later `*` is symbol kstop >= 1, every symbol before it matched and the gap after it is at most two modules.  At
most 64 symbols.  The gap before bar t is at least quiet module widths of symbol 0 (gap M >= quiet S; the page edge is quiet).
Code 128 is tried first.

A row's reads: going right, bar by bar, a read claims its bars and the scan goes on behind them; the same going left.  A read going
left that shares a bar with one going right is dropped; of what remains the four leftmost are the row's.  The transposed mask gives
the vertical reads.  Reads of one direction join when kind, reversal and symbols are equal, their ranges along the code overlap and
their rows are at most row_gap apart; a group of at least min_rows reads is a barcode, its box the hull."""
from __future__ import annotations

from typing import List, Tuple

import numpy as np

from lumina_ocr import arch
from lumina_ocr.utils import barcodes as bc

from table_reference import ink_mask, pack_mask

P = arch.BARCODE_PARAMS
MAX_SYMS = bc.MAX_SYMS
ROW_READS = 4

_T128 = [[int(c) for c in p] for p in bc.CODE128_MATCH]
_T39 = [[int(c) for c in p] for p in bc.CODE39_PATTERNS]


def row_runs(row: np.ndarray) -> List[Tuple[int, int]]:
    out, x, n = [], 0, len(row)
    while x < n:
        if row[x]:
            s = x
            while x + 1 < n and row[x + 1]:
                x += 1
            out.append((s, x))
        x += 1
    return out


def element(runs, t: int, d: int, m: int):
    """Element m read from bar t in direction d, or None when it is not on the row."""
    j = t + d * (m // 2)
    if not 0 <= j < len(runs):
        return None
    if m % 2 == 0:
        return runs[j][1] - runs[j][0] + 1
    j2 = j + d
    if not 0 <= j2 < len(runs):
        return None
    lo = min(j, j2)
    return runs[lo + 1][0] - runs[lo][1] - 1


def match(w: List[int], table, modules: int, max_dist: int):
    """-> (value, S) of the best pattern, value None when rejected."""
    s = sum(w)
    best, bd = None, None
    for v, p in enumerate(table):
        d = sum(abs(wi * modules - pi * s) for wi, pi in zip(w, p))
        if bd is None or d < bd:
            best, bd = v, d
    return (best if bd <= max_dist * s * modules // 256 else None), s


def quiet_ok(runs, t: int, d: int, s0: int, modules: int, quiet: int) -> bool:
    j = t - d
    if not 0 <= j < len(runs):
        return True
    lo = min(j, t)
    return (runs[lo + 1][0] - runs[lo][1] - 1) * modules >= quiet * s0


def read128(runs, t: int, d: int, quiet: int, max_dist: int):
    """-> (symbols, bars used) or None."""
    vals = []
    for k in range(MAX_SYMS):
        w = [element(runs, t, d, 6 * k + i) for i in range(6)]
        term = element(runs, t, d, 6 * k + 6)      # the bar behind the symbol: the next symbol's first, or the stop's last
        if None in w or term is None:
            return None
        if k == 0 and not quiet_ok(runs, t, d, sum(w), bc.C128_MODULES, quiet):     # (first: it is the cheap test)
            return None
        v, s = match(w, _T128, bc.C128_MODULES, max_dist)
        if v is None:
            return None
        if k == 0 and (v < bc.C128_START_A or v > bc.C128_START_C):
            return None
        vals.append(v)
        if v == bc.C128_STOP:
            if k < 2 or not (3 * s <= 2 * term * bc.C128_MODULES <= 5 * s):
                return None
            if (vals[0] + sum(i * x for i, x in enumerate(vals[1:-2], 1))) % 103 != vals[-2]:
                return None
            return vals, 3 * k + 4
        if k > 0 and v > 102:
            return None
    return None


def read39(runs, t: int, d: int, quiet: int, max_dist: int):
    vals = []
    for k in range(MAX_SYMS):
        w = [element(runs, t, d, 10 * k + i) for i in range(9)]
        if None in w:
            return None
        if k == 0 and not quiet_ok(runs, t, d, sum(w), bc.C39_MODULES, quiet):
            return None
        v, s = match(w, _T39, bc.C39_MODULES, max_dist)
        if v is None:
            return None
        if k == 0 and v != bc.C39_STAR:
            return None
        vals.append(v)
        if k > 0 and v == bc.C39_STAR:
            return vals, 5 * k + 5
        gap = element(runs, t, d, 10 * k + 9)
        if gap is None or gap * bc.C39_MODULES > 2 * s:
            return None
    return None


def scan(runs, d: int, quiet: int, max_dist: int):
    """Greedy reads of a row in direction d -> [(first bar, last bar, kind, symbols)] (bars as run indices, first <= last)."""
    n = len(runs)
    out = []
    order = range(n) if d > 0 else range(n - 1, -1, -1)
    free = 0            # in scan order: the first position not yet claimed
    for pos, t in enumerate(order):
        if pos < free:
            continue
        got, kind = read128(runs, t, d, quiet, max_dist), 0
        if got is None:
            got, kind = read39(runs, t, d, quiet, max_dist), 1
        if got is None:
            continue
        vals, bars = got
        free = pos + bars
        last = t + d * (bars - 1)
        out.append((min(t, last), max(t, last), kind, vals))
    return out


def row_reads(row: np.ndarray, quiet: int, max_dist: int):
    """-> up to four (a0, a1, kind, reversed, symbols), by a0."""
    runs = row_runs(row)
    if len(runs) < 10:       # (the shortest code has ten bars)
        return []
    fwd = scan(runs, +1, quiet, max_dist)
    bwd = [r for r in scan(runs, -1, quiet, max_dist) if not any(r[0] <= f[1] and f[0] <= r[1] for f in fwd)]
    reads = [(runs[b0][0], runs[b1][1], kind, rev, tuple(vals)) for rev, lst in ((0, fwd), (1, bwd)) for b0, b1, kind, vals in lst]
    reads.sort(key=lambda r: r[0])
    return reads[:ROW_READS]


def codes_of_ink(ink: np.ndarray, quiet: int = None, max_dist: int = None, min_rows: int = None, row_gap: int = None):
    """bool [H,W] -> (codes int32 [m,8], syms int32 [m,64])."""
    quiet = P["quiet"] if quiet is None else quiet
    max_dist = P["max_dist"] if max_dist is None else max_dist
    min_rows = P["min_rows"] if min_rows is None else min_rows
    row_gap = P["row_gap"] if row_gap is None else row_gap
    H, W = ink.shape
    found = []
    for vertical, img in ((0, ink), (1, ink.T)):
        per_row = [row_reads(img[r], quiet, max_dist) for r in range(img.shape[0])]
        reads = [(r, s, rd) for r, lst in enumerate(per_row) for s, rd in enumerate(lst)]
        root = list(range(len(reads)))

        def find(i):
            while root[i] != i:
                i = root[i]
            return i
        for i, (r, s, rd) in enumerate(reads):
            for j in range(i - 1, -1, -1):
                r2, _, rd2 = reads[j]
                if r - r2 > row_gap:
                    break
                if r2 < r and rd[2:] == rd2[2:] and rd[0] <= rd2[1] and rd2[0] <= rd[1]:
                    a, b = find(i), find(j)
                    if a != b:
                        root[max(a, b)] = min(a, b)
        groups = {}
        for i in range(len(reads)):
            groups.setdefault(find(i), []).append(i)
        for g, members in groups.items():
            if len(members) < min_rows:
                continue
            r0, s0, rd = reads[g]
            a0 = min(reads[i][2][0] for i in members)
            a1 = max(reads[i][2][1] for i in members)
            p0 = min(reads[i][0] for i in members)
            p1 = max(reads[i][0] for i in members)
            box = (p0, a0, p1, a1) if vertical else (a0, p0, a1, p1)
            ident = (4 * H if vertical else 0) + 4 * r0 + s0
            found.append((box[1], box[0], box[3], box[2], ident, rd[2], len(rd[4]), len(members), rd[3] | (vertical << 1), rd[4]))
    found.sort(key=lambda t: t[:5])
    codes = np.array([(t[1], t[0], t[3], t[2], t[5], t[6], t[7], t[8]) for t in found], np.int32).reshape(-1, 8)
    syms = np.zeros((len(found), MAX_SYMS), np.int32)
    for i, t in enumerate(found):
        syms[i, :len(t[9])] = t[9]
    return codes, syms


def barcodes(page: np.ndarray, threshold: int = None, **kw):
    """uint8 [H,W,3] -> (mask uint64 [H, ceil(W/64)], codes int32 [m,8], syms int32 [m,64])."""
    ink = ink_mask(page, P["threshold"] if threshold is None else threshold)
    return (pack_mask(ink),) + codes_of_ink(ink, **kw)


def decoded(codes: np.ndarray, syms: np.ndarray) -> List[str]:
    return [bc.symbols_text(int(c[4]), list(s[:int(c[5])])) for c, s in zip(codes, syms)]
