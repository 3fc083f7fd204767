"""Restatement (test infrastructure, plain Python) of the barcode pass with a set of kinds, as lumina_ocr_barcodes_kinds runs it on the
device: tests/barcode_reference.py's row read with EAN-13 / UPC-A, EAN-8, UPC-E and ITF beside Code 128 and Code 39.  Elements, the
match d = sum |w_i M - p_i S| <= max_dist S M / 256 (lowest d, ties to the lowest value), the scan, the claims, the four slots and the
merge are that file's; with kinds = 3 the result is that file's.

`kinds` is a bit mask, bit k = kind k.  At a bar the kinds are tried in the order 0..5 and the first that reads claims its bars.

A GUARD of n elements beside a digit of S pixels (7 modules) holds when it matches n single modules by the measure above (M = n) and
its pixels G are n modules within a quarter: 4 |7 G - n S| <= n S.

EAN-13 (kind 2, 30 bars), EAN-8 (3, 22 bars), UPC-E (4, 17 bars): start guard = elements 0-2, beside digit 0; digit k = the four
elements from 3 + 4 k, behind the centre guard from 8 + 4 k; centre guard = five elements behind the left half, beside the digit
before it; end guard = three elements (UPC-E: six) behind the last digit, beside it.  The gap before the first bar is at least
`quiet` modules of digit 0 (gap 7 >= quiet S), the gap behind the last bar the same of the last digit; the page edge is quiet.  A
left-half digit is matched against sets L and G (values 0..19), a right-half digit against set R (L's widths).  EAN-13: the L / G
pattern of the left half gives the first digit (no row: no read); the 13 digits pass mod 10.  EAN-8: the left half is all L; the 8
digits pass mod 10.  UPC-E: the pattern gives number system and check digit; the UPC-A expansion (barcodes.upce_to_upca) passes mod 10;
the symbols are number system, six digits, check digit.

ITF (kind 5): start = elements 0-3, four single modules by the measure (M = 4), the gap before it at least `quiet` of its modules
(gap 4 >= quiet S).  Pair k = elements 4 + 10 k .. 13 + 10 k, its bars one quintuple and its spaces the next; the three elements behind it
are read with it (a pair without them on the row is no pair).  The RATIO is decided by pair 0's bars: of M = 14, 16, 18 half-modules
(narrow 2, wide 4, 5, 6) the one whose best pattern has the lowest d * (1008 / M), ties to the lower M; the start's S4 pixels are 8
half-modules of that quintuple within a quarter (4 |S4 M - 8 S| <= 8 S).  Every quintuple is matched at that M against the ten digits.
The stop behind pair k is its three elements matched against wide, narrow, narrow (Ms = M / 2 + 1 half-modules: 8, 9, 10), with Ms
half-modules of the pair's bar quintuple within a quarter, and behind it a gap of at least `quiet` modules of the stop (gap Ms >= 2
quiet S3) or the page edge.  The code ends at the first pair k >= 2 (six digits) with a stop behind it; every pair up to it matched;
at most 32 pairs.  14 digits that pass mod 10 set flag bit 2 (ITF-14)."""
from __future__ import annotations

from typing import List

import numpy as np

from lumina_ocr import arch
from lumina_ocr.utils import barcodes as bc

from barcode_reference import MAX_SYMS, ROW_READS, element, match, quiet_ok, read128, read39, row_runs
from table_reference import ink_mask, pack_mask

P = arch.BARCODE_PARAMS
ALL_KINDS = (1 << len(bc.KINDS)) - 1

_TEAN = [[int(c) for c in p] for p in bc.EAN_MATCH]
_TITF = {m: [bc.itf_widths(v, m) for v in range(10)] for m in bc.ITF_RATIOS}
_P13 = [sum((c == "G") << i for i, c in enumerate(p)) for p in bc.EAN13_PARITY]
_PE = [sum((c == "E") << i for i, c in enumerate(p)) for p in bc.UPCE_PARITY]


def elements(runs, t: int, d: int, m0: int, n: int):
    w = [element(runs, t, d, m0 + i) for i in range(n)]
    return None if None in w else w


def units_ok(w: List[int], max_dist: int) -> bool:
    """n elements of one module each, by the measure"""
    n, s = len(w), sum(w)
    return sum(abs(wi * n - s) for wi in w) <= max_dist * s * n // 256


def guard_ok(w: List[int], s_digit: int, max_dist: int) -> bool:
    n, g = len(w), sum(w)
    return units_ok(w, max_dist) and 4 * abs(7 * g - n * s_digit) <= n * s_digit


def digit_at(kind: int, k: int) -> int:
    nleft, centre = bc.EAN_LAYOUT[kind][1:3]
    return 3 + 4 * k + (5 if centre is not None and k >= nleft else 0)


def read_ean(kind: int, runs, t: int, d: int, quiet: int, max_dist: int):
    """-> (symbols, bars used, flags) or None."""
    nd, nleft, centre, end, nend, bars = bc.EAN_LAYOUT[kind]
    last = t + d * (bars - 1)
    if not 0 <= last < len(runs):
        return None
    dig = [elements(runs, t, d, digit_at(kind, k), 4) for k in range(nd)]
    if not guard_ok(elements(runs, t, d, 0, 3), sum(dig[0]), max_dist):
        return None
    if centre is not None and not guard_ok(elements(runs, t, d, centre, 5), sum(dig[nleft - 1]), max_dist):
        return None
    if not guard_ok(elements(runs, t, d, end, nend), sum(dig[nd - 1]), max_dist):
        return None
    if not quiet_ok(runs, t, d, sum(dig[0]), bc.EAN_MODULES, quiet) or not quiet_ok(runs, last, -d, sum(dig[nd - 1]), bc.EAN_MODULES, quiet):
        return None
    vals = []
    for k in range(nd):
        v, _ = match(dig[k], _TEAN if k < nleft else _TEAN[:10], bc.EAN_MODULES, max_dist)
        if v is None:
            return None
        vals.append(v)
    gmask = sum((v >= 10) << k for k, v in enumerate(vals[:nleft]))
    digits = [v % 10 for v in vals]
    if kind == bc.KIND_EAN13:
        if gmask not in _P13:
            return None
        out = [_P13.index(gmask)] + digits
        ok = bc.mod10_ok(out)
    elif kind == bc.KIND_EAN8:
        out = digits
        ok = gmask == 0 and bc.mod10_ok(out)
    else:
        if gmask not in _PE:
            return None
        row = _PE.index(gmask)
        out = [row // 10] + digits + [row % 10]
        a, b, c, dd, e, f = digits       # the expansion, written out (barcodes.upce_to_upca is the host's)
        body = [a, b, f, 0, 0, 0, 0, c, dd, e] if f <= 2 else [a, b, c, 0, 0, 0, 0, 0, dd, e] if f == 3 else \
            [a, b, c, dd, 0, 0, 0, 0, 0, e] if f == 4 else [a, b, c, dd, e, 0, 0, 0, 0, f]
        full = [out[0]] + body + [out[7]]
        ok = sum(v * (3 if i % 2 == 0 else 1) for i, v in enumerate(full)) % 10 == 0
    return (out, bars, 0) if ok else None


def best(w: List[int], table, modules: int):
    """-> (value, d) of the nearest pattern, ties to the lowest value"""
    s = sum(w)
    return min(((v, sum(abs(wi * modules - pi * s) for wi, pi in zip(w, p))) for v, p in enumerate(table)), key=lambda t: (t[1], t[0]))


def read_itf(runs, t: int, d: int, quiet: int, max_dist: int):
    start = elements(runs, t, d, 0, 4)
    if start is None or not units_ok(start, max_dist) or not quiet_ok(runs, t, d, sum(start), 4, quiet):
        return None
    vals, M = [], None
    for k in range(bc.ITF_MAX_DIGITS // 2):
        w = elements(runs, t, d, 4 + 10 * k, 13)
        if w is None:
            return None
        wb, ws, stop = w[0:10:2], w[1:10:2], w[10:13]
        sb = sum(wb)
        if k == 0:
            M = min(bc.ITF_RATIOS, key=lambda m: (best(wb, _TITF[m], m)[1] * (1008 // m), m))
            if 4 * abs(sum(start) * M - 8 * sb) > 8 * sb:
                return None
        vb, _ = match(wb, _TITF[M], M, max_dist)
        vs, _ = match(ws, _TITF[M], M, max_dist)
        if vb is None or vs is None:
            return None
        vals += [vb, vs]
        ms, s3 = M // 2 + 1, sum(stop)
        dist = sum(abs(wi * ms - pi * s3) for wi, pi in zip(stop, (ms - 4, 2, 2)))
        last = t + d * (5 * k + 8)
        if k >= 2 and dist <= max_dist * s3 * ms // 256 and 4 * abs(s3 * M - ms * sb) <= ms * sb and quiet_ok(runs, last, -d, s3, ms, 2 * quiet):
            return vals, 5 * k + 9, bc.FLAG_ITF14 if len(vals) == 14 and bc.mod10_ok(vals) else 0
    return None


def read_at(runs, t: int, d: int, quiet: int, max_dist: int, kinds: int):
    """-> (kind, symbols, bars, flags) of the first kind of the set that reads at bar t, or None"""
    for kind in range(len(bc.KINDS)):
        if not kinds >> kind & 1:
            continue
        if kind == bc.KIND_CODE128:
            got = read128(runs, t, d, quiet, max_dist)
        elif kind == bc.KIND_CODE39:
            got = read39(runs, t, d, quiet, max_dist)
        elif kind == bc.KIND_ITF:
            got = read_itf(runs, t, d, quiet, max_dist)
        else:
            got = read_ean(kind, runs, t, d, quiet, max_dist)
        if got is not None:
            return (kind,) + tuple(got) + ((0,) if len(got) == 2 else ())
    return None


def scan(runs, d: int, quiet: int, max_dist: int, kinds: int):
    """Greedy reads of a row in direction d -> [(first bar, last bar, kind, symbols, flags)] (bars as run indices, first <= last)."""
    n = len(runs)
    out = []
    order = range(n) if d > 0 else range(n - 1, -1, -1)
    free = 0
    for pos, t in enumerate(order):
        if pos < free:
            continue
        got = read_at(runs, t, d, quiet, max_dist, kinds)
        if got is None:
            continue
        kind, vals, bars, flags = got
        free = pos + bars
        last = t + d * (bars - 1)
        out.append((min(t, last), max(t, last), kind, vals, flags))
    return out


def row_reads(row: np.ndarray, quiet: int, max_dist: int, kinds: int):
    """-> up to four (a0, a1, kind, reversed | ITF-14 flag, symbols), by a0."""
    runs = row_runs(row)
    if len(runs) < 10:
        return []
    fwd = scan(runs, +1, quiet, max_dist, kinds)
    bwd = [r for r in scan(runs, -1, quiet, max_dist, kinds) if not any(r[0] <= f[1] and f[0] <= r[1] for f in fwd)]
    reads = [(runs[b0][0], runs[b1][1], kind, rev | flags, tuple(vals)) for rev, lst in ((0, fwd), (1, bwd)) for b0, b1, kind, vals, flags in lst]
    reads.sort(key=lambda r: r[0])
    return reads[:ROW_READS]


def codes_of_ink(ink: np.ndarray, kinds: int = 3, quiet: int = None, max_dist: int = None, min_rows: int = None, row_gap: int = None):
    """bool [H,W] -> (codes int32 [m,8], syms int32 [m,64]): barcode_reference.codes_of_ink on this file's row reads."""
    assert 0 < kinds <= ALL_KINDS
    quiet = P["quiet"] if quiet is None else quiet
    max_dist = P["max_dist"] if max_dist is None else max_dist
    min_rows = P["min_rows"] if min_rows is None else min_rows
    row_gap = P["row_gap"] if row_gap is None else row_gap
    H, W = ink.shape
    found = []
    for vertical, img in ((0, ink), (1, ink.T)):
        per_row = [row_reads(img[r], quiet, max_dist, kinds) for r in range(img.shape[0])]
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


def barcodes(page: np.ndarray, kinds: int = 3, threshold: int = None, **kw):
    """uint8 [H,W,3] -> (mask uint64 [H, ceil(W/64)], codes int32 [m,8], syms int32 [m,64])."""
    ink = ink_mask(page, P["threshold"] if threshold is None else threshold)
    return (pack_mask(ink),) + codes_of_ink(ink, kinds, **kw)


def decoded(codes: np.ndarray, syms: np.ndarray) -> List[str]:
    return [bc.symbols_text(int(c[4]), list(s[:int(c[5])])) for c, s in zip(codes, syms)]
