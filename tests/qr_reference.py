"""Restatement (test infrastructure, NumPy / plain Python) of the QR pass that lumina_ocr_qrcodes runs on the device.  It shares the
tables of lumina_ocr/utils/qrcodes.py with the product code and nothing else; it is the definition the kernels must equal.

Components: the 8-connected components of the ink, each with its box and its ink area (runs and roots as tests/mark_reference.py).

Finders: a CORE is a component with 3 min_module <= w, h <= 3 max_module, 4 |w - h| <= min(w, h) and 4 area >= 3 w h.  In the row
yc = (y0 + y1) // 2 the run holding xc = (x0 + x1) // 2 must be the core's; the run before it and the run after it in that row must
have one common root, not the core: the RING.  With (rw, rh) the ring's box sides the ring is concentric with the core when
112 |(rx0 + rx1) - (x0 + x1)| <= centre_tol (rw + rh) (centre_tol sixteenths of a module, rw + rh standing for 14 modules), the same
in y, and 7/3 of its size when 224 |3 rw - 7 w| <= 3 ring_tol (rw + rh), the same for rh and h.  A finder is (cx2, cy2, me, id):
the ring's centre in doubled pixel coordinates (rx0 + rx1 + 1, ry0 + ry1 + 1), me = rw + rh and the core's root.  A page with more
than max_finders finders is not read.

Grouping: for a finder A the pair (B, C) of two others is valid when, with AB = B - A, AC = C - A in doubled coordinates,
|d| <= 8192 for all four differences, 4 |AB^2 - AC^2| <= min(AB^2, AC^2), 64 (AB . AC)^2 <= AB^2 AC^2, cross(AB, AC) > 0,
4 |meA - meX| <= min(meA, meX) for X = B and C, and some version 1..10 is in reach; version v (n = 10 + 4 v modules between finder
centres) is in reach when (2 (n - 3) M)^2 <= 882 (AB^2 + AC^2) <= (2 (n + 3) M)^2, M = meA + meB + meC.  A's valid pairs are tried
in the order of (AB^2 + AC^2, id B, id C), the first PAIR_TRIES of them at most, and the first that decodes is A's symbol (a
neighbouring symbol's finder can lie nearer than A's own partners); A without such a pair is no corner.

Decode, per pair: module (col i, row j) of a version is the ink at pixel (nx // 2n, ny // 2n), nx = ax2 n + (i - 3) ABx +
(j - 3) ACx, ny the same in y; a negative numerator or a pixel off the page reads clear.  Of the versions in reach the one with the
fewest mismatches in the timing patterns (row 6 and column 6, indices 8 .. D - 9, dark on even) is kept, the smaller on a tie; more
than timing_max mismatches drop the candidate.  The `quiet` rings of modules round the symbol must be clear.  The first copy of the
format information is matched against the 32 words; within distance 3 it gives level and mask, otherwise the second copy does, or
the candidate is dropped.  Unmask, read the codewords in placement order, de-interleave, correct every block (syndromes,
Berlekamp-Massey, Chien, Forney over GF(256) / 0x11D, roots a^0 ...), recompute the syndromes: a block with more than ec // 2 errors
drops the candidate.  The hull is the box of the four outer module corners."""
from __future__ import annotations

from typing import List, Optional, Tuple

import numpy as np

from lumina_ocr import arch
from lumina_ocr.utils import qrcodes as qr

from mark_reference import run_roots, runs_of
from table_reference import ink_mask, pack_mask

P = arch.QR_PARAMS
MAX_DATA = qr.MAX_DATA
SPAN = 8192
PAIR_TRIES = 8
EXP, LOG = qr.GF_EXP, qr.GF_LOG


def mul(a: int, b: int) -> int:
    return EXP[LOG[a] + LOG[b]] if a and b else 0


def find_finders(ink: np.ndarray, min_module: int, max_module: int, centre_tol: int, ring_tol: int) -> List[Tuple[int, int, int, int]]:
    """-> [(cx2, cy2, me, id)] in the order of the cores' roots."""
    row, s, e = runs_of(ink)
    n = len(row)
    if n == 0:
        return []
    root = run_roots(row, s, e)
    x0, x1, y1, area = np.full(n, 1 << 30), np.full(n, -1), np.full(n, -1), np.zeros(n, np.int64)
    np.minimum.at(x0, root, s)
    np.maximum.at(x1, root, e)
    np.maximum.at(y1, root, row)
    np.add.at(area, root, e - s + 1)
    first = np.searchsorted(row, np.arange(ink.shape[0] + 1), "left")       # runs of row y: first[y] .. first[y + 1]
    out = []
    for r in np.nonzero(root == np.arange(n))[0]:
        bx0, by0, bx1, by1 = int(x0[r]), int(row[r]), int(x1[r]), int(y1[r])
        w, h = bx1 - bx0 + 1, by1 - by0 + 1
        if not (3 * min_module <= w <= 3 * max_module and 3 * min_module <= h <= 3 * max_module and 4 * abs(w - h) <= min(w, h)
                and 4 * int(area[r]) >= 3 * w * h):
            continue
        yc, xc = (by0 + by1) // 2, (bx0 + bx1) // 2
        lo, hi = int(first[yc]), int(first[yc + 1])
        j = next((k for k in range(lo, hi) if s[k] <= xc <= e[k]), None)
        if j is None or root[j] != r or j - 1 < lo or j + 1 >= hi or root[j - 1] != root[j + 1] or root[j - 1] == r:
            continue
        q = int(root[j - 1])
        rx0, ry0, rx1, ry1 = int(x0[q]), int(row[q]), int(x1[q]), int(y1[q])
        rw, rh = rx1 - rx0 + 1, ry1 - ry0 + 1
        if 112 * abs((rx0 + rx1) - (bx0 + bx1)) > centre_tol * (rw + rh) or 112 * abs((ry0 + ry1) - (by0 + by1)) > centre_tol * (rw + rh):
            continue
        if 224 * abs(3 * rw - 7 * w) > 3 * ring_tol * (rw + rh) or 224 * abs(3 * rh - 7 * h) > 3 * ring_tol * (rw + rh):
            continue
        out.append((rx0 + rx1 + 1, ry0 + ry1 + 1, rw + rh, int(r)))
    return out


def versions_in_reach(l2: int, m: int) -> List[int]:
    return [v for v in range(1, 11) if (2 * (6 + 4 * v + 1) * m) ** 2 <= 882 * l2 <= (2 * (6 + 4 * v + 7) * m) ** 2]


def pairs_of(fs, a: int) -> List[Tuple[int, int]]:
    """-> [(b, c)], finder a's valid pairs with the PAIR_TRIES smallest keys, in key order."""
    ax, ay, ma, _ = fs[a]
    found = []
    for b, (bx, by, mb, idb) in enumerate(fs):
        for c, (cx, cy, mc, idc) in enumerate(fs):
            if a == b or a == c or b == c:
                continue
            abx, aby, acx, acy = bx - ax, by - ay, cx - ax, cy - ay
            if max(abs(abx), abs(aby), abs(acx), abs(acy)) > SPAN:
                continue
            lab, lac = abx * abx + aby * aby, acx * acx + acy * acy
            dot, cross = abx * acx + aby * acy, abx * acy - aby * acx
            if 4 * abs(lab - lac) > min(lab, lac) or 64 * dot * dot > lab * lac or cross <= 0:
                continue
            if 4 * abs(ma - mb) > min(ma, mb) or 4 * abs(ma - mc) > min(ma, mc):
                continue
            if not versions_in_reach(lab + lac, ma + mb + mc):
                continue
            found.append(((lab + lac, idb, idc), b, c))
    return [(b, c) for _, b, c in sorted(found)[:PAIR_TRIES]]


class Grid:
    """The affine sampling grid of a candidate at a version."""

    def __init__(self, ink, A, B, C, version):
        self.ink, self.n, self.d = ink, 10 + 4 * version, 17 + 4 * version
        self.ax, self.ay = A[0], A[1]
        self.abx, self.aby, self.acx, self.acy = B[0] - A[0], B[1] - A[1], C[0] - A[0], C[1] - A[1]

    def at(self, i: int, j: int) -> int:
        nx = self.ax * self.n + (i - 3) * self.abx + (j - 3) * self.acx
        ny = self.ay * self.n + (i - 3) * self.aby + (j - 3) * self.acy
        if nx < 0 or ny < 0:
            return 0
        px, py = nx // (2 * self.n), ny // (2 * self.n)
        return int(px < self.ink.shape[1] and py < self.ink.shape[0] and self.ink[py, px])

    def rows(self) -> List[int]:
        return [sum(self.at(i, j) << i for i in range(self.d)) for j in range(self.d)]

    def hull(self) -> Tuple[int, int, int, int]:
        H, W = self.ink.shape
        qx, qy = [], []
        for u in (-7, 2 * self.n + 7):
            for v in (-7, 2 * self.n + 7):
                qx.append((self.ax * 2 * self.n + u * self.abx + v * self.acx) // (4 * self.n))      # (Python's // is the floor)
                qy.append((self.ay * 2 * self.n + u * self.aby + v * self.acy) // (4 * self.n))
        cl = lambda v, hi: max(0, min(hi, v))
        return cl(min(qx), W - 1), cl(min(qy), H - 1), cl(max(qx) - 1, W - 1), cl(max(qy) - 1, H - 1)


def timing_mismatches(rows: List[int], d: int) -> int:
    return sum((((rows[6] >> k) & 1) != (k % 2 == 0)) + (((rows[k] >> 6) & 1) != (k % 2 == 0)) for k in range(8, d - 8))


def read_format(rows: List[int], version: int) -> Optional[Tuple[int, int, int]]:
    """-> (level index, mask, reported distance) or None."""
    for copy, pos in enumerate(qr.format_positions(version)):
        word = sum(((rows[r] >> c) & 1) << i for i, (r, c) in enumerate(pos))
        d, w = min((bin(word ^ fw).count("1"), w) for w, fw in enumerate(qr.FORMAT_WORDS))
        if d <= 3:
            return (w >> 3) ^ 1, w & 7, d + qr.SECOND_COPY * copy
    return None


def rs_correct(block: List[int], ec: int) -> Optional[Tuple[List[int], int]]:
    """A block (data then check codewords, the first the highest power) -> (corrected block, errors) or None."""
    n = len(block)
    synd = lambda blk: [_eval_desc(blk, EXP[k]) for k in range(ec)]
    S = synd(block)
    if not any(S):
        return list(block), 0
    C, Bp, L, m, b = [1] + [0] * ec, [1] + [0] * ec, 0, 1, 1
    for k in range(ec):
        d = S[k]
        for i in range(1, L + 1):
            d ^= mul(C[i], S[k - i])
        if d == 0:
            m += 1
            continue
        T = list(C)
        f = mul(d, EXP[255 - LOG[b]])
        for i in range(ec + 1 - m):
            C[i + m] ^= mul(f, Bp[i])
        if 2 * L <= k:
            L, Bp, b, m = k + 1 - L, T, d, 1
        else:
            m += 1
    if L > ec // 2:
        return None
    omega = [0] * L
    for i in range(L):
        for j in range(i + 1):
            omega[i] ^= mul(S[i - j], C[j])
    out, roots = list(block), 0
    for p in range(n):
        e = n - 1 - p
        xi = EXP[(255 - e % 255) % 255]                   # X^-1, X = a^e
        if _eval_asc(C[:L + 1], xi):
            continue
        roots += 1
        den = 0
        for i in range(1, L + 1, 2):
            den ^= mul(C[i], _pow(xi, i - 1))
        if den == 0:
            return None
        num = _eval_asc(omega, xi)
        out[p] ^= mul(EXP[e % 255], mul(num, EXP[255 - LOG[den]]))
    if roots != L or any(synd(out)):
        return None
    return out, L


def _pow(x: int, k: int) -> int:
    return EXP[(LOG[x] * k) % 255] if x else int(k == 0)


def _eval_desc(poly, x: int) -> int:
    y = 0
    for c in poly:
        y = mul(y, x) ^ c
    return y


def _eval_asc(poly, x: int) -> int:
    return _eval_desc(list(poly)[::-1], x)


def decode_candidate(ink, A, B, C, quiet: int, timing_max: int):
    """-> the output row's tail (hull, version, level, mask, ndata, errors, rotation, fdist, timing, data) or None."""
    abx, aby, acx, acy = B[0] - A[0], B[1] - A[1], C[0] - A[0], C[1] - A[1]
    best = None
    for v in versions_in_reach(abx * abx + aby * aby + acx * acx + acy * acy, A[2] + B[2] + C[2]):
        g = Grid(ink, A, B, C, v)
        rows = g.rows()
        t = timing_mismatches(rows, g.d)
        if best is None or t < best[0]:
            best = (t, v, g, rows)
    if best is None or best[0] > timing_max:
        return None
    timing, version, g, rows = best
    d = g.d
    for k in range(1, quiet + 1):
        for t in range(-k, d + k):
            if g.at(t, -k) or g.at(t, d - 1 + k) or g.at(-k, t) or g.at(d - 1 + k, t):
                return None
    fmt = read_format(rows, version)
    if fmt is None:
        return None
    level, mask, fdist = fmt
    place = qr.placement_of(version)
    total = qr.TOTAL_CODEWORDS[version - 1]
    raw = []
    for k in range(total):
        v = 0
        for bit in range(8):
            r, c = place[8 * k + bit]
            v = (v << 1) | (((rows[r] >> c) & 1) ^ int(qr.mask_bit(mask, r, c)))
        raw.append(v)
    nb, short, dlen, ec = qr.block_structure(version, level)
    ndata = nb * dlen + (nb - short)
    data, errors = [], 0
    for b in range(nb):
        n = dlen + (b >= short)
        blk = [raw[i * nb + b] for i in range(dlen)] + ([raw[dlen * nb + b - short]] if b >= short else []) + [raw[ndata + i * nb + b] for i in range(ec)]
        got = rs_correct(blk, ec)
        if got is None:
            return None
        data += got[0][:n]
        errors += got[1]
    rot = (0 if abx > 0 else 2) if abs(abx) >= abs(aby) else (1 if aby > 0 else 3)
    return g.hull() + (version, level, mask, ndata, errors, rot, fdist, timing), data


def codes_of_ink(ink: np.ndarray, min_module=None, max_module=None, quiet=None, centre_tol=None, ring_tol=None, timing_max=None,
                 max_finders=None):
    """bool [H,W] -> (codes int32 [m,12], data int32 [m,MAX_DATA], finders found)."""
    g = lambda k, v: P[k] if v is None else v
    fs = find_finders(ink, g("min_module", min_module), g("max_module", max_module), g("centre_tol", centre_tol), g("ring_tol", ring_tol))
    found = []
    if len(fs) <= g("max_finders", max_finders):
        for a in range(len(fs)):
            for b, c in pairs_of(fs, a):
                got = decode_candidate(ink, fs[a], fs[b], fs[c], g("quiet", quiet), g("timing_max", timing_max))
                if got is not None:
                    row, data = got
                    found.append(((row[1], row[0], row[3], row[2], fs[a][3]), row, data))
                    break
    found.sort(key=lambda t: t[0])
    codes = np.array([t[1] for t in found], np.int32).reshape(-1, 12)
    data = np.zeros((len(found), MAX_DATA), np.int32)
    for i, t in enumerate(found):
        data[i, :len(t[2])] = t[2]
    return codes, data, len(fs)


def qrcodes(page: np.ndarray, threshold: int = None, **kw):
    """uint8 [H,W,3] -> (mask uint64 [H, ceil(W/64)], codes int32 [m,12], data int32 [m,MAX_DATA], finders found)."""
    ink = ink_mask(page, P["threshold"] if threshold is None else threshold)
    return (pack_mask(ink),) + codes_of_ink(ink, **kw)


def texts(codes: np.ndarray, data: np.ndarray) -> List[str]:
    return [e["content"] for e in qr.read_qrcodes(codes, data)]
