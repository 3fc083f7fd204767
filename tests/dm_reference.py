"""Restatement (test infrastructure, NumPy / plain Python) of the Data Matrix pass that lumina_ocr_datamatrix runs on the device.  It
shares the tables of lumina_ocr/utils/datamatrix.py with the product code and nothing else; it is the definition the kernels must
equal.

Components: the 8-connected components of the ink (runs and roots as tests/mark_reference.py), each with its box, its ink area and
its four diagonal extremes E0..E3: the pixels that minimise x + y, maximise x - y, maximise x + y and minimise x - y, ties by the
smaller y.  Their OUTER CORNERS in doubled coordinates are P0 = (2x, 2y), P1 = (2x + 2, 2y), P2 = (2x + 2, 2y + 2), P3 = (2x, 2y + 2):
of an upright symbol with nothing touching it P3 is the L's elbow, P0 the top of its upright and P2 the end of its foot.

Candidates: a root with 8 min_module <= w, h <= 52 max_module and 32 area >= w h, in the order of the roots.  A page with more
than max_candidates of them (<= 1024, not the outline's 64: every large glyph is a candidate) is not read.

Tries: every size of the table (in its order) at every rotation k = 0..3 (quarter turns clockwise): the elbow O = P[(k + 3) % 4],
U = P[k] - O runs up the L's upright (R rows), V = P[(k + 2) % 4] - O along its foot (C columns).  The try is IN REACH when
(2 R min_module)^2 <= |U|^2 <= (2 R max_module)^2, the same for |V|^2 with C, and the two module sizes agree within a quarter:
16 max(a, b) <= 25 min(a, b) with a = |U|^2 C^2, b = |V|^2 R^2.  Module (row r, col c) is the ink at the pixel (nx // 4RC, ny // 4RC),
nx = Ox 2RC + Vx (2c + 1) R + Ux (2R - 2r - 1) C, ny the same in y: the module's centre.  A negative numerator or a pixel off the page
reads clear.  L misses: modules of the L and of the inner solid bars that are clear; timing mismatches: modules of the clock tracks
and inner clock bars that differ from their alternation.  The try with the smallest (timing mismatches, L misses, R C, k, size index)
is kept; more than timing_max mismatches or solid_max misses drop the candidate.

The `quiet` rings of modules round the symbol must be clear.  The codewords are read through the placement, de-interleaved
(block b of nb takes every nb-th codeword from b on, in the data and in the check part alike) and corrected block by block
(syndromes, Berlekamp-Massey, Chien, Forney over GF(256) / 0x12D, roots a^1 ...); the syndromes are recomputed: a block with more
than ec // 2 errors drops the candidate.  The hull is the box of the parallelogram O, O + U, O + V, O + U + V.

A row is x0, y0, x1, y1, rows, cols, ndata, corrected errors, rotation, timing mismatches, L misses, 0; rows are sorted by
(y0, x0, y1, x1, root)."""
from __future__ import annotations

from typing import List, Optional, Tuple

import numpy as np

from lumina_ocr import arch
from lumina_ocr.utils import datamatrix as dm

from mark_reference import run_roots, runs_of
from table_reference import ink_mask, pack_mask

P = arch.DM_PARAMS
MAX_DATA = dm.MAX_DATA
EXP, LOG = dm.GF_EXP, dm.GF_LOG
_MASKS = [dm.function_masks(s) for s in range(dm.NUM_SIZES)]


def mul(a: int, b: int) -> int:
    return EXP[LOG[a] + LOG[b]] if a and b else 0


def find_candidates(ink: np.ndarray, min_module: int, max_module: int) -> List[Tuple[int, List[Tuple[int, int]]]]:
    """-> [(root, [P0, P1, P2, P3])] in the order of the roots."""
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
    # (key, y) packed so that one min / max is the extreme with its tie rule
    big = np.int64(1) << 40
    e0, e3 = np.full(n, big), np.full(n, big)
    e1, e2 = np.full(n, -big), np.full(n, -big)
    np.minimum.at(e0, root, ((s + row) << 17) | row)
    np.maximum.at(e1, root, ((e - row + 65536) << 17) | (65535 - row))
    np.maximum.at(e2, root, ((e + row) << 17) | (65535 - row))
    np.minimum.at(e3, root, ((s - row + 65536) << 17) | row)
    out = []
    for r in np.nonzero(root == np.arange(n))[0]:
        w, h = int(x1[r] - x0[r] + 1), int(y1[r] - row[r] + 1)
        if not (8 * min_module <= w <= 52 * max_module and 8 * min_module <= h <= 52 * max_module and 32 * int(area[r]) >= w * h):
            continue
        y = [int(e0[r]) & 0x1FFFF, 65535 - (int(e1[r]) & 0x1FFFF), 65535 - (int(e2[r]) & 0x1FFFF), int(e3[r]) & 0x1FFFF]
        k = [int(v) >> 17 for v in (e0[r], e1[r], e2[r], e3[r])]
        x = [k[0] - y[0], k[1] - 65536 + y[1], k[2] - y[2], k[3] - 65536 + y[3]]
        out.append((int(r), [(2 * x[0], 2 * y[0]), (2 * x[1] + 2, 2 * y[1]), (2 * x[2] + 2, 2 * y[2] + 2), (2 * x[3], 2 * y[3] + 2)]))
    return out


class Grid:
    """The affine sampling grid of a candidate at a size and a rotation."""

    def __init__(self, ink, corners, size: int, k: int):
        self.ink, self.size, self.k = ink, size, k
        self.R, self.C = dm.SIZES[size][:2]
        self.ox, self.oy = corners[(k + 3) % 4]
        self.ux, self.uy = corners[k][0] - self.ox, corners[k][1] - self.oy
        self.vx, self.vy = corners[(k + 2) % 4][0] - self.ox, corners[(k + 2) % 4][1] - self.oy

    def in_reach(self, min_module: int, max_module: int) -> bool:
        lu, lv = self.ux ** 2 + self.uy ** 2, self.vx ** 2 + self.vy ** 2
        R, C = self.R, self.C
        if not ((2 * R * min_module) ** 2 <= lu <= (2 * R * max_module) ** 2 and (2 * C * min_module) ** 2 <= lv <= (2 * C * max_module) ** 2):
            return False
        a, b = lu * C * C, lv * R * R
        return 16 * max(a, b) <= 25 * min(a, b)

    def at(self, r: int, c: int) -> int:
        R, C = self.R, self.C
        nx = self.ox * 2 * R * C + self.vx * (2 * c + 1) * R + self.ux * (2 * R - 2 * r - 1) * C
        ny = self.oy * 2 * R * C + self.vy * (2 * c + 1) * R + self.uy * (2 * R - 2 * r - 1) * C
        if nx < 0 or ny < 0:
            return 0
        px, py = nx // (4 * R * C), ny // (4 * R * C)
        return int(px < self.ink.shape[1] and py < self.ink.shape[0] and self.ink[py, px])

    def rows(self) -> List[int]:
        return [sum(self.at(r, c) << c for c in range(self.C)) for r in range(self.R)]

    def score(self) -> Tuple[int, int]:
        """-> (timing mismatches, L misses): only the function modules are sampled."""
        solid, clock, dark = _MASKS[self.size]
        timing = misses = 0
        for r in range(self.R):
            for c in range(self.C):
                if (solid[r] >> c) & 1:
                    misses += 1 - self.at(r, c)
                elif (clock[r] >> c) & 1:
                    timing += self.at(r, c) != ((dark[r] >> c) & 1)
        return timing, misses

    def hull(self) -> Tuple[int, int, int, int]:
        H, W = self.ink.shape
        qx = [(self.ox + a * self.ux + b * self.vx) // 2 for a in (0, 1) for b in (0, 1)]      # (every term is even)
        qy = [(self.oy + a * self.uy + b * self.vy) // 2 for a in (0, 1) for b in (0, 1)]
        cl = lambda v, hi: max(0, min(hi, v))
        return cl(min(qx), W - 1), cl(min(qy), H - 1), cl(max(qx) - 1, W - 1), cl(max(qy) - 1, H - 1)


def rs_correct(block: List[int], ec: int) -> Optional[Tuple[List[int], int]]:
    """A block (data then check codewords, the first the highest power) -> (corrected block, errors) or None.  Roots a^1 .. a^ec."""
    n = len(block)
    synd = lambda blk: [_eval_desc(blk, EXP[k + 1]) for k in range(ec)]
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
        out[p] ^= mul(_eval_asc(omega, xi), EXP[255 - LOG[den]])          # first root a^1: no factor X
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


def decode_candidate(ink, corners, min_module: int, max_module: int, quiet: int, timing_max: int, solid_max: int):
    """-> (the output row, data codewords) or None."""
    best = None
    for size in range(dm.NUM_SIZES):
        for k in range(4):
            g = Grid(ink, corners, size, k)
            if not g.in_reach(min_module, max_module):
                continue
            timing, misses = g.score()
            key = (timing, misses, g.R * g.C, k, size)
            if best is None or key < best[0]:
                best = (key, g)
    if best is None or best[0][0] > timing_max or best[0][1] > solid_max:
        return None
    (timing, misses, _, k, size), g = best
    R, C, ndata, ncheck, _, _, nb = dm.SIZES[size]
    for q in range(1, quiet + 1):
        for t in range(-q, max(R, C) + q):
            if (t < C + q and (g.at(-q, t) or g.at(R - 1 + q, t))) or (t < R + q and (g.at(t, -q) or g.at(t, C - 1 + q))):
                return None
    rows = g.rows()
    place = dm.placement_of(size)
    raw = []
    for i in range(ndata + ncheck):
        v = 0
        for bit in range(8):
            r, c = place[8 * i + bit]
            v = (v << 1) | ((rows[r] >> c) & 1)
        raw.append(v)
    data, errors, ec = [0] * ndata, 0, ncheck // nb
    for b in range(nb):
        got = rs_correct(raw[b:ndata:nb] + raw[ndata + b::nb], ec)
        if got is None:
            return None
        data[b::nb] = got[0][:len(range(b, ndata, nb))]
        errors += got[1]
    return g.hull() + (R, C, ndata, errors, k, timing, misses, 0), data


def codes_of_ink(ink: np.ndarray, min_module=None, max_module=None, quiet=None, timing_max=None, solid_max=None, max_candidates=None):
    """bool [H,W] -> (codes int32 [m,12], data int32 [m,MAX_DATA], candidates found)."""
    g = lambda k, v: P[k] if v is None else v
    mn, mx = g("min_module", min_module), g("max_module", max_module)
    cands = find_candidates(ink, mn, mx)
    found = []
    if len(cands) <= g("max_candidates", max_candidates):
        for root, corners in cands:
            got = decode_candidate(ink, corners, mn, mx, g("quiet", quiet), g("timing_max", timing_max), g("solid_max", solid_max))
            if got is not None:
                row, data = got
                found.append(((row[1], row[0], row[3], row[2], root), row, data))
    found.sort(key=lambda t: t[0])
    codes = np.array([t[1] for t in found], np.int32).reshape(-1, 12)
    data = np.zeros((len(found), MAX_DATA), np.int32)
    for i, t in enumerate(found):
        data[i, :len(t[2])] = t[2]
    return codes, data, len(cands)


def datamatrix(page: np.ndarray, threshold: int = None, **kw):
    """uint8 [H,W,3] -> (mask uint64 [H, ceil(W/64)], codes int32 [m,12], data int32 [m,MAX_DATA], candidates found)."""
    ink = ink_mask(page, P["threshold"] if threshold is None else threshold)
    return (pack_mask(ink),) + codes_of_ink(ink, **kw)


def texts(codes: np.ndarray, data: np.ndarray) -> List[str]:
    return [e["content"] for e in dm.read_datamatrix(codes, data)]
