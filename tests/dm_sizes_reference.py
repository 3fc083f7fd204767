"""Restatement (test infrastructure, NumPy / plain Python) of the two-stage Data Matrix pass that lumina_ocr_datamatrix_sizes runs on the
device: every ECC 200 size up to max_size (52 .. 144).  It shares the tables of lumina_ocr/utils/datamatrix.py with the product code
and nothing else; it is the definition the kernels must equal.

Stage 1 is tests/dm_reference.py's pass, called, not copied: its candidates, its tries, its rows and codewords.

Stage 2 (max_size >= 64) has a candidate list of its own: the roots with 64 min_module <= w, h <= 144 max_module and 32 area >= w h, in
the order of the roots; a page with more than max_candidates of them is not read by stage 2 (stage 1's rows stand).  A root that gave
a stage-1 row is skipped.  Tries: every size of LARGE_SIZES with rows <= max_size at every rotation, in reach by dm_reference's rule
(its Grid, over ALL_SIZES); the score counts, over all 2 nr clock and solid rows and 2 nc columns of the regions, the clear modules of
the L and the inner solid bars and the clock modules off their alternation; the smallest (timing mismatches, L misses, R C, k, size)
is kept and dropped above timing_max / solid_max.  Quiet rings, placement, Reed-Solomon and hull as in stage 1, except that the blocks
are dealt by STREAM POSITION: the codeword at position p of data + check belongs to block p mod nb, so block b is the positions b,
b + nb, ... and its last ec codewords are its check codewords.  For every size but 144 x 144 that is stage 1's rule; 144 x 144 has
1558 data codewords in ten blocks, so its check codewords carry on from block 8.

Both stages' rows are sorted together by (y0, x0, y1, x1, root).  Data rows are bytes [m, 1560], zero behind ndata.  The candidate
count reported is stage 1's."""
from __future__ import annotations

from typing import List, Tuple

import numpy as np

from lumina_ocr import arch
from lumina_ocr.utils import datamatrix as dm

import dm_reference as dmr
from mark_reference import run_roots, runs_of
from table_reference import ink_mask, pack_mask

P = arch.DM_PARAMS
MAX_DATA_ALL = dm.MAX_DATA_ALL
_FUNCTION = {}


def function_lists(size: int):
    """-> (rows, cols, solid, dark) arrays of the size's function modules."""
    if size not in _FUNCTION:
        rows, cols, _, _, nr, nc, _ = dm.ALL_SIZES[size]
        rh, rw = rows // nr, cols // nc
        f = sorted(dm.function_modules(size).items())
        r, c = np.array([k[0] for k, _ in f], np.int64), np.array([k[1] for k, _ in f], np.int64)
        _FUNCTION[size] = (r, c, (c % rw == 0) | (r % rh == rh - 1), np.array([d for _, d in f], bool))
    return _FUNCTION[size]


def large_candidates(ink: np.ndarray, min_module: int, max_module: int) -> List[Tuple[int, List[Tuple[int, int]]]]:
    """-> [(root, [P0, P1, P2, P3])] of stage 2, in the order of the roots."""
    row, s, e = runs_of(ink)
    n = len(row)
    if n == 0:
        return []
    root = run_roots(row, s, e)
    x0, x1, y1 = np.full(n, 1 << 30), np.full(n, -1), np.full(n, -1)
    np.minimum.at(x0, root, s)
    np.maximum.at(x1, root, e)
    np.maximum.at(y1, root, row)
    out = []
    for r, corners in dmr.find_candidates(ink, 1, 1 << 20):          # every root of 8 pixels and more a side that passes the area test
        w, h = int(x1[r] - x0[r] + 1), int(y1[r] - row[r] + 1)
        if 64 * min_module <= w <= 144 * max_module and 64 * min_module <= h <= 144 * max_module:
            out.append((r, corners))
    return out


class LargeGrid(dmr.Grid):
    """dm_reference's grid at a size of ALL_SIZES."""

    def __init__(self, ink, corners, size: int, k: int):
        self.ink, self.size, self.k = ink, size, k
        self.R, self.C = dm.ALL_SIZES[size][:2]
        self.ox, self.oy = corners[(k + 3) % 4]
        self.ux, self.uy = corners[k][0] - self.ox, corners[k][1] - self.oy
        self.vx, self.vy = corners[(k + 2) % 4][0] - self.ox, corners[(k + 2) % 4][1] - self.oy

    def sample(self, r: np.ndarray, c: np.ndarray) -> np.ndarray:
        """Grid.at of arrays of modules (64-bit: the terms pass 2^32)."""
        R, C = self.R, self.C
        nx = self.ox * 2 * R * C + self.vx * (2 * c + 1) * R + self.ux * (2 * R - 2 * r - 1) * C
        ny = self.oy * 2 * R * C + self.vy * (2 * c + 1) * R + self.uy * (2 * R - 2 * r - 1) * C
        px, py = nx // (4 * R * C), ny // (4 * R * C)
        H, W = self.ink.shape
        ok = (nx >= 0) & (ny >= 0) & (px < W) & (py < H)
        return ok & self.ink[np.clip(py, 0, H - 1), np.clip(px, 0, W - 1)]

    def score(self) -> Tuple[int, int]:
        r, c, solid, dark = function_lists(self.size)
        v = self.sample(r, c)
        return int(np.sum(~solid & (v != dark))), int(np.sum(solid & ~v))

    def rows(self) -> List[int]:
        r, c = np.divmod(np.arange(self.R * self.C, dtype=np.int64), self.C)
        v = self.sample(r, c).reshape(self.R, self.C)
        return [sum(1 << int(j) for j in np.nonzero(v[i])[0]) for i in range(self.R)]


def decode_large(ink, corners, min_module: int, max_module: int, quiet: int, timing_max: int, solid_max: int, max_size: int):
    """-> (the output row, data codewords) or None."""
    best = None
    for size in range(dm.NUM_SIZES, dm.NUM_SIZES_ALL):
        if dm.ALL_SIZES[size][0] > max_size:
            continue
        for k in range(4):
            g = LargeGrid(ink, corners, size, k)
            if not g.in_reach(min_module, max_module):
                continue
            timing, misses = g.score()
            key = (timing, misses, g.R * g.C, k, size)
            if best is None or key < best[0]:
                best = (key, g)
    if best is None or best[0][0] > timing_max or best[0][1] > solid_max:
        return None
    (timing, misses, _, k, size), g = best
    R, C, ndata, ncheck, _, _, nb = dm.ALL_SIZES[size]
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
    errors, ec = 0, ncheck // nb
    for b in range(nb):                                    # block b: the stream positions b, b + nb, ...
        got = dmr.rs_correct(raw[b::nb], ec)
        if got is None:
            return None
        raw[b::nb] = got[0]
        errors += got[1]
    return g.hull() + (R, C, ndata, errors, k, timing, misses, 0), raw[:ndata]


def codes_of_ink(ink: np.ndarray, max_size: int, min_module=None, max_module=None, quiet=None, timing_max=None, solid_max=None, max_candidates=None):
    """bool [H,W] -> (codes int32 [m,12], data uint8 [m,MAX_DATA_ALL], stage 1's candidates found)."""
    assert dm.MIN_MAX_SIZE <= max_size <= dm.MAX_MAX_SIZE
    g = lambda k, v: P[k] if v is None else v
    mn, mx, cap = g("min_module", min_module), g("max_module", max_module), g("max_candidates", max_candidates)
    rest = (g("quiet", quiet), g("timing_max", timing_max), g("solid_max", solid_max))
    found, read = [], set()
    cands = dmr.find_candidates(ink, mn, mx)
    if len(cands) <= cap:
        for root, corners in cands:
            got = dmr.decode_candidate(ink, corners, mn, mx, *rest)
            if got is not None:
                found.append(((got[0][1], got[0][0], got[0][3], got[0][2], root),) + got)
                read.add(root)
    if max_size >= 64:
        large = large_candidates(ink, mn, mx)
        if len(large) <= cap:
            for root, corners in large:
                if root in read:
                    continue
                got = decode_large(ink, corners, mn, mx, *rest, max_size)
                if got is not None:
                    found.append(((got[0][1], got[0][0], got[0][3], got[0][2], root),) + got)
    found.sort(key=lambda t: t[0])
    codes = np.array([t[1] for t in found], np.int32).reshape(-1, 12)
    data = np.zeros((len(found), MAX_DATA_ALL), np.uint8)
    for i, t in enumerate(found):
        data[i, :len(t[2])] = t[2]
    return codes, data, len(cands)


def datamatrix_sizes(page: np.ndarray, max_size: int, threshold: int = None, **kw):
    """uint8 [H,W,3] -> (mask uint64 [H, ceil(W/64)], codes int32 [m,12], data uint8 [m,MAX_DATA_ALL], stage 1's candidates found)."""
    ink = ink_mask(page, P["threshold"] if threshold is None else threshold)
    return (pack_mask(ink),) + codes_of_ink(ink, max_size, **kw)


def texts(codes: np.ndarray, data: np.ndarray) -> List[str]:
    return [e["content"] for e in dm.read_datamatrix(codes, data)]
