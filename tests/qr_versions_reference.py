"""Restatement (test infrastructure, NumPy / plain Python) of the two-stage QR pass that lumina_ocr_qrcodes_versions runs on the
device.  Stage 1 is tests/qr_reference.py, imported and unchanged: finders, pairs and the decode of versions 1-10.  Stage 2 is stated
here; it shares the tables of lumina_ocr/utils/qrcodes.py with the product code and nothing else.

Stage 2 runs for a finder A to which stage 1 gave no symbol, when max_version > 10.  A's pairs (B, C) pass stage 1's geometric
tests; version v in 11..max_version is in reach when (2 (n - w) M)^2 <= 882 (AB^2 + AC^2) <= (2 (n + w) M)^2 with n = 10 + 4 v,
w = 3 + n // 16 and M = meA + meB + meC.  The PAIR_TRIES valid pairs with the smallest keys (AB^2 + AC^2, id B, id C) are tried in
key order and the first that decodes is A's symbol.

Per pair: for every version in reach row 6 and column 6 (indices 8 .. D - 9) are sampled on that version's affine grid (stage 1's
module formula with that n); the version with the fewest mismatches is kept, the smaller on a tie; more than timing_max * D // 57
mismatches drop the candidate.  The version information must agree: the top-right copy within Hamming distance 3 of
version_word(v), otherwise the bottom-left copy, otherwise the candidate is dropped.  Then as stage 1: the whole grid, the quiet
rings, the format information (first copy, then second), unmask, the codewords in placement order, de-interleave, correct every
block, the hull.  Alignment patterns are function modules only: the grid is affine through the three finders."""
from __future__ import annotations

from typing import List, Tuple

import numpy as np

from lumina_ocr.utils import qrcodes as qr

import qr_reference as R1
from table_reference import ink_mask, pack_mask

P = R1.P
MAX_DATA = qr.MAX_DATA_ALL
PAIR_TRIES = R1.PAIR_TRIES
SPAN = R1.SPAN


def versions_in_reach(l2: int, m: int, max_version: int) -> List[int]:
    out = []
    for v in range(11, max_version + 1):
        n = 10 + 4 * v
        w = 3 + n // 16
        if (2 * (n - w) * m) ** 2 <= 882 * l2 <= (2 * (n + w) * m) ** 2:
            out.append(v)
    return out


def pairs_of(fs, a: int, max_version: int) -> List[Tuple[int, int]]:
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
            if not versions_in_reach(lab + lac, ma + mb + mc, max_version):
                continue
            found.append(((lab + lac, idb, idc), b, c))
    return [(b, c) for _, b, c in sorted(found)[:PAIR_TRIES]]


def timing_of(g: R1.Grid) -> int:
    return sum((g.at(k, 6) != (k % 2 == 0)) + (g.at(6, k) != (k % 2 == 0)) for k in range(8, g.d - 8))


def version_agrees(g: R1.Grid, version: int) -> bool:
    want = qr.version_word(version)
    for copy in (0, 1):                       # top right, then bottom left
        word = sum(g.at(pos[copy][1], pos[copy][0]) << i for i, pos in enumerate(qr.version_positions(version)))
        if bin(word ^ want).count("1") <= 3:
            return True
    return False


def decode_candidate(ink, A, B, C, quiet: int, timing_max: int, max_version: int):
    """-> (the output row's tail, data codewords) or None."""
    abx, aby, acx, acy = B[0] - A[0], B[1] - A[1], C[0] - A[0], C[1] - A[1]
    best = None
    for v in versions_in_reach(abx * abx + aby * aby + acx * acx + acy * acy, A[2] + B[2] + C[2], max_version):
        g = R1.Grid(ink, A, B, C, v)
        t = timing_of(g)
        if best is None or t < best[0]:
            best = (t, v, g)
    if best is None:
        return None
    timing, version, g = best
    d = g.d
    if timing > timing_max * d // 57 or not version_agrees(g, version):
        return None
    rows = g.rows()
    for k in range(1, quiet + 1):
        for t in range(-k, d + k):
            if g.at(t, -k) or g.at(t, d - 1 + k) or g.at(-k, t) or g.at(d - 1 + k, t):
                return None
    fmt = R1.read_format(rows, version)
    if fmt is None:
        return None
    level, mask, fdist = fmt
    got = blocks_of_rows(rows, version, level, mask)
    if got is None:
        return None
    data, errors = got
    rot = (0 if abx > 0 else 2) if abs(abx) >= abs(aby) else (1 if aby > 0 else 3)
    return g.hull() + (version, level, mask, len(data), errors, rot, fdist, timing), data


def blocks_of_rows(rows: List[int], version: int, level: int, mask: int):
    """The module rows of a symbol -> (corrected data codewords, corrected errors) or None: unmask, placement order, de-interleave,
    every block corrected."""
    place = qr.placement_of(version)
    total = qr.TOTAL_CODEWORDS_ALL[version - 1]
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
        got = R1.rs_correct(blk, ec)
        if got is None:
            return None
        data += got[0][:n]
        errors += got[1]
    return data, errors


def codes_of_ink(ink: np.ndarray, max_version: int, min_module=None, max_module=None, quiet=None, centre_tol=None, ring_tol=None,
                 timing_max=None, max_finders=None):
    """bool [H,W] -> (codes int32 [m,12], data uint8 [m,MAX_DATA], finders found)."""
    g = lambda k, v: P[k] if v is None else v
    fs = R1.find_finders(ink, g("min_module", min_module), g("max_module", max_module), g("centre_tol", centre_tol), g("ring_tol", ring_tol))
    quiet, timing_max = g("quiet", quiet), g("timing_max", timing_max)
    found = []
    if len(fs) <= g("max_finders", max_finders):
        for a in range(len(fs)):
            got = None
            for b, c in R1.pairs_of(fs, a):
                got = R1.decode_candidate(ink, fs[a], fs[b], fs[c], quiet, timing_max)
                if got is not None:
                    break
            if got is None and max_version > 10:
                for b, c in pairs_of(fs, a, max_version):
                    got = decode_candidate(ink, fs[a], fs[b], fs[c], quiet, timing_max, max_version)
                    if got is not None:
                        break
            if got is not None:
                row, data = got
                found.append(((row[1], row[0], row[3], row[2], fs[a][3]), row, data))
    found.sort(key=lambda t: t[0])
    codes = np.array([t[1] for t in found], np.int32).reshape(-1, 12)
    data = np.zeros((len(found), MAX_DATA), np.uint8)
    for i, t in enumerate(found):
        data[i, :len(t[2])] = t[2]
    return codes, data, len(fs)


def qrcodes(page: np.ndarray, max_version: int, threshold: int = None, **kw):
    """uint8 [H,W,3] -> (mask uint64 [H, ceil(W/64)], codes int32 [m,12], data uint8 [m,MAX_DATA], finders found)."""
    ink = ink_mask(page, P["threshold"] if threshold is None else threshold)
    return (pack_mask(ink),) + codes_of_ink(ink, max_version, **kw)


def texts(codes: np.ndarray, data: np.ndarray) -> List[str]:
    return [e["content"] for e in qr.read_qrcodes(codes, data)]
