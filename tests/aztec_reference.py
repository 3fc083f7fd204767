"""Restatement (test infrastructure, NumPy / plain Python) of the Aztec pass that lumina_ocr_aztec runs on the device.  It shares the
tables and the geometry of lumina_ocr/utils/aztec.py with the product code and nothing else; it is the definition the kernels must
equal.  Everything is integer.

Components: the 8-connected components of the ink (runs and roots as tests/mark_reference.py), each with its box and its ink area.

Finders, in the order of the roots: the CORE is a root whose box (w, h) has min_module <= w, h <= max_module, 4 |w - h| <= max(w, h)
and 4 area >= 3 w h.  On its centre row (y0 + y1) >> 1 the run that holds x = (x0 + x1) >> 1 belongs to the core, and the runs before
and behind it in that row both belong to one other component, the RING, whose box (w5, h5) has 16 |5 w - w5| <= ring_tol w5,
5 * 16 |xsum5 - xsum| <= 2 centre_tol w5 (xsum = x0 + x1), the same in y, and 12 w5 h5 <= 25 area5 <= 20 w5 h5.  A page with more than
max_finders finders is not read.

Frame: the centre is (cx2, cy2) = (x0 + x1 + 1, y0 + y1 + 1) of the ring's box in doubled pixels, S = w5 + h5 (ten modules).  A frame
is a slope t (128ths) and a pitch step k (128ths of the pitch): P = (S << 20) // (5 (128 + |t|)), Q = P (256 + 2 k), and the point
(u, v), in QUARTER modules from the centre, is the pixel ((cx2 << 30) + Q (128 u - t v)) >> 31, ((cy2 << 30) + Q (t u + 128 v)) >> 31;
a negative coordinate or a pixel off the page reads clear.

Kind: for compact (s = 5) and full (s = 7) the frame of k in -12, -10 .. 12 and t in -4, 0, 4 with the smallest (bullseye mismatches,
|k|, |t|, k, t) is taken: the modules at Chebyshev distance < s are dark at the even distances.  The rotation r (quarter turns
clockwise; a symbol offset turns by (x, y) -> (-y, x) r times) is the one with the fewest mismatches in the twelve modules at the
mode ring's corners, ties to the smaller r.  The mode message is read round the ring and corrected over GF(16).  A kind is VALID when
bullseye + corner mismatches <= mark_max, the message corrects, layers is in scope and 2 <= total - ndata; the valid kind with the
smallest (mismatches, mode errors, full) is taken.

Refinement: N = the symbol's modules, h = N // 2.  Of the frames k in -12 .. 12, t in -6 .. 6 the one with the smallest (out > 0, ref,
-in, |k|, |t|, k, t) is taken and must have out = 0: `out` counts ink on the square at 4 h + 3 quarter modules (points every half
module, corners included), `in` the same at 4 h + 1, and `ref` (full symbols) the mismatches of the centre row's and column's modules
at distances 8 .. h, dark at the even ones.

The `quiet` rings of modules round the symbol must be clear.  Module (x, y) is the ink at the point 4 (x - h, y - h) turned by r;
the bit stream is read through utils/aztec.data_bit_position, total_bits % width pad bits first, and the one block is corrected
(syndromes, Berlekamp-Massey, Chien, Forney over the width's field, roots a^1 ...); the syndromes are recomputed: more than ec // 2
errors drop the finder.  The hull is the box of the four points (+-(4 h + 2), +-(4 h + 2)), the far sides less one pixel.

A row is x0, y0, x1, y1, layers, compact, width, ndata, corrected errors, rotation, mode errors, mismatches (bullseye + corners +
ref); rows are sorted by (y0, x0, y1, x1, core root)."""
from __future__ import annotations

from typing import List, Optional, Tuple

import numpy as np

from lumina_ocr import arch
from lumina_ocr.utils import aztec as az

from mark_reference import run_roots, runs_of
from table_reference import ink_mask, pack_mask

P = arch.AZTEC_PARAMS
MAX_DATA = az.MAX_DATA


def find_finders(ink: np.ndarray, min_module: int, max_module: int, centre_tol: int, ring_tol: int) -> List[Tuple[int, Tuple[int, int, int, int]]]:
    """-> [(core root, the ring's box x0, x1, y0, y1)] in the order of the roots."""
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
    first = np.searchsorted(row, np.arange(ink.shape[0] + 1))
    out = []
    for r in np.nonzero(root == np.arange(n))[0]:
        w, h = int(x1[r] - x0[r] + 1), int(y1[r] - row[r] + 1)
        if not (min_module <= w <= max_module and min_module <= h <= max_module and 4 * abs(w - h) <= max(w, h) and 4 * int(area[r]) >= 3 * w * h):
            continue
        cy, cx = int(row[r] + y1[r]) >> 1, int(x0[r] + x1[r]) >> 1
        lo, hi = int(first[cy]), int(first[cy + 1])
        j = next((i for i in range(lo, hi) if s[i] <= cx <= e[i]), -1)
        if j < 0 or root[j] != r or j - 1 < lo or j + 1 >= hi:
            continue
        g = int(root[j - 1])
        if g != root[j + 1] or g == r:
            continue
        w5, h5 = int(x1[g] - x0[g] + 1), int(y1[g] - row[g] + 1)
        if 16 * abs(5 * w - w5) > ring_tol * w5 or 16 * abs(5 * h - h5) > ring_tol * h5:
            continue
        if 80 * abs(int(x0[g] + x1[g]) - int(x0[r] + x1[r])) > 2 * centre_tol * w5 or 80 * abs(int(row[g] + y1[g]) - int(row[r] + y1[r])) > 2 * centre_tol * h5:
            continue
        if not 12 * w5 * h5 <= 25 * int(area[g]) <= 20 * w5 * h5:
            continue
        out.append((int(r), (int(x0[g]), int(x1[g]), int(row[g]), int(y1[g]))))
    return out


def turn(x, y, r: int):
    for _ in range(r):
        x, y = -y, x
    return x, y


class Frame:
    def __init__(self, ink: np.ndarray, box, t: int, k: int):
        self.ink, self.t, self.k = ink, t, k
        self.cx2, self.cy2 = box[0] + box[1] + 1, box[2] + box[3] + 1
        s = (box[1] - box[0] + 1) + (box[3] - box[2] + 1)
        self.q = ((s << 20) // (5 * (128 + abs(t)))) * (256 + 2 * k)

    def pixel(self, u, v):
        return ((self.cx2 << 30) + self.q * (128 * u - self.t * v)) >> 31, ((self.cy2 << 30) + self.q * (self.t * u + 128 * v)) >> 31

    def at(self, u, v) -> np.ndarray:
        """Points in quarter modules (arrays or ints) -> 0 / 1."""
        u, v = np.asarray(u, np.int64), np.asarray(v, np.int64)
        px, py = self.pixel(u, v)
        h, w = self.ink.shape
        ok = (px >= 0) & (py >= 0) & (px < w) & (py < h)
        return np.where(ok, self.ink[np.clip(py, 0, h - 1), np.clip(px, 0, w - 1)], False).astype(np.int64)


def square_points(d: int) -> Tuple[np.ndarray, np.ndarray]:
    """The points of the square at d quarter modules, every half module, corners included (on the two horizontal sides and again
    on the two vertical ones)."""
    a = np.arange(-d, d + 1, 2)
    f = np.full(len(a), d)
    return np.concatenate([a, a, -f, f]), np.concatenate([-f, f, a, a])


def rs_correct(block: List[int], ec: int, m: int) -> Optional[Tuple[List[int], int]]:
    """A block (data then check words, the first the highest power) -> (corrected block, errors) or None.  Roots a^1 .. a^ec."""
    exp, log = az.gf_tables(m) if m not in az._TABLES else az._TABLES[m]
    order = (1 << m) - 1
    mul = lambda a, b: exp[log[a] + log[b]] if a and b else 0
    n = len(block)

    def ev(poly_asc, x):
        y = 0
        for c in reversed(poly_asc):
            y = mul(y, x) ^ c
        return y

    synd = lambda blk: [ev(blk[::-1], exp[k + 1]) for k in range(ec)]
    S = synd(block)
    if not any(S):
        return list(block), 0
    C, Bp, L, mm, b = [1] + [0] * ec, [1] + [0] * ec, 0, 1, 1
    for k in range(ec):
        d = S[k]
        for i in range(1, L + 1):
            d ^= mul(C[i], S[k - i])
        if d == 0:
            mm += 1
            continue
        T = list(C)
        f = mul(d, exp[order - log[b]])
        for i in range(ec + 1 - mm):
            C[i + mm] ^= mul(f, Bp[i])
        if 2 * L <= k:
            L, Bp, b, mm = k + 1 - L, T, d, 1
        else:
            mm += 1
    if L > ec // 2:
        return None
    omega = [0] * L
    for i in range(L):
        for j in range(i + 1):
            omega[i] ^= mul(S[i - j], C[j])
    out, roots = list(block), 0
    for p in range(n):
        e = (n - 1 - p) % order
        xi = exp[(order - e) % order]
        if ev(C[:L + 1], xi):
            continue
        roots += 1
        den = 0
        for i in range(1, L + 1, 2):
            den ^= mul(C[i], exp[(log[xi] * (i - 1)) % order])
        if den == 0:
            return None
        out[p] ^= mul(ev(omega, xi), exp[order - log[den]])
    if roots != L or any(synd(out)):
        return None
    return out, L


def read_kind(ink, box, compact: bool, mark_max: int):
    """-> (mismatches, mode errors, layers, ndata, rotation) or None."""
    s = az.ring_distance(compact)
    d = np.arange(-(s - 1), s)
    dx, dy = (a.ravel() for a in np.meshgrid(d, d))
    want = (np.maximum(abs(dx), abs(dy)) % 2 == 0).astype(np.int64)
    best = None
    for k in range(-12, 13, 2):
        for t in (-4, 0, 4):
            f = Frame(ink, box, t, k)
            key = (int((f.at(4 * dx, 4 * dy) != want).sum()), abs(k), abs(t), k, t)
            if best is None or key < best[0]:
                best = (key, f)
    bull, f = best[0][0], best[1]
    marks = az.orientation_marks(compact)
    rot = None
    for r in range(4):
        mm = 0
        for mx, my, dark in marks:
            x, y = turn(mx, my, r)
            mm += int(f.at(4 * x, 4 * y)) != int(dark)
        if rot is None or mm < rot[0]:
            rot = (mm, r)
    mm, r = rot
    if bull + mm > mark_max:
        return None
    bits = []
    for mx, my in az.mode_bit_positions(compact):
        x, y = turn(mx, my, r)
        bits.append(int(f.at(4 * x, 4 * y)))
    words = [bits[4 * i] << 3 | bits[4 * i + 1] << 2 | bits[4 * i + 2] << 1 | bits[4 * i + 3] for i in range(len(bits) // 4)]
    got = rs_correct(words, 5 if compact else 6, 4)
    if got is None:
        return None
    words, merr = got
    if compact:
        v = words[0] << 4 | words[1]
        layers, ndata = (v >> 6) + 1, (v & 63) + 1
    else:
        v = words[0] << 12 | words[1] << 8 | words[2] << 4 | words[3]
        layers, ndata = (v >> 11) + 1, (v & 2047) + 1
        if layers > az.MAX_FULL_LAYERS:
            return None
    if az.total_words(compact, layers) - ndata < 2:
        return None
    return bull + mm, merr, layers, ndata, r


def decode_finder(ink, box, quiet: int, mark_max: int):
    """-> (the output row, data codewords) or None."""
    kinds = []
    for compact in (True, False):
        got = read_kind(ink, box, compact, mark_max)
        if got is not None:
            kinds.append((got[0], got[1], int(not compact)) + got[2:])
    if not kinds:
        return None
    mism, merr, full, layers, ndata, r = min(kinds)
    compact = not full
    n = az.modules(compact, layers)
    h = n // 2
    ou, ov = square_points(4 * h + 3)
    iu, iv = square_points(4 * h + 1)
    d = np.arange(8, h + 1)
    z = np.zeros(len(d), np.int64)
    ru, rv = 4 * np.concatenate([d, -d, z, z]), 4 * np.concatenate([z, z, d, -d])
    rwant = np.tile((d % 2 == 0).astype(np.int64), 4)
    best = None
    for k in range(-12, 13):
        for t in range(-6, 7):
            f = Frame(ink, box, t, k)
            out = int(f.at(ou, ov).sum())
            ref = 0 if compact else int((f.at(ru, rv) != rwant).sum())
            key = (int(out > 0), ref, -int(f.at(iu, iv).sum()), abs(k), abs(t), k, t)
            if best is None or key < best[0]:
                best = (key, f)
    if best[0][0]:
        return None
    ref, f = best[0][1], best[1]
    for q in range(1, quiet + 1):
        a = np.arange(-(h + q), h + q + 1)
        e = np.full(len(a), h + q)
        if f.at(4 * np.concatenate([a, a, -e, e]), 4 * np.concatenate([-e, e, a, a])).any():
            return None
    ys, xs = np.mgrid[0:n, 0:n]
    tx, ty = turn(xs - h, ys - h, r)
    m = f.at(4 * tx, 4 * ty)
    w = az.word_width(layers)
    total, pad = az.total_words(compact, layers), az.total_bits(compact, layers) % w
    words = []
    for j in range(total):
        v = 0
        for b in range(w):
            x, y = az.data_bit_position(compact, layers, pad + j * w + b)
            v = (v << 1) | int(m[y, x])
        words.append(v)
    got = rs_correct(words, total - ndata, w)
    if got is None:
        return None
    e = 4 * h + 2
    px, py = f.pixel(np.array([-e, e, -e, e]), np.array([-e, -e, e, e]))
    H, W = ink.shape
    cl = lambda v, hi: max(0, min(hi, int(v)))
    hull = (cl(px.min(), W - 1), cl(py.min(), H - 1), cl(px.max() - 1, W - 1), cl(py.max() - 1, H - 1))
    return hull + (layers, int(compact), w, ndata, got[1], r, merr, mism + ref), got[0][:ndata]


def codes_of_ink(ink: np.ndarray, min_module=None, max_module=None, quiet=None, centre_tol=None, ring_tol=None, mark_max=None, max_finders=None):
    """bool [H,W] -> (codes int32 [m,12], data int32 [m,MAX_DATA], finders found)."""
    g = lambda k, v: P[k] if v is None else v
    finders = find_finders(ink, g("min_module", min_module), g("max_module", max_module), g("centre_tol", centre_tol), g("ring_tol", ring_tol))
    found = []
    if len(finders) <= g("max_finders", max_finders):
        for root, box in finders:
            got = decode_finder(ink, box, g("quiet", quiet), g("mark_max", mark_max))
            if got is not None:
                row, data = got
                found.append(((row[1], row[0], row[3], row[2], root), row, data))
    found.sort(key=lambda t: t[0])
    codes = np.array([t[1] for t in found], np.int32).reshape(-1, 12)
    data = np.zeros((len(found), MAX_DATA), np.int32)
    for i, t in enumerate(found):
        data[i, :len(t[2])] = t[2]
    return codes, data, len(finders)


def aztec(page: np.ndarray, threshold: int = None, **kw):
    """uint8 [H,W,3] -> (mask uint64 [H, ceil(W/64)], codes int32 [m,12], data int32 [m,MAX_DATA], finders found)."""
    ink = ink_mask(page, P["threshold"] if threshold is None else threshold)
    return (pack_mask(ink),) + codes_of_ink(ink, **kw)


def texts(codes: np.ndarray, data: np.ndarray) -> List[str]:
    return [e["content"] for e in az.read_aztec(codes, data)]
