"""Restatement (test infrastructure, NumPy / plain Python) of lumina_ocr_aztec_layers: the Aztec pass for full-range symbols of every
size, 1 .. 32 layers.  It is built on tests/aztec_reference.py (stage 1) and is the definition the kernels must equal.  Everything is
integer.

Stage 1 is aztec_reference.decode_finder, unchanged, for every finder.  A finder it gives no row for is PENDING when its full-range
kind is valid as there (bullseye + corner mismatches <= mark_max, the mode message corrects, 2 <= total - ndata) with
12 <= layers <= max_layers; the bullseye's best frame (t0 in 128ths, k0), the rotation, the mode errors and the mismatches are kept.

Stage 2, a pending finder.  A frame is a slope t and a pitch k, both in 1024ths: P = (S << 20) // 5120, Q = P (1024 + k), and the point
(u, v), in quarter modules from the centre, is the pixel ((cx2 << 32) + Q (1024 u - t v)) >> 33, ((cy2 << 32) + Q (t u + 1024 v)) >> 33;
a pixel off the page reads clear.  The slope is not in P as it is in stage 1's frames: there the best pitches of different slopes lie
on a slant, and the middle of the ties below would be off.  N = the symbol's modules, h = N // 2.

Refinement: from (t, k) = (8 t0, 8 (k0 - |t0|)), stage 1's frame in these units, for (R, step) in (16, 8), (32, 4), (64, 2), (h, 1), R capped at h: the 81 frames
(t + step i, k + step j), i, j in -4 .. 4, are scored by their mismatches on the centre row's and column's modules at the distances
d = 8 .. R on all four arms, each at the four points a quarter module off its centre along and across the line ((4 d +- 1, +-1) on the
arm to the right); a module is dark at the even distances.  The frames with the fewest mismatches are TIED: a quarter module of
play at the radius R, so picking the smallest |k| would pick the edge of that play and the next radius would start half a module off.
With jc = (min j + max j) >> 1 and ic likewise over the tied frames, the tied frame with the smallest (|j - jc|, |i - ic|, j, i) becomes
(t, k).

Outline: of the 81 frames (t + i, k + j), i, j in -4 .. 4, with out = 0 and in > 0 the one with the smallest (ref, |j|, |i|, j, i) is
taken; there must be one.  `out` counts ink on the square at 4 h + 3 quarter modules (points every half module, corners included), `in`
the same at 4 h + 1, `ref` the mismatches of the centre row's and column's module centres at the distances 8 .. h.

From there as stage 1: the `quiet` rings are clear; module (x, y) is the ink at 4 (x - h, y - h) turned by the rotation; the codewords
are read through utils/aztec.data_bit_position, pad bits first, 10 bits wide up to 22 layers over GF(1024), 12 bits from 23 layers over
GF(4096) / 0x1069; the one block is corrected; the hull is the box of the four points (+-(4 h + 2), +-(4 h + 2)), each at its NEAREST
pixel (2^32 added before the shift: a frame one 1024th off the drawn one must not move a side), the far sides less one pixel.  Rows of
both stages are sorted together by (y0, x0, y1, x1, core root); a data row has MAX_DATA_ALL words."""
from __future__ import annotations

from typing import List, Optional, Tuple

import numpy as np

from lumina_ocr import arch
from lumina_ocr.utils import aztec as az

import aztec_reference as R1
from table_reference import ink_mask, pack_mask

P = arch.AZTEC_PARAMS
MAX_DATA = az.MAX_DATA_ALL
LEVELS = ((16, 8), (32, 4), (64, 2), (1 << 30, 1))
SPAN = 4


class Frame2:
    def __init__(self, ink: np.ndarray, box, t: int, k: int):
        self.ink, self.t, self.k = ink, t, k
        self.cx2, self.cy2 = box[0] + box[1] + 1, box[2] + box[3] + 1
        s = (box[1] - box[0] + 1) + (box[3] - box[2] + 1)
        self.q = ((s << 20) // 5120) * (1024 + k)

    def pixel(self, u, v, half=0):
        return ((self.cx2 << 32) + self.q * (1024 * u - self.t * v) + half) >> 33, ((self.cy2 << 32) + self.q * (self.t * u + 1024 * v) + half) >> 33

    def at(self, u, v) -> np.ndarray:
        u, v = np.asarray(u, np.int64), np.asarray(v, np.int64)
        px, py = self.pixel(u, v)
        h, w = self.ink.shape
        ok = (px >= 0) & (py >= 0) & (px < w) & (py < h)
        return np.where(ok, self.ink[np.clip(py, 0, h - 1), np.clip(px, 0, w - 1)], False).astype(np.int64)


def rs_correct(block: List[int], ec: int, m: int) -> Optional[Tuple[List[int], int]]:
    """aztec_reference.rs_correct with its loops over positions and coefficients as array operations (the same algorithm step for
    step, so the same answer for every block, correctable or not)."""
    exp, log = az._NP_TABLES[m]
    order = (1 << m) - 1
    n = len(block)

    def mul(a, b):
        a, b = np.asarray(a, np.int64), np.asarray(b, np.int64)
        return np.where((a != 0) & (b != 0), exp[log[a] + log[b]], 0)

    def mul_exp(a, e):
        a = np.asarray(a, np.int64)
        return np.where(a != 0, exp[log[a] + e], 0)

    def synd(blk):
        y, lx = np.zeros(ec, np.int64), np.arange(1, ec + 1, dtype=np.int64) % order
        for c in blk:
            y = mul_exp(y, lx) ^ int(c)
        return y

    S = synd(block)
    if not S.any():
        return list(block), 0
    C, Bp = np.zeros(ec + 1, np.int64), np.zeros(ec + 1, np.int64)
    C[0] = Bp[0] = 1
    L, mm, b = 0, 1, 1
    for k in range(ec):
        d = int(S[k])
        if L:
            d ^= int(np.bitwise_xor.reduce(mul(C[1:L + 1], S[k - L:k][::-1])))
        if d == 0:
            mm += 1
            continue
        T = C.copy()
        f = int(mul(d, exp[order - log[b]]))
        C[mm:] ^= mul(f, Bp[:ec + 1 - mm])
        if 2 * L <= k:
            L, Bp, b, mm = k + 1 - L, T, d, 1
        else:
            mm += 1
    if L > ec // 2:
        return None
    omega = np.zeros(L, np.int64)
    for j in range(L):
        omega[j:] ^= mul(S[:L - j], C[j])
    p = np.arange(n, dtype=np.int64)
    xi = (order - (n - 1 - p) % order) % order          # log of X^-1 at every position
    val, den, num = np.zeros(n, np.int64), np.zeros(n, np.int64), np.zeros(n, np.int64)
    for i in range(L + 1):
        e = (xi * i) % order
        val ^= mul_exp(np.full(n, C[i]), e)
        if i & 1:
            den ^= mul_exp(np.full(n, C[i]), (xi * (i - 1)) % order)
        if i < L:
            num ^= mul_exp(np.full(n, omega[i]), e)
    root = val == 0
    if int(root.sum()) != L or (den[root] == 0).any():
        return None
    out = np.array(block, np.int64)
    out[root] ^= mul(num[root], exp[order - log[den[root]]])
    if synd(out).any():
        return None
    return [int(v) for v in out], L


def read_full_kind(ink, box, mark_max: int, max_layers: int):
    """aztec_reference.read_kind for the full-range kind without its layer limit -> (mismatches, mode errors, layers, ndata, rotation,
    t0, k0) or None."""
    s = az.ring_distance(False)
    d = np.arange(-(s - 1), s)
    dx, dy = (a.ravel() for a in np.meshgrid(d, d))
    want = (np.maximum(abs(dx), abs(dy)) % 2 == 0).astype(np.int64)
    best = None
    for k in range(-12, 13, 2):
        for t in (-4, 0, 4):
            f = R1.Frame(ink, box, t, k)
            key = (int((f.at(4 * dx, 4 * dy) != want).sum()), abs(k), abs(t), k, t)
            if best is None or key < best[0]:
                best = (key, f)
    bull, f = best[0][0], best[1]
    rot = None
    for r in range(4):
        mm = 0
        for mx, my, dark in az.orientation_marks(False):
            x, y = R1.turn(mx, my, r)
            mm += int(f.at(4 * x, 4 * y)) != int(dark)
        if rot is None or mm < rot[0]:
            rot = (mm, r)
    mm, r = rot
    if bull + mm > mark_max:
        return None
    bits = []
    for mx, my in az.mode_bit_positions(False):
        x, y = R1.turn(mx, my, r)
        bits.append(int(f.at(4 * x, 4 * y)))
    words = [bits[4 * i] << 3 | bits[4 * i + 1] << 2 | bits[4 * i + 2] << 1 | bits[4 * i + 3] for i in range(len(bits) // 4)]
    got = R1.rs_correct(words, 6, 4)
    if got is None:
        return None
    words, merr = got
    v = words[0] << 12 | words[1] << 8 | words[2] << 4 | words[3]
    layers, ndata = (v >> 11) + 1, (v & 2047) + 1
    if not az.MAX_FULL_LAYERS < layers <= max_layers or az.total_words(False, layers) - ndata < 2:
        return None
    return bull + mm, merr, layers, ndata, r, f.t, f.k


def arm_points(lo: int, hi: int, offsets) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """The modules of the centre row and column at the distances lo .. hi on the four arms, each at the given (along, across) offsets in
    quarter modules -> (u, v, dark)."""
    d = np.arange(lo, hi + 1)
    us, vs, ws = [], [], []
    for a, c in offsets:
        for sx, sy in ((1, 0), (-1, 0), (0, 1), (0, -1)):
            us.append(sx * (4 * d + a) - sy * c)
            vs.append(sy * (4 * d + a) + sx * c)
            ws.append((d % 2 == 0).astype(np.int64))
    return np.concatenate(us), np.concatenate(vs), np.concatenate(ws)


def refine(ink, box, h: int, t0: int, k0: int):
    """-> (reference-line mismatches, the frame) or None when every frame has ink outside the outline."""
    t, k = 8 * t0, 8 * (k0 - abs(t0))
    span = np.arange(-SPAN, SPAN + 1)
    jj, ii = (a.ravel() for a in np.meshgrid(span, span, indexing="ij"))
    for radius, step in LEVELS:
        u, v, want = arm_points(8, min(radius, h), ((-1, -1), (-1, 1), (1, -1), (1, 1)))
        mism = np.array([int((Frame2(ink, box, t + step * i, k + step * j).at(u, v) != want).sum()) for j, i in zip(jj, ii)])
        tied = mism == mism.min()
        jc, ic = (int(jj[tied].min()) + int(jj[tied].max())) >> 1, (int(ii[tied].min()) + int(ii[tied].max())) >> 1
        _, _, j, i = min((abs(int(j) - jc), abs(int(i) - ic), int(j), int(i)) for j, i in zip(jj[tied], ii[tied]))
        t, k = t + step * i, k + step * j
    ou, ov = R1.square_points(4 * h + 3)
    iu, iv = R1.square_points(4 * h + 1)
    ru, rv, rwant = arm_points(8, h, ((0, 0),))
    best = None
    for j, i in zip(jj, ii):
        f = Frame2(ink, box, t + int(i), k + int(j))
        if f.at(ou, ov).any() or not f.at(iu, iv).any():
            continue
        key = (int((f.at(ru, rv) != rwant).sum()), abs(int(j)), abs(int(i)), int(j), int(i))
        if best is None or key < best[0]:
            best = (key, f)
    if best is None:
        return None
    return best[0][0], best[1]


def decode_pending(ink, box, quiet: int, pending):
    """-> (the output row, data codewords) or None."""
    mism, merr, layers, ndata, r, t0, k0 = pending
    n = az.modules(False, layers)
    h = n // 2
    got = refine(ink, box, h, t0, k0)
    if got is None:
        return None
    ref, f = got
    for q in range(1, quiet + 1):
        a = np.arange(-(h + q), h + q + 1)
        e = np.full(len(a), h + q)
        if f.at(4 * np.concatenate([a, a, -e, e]), 4 * np.concatenate([-e, e, a, a])).any():
            return None
    ys, xs = np.mgrid[0:n, 0:n]
    tx, ty = R1.turn(xs - h, ys - h, r)
    m = f.at(4 * tx, 4 * ty)
    w = az.word_width(layers)
    total, pad = az.total_words(False, layers), az.total_bits(False, layers) % w
    pos = np.array([az.data_bit_position(False, layers, pad + b) for b in range(total * w)])
    bits = m[pos[:, 1], pos[:, 0]].reshape(total, w)
    words = [int(v) for v in (bits << np.arange(w - 1, -1, -1)).sum(axis=1)]
    got = rs_correct(words, total - ndata, w)
    if got is None:
        return None
    e = 4 * h + 2
    px, py = f.pixel(np.array([-e, e, -e, e]), np.array([-e, -e, e, e]), 1 << 32)
    H, W = ink.shape
    cl = lambda v, hi: max(0, min(hi, int(v)))
    hull = (cl(px.min(), W - 1), cl(py.min(), H - 1), cl(px.max() - 1, W - 1), cl(py.max() - 1, H - 1))
    return hull + (layers, 0, w, ndata, got[1], r, merr, mism + ref), got[0][:ndata]


def codes_of_ink(ink: np.ndarray, max_layers: int, min_module=None, max_module=None, quiet=None, centre_tol=None, ring_tol=None, mark_max=None,
                 max_finders=None):
    """bool [H,W] -> (codes int32 [m,12], data uint16 [m,MAX_DATA], finders found)."""
    g = lambda k, v: P[k] if v is None else v
    finders = R1.find_finders(ink, g("min_module", min_module), g("max_module", max_module), g("centre_tol", centre_tol), g("ring_tol", ring_tol))
    found = []
    if len(finders) <= g("max_finders", max_finders):
        for root, box in finders:
            got = R1.decode_finder(ink, box, g("quiet", quiet), g("mark_max", mark_max))
            if got is None and max_layers > az.MAX_FULL_LAYERS:
                pending = read_full_kind(ink, box, g("mark_max", mark_max), max_layers)
                if pending is not None:
                    got = decode_pending(ink, box, g("quiet", quiet), pending)
            if got is not None:
                row, data = got
                found.append(((row[1], row[0], row[3], row[2], root), row, data))
    found.sort(key=lambda t: t[0])
    codes = np.array([t[1] for t in found], np.int32).reshape(-1, 12)
    data = np.zeros((len(found), MAX_DATA), np.uint16)
    for i, t in enumerate(found):
        data[i, :len(t[2])] = t[2]
    return codes, data, len(finders)


def aztec_layers(page: np.ndarray, max_layers: int = az.MAX_LAYERS_ALL, threshold: int = None, **kw):
    """uint8 [H,W,3] -> (mask uint64 [H, ceil(W/64)], codes int32 [m,12], data uint16 [m,MAX_DATA], finders found)."""
    ink = ink_mask(page, P["threshold"] if threshold is None else threshold)
    return (pack_mask(ink),) + codes_of_ink(ink, max_layers, **kw)


def texts(codes: np.ndarray, data: np.ndarray, max_layers: int = az.MAX_LAYERS_ALL) -> List[str]:
    return [e["content"] for e in az.read_aztec(codes, data, max_layers=max_layers)]
