"""The words of a recognised line, restated in numpy from the definition of lumina_ocr_ctc_decode_words (include/lumina_ocr.h) — what
the device kernel is compared against for EQUALITY.  Nothing here looks at the kernel: it is the definition, one line at a time.

  kept character  a step t with idx[t] != 0 and idx[t] != idx[t-1]; its run ends at the last consecutive step with the same class
  word            a maximal run of kept characters whose class is not space_id (space_id < 0: the whole line, when it is not empty)
  columns         c0 = min(4 t_first, wc), c1 = max(min(4 (run end of the last character + 1), wc), c0); flipped: [wc - c1, wc - c0)
  quad            corners in the crop's order (rotated by one when 4 ch^2 >= 9 cw^2), top edge P0 -> P1 and bottom edge P3 -> P2 at
                  c / wc, integers, round half away from zero; the points go back to the line quad's own corner order
  score           fp32 sum of the kept probabilities of the word's characters in time order, divided by their count
"""
from __future__ import annotations

import numpy as np

T = 80
MAX_WORDS = 40


def round_div(a: int, c: int, wc: int) -> int:
    """round half away from zero of a * c / wc, in exact integers (wc > 0)"""
    num = a * c
    mag = (2 * abs(num) + wc) // (2 * wc)
    return -mag if num < 0 else mag


def crop_corners(quad):
    """-> (the four corners in the order the crop used them, 1 when that is the line's order rotated by one else 0)"""
    p = [(int(quad[2 * k]), int(quad[2 * k + 1])) for k in range(4)]
    d2 = lambda a, b: (p[a][0] - p[b][0]) ** 2 + (p[a][1] - p[b][1]) ** 2
    cw2 = max(d2(1, 0), d2(2, 3))
    ch2 = max(d2(3, 0), d2(2, 1))
    if 4 * ch2 >= 9 * cw2:
        return [p[1], p[2], p[3], p[0]], 1
    return p, 0


def kept_characters(row):
    """-> [(first step, last step of the run, class)] of the kept characters of one line"""
    out = []
    prev = -1
    n = len(row)
    for t in range(n):
        k = int(row[t])
        if k != 0 and k != prev:
            e = t
            while e + 1 < n and int(row[e + 1]) == k:
                e += 1
            out.append((t, e, k))
        prev = k
    return out


def mean_fp32(ps):
    s = np.float32(0.0)
    for p in ps:
        s = np.float32(s + np.float32(p))
    return np.float32(s / np.float32(len(ps))) if len(ps) else np.float32(0.0)


def line_words(row, prow, quad, wc, flip, space_id):
    """One line -> (text ids, score, [(first character, count, quad 8 ints, score)])"""
    kept = kept_characters(row)
    text = [k for _, _, k in kept]
    score = mean_fp32([prow[t] for t, _, _ in kept])
    words = []
    wc = int(wc)
    if wc <= 0:
        return text, score, words
    groups, cur = [], []
    for i, (_, _, k) in enumerate(kept):
        if space_id >= 0 and k == space_id:
            if cur:
                groups.append(cur)
            cur = []
        else:
            cur.append(i)
    if cur:
        groups.append(cur)
    P, rot = crop_corners(quad)
    for g in groups:
        c0 = min(4 * kept[g[0]][0], wc)
        c1 = min(4 * (kept[g[-1]][1] + 1), wc)
        c1 = max(c1, c0)
        if flip:
            c0, c1 = wc - c1, wc - c0

        def top(c):
            return tuple(P[0][d] + round_div(P[1][d] - P[0][d], c, wc) for d in (0, 1))

        def bottom(c):
            return tuple(P[3][d] + round_div(P[2][d] - P[3][d], c, wc) for d in (0, 1))

        pts = [top(c0), top(c1), bottom(c1), bottom(c0)]   # on the side of crop corner 0, 1, 2, 3
        out = [None] * 4
        for k in range(4):
            out[(k + rot) % 4] = pts[k]                    # crop corner k is line corner (k + rot) % 4
        q = [v for pt in out for v in pt]
        words.append((g[0], len(g), q, mean_fp32([prow[kept[i][0]] for i in g])))
    return text, score, words[:MAX_WORDS]


def decode_words(idx, prob, quads, widths, flip=None, space_id=-1):
    """idx int [n, T], prob float32 [n, T], quads int [n, 8], widths int [n], flip int [n] or None ->
    dict(text int32 [n, T] (-1 padded), len int32 [n], score float32 [n], word_quads int32 [n, 40, 8], word_spans int32 [n, 40, 2],
    word_scores float32 [n, 40], word_counts int32 [n]); rows past a line's count are zero."""
    idx = np.asarray(idx)
    prob = np.asarray(prob, np.float32)
    n, t = idx.shape
    out = dict(text=np.full((n, t), -1, np.int32), len=np.zeros(n, np.int32), score=np.zeros(n, np.float32),
               word_quads=np.zeros((n, MAX_WORDS, 8), np.int32), word_spans=np.zeros((n, MAX_WORDS, 2), np.int32),
               word_scores=np.zeros((n, MAX_WORDS), np.float32), word_counts=np.zeros(n, np.int32))
    for i in range(n):
        text, score, words = line_words(idx[i], prob[i], quads[i], widths[i], bool(flip[i]) if flip is not None else False, space_id)
        out["text"][i, :len(text)] = text
        out["len"][i] = len(text)
        out["score"][i] = score
        out["word_counts"][i] = len(words)
        for w, (first, count, q, s) in enumerate(words):
            out["word_quads"][i, w] = q
            out["word_spans"][i, w] = (first, count)
            out["word_scores"][i, w] = s
    return out


def crop_width(quad, ch=32, cw=320):
    """The valid width lumina_ocr_rec_crop gives the crop of a quad (crop_kernel: ceil(ch * sqrt(cw2 / ch2)) clamped to 1..cw in
    float64; 0 for a degenerate quad)."""
    p = [(int(quad[2 * k]), int(quad[2 * k + 1])) for k in range(4)]
    d2 = lambda a, b: (p[a][0] - p[b][0]) ** 2 + (p[a][1] - p[b][1]) ** 2
    cw2 = max(d2(1, 0), d2(2, 3))
    ch2 = max(d2(3, 0), d2(2, 1))
    if 4 * ch2 >= 9 * cw2:
        cw2, ch2 = ch2, cw2
    if ch2 == 0 or cw2 == 0:
        return 0
    return int(min(max(int(np.ceil(np.float64(ch) * np.sqrt(np.float64(cw2) / np.float64(ch2)))), 1), cw))
