"""CPU restatement of the text-line orientation classifier (test infrastructure; oracle/ is left as it is and only read):
  * the 48 x 192 classifier crop and the turned recognition crop in numpy float32, in the crop kernel's operation order
    (csrc/dbpost.hip crop_kernel): bit-exact;
  * the backbone in torch-CPU through oracle.nets' conv_bn_act / _rb (the arithmetic definition of the det / rec networks);
  * the head in numpy float32 in the head kernel's fixed order (ops.hip cls_head_kernel);
  * "oracle pipeline + cls": oracle/pipeline.py's run_pages with the classifier between the boxes and the recogniser."""
from __future__ import annotations

import numpy as np
import torch
import torch.nn.functional as F

from lumina_ocr import arch, synth
from oracle import dbpost, nets, preprocess
from oracle.nets import _rb, conv_bn_act

F32 = np.float32


def crop_geometry(box8):
    """crop_kernel's corner handling: -> (corners int64 [4, 2] after the vertical-box rotation, cw2, ch2)."""
    p = np.asarray(box8, np.int64).reshape(4, 2).copy()

    def d2(a, b):
        d = p[a] - p[b]
        return int(d[0] * d[0] + d[1] * d[1])
    cw2, ch2 = max(d2(1, 0), d2(2, 3)), max(d2(3, 0), d2(2, 1))
    if 4 * ch2 >= 9 * cw2:
        p = p[[1, 2, 3, 0]]
        cw2, ch2 = ch2, cw2
    return p, cw2, ch2


def crop_width(box8, h: int = arch.CLS_H, cap: int = arch.CLS_W) -> int:
    """min(cap, ceil(h * ratio)), at least 1; 0 for a degenerate box."""
    _, cw2, ch2 = crop_geometry(box8)
    if cw2 == 0 or ch2 == 0:
        return 0
    ratio = np.sqrt(np.float64(cw2) / np.float64(ch2))
    return int(min(max(int(np.ceil(np.float64(h) * ratio)), 1), cap))


def crop(page: np.ndarray, box8, h: int = arch.CLS_H, w: int = arch.CLS_W, flip: bool = False):
    """page uint8 [H, W, 3], one quad -> (crop uint8 [h, w, 3], valid width).  flip: the 180-degree turn within the valid width."""
    H, W, _ = page.shape
    p, _, _ = crop_geometry(box8)
    wc = crop_width(box8, h, w)
    out = np.zeros((h, w, 3), np.uint8)
    if wc == 0:
        return out, 0
    tlx, tly = F32(p[0, 0]), F32(p[0, 1])
    ex, ey = F32(p[1, 0] - p[0, 0]), F32(p[1, 1] - p[0, 1])
    fx, fy = F32(p[3, 0] - p[0, 0]), F32(p[3, 1] - p[0, 1])
    i, j = np.mgrid[0:h, 0:wc]
    if flip:
        i, j = h - 1 - i, wc - 1 - j
    u = (j.astype(F32) + F32(0.5)) / F32(wc)
    v = (i.astype(F32) + F32(0.5)) / F32(h)
    sx = (tlx + u * ex) + v * fx
    sy = (tly + u * ey) + v * fy
    x0f, y0f = np.floor(sx), np.floor(sy)
    ax, ay = sx - x0f, sy - y0f
    x0, y0 = x0f.astype(np.int64), y0f.astype(np.int64)
    x1, y1 = np.clip(x0 + 1, 0, W - 1), np.clip(y0 + 1, 0, H - 1)
    x0, y0 = np.clip(x0, 0, W - 1), np.clip(y0, 0, H - 1)
    bx, by = F32(1.0) - ax, F32(1.0) - ay
    pg = page.astype(F32)
    for c in range(3):
        top = bx * pg[y0, x0, c] + ax * pg[y0, x1, c]
        bot = bx * pg[y1, x0, c] + ax * pg[y1, x1, c]
        out[:, :wc, c] = np.clip(np.rint(by * top + ay * bot), 0, 255).astype(np.uint8)
    return out, wc


def turn(crop_u8: np.ndarray, wc: int) -> np.ndarray:
    """The 180-degree turn of a crop within its valid width: out[i][j] = crop[H-1-i][wc-1-j] for j < wc, padding unchanged."""
    out = crop_u8.copy()
    out[:, :wc] = crop_u8[::-1, :wc][:, ::-1]
    return out


def normalize(crops_u8: np.ndarray, widths, mode: str = "bf16") -> torch.Tensor:
    """[N,48,192,3] u8 -> [N,3,48,192]; columns >= a crop's width are 0 in normalised space (the stem's valid_w_per_img)."""
    x = nets.rec_normalize(crops_u8, mode)
    for i, wv in enumerate(widths):
        x[i, :, :, int(wv):] = 0
    return x


def cls_block(wd, x, b: dict, mode: str = "bf16"):
    """Block cls.b{i} of arch.cls_block_table(): nets.rec_block's arithmetic under the classifier's names and strides."""
    p = f"cls.b{b['idx']}"
    y = conv_bn_act(x, wd, p + ".expand", 1, b["act"], mode=mode)
    y = conv_bn_act(y, wd, p + ".dw", (b["stride_h"], 1), b["act"], mode=mode, groups=b["exp"])
    if b["se"]:
        s = _rb(y.mean(dim=(2, 3), keepdim=True), mode)
        s = conv_bn_act(s, wd, p + ".se1", 1, "relu", mode=mode)
        s = conv_bn_act(s, wd, p + ".se2", 1, "hsigmoid", mode=mode)
        y = _rb(y * s, mode)
    return conv_bn_act(y, wd, p + ".project", 1, "none", residual=x if b["res"] else None, mode=mode)


def cls_conv1(wd, x, mode: str = "bf16"):
    """Normalised crops [N,3,48,192] (columns past a crop's width already 0) -> the stem [N,8,24,96]."""
    return conv_bn_act(x, wd, "cls.conv1", 2, "hswish", mode=mode)


def cls_conv2(wd, x, mode: str = "bf16"):
    """cls.b10 [N,32,2,96] -> [N,200,2,96]: 1x1, hswish."""
    return conv_bn_act(x, wd, "cls.conv2", 1, "hswish", mode=mode)


def cls_pool(x):
    """cls.conv2 [N,200,2,96] -> tap "cls.feat" [N,200,1,48]: the 2x2 max pool."""
    return F.max_pool2d(x, 2, 2)


# The inputs of the per-layer grading (tests/test_gpu_layer_parity.py): valid widths the stem masks by (1 and 191 / 192 are the mask's
# edges), cycled over the crops, and 48 x 192 crops with real structure.
LAYER_WIDTHS = [1, 8, 31, 77, 150, 191, 192]


def layer_crops(n: int, seed: int = 31):
    """-> (crops uint8 [n,48,192,3], widths int32 [n]).  Crop 0 is uniform noise (every tap of every depthwise window matters); the
    others are crop() of the rendered lines' boxes of synthetic pages (no detector needed), with a margin that varies per line.  The
    widths are LAYER_WIDTHS cycled from 191 on (the noise crop keeps nearly all its columns), not the crops' own: the pixels past a
    width stay in the crop and the stem must zero them."""
    rng = np.random.default_rng(seed)
    crops = [rng.integers(0, 256, (arch.CLS_H, arch.CLS_W, 3), dtype=np.uint8)]
    page_seed = seed
    while len(crops) < n:
        page, lines = synth.synth_page(480, 640, page_seed, n_lines=8)
        page_seed += 1
        for g in lines:
            x0, y0, x1, y1 = g["box"]
            m = 1 + len(crops) % 4
            c, wc = crop(page, [x0 - m, y0 - m, x1 + m, y0 - m, x1 + m, y1 + m, x0 - m, y1 + m])
            if wc > 0 and len(crops) < n:
                crops.append(c)
    widths = np.array([LAYER_WIDTHS[(i + 5) % len(LAYER_WIDTHS)] for i in range(n)], np.int32)
    return np.stack(crops), widths


def backbone(wd, x: torch.Tensor, mode: str = "bf16", taps=None) -> np.ndarray:
    """Normalised crops [N,3,48,192] -> pooled features float32 [N, 48, 200] (tap "cls.feat"); taps: NHWC per layer."""
    def tap(name, t):
        if taps is not None:
            taps[name] = t.permute(0, 2, 3, 1).contiguous().numpy()

    with torch.no_grad():
        x = conv_bn_act(x, wd, "cls.conv1", 2, "hswish", mode=mode); tap("cls.conv1", x)
        for b in arch.cls_block_table():
            x = cls_block(wd, x, b, mode); tap(f"cls.b{b['idx']}", x)
        x = conv_bn_act(x, wd, "cls.conv2", 1, "hswish", mode=mode); tap("cls.conv2", x)
        x = F.max_pool2d(x, 2, 2); tap("cls.feat", x)
    return x[:, :, 0, :].permute(0, 2, 1).contiguous().numpy()


def head(wd, feat: np.ndarray, thresh: float = arch.CLS_THRESH):
    """feat float32 [N, P, C] -> (label int32 [N], score float32 [N], flip int32 [N], logits float32 [N, 2]): the head kernel's
    order — the P positions summed in position order and divided by P, the FC summed in channel order and the bias added last,
    every operation one fp32 rounding; score = 1 / (1 + exp(-|logit1 - logit0|))."""
    feat = np.asarray(feat, F32)
    n, npos, c = feat.shape
    s = np.zeros((n, c), F32)
    for q in range(npos):
        s = s + feat[:, q, :]
    mean = s / F32(npos)
    fw, fb = np.asarray(wd["cls.fc.w"], F32), np.asarray(wd["cls.fc.b"], F32)
    acc = np.zeros((n, 2), F32)
    for k in range(c):
        acc = acc + fw[None, :, k] * mean[:, k:k + 1]
    logits = acc + fb[None, :]
    label = (logits[:, 1] > logits[:, 0]).astype(np.int32)
    d = np.abs(logits[:, 1] - logits[:, 0])
    score = (F32(1.0) / (F32(1.0) + np.exp(-d))).astype(F32)
    flip = ((label == 1) & (score > F32(thresh))).astype(np.int32)
    return label, score, flip, logits


def classify(wd, crops_u8: np.ndarray, widths, thresh: float = arch.CLS_THRESH, mode: str = "bf16", taps=None):
    """48 x 192 crops -> (label, score, flip, logits)."""
    feat = backbone(wd, normalize(crops_u8, widths, mode), mode, taps)
    return head(wd, feat, thresh)


def run_pages(det_w, rec_w, cls_w, pages_u8: np.ndarray, charset, post: dict = None, thresh: float = arch.CLS_THRESH, mode: str = "bf16"):
    """oracle/pipeline.py run_pages (enhance on, max_dim 2000) with the classifier between the boxes and the recogniser:
    -> list per page of dict(quads, texts, scores, labels, cls_scores, flips)."""
    processed = np.stack([preprocess.enhance_sharpness(preprocess.enhance_contrast(preprocess.resize_if_needed(pg, 2000), 1.2), 1.1)
                          for pg in pages_u8])
    b, h, w, _ = processed.shape
    bits = arch.f32_to_bf16_bits(nets.det_forward(det_w, processed, mode=mode))
    out = []
    for i in range(b):
        quads, _, _ = dbpost.db_postprocess(bits[i], h, w, **(post or {}))
        if len(quads) == 0:
            out.append(dict(quads=quads, texts=[], scores=np.zeros(0, F32), labels=np.zeros(0, np.int32), cls_scores=np.zeros(0, F32),
                            flips=np.zeros(0, np.int32)))
            continue
        ccrops, cwidths = zip(*[crop(processed[i], q) for q in quads])
        label, score, flip, _ = classify(cls_w, np.stack(ccrops), cwidths, thresh, mode)
        rcrops = []
        for q, f in zip(quads, flip):
            c, wc = dbpost.rec_crop(processed[i], q)
            rcrops.append((turn(c, wc) if f else c, wc))
        crops, widths = zip(*rcrops)
        x = nets.rec_normalize(np.stack(crops), mode)
        for j, wv in enumerate(widths):
            x[j, :, :, wv:] = 0
        with torch.no_grad():
            idx, prob_t, _, _ = nets.rec_head(rec_w, nets.rec_backbone(rec_w, x, mode), mode)
        dec = nets.ctc_greedy(idx, prob_t, charset)
        out.append(dict(quads=quads, texts=[d[0] for d in dec], scores=np.array([d[1] for d in dec], F32), labels=label,
                        cls_scores=score, flips=flip))
    return out, processed
