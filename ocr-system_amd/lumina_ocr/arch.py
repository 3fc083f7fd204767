"""Architecture tables, seeded weights and the weight-blob format of the det+rec engine.

The reference ships no det+rec network: the engine slot is a remote
call (/root/reference/backend/services/ocr_service.py:213-246) or a third-party VLM
(/root/reference/backend/services/ocr_service_paddleocr_backup.py:285).  The networks
here are the ones BASELINE.json names, laid out after the public PaddleOCR model
definitions (det_r18_vd_db; rec_mv3_none_bilstm_ctc): *defined by this build*.

Everything in this file is host-side plumbing shared by the ctypes host, the C++
engine (which hard-codes the same layer names) and the test oracle:
  * DET_LAYERS / REC_* tables  — layer names, shapes, strides, activations
  * make_det_weights / make_rec_weights — deterministic seeded weights, BN folded
  * write_blob / read_blob — the "LOCW" weight container the C-ABI loads
"""
from __future__ import annotations

import struct
from typing import Dict, List, Sequence, Tuple

import numpy as np

# --------------------------------------------------------------------------------------
# bf16 helpers (numpy has no bf16: values are kept as float32 that are exactly bf16)
# --------------------------------------------------------------------------------------


def bf16_round(x: np.ndarray) -> np.ndarray:
    """Round float32 -> nearest-even bf16, returned as float32 (exactly representable)."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    u = x.view(np.uint32).astype(np.uint64)
    r = ((u + 0x7FFF + ((u >> 16) & 1)) >> 16) << 16
    return r.astype(np.uint32).view(np.float32).reshape(x.shape)


def f32_to_bf16_bits(x: np.ndarray) -> np.ndarray:
    x = np.ascontiguousarray(x, dtype=np.float32)
    u = x.view(np.uint32).astype(np.uint64)
    return ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16).reshape(x.shape)


def bf16_bits_to_f32(b: np.ndarray) -> np.ndarray:
    b = np.ascontiguousarray(b, dtype=np.uint16)
    return (b.astype(np.uint32) << 16).view(np.float32).reshape(b.shape)


# --------------------------------------------------------------------------------------
# Detection: DBNet = ResNet18_vd + DBFPN(256) + DBHead (probability branch)
# --------------------------------------------------------------------------------------
# conv entry: (name, cin, cout, k, stride, act, residual_from, kind)
#   kind: "conv" | "short_vd" (2x2 avg-pool fused as a 2x2/s2 conv) | "convt" (2x2/s2 transposed)
#   act : "relu" | "none" | "sigmoid"
DET_MEAN = (0.485, 0.456, 0.406)
DET_STD = (0.229, 0.224, 0.225)
DET_STAGE_CH = (64, 128, 256, 512)
DET_FPN_CH = 256
DET_THRESH = 0.3
DET_BOX_THRESH = 0.6
DET_UNCLIP_RATIO = 1.5
DET_MIN_SIZE = 3
DET_MAX_CANDIDATES = 1000


def det_conv_table() -> List[dict]:
    t: List[dict] = []

    def add(name, cin, cout, k, stride, act, kind="conv"):
        t.append(dict(name=name, cin=cin, cout=cout, k=k, stride=stride, act=act, kind=kind))

    add("stem.conv1", 3, 32, 3, 2, "relu")
    add("stem.conv2", 32, 32, 3, 1, "relu")
    add("stem.conv3", 32, 64, 3, 1, "relu")
    cin = 64
    for i, ch in enumerate(DET_STAGE_CH):
        for j in range(2):
            stride = 2 if (i > 0 and j == 0) else 1
            add(f"s{i}.b{j}.conv0", cin, ch, 3, stride, "relu")
            add(f"s{i}.b{j}.conv1", ch, ch, 3, 1, "relu")  # relu applied after the residual add
            if j == 0:
                if i == 0:
                    add(f"s{i}.b{j}.short", cin, ch, 1, 1, "none")
                else:
                    add(f"s{i}.b{j}.short", cin, ch, 2, 2, "none", kind="short_vd")
            cin = ch
    for lvl, ch in zip((5, 4, 3, 2), reversed(DET_STAGE_CH)):
        add(f"fpn.in{lvl}", ch, DET_FPN_CH, 1, 1, "none")
    for lvl in (5, 4, 3, 2):
        add(f"fpn.p{lvl}", DET_FPN_CH, DET_FPN_CH // 4, 3, 1, "none")
    add("head.conv1", DET_FPN_CH, 64, 3, 1, "relu")
    add("head.convt2", 64, 64, 2, 2, "relu", kind="convt")
    add("head.convt3", 64, 1, 2, 2, "sigmoid", kind="convt")
    return t


def det_macs_per_page(h: int, w: int) -> int:
    """Algorithmic MACs of one det forward on an h x w page (h, w multiples of 32)."""
    assert h % 32 == 0 and w % 32 == 0
    macs = 0
    res = {"stem.conv1": 2, "stem.conv2": 2, "stem.conv3": 2}
    for e in det_conv_table():
        n = e["name"]
        if n in res:
            s = res[n]
        elif n.startswith("s"):
            s = 4 << int(n[1])
        elif n.startswith("fpn.in") or n.startswith("fpn.p"):
            s = 1 << int(n[-1])
        elif n == "head.conv1":
            s = 4
        elif n == "head.convt2":
            s = 4  # input resolution; 4 output taps each 1x1
        elif n == "head.convt3":
            s = 2
        ho, wo = h // s, w // s
        taps = e["k"] * e["k"]
        if e["kind"] == "convt":
            macs += ho * wo * 4 * e["cin"] * e["cout"]
        elif e["kind"] == "short_vd":
            macs += ho * wo * e["cin"] * e["cout"]  # avg-pool + 1x1 (the algorithmic count)
        else:
            macs += ho * wo * taps * e["cin"] * e["cout"]
    return macs


# --------------------------------------------------------------------------------------
# Recognition: CRNN = MobileNetV3-small x0.5 -> 2 x BiLSTM(96) -> FC -> CTC greedy
# --------------------------------------------------------------------------------------
REC_H, REC_W, REC_T = 32, 320, 80
REC_HIDDEN = 96
REC_FEAT = 288


def _make_div(v: float, d: int = 8) -> int:
    nv = max(d, int(v + d / 2) // d * d)
    if nv < 0.9 * v:
        nv += d
    return nv


# (k, exp, c, se, act, stride_h) at scale 1.0; width stride is always 1
_MV3_SMALL = [
    (3, 16, 16, True, "relu", 1),
    (3, 72, 24, False, "relu", 2),
    (3, 88, 24, False, "relu", 1),
    (5, 96, 40, True, "hswish", 2),
    (5, 240, 40, True, "hswish", 1),
    (5, 240, 40, True, "hswish", 1),
    (5, 120, 48, True, "hswish", 1),
    (5, 144, 48, True, "hswish", 1),
    (5, 288, 96, True, "hswish", 2),
    (5, 576, 96, True, "hswish", 1),
    (5, 576, 96, True, "hswish", 1),
]


def rec_block_table(scale: float = 0.5, strides: Sequence[int] = None) -> List[dict]:
    """strides: vertical stride per block (default: the CRNN's, the last field of _MV3_SMALL)."""
    blocks = []
    cin = _make_div(16 * scale)
    for i, (k, exp, c, se, act, sh) in enumerate(_MV3_SMALL):
        if strides is not None:
            sh = strides[i]
        e, co = _make_div(exp * scale), _make_div(c * scale)
        blocks.append(dict(idx=i, k=k, cin=cin, exp=e, cout=co, se=se, act=act, stride_h=sh,
                           res=(sh == 1 and cin == co), se_mid=e // 4))
        cin = co
    return blocks


def rec_stem_ch(scale: float = 0.5) -> int:
    return _make_div(16 * scale)


# --------------------------------------------------------------------------------------
# CTC dictionary (the PP-OCR key file is absent offline: the build ships its own list)
# --------------------------------------------------------------------------------------


def ctc_charset(num_classes: int = 6625) -> List[str]:
    """index 0 = blank, last index = space (PP-OCR `use_space_char` convention)."""
    n_chars = num_classes - 2
    chars = [chr(c) for c in range(0x21, 0x7F)]
    cp = 0x4E00
    while len(chars) < n_chars:
        chars.append(chr(cp))
        cp += 1
    return ["\x00"] + chars[:n_chars] + [" "]


class TextDecoder:
    """class ids [n, T] (-1 padded) + lengths [n] -> strings.  Dictionaries whose symbols are single code points (every PP-OCR
    key file) decode vectorised through utf-32; multi-code-point symbols fall back to a join per line."""

    def __init__(self, charset: List[str]):
        self.charset = list(charset)
        self.single = all(len(c) == 1 for c in self.charset)
        self._cp = np.array([ord(c) for c in self.charset], dtype="<u4") if self.single else None

    def decode(self, ids: np.ndarray, lens: np.ndarray) -> List[str]:
        if len(ids) == 0:
            return []
        if self.single:
            cps = self._cp[np.maximum(ids, 0)]
            return [cps[i, : lens[i]].tobytes().decode("utf-32-le") for i in range(len(ids))]
        return ["".join(self.charset[k] for k in ids[i, : lens[i]]) for i in range(len(ids))]


def load_charset(path, use_space_char: bool = True) -> List[str]:
    """Dictionary FILE -> class list.  Format = PP-OCR key files (ppocr_keys_v1.txt, devanagari_dict.txt ...): UTF-8, one symbol
    per line, no header.  Class 0 is the CTC blank, the file's symbols follow in file order, a space is appended last
    (PP-OCR `use_space_char`).  The provider checks len(result) against the recogniser head's class count."""
    from pathlib import Path
    lines = Path(path).read_text(encoding="utf-8").split("\n")
    if lines and lines[-1] == "":
        lines.pop()
    syms = [ln.rstrip("\r") for ln in lines]
    if any(len(s) == 0 for s in syms):
        raise ValueError("dictionary %s holds an empty line" % path)
    if len(set(syms)) != len(syms):
        raise ValueError("dictionary %s holds duplicate symbols" % path)
    return ["\x00"] + syms + ([" "] if use_space_char and " " not in syms else [])


def save_charset(path, charset: List[str]) -> None:
    """Inverse of load_charset for a class list that starts with the blank and ends with the space."""
    from pathlib import Path
    assert charset[0] == "\x00" and charset[-1] == " "
    Path(path).write_text("".join(c + "\n" for c in charset[1:-1]), encoding="utf-8")


def devanagari_charset() -> List[str]:
    """blank + Devanagari block + digits/latin punctuation + space (config 5; build's own list)."""
    chars = [chr(c) for c in range(0x0900, 0x0980)] + [chr(c) for c in range(0x21, 0x7F) if not chr(c).isalpha()]
    return ["\x00"] + chars + [" "]


# --------------------------------------------------------------------------------------
# Seeded weights (BN folded into conv weight + bias; conv weights are bf16-exact float32)
# --------------------------------------------------------------------------------------


def _he(rng, cout, k, cin, gain=1.0, depthwise=False):
    fan_in = k * k * (1 if depthwise else cin)
    w = rng.standard_normal((cout, k, k, cin), dtype=np.float32) * np.float32(gain * np.sqrt(2.0 / fan_in))
    return bf16_round(w)


# Hand-set "text kernel" path (channel 0 of every tensor it crosses), installed on top of the seeded random
# weights so that synthetic pages produce real line boxes (no trained checkpoint exists offline):
#   stem.conv1 ch k<9 : relu(-mean_rgb(xn at tap k) - 0.5)            per-pixel "ink" (darker than mid-gray)
#   stem.conv2 ch 0   : sum of the 9 ink taps                          ink in a 3x3 window
#   stem.conv3 ch 0   : 1x3 horizontal sum / 4 ; max-pool              (1/4 resolution)
#   s0.*              : carried unchanged (shortcut = identity on ch 0, residual branch row 0 = 0)
#   fpn.in2/p2, head  : ch 0 -> 1x3 horizontal smoothing twice -> logit = gain * S - offset
# Rows feeding channel 0 read nothing else; every other row stays random (dense, realistic operands).
TEXT_GAIN, TEXT_OFFSET = 8.0, 26.0
# Post-process parameters that go with the hand-set kernel: it spans the full glyph height and is near-binary, whereas a
# trained DB kernel is shrunk (ratio 0.4) and soft, for which PaddleOCR's defaults (unclip 1.5, box_thresh 0.6) are meant.
TEXT_PATH_POST = dict(unclip_ratio=0.35, box_thresh=0.5)
DEFAULT_POST = dict(unclip_ratio=DET_UNCLIP_RATIO, box_thresh=DET_BOX_THRESH)


def _install_text_path(w: Dict[str, np.ndarray]) -> None:
    def zero_row(name, row=0):
        w[name + ".w"][row] = 0.0
        w[name + ".b"][row % len(w[name + ".b"])] = 0.0

    for k in range(9):
        zero_row("stem.conv1", k)
        w["stem.conv1.w"][k, k // 3, k % 3, :] = -1.0 / 3.0
        w["stem.conv1.b"][k] = -0.5
    zero_row("stem.conv2")
    w["stem.conv2.w"][0, 1, 1, :9] = 1.0
    zero_row("stem.conv3")
    w["stem.conv3.w"][0, 1, :, 0] = 0.25
    # 1/4 resolution: four horizontal 1x3 low-pass stages inside stage 0 (long horizontal runs = text lines survive,
    # short blobs such as descenders bridging two lines are attenuated)
    zero_row("s0.b0.short")
    zero_row("s0.b0.conv0", 1)
    w["s0.b0.conv0.w"][1, 1, :, 0] = 1.0 / 3.0
    zero_row("s0.b0.conv1")
    w["s0.b0.conv1.w"][0, 1, :, 1] = 1.0 / 3.0
    zero_row("s0.b1.conv0", 1)
    w["s0.b1.conv0.w"][1, 1, :, 0] = 1.0 / 3.0
    zero_row("s0.b1.conv1")
    w["s0.b1.conv1.w"][0, 1, :, 1] = 1.0 / 3.0
    for lvl in (3, 4, 5):
        zero_row(f"fpn.in{lvl}")
    zero_row("fpn.in2")
    w["fpn.in2.w"][0, 0, 0, 0] = 1.0
    zero_row("fpn.p2")
    w["fpn.p2.w"][0, 1, :, 0] = 1.0 / 3.0
    zero_row("head.conv1")
    w["head.conv1.w"][0, 1, :, 192] = 1.0 / 3.0
    for q in range(4):
        zero_row("head.convt2", q * 64)
        w["head.convt2.w"][q * 64, 0, 0, 0] = 1.0
        w["head.convt3.w"][q] = 0.0
        w["head.convt3.w"][q, 0, 0, 0] = TEXT_GAIN
    w["head.convt3.b"][:] = -TEXT_OFFSET
    for k in list(w):
        if k.endswith(".w"):
            w[k] = bf16_round(w[k])


def make_det_weights(seed: int = 1234, text_path: bool = True) -> Dict[str, np.ndarray]:
    """name.w: OHWI float32 (bf16-exact), name.b: float32 [cout]. convT: [(dy*2+dx)*cout+co][cin]."""
    rng = np.random.default_rng(seed)
    w: Dict[str, np.ndarray] = {}
    for e in det_conv_table():
        n, cin, cout, k = e["name"], e["cin"], e["cout"], e["k"]
        gain = 1.0
        if n.endswith(".conv1") and n.startswith("s"):
            gain = 0.5  # second conv of a residual branch
        if n.endswith(".short"):
            gain = 0.7071
        if n.startswith("fpn."):
            gain = 0.7071
        if e["kind"] == "convt":
            fan_in = cin
            wt = rng.standard_normal((4 * cout, 1, 1, cin), dtype=np.float32) * np.float32(np.sqrt(2.0 / fan_in))
            w[n + ".w"] = bf16_round(wt)
        elif e["kind"] == "short_vd":
            base = rng.standard_normal((cout, 1, 1, cin), dtype=np.float32) * np.float32(gain * np.sqrt(2.0 / cin))
            base = bf16_round(base)  # the 1x1 weight; the fused 2x2 taps are base/4 (exact in bf16)
            w[n + ".w"] = np.broadcast_to(base / 4.0, (cout, 2, 2, cin)).astype(np.float32).copy()
        else:
            w[n + ".w"] = _he(rng, cout, k, cin, gain)
        b = rng.standard_normal(cout, dtype=np.float32) * np.float32(0.05)
        if n.startswith("fpn."):
            b[:] = 0.0  # DBFPN convs carry no bias / BN
        if n == "head.convt3":
            b[:] = np.float32(-0.5)
        w[n + ".b"] = b.astype(np.float32)
    if text_path:
        _install_text_path(w)
    return w


# Hand-set "code path" of the recogniser (the counterpart of the detector's text path; installed by make_rec_weights(code_path=True)).
# A seeded-random CRNN decides every time step between near-ties (top-1 / top-2 logit margins of ~0.1 sigma), so bf16 drift flips a
# few arg-maxes per line and string parity can only be bounded.  A trained network has margins of many logits; this path gives the
# seeded one the same property, through arithmetic that is EXACT (order-independent), so the engine and the oracle agree bit for bit on it:
#   rec.conv1 ch 0      : hswish(-4 * xn_G(centre tap))                         "ink" of one pixel (0 for paper, 3.4 .. 4 for ink)
#   res blocks          : carried by the residual (project row = 0)
#   b1 / b3 / b8 (the three vertical stride-2 blocks): five channels, each a chain of single-tap depthwise filters, i.e. each
#                         samples the ink at one pair of crop rows (2a, 2a + 16), a = 3 .. 7, at its own horizontal offset
#   rec.conv2, max pool : carried (single unit weights: a contraction with one non-zero product is exact in any order)
#   lstm.l0 / l1 fw 0..4: saturated gates (i = o = 1, f = 0), g = tanh(BIG * (x - thr)) -> h = +-0.7617, no recurrence;
#                         thr sits half-way between two bf16 values, so |BIG * (x - thr)| >= 16 for EVERY bf16 x
#   ctc.fc              : the 32 code classes read +-16 on the five bits: the best code leads the runner-up by >= 24 logits
#                         (dense part: sigma ~2); code 0 = CTC blank, codes 1..31 = CODE_PATH_SYMBOLS
# Every other row of every layer stays seeded-random and dense.
CODE_PATH_SYMBOLS = "etaoinshrdlucmf wypvbgkqjxz0123"          # code v (1..31) -> symbol v - 1; the space exercises word splitting
_CODE_TAPS = [(2, 4, 0), (2, 4, 1), (2, 4, 2), (3, 3, 1), (3, 3, 2)]   # (kh in b8, kh in b3, kh in b1) -> stem rows (a, a + 8), a = 3 .. 7
_CODE_KW = [(2, 2, 1), (1, 3, 0), (3, 1, 2), (2, 4, 1), (4, 2, 0)]
CODE_THR = 1.0 + 2.0 ** -8        # half-way between the bf16 neighbours 1.0 and 1.0078125: |x - thr| >= 2^-8 for every bf16 x
CODE_BIG = 4096.0                 # 2^12: |BIG * (x - thr)| >= 16


def _install_code_path(w: Dict[str, np.ndarray], num_classes: int, scale: float) -> None:
    def zero_rows(name, rows):
        for r in rows:
            w[name + ".w"][r] = 0.0
            w[name + ".b"][r] = 0.0

    bits = range(5)
    zero_rows("rec.conv1", [0])
    w["rec.conv1.w"][0, 1, 1, 1] = -4.0
    for b in rec_block_table(scale):
        p = f"rec.b{b['idx']}"
        if b["res"]:
            zero_rows(p + ".project", range(1 if b["idx"] == 0 else 5))
            continue
        stage = {1: 2, 3: 1, 8: 0}[b["idx"]]
        zero_rows(p + ".expand", bits); zero_rows(p + ".dw", bits); zero_rows(p + ".project", bits)
        for k in bits:
            w[p + ".expand.w"][k, 0, 0, 0 if b["idx"] == 1 else k] = 1.0
            w[p + ".dw.w"][k, _CODE_TAPS[k][stage], _CODE_KW[k][stage], 0] = 1.0
            w[p + ".project.w"][k, 0, 0, k] = 1.0
        if b["se"]:
            zero_rows(p + ".se2", bits)
            w[p + ".se2.b"][:5] = 4.0          # hard-sigmoid(4) = 1: the squeeze-excite gate of the path channels is exactly 1
    zero_rows("rec.conv2", bits)
    for k in bits:
        w["rec.conv2.w"][k, 0, 0, k] = 1.0
    h = REC_HIDDEN
    for layer, big, thr in ((0, CODE_BIG, CODE_THR), (1, 32.0, 0.0)):
        p = f"lstm.l{layer}.fw"
        for k in bits:
            for gate, bias in ((0, 20.0), (1, -20.0), (2, -big * thr), (3, 20.0)):   # i, f, g, o
                w[p + ".w_ih"][gate * h + k] = 0.0
                w[p + ".w_hh"][gate * h + k] = 0.0
                w[p + ".b"][gate * h + k] = bias
            w[p + ".w_ih"][2 * h + k, k] = big
    w["ctc.fc.w"][:, :5] = 0.0
    space = num_classes - 1
    for v in range(32):
        cls = 0 if v == 0 else (space if CODE_PATH_SYMBOLS[v - 1] == " " else 1 + ord(CODE_PATH_SYMBOLS[v - 1]) - 0x21)
        for k in bits:
            w["ctc.fc.w"][cls, k] = 16.0 if (v >> k) & 1 else -16.0


def make_rec_weights(seed: int = 4321, num_classes: int = 6625, scale: float = 0.5, code_path: bool = False) -> Dict[str, np.ndarray]:
    """code_path: install the hand-set exact path described above (strings then have trained-like arg-max margins)."""
    rng = np.random.default_rng(seed)
    w: Dict[str, np.ndarray] = {}

    def conv(name, cout, k, cin, gain=1.0, depthwise=False):
        w[name + ".w"] = _he(rng, cout, k, 1 if depthwise else cin, gain, depthwise)
        w[name + ".b"] = (rng.standard_normal(cout, dtype=np.float32) * np.float32(0.05)).astype(np.float32)

    c0 = rec_stem_ch(scale)
    conv("rec.conv1", c0, 3, 3)
    for b in rec_block_table(scale):
        p = f"rec.b{b['idx']}"
        hs = b["act"] == "hswish"  # hard-swish roughly halves small activations: compensate so the signal survives 11 blocks
        conv(p + ".expand", b["exp"], 1, b["cin"], gain=1.25 if hs else 1.0)
        conv(p + ".dw", b["exp"], b["k"], b["exp"], gain=1.25 if hs else 1.0, depthwise=True)
        if b["se"]:
            conv(p + ".se1", b["se_mid"], 1, b["exp"])
            conv(p + ".se2", b["exp"], 1, b["se_mid"], gain=0.7071)
        conv(p + ".project", b["cout"], 1, b["exp"], gain=(0.5 if b["res"] else 1.4) * (1.4 if b["se"] else 1.0))
    conv("rec.conv2", REC_FEAT, 1, rec_block_table(scale)[-1]["cout"], gain=1.0)
    h = REC_HIDDEN
    for layer, din in ((0, REC_FEAT), (1, 2 * h)):
        for d in ("fw", "bw"):
            p = f"lstm.l{layer}.{d}"
            w[p + ".w_ih"] = bf16_round(rng.uniform(-1, 1, (4 * h, din)).astype(np.float32) * np.float32(1.0 / np.sqrt(h)))
            w[p + ".w_hh"] = bf16_round(rng.uniform(-1, 1, (4 * h, h)).astype(np.float32) * np.float32(1.0 / np.sqrt(h)))
            w[p + ".b"] = (rng.uniform(-1, 1, 4 * h).astype(np.float32) * np.float32(1.0 / np.sqrt(h))).astype(np.float32)
    w["ctc.fc.w"] = bf16_round(rng.standard_normal((num_classes, 2 * h), dtype=np.float32) * np.float32(12.0 / np.sqrt(2 * h)))
    w["ctc.fc.b"] = (rng.standard_normal(num_classes, dtype=np.float32) * np.float32(0.1)).astype(np.float32)
    if code_path:
        _install_code_path(w, num_classes, scale)
    return w


# --------------------------------------------------------------------------------------
# Text-line orientation classifier (PP-OCR `cls`, ch_ppocr_mobile_v2.0_cls): the recogniser's MobileNetV3-small backbone at
# scale 0.35 on 48 x 192 crops with small_stride [2, 2, 2, 2] (block 0 halves the height too) -> conv2 (1x1, 200, hswish) ->
# 2x2 max pool -> mean over the 48 positions -> FC(2) -> soft-max.  Label 0 = "0", 1 = "180"; a crop is turned when
# label == 1 and its probability > CLS_THRESH (PaddleOCR's cls_thresh).
# --------------------------------------------------------------------------------------
CLS_H, CLS_W = 48, 192
CLS_SCALE = 0.35
CLS_STRIDES = (2, 2, 1, 2, 1, 1, 1, 1, 2, 1, 1)
CLS_FEAT = 200
CLS_THRESH = 0.9

# Ruled tables (lumina_ocr_table_rules + utils/tables.py): ink = L < threshold; runs of a row / column at most `gap` apart merge and
# count from min_len pixels on; a component of such runs is a rule when its area <= max_thick x its length; max_rules = capacity of a
# page's list per direction; snap = the distance (pixels) within which rule ends, centre-lines and grid lines count as meeting.
TABLE_PARAMS = dict(threshold=128, gap=2, min_len=64, max_thick=12, max_rules=512, snap=8)

# Selection marks (lumina_ocr_selection_marks + utils/marks.py): ink as above; a connected component of the ink is a candidate when its
# bounding box has min_side <= w, h <= max_side and is nearly square; a candidate whose box carries ink along all four sides is a mark,
# selected when a sixteenth of its interior is ink.  max_side <= 64 is part of the contract (one 64-bit word and one wave64 lane per
# row of a box); max_marks = capacity of a page's list.
MARK_PARAMS = dict(threshold=128, min_side=12, max_side=64, max_marks=256)

# Round selection marks (radio buttons; lumina_ocr_selection_marks_round, definition restated in tests/radio_reference.py): a candidate
# of the checkboxes that is no frame, read in doubled coordinates about the centre of its box (u = 2x - (x0 + x1), v = 2y - (y0 + y1),
# q = u^2 + v^2, D = max(w, h)).  At most out_max ink pixels lie beyond the outer circle q <= (D + 1)^2; the ring zone
# (D - 2T)^2 < q <= (D + 1)^2, T = 1 + D / ring_div, carries ink over all but an eighth of the columns of the top and of the bottom half
# and of the rows of the left and of the right half; the moat between the ring zone and the core q <= D^2 / 4 is empty; a band of
# band_min + min(w, h) / band_div pixels around the box, clipped to the page, is empty.  State from the core as for the checkboxes.
ROUND_MARK_PARAMS = dict(out_max=0, ring_div=12, band_div=4, band_min=4)

# Barcodes (lumina_ocr_barcodes + utils/barcodes.py, definition restated in tests/barcode_reference.py): ink as above.  A row reads a
# Code 128 or a Code 39 when every symbol from a start to a stop matches its table within max_dist / 256 of the symbol's width (summed
# over its elements, in modules), the gap before the start is `quiet` modules wide and, for Code 128, the checksum holds; equal reads
# at most row_gap rows apart join, and min_rows of them make a barcode.  The issue's proposed values are kept but for max_dist, which
# the synthetic set moved from 64 to 24: a Code 128 symbol with one element a module too wide (13 px over 12 modules of m px) lies at
# least 14 m from every pattern and 64 accepts up to 16.5 m, so the widened-bar decoy read whenever its checksum happened to hold; 24
# accepts 12.4 m and never takes a module's error, while an edge off by one pixel inside a symbol (22 at most) still passes from
# m = 2 px on.  The nearest pattern wins anyway; the checksum, the stop and min_rows equal reads carry the rest of the rejection.
# quiet = 5 is half the standard's ten modules: forms crowd their codes.  max_codes = capacity of a page's list (<= 256).
BARCODE_PARAMS = dict(threshold=MARK_PARAMS["threshold"], quiet=5, max_dist=24, min_rows=8, row_gap=2, max_codes=64)
# The kinds lumina_ocr_barcodes_kinds reads, name -> bit of its mask (definition restated in tests/linear_reference.py).  "ean13" reads
# UPC-A as well (an EAN-13 whose first digit is 0).  The same parameters serve every kind: the guards of EAN / UPC and the start and stop
# of ITF are matched by the same measure, both of their ends need the quiet gap, and ITF reads from 6 digits on.
BARCODE_KINDS = dict(code128=1, code39=2, ean13=4, ean8=8, upce=16, itf=32)
BARCODE_KINDS_DEFAULT = ("code128", "code39")


def barcode_kinds_mask(names) -> int:
    """Names of BARCODE_KINDS (a sequence, or a comma list; "all" is every kind) -> the bit mask; an unknown name or an empty set is a
    ValueError."""
    if isinstance(names, str):
        names = [n.strip().lower() for n in names.split(",") if n.strip()]
    mask = 0
    for n in names:
        if n == "all":
            mask |= sum(BARCODE_KINDS.values())
        elif n in BARCODE_KINDS:
            mask |= BARCODE_KINDS[n]
        else:
            raise ValueError("unknown barcode kind %r: one of %s, or all" % (n, ", ".join(BARCODE_KINDS)))
    if not mask:
        raise ValueError("no barcode kind given: some of %s, or all" % ", ".join(BARCODE_KINDS))
    return mask

# QR codes (lumina_ocr_qrcodes + utils/qrcodes.py, definition restated in tests/qr_reference.py): ink as above, at the barcodes'
# threshold so that one mask serves both.  min_module = 3 px is the issue's floor; max_module = 24 px lets a version 10 symbol span 1368 of the 2000 processed pixels.  centre_tol and ring_tol
# are sixteenths of a module (the ring's w + h stands for 14 modules): 8 = half a module between the centres of core and ring, 12 =
# three quarters of a module on the ring's side against 7/3 of the core's, which is one pixel at each edge of a 3 px module and a
# little ink spread.  quiet = 2 modules, half the standard's four, as the 1-D codes halve theirs: forms crowd their codes; the rings
# of modules round the symbol are sampled on the decode grid and must be clear.  timing_max = 3 mismatches in the two timing
# patterns: a clean symbol has none, a wrong version about half of its 10..82 timing modules, and Reed-Solomon carries the rest of
# the rejection.  Changed against the issue's outline, the restatement being the definition: a core is solid when 4 area >= 3 w h, not
# 8 area >= 7 w h: half a degree of tilt puts a one-pixel stair on every edge, a 12 px core then has a 13 x 13 box and 146 of its 169
# pixels (0.86), and a 9 px core 81 of 100; three quarters keeps both and still refuses rings, frames and text; grouping is the decode wave's first step,
# not a kernel of its own (the finders of a page are one int4 a lane); a corner finder tries its valid pairs in the order of
# |AB|^2 + |AC|^2 (ties by the partners' roots), eight at most, until one decodes: on a page of several symbols a neighbour's finder
# can lie nearer than the corner's own partners, and the nearest pair alone lost one of 64 symbols of the probe's pages; a page has
# at most one symbol per finder and the decode kernel's grid is max_finders waves a page; the version's reach is three modules either side of n = 10 + 4 v (neighbouring
# versions lie four apart, so at most two are tried); the reported format distance has 16 added when the second copy was read.
# max_finders <= 64 (one wave sorts them), max_codes <= 64.
QR_PARAMS = dict(threshold=BARCODE_PARAMS["threshold"], min_module=3, max_module=24, quiet=2, centre_tol=8, ring_tol=12, timing_max=3,
                 max_finders=64, max_codes=16)

# Data Matrix (lumina_ocr_datamatrix + utils/datamatrix.py, definition restated in tests/dm_reference.py): ink at the barcodes'
# threshold so that one mask serves the three passes.  A candidate is a component whose box sides lie in 8 min_module .. 52 max_module
# with 32 area >= w h (the L alone is 3.8 % of a 52 x 52 symbol).  quiet = 1 module, the standard's own.  timing_max = 3 mismatches in
# the clock tracks and solid_max = 3 clear modules in the L and the inner solid bars: a clean symbol has none of either, a wrong size
# or orientation about half of its clock modules, a letter L or a frame all of the dark or all of the light ones (at least 8), and
# Reed-Solomon carries the rest of the rejection.  Changed against the issue's outline, which capped max_candidates at 64: the box and
# area filter lets every glyph of 24 px and more through, the benchmark's A4 text pages have 50 candidates on average and up to 98,
# and a page above the capacity is not read at all; nothing in the pass needs a lane per candidate (the decode kernel's grid is
# max_candidates waves a page, all but the candidates' exit after one load), so the capacity is max_candidates <= 1024 and 256 by
# default.  max_codes <= 64.  lumina_ocr_datamatrix_sizes takes the same parameters: its second stage (64 x 64 .. 144 x 144) has a candidate
# list of its own with the same capacity, box sides in 64 min_module .. 144 max_module (tests/dm_sizes_reference.py).
DM_PARAMS = dict(threshold=BARCODE_PARAMS["threshold"], min_module=3, max_module=24, quiet=1, timing_max=3, solid_max=3, max_candidates=256,
                 max_codes=16)

# Aztec (lumina_ocr_aztec + utils/aztec.py, definition restated in tests/aztec_reference.py): ink at the barcodes' threshold so that
# one mask serves the four passes.  The finder is the bullseye's core, a solid square of one module, inside the component of its
# 5-module ring: the ring's sides are 5 cores within ring_tol / 16 of a module and the two are concentric within centre_tol / 16.
# quiet = 1 module.  mark_max = 4 mismatches in the bullseye's modules and the twelve corner modules of the mode ring together: a
# clean symbol has none, the wrong kind (compact read as full or the reverse) at least six.  max_finders <= 64, max_codes <= 64.
AZTEC_PARAMS = dict(threshold=BARCODE_PARAMS["threshold"], min_module=3, max_module=24, quiet=1, centre_tol=8, ring_tol=8, mark_max=4,
                    max_finders=64, max_codes=16)

# Page orientation (lumina_ocr_page_quarter / _page_turn / _page_vote + utils/page_orient.py): ink as above; a page is sideways when the
# energy of its column profile exceeds `ratio` times that of its row profile (text lines make the profile across them jagged), and an
# upright-or-upside-down page is upside-down when it has at least min_lines lines and the classifier flips more than half of them.
PAGE_ORIENT_PARAMS = dict(threshold=TABLE_PARAMS["threshold"], ratio=2, min_lines=3)


def cls_block_table() -> List[dict]:
    """rec_block_table at scale 0.35 with the classifier's strides; `h` = the block's output height on a 48-row crop."""
    blocks = rec_block_table(CLS_SCALE, CLS_STRIDES)
    h = CLS_H // 2
    for b in blocks:
        h = (h + 2 * (b["k"] // 2) - b["k"]) // b["stride_h"] + 1
        b["h"] = h
    return blocks


# Hand-set "orientation path" of the classifier (the counterpart of the text path and the code path; make_cls_weights(orientation_path=True)).
# What it reads: a SOLID horizontal ink band, such as the rule under each line of synth.synth_page(..., ruled=True) (a filled-in
# form); a glyph stroke is rarely 3 px wide and 2 rows high at once.  Channel 0 of every tensor up to block 7 carries it; block 8 splits
# it into T (channel 0, crop rows 0..15) and B (channel 1, crop rows 32..47):
#   cls.conv1 ch 0  : hswish(-(sum of the G channel over crop rows 2r, 2r + 1 x 3 columns) - 3.5): > 0 only where all six pixels are
#                     dark (the ink shades of synth pages, 0..40, give 0.62..2.5); relu in b0 drops the rest
#   b0, b1, b3      : expand 1.0, depthwise with TWO unit taps (rows 2o, 2o + 1), project 1.0: each stride-2 stage sums a pair of
#                     rows, so b3's output row 0 holds crop rows 0..15 and its row 2 crop rows 32..47
#   residual blocks : carried by the shortcut (project row = 0); squeeze-excite gates of the path channels pinned to 1
#   b8 (k 5, s 2)   : T = one tap kh = 0 (output row 0 reads the zero padding, row 1 = b3's row 0), B = one tap kh = 4 (row 0 = b3's
#                     row 2, row 1 reads the padding); conv2 and the max pool carry both (unit weights, the padding row gives 0)
#   cls.fc          : logit0 = CLS_GAIN * mean(B), logit1 = CLS_GAIN * mean(T) + the FC's dense columns scaled by 2^-6
# Exactness: the stem's six G values are bf16 in [-1, 1] (multiples of 2^-15), so its sum is exact in any order; every later value on
# the path is a bf16 number >= 2^-16 or 0 and <= 2^7, and sums of a few such values are exact in fp32 in any order.  The head sums
# positions and channels in a fixed order.  Engine and restatement agree on the path bit for bit.
# Decision rule: a line is read upside down when its top band holds more solid ink than its bottom band.  The detector's boxes
# reach further below the ink than above it, so an upright line's rule falls in the bottom band only when it is thick: the ruled
# pages draw it size // 3 px thick, 2 px under the text.  Measured with the restatement (seeds 3 / 7 / 21, detector text path):
# every line of every page labelled right, upright and turned; on pages 480 and 640 rows high (fonts 16-25 px) |logit1 - logit0|
# >= 9.7 on every line (score > 0.9999); on 320-row pages (10-15 px fonts) the thinnest rules miss the bottom band of some upright
# lines, whose label stays 0 with a margin down to 0.85.
# All other rows of every layer stay seeded and dense.
CLS_GAIN = 16.0
CLS_DENSE_SCALE = 2.0 ** -6     # the FC's dense columns, scaled (exactly) so that the seeded part cannot outvote the path
CLS_MARGIN = 8.0                # |logit1 - logit0| the tests require on every line of ruled pages >= 480 rows high


def _install_orientation_path(w: Dict[str, np.ndarray]) -> None:
    def zero_rows(name, rows):
        for r in rows:
            w[name + ".w"][r] = 0.0
            w[name + ".b"][r] = 0.0

    zero_rows("cls.conv1", [0])
    w["cls.conv1.w"][0, 1:3, :, 1] = -1.0
    w["cls.conv1.b"][0] = -3.5
    for b in cls_block_table():
        p, c = f"cls.b{b['idx']}", b["k"] // 2
        if b["res"]:
            zero_rows(p + ".project", [0, 1] if b["idx"] > 8 else [0])
            continue
        rows = [0, 1] if b["idx"] == 8 else [0]
        zero_rows(p + ".expand", rows); zero_rows(p + ".dw", rows); zero_rows(p + ".project", rows)
        for r in rows:
            w[p + ".expand.w"][r, 0, 0, 0] = 1.0
            w[p + ".project.w"][r, 0, 0, r] = 1.0
        if b["idx"] == 8:
            w[p + ".dw.w"][0, 0, c, 0] = 1.0          # T: the top band
            w[p + ".dw.w"][1, 4, c, 0] = 1.0          # B: the bottom band
        else:
            w[p + ".dw.w"][0, c, c, 0] = 1.0          # rows 2o, 2o + 1
            w[p + ".dw.w"][0, c + 1, c, 0] = 1.0
        if b["se"]:
            zero_rows(p + ".se2", rows)
            w[p + ".se2.b"][rows] = 4.0               # hard-sigmoid(4) = 1
    zero_rows("cls.conv2", [0, 1])
    w["cls.conv2.w"][0, 0, 0, 0] = 1.0
    w["cls.conv2.w"][1, 0, 0, 1] = 1.0
    w["cls.fc.w"][:, 2:] *= CLS_DENSE_SCALE
    w["cls.fc.w"][:, :2] = 0.0
    w["cls.fc.w"][0, 1] = CLS_GAIN
    w["cls.fc.w"][1, 0] = CLS_GAIN
    w["cls.fc.b"][:] = 0.0


def make_cls_weights(seed: int = 2718, orientation_path: bool = False) -> Dict[str, np.ndarray]:
    """Seeded classifier weights in the LOCW naming (cls.*), every row dense; orientation_path: install the hand-set exact path above."""
    rng = np.random.default_rng(seed)
    w: Dict[str, np.ndarray] = {}

    def conv(name, cout, k, cin, gain=1.0, depthwise=False):
        w[name + ".w"] = _he(rng, cout, k, 1 if depthwise else cin, gain, depthwise)
        w[name + ".b"] = (rng.standard_normal(cout, dtype=np.float32) * np.float32(0.05)).astype(np.float32)

    conv("cls.conv1", rec_stem_ch(CLS_SCALE), 3, 3)
    for b in cls_block_table():
        p = f"cls.b{b['idx']}"
        hs = b["act"] == "hswish"
        conv(p + ".expand", b["exp"], 1, b["cin"], gain=1.25 if hs else 1.0)
        conv(p + ".dw", b["exp"], b["k"], b["exp"], gain=1.25 if hs else 1.0, depthwise=True)
        if b["se"]:
            conv(p + ".se1", b["se_mid"], 1, b["exp"])
            conv(p + ".se2", b["exp"], 1, b["se_mid"], gain=0.7071)
        conv(p + ".project", b["cout"], 1, b["exp"], gain=(0.5 if b["res"] else 1.4) * (1.4 if b["se"] else 1.0))
    conv("cls.conv2", CLS_FEAT, 1, cls_block_table()[-1]["cout"])
    w["cls.fc.w"] = bf16_round(rng.standard_normal((2, CLS_FEAT), dtype=np.float32) * np.float32(1.0 / np.sqrt(CLS_FEAT)))
    w["cls.fc.b"] = (rng.standard_normal(2, dtype=np.float32) * np.float32(0.05)).astype(np.float32)
    if orientation_path:
        _install_orientation_path(w)
    return w


# --------------------------------------------------------------------------------------
# Recognition, second family: SVTR-Tiny (single visual model: patch embedding -> local / global mixing blocks with height
# merging -> CTC).  BASELINE configs[4] names an SVTR recogniser with a Hindi dictionary; no implementation, weights or
# dictionary exist offline, so the architecture below is the build's restatement of the published design
# (Du et al., "SVTR: Scene Text Recognition with a Single Visual Model", tiny configuration, post-norm blocks) on the 32 x 320
# crops of this pipeline: 8 x 80 tokens -> 4 x 80 -> 2 x 80 -> 80 time steps.  "Parity unpinned".
# --------------------------------------------------------------------------------------
SVTR_VARIANTS = {
    # dims, depths, heads (head width 32), local mixing blocks (the first ones), channels of the sequence handed to the CTC head
    "tiny": dict(dims=(64, 128, 256), depths=(3, 6, 3), heads=(2, 4, 8), local_blocks=6, out=192),
    "base": dict(dims=(128, 256, 384), depths=(3, 6, 9), heads=(4, 8, 12), local_blocks=8, out=192),   # BASELINE configs[4]
}
SVTR_DIMS, SVTR_DEPTHS, SVTR_HEADS = SVTR_VARIANTS["tiny"]["dims"], SVTR_VARIANTS["tiny"]["depths"], SVTR_VARIANTS["tiny"]["heads"]
SVTR_LOCAL_BLOCKS = 6            # (tiny) the first 6 of the 12 blocks mix locally (window 7 x 11 tokens), the rest globally
SVTR_WINDOW = (7, 11)
SVTR_OUT = 192                   # channels of the sequence handed to the CTC head
SVTR_LN_EPS = 1e-6
SVTR_DTYPES = {"bf16": 0, "f16": 1}


def svtr_config(weights=None, variant: str = "tiny") -> dict:
    """The variant a weight dict / blob describes (its `svtr.config` tensor), or the named one."""
    if weights is not None and "svtr.config" in weights:
        c = [int(v) for v in np.asarray(weights["svtr.config"]).tolist()]
        return dict(dims=tuple(c[0:3]), depths=tuple(c[3:6]), heads=tuple(c[6:9]), local_blocks=c[9], out=c[10], dtype="f16" if c[11] else "bf16")
    return dict(SVTR_VARIANTS[variant], dtype="bf16")


def svtr_block_table(cfg=None) -> List[dict]:
    """One entry per mixing block: stage, dim, heads, token grid (h, w), local / global."""
    cfg = cfg or svtr_config()
    rows, idx, h = [], 0, REC_H // 4
    for s, (dim, depth, heads) in enumerate(zip(cfg["dims"], cfg["depths"], cfg["heads"])):
        for _ in range(depth):
            rows.append(dict(idx=idx, stage=s, dim=dim, heads=heads, h=h, w=REC_W // 4, local=idx < cfg["local_blocks"]))
            idx += 1
        h //= 2
    return rows


def make_svtr_weights(seed: int = 2468, num_classes: int = 6625, variant: str = "tiny", dtype: str = "bf16") -> Dict[str, np.ndarray]:
    """Seeded weights in the LOCW naming: conv / linear weights OHWI `[out, kh, kw, in]` (.w, bf16), biases and LayerNorm
    gamma / beta fp32 (.b / .g); `svtr.config` (f32 [12]) carries the variant and the storage / MFMA type the engine shall use."""
    rng = np.random.default_rng(seed)
    cfg = SVTR_VARIANTS[variant]
    dims = cfg["dims"]
    w: Dict[str, np.ndarray] = {}
    w["svtr.config"] = np.array(list(dims) + list(cfg["depths"]) + list(cfg["heads"]) + [cfg["local_blocks"], cfg["out"], SVTR_DTYPES[dtype]], np.float32)

    def conv(name, cout, k, cin, gain=1.0):
        w[name + ".w"] = _he(rng, cout, k, cin, gain)
        w[name + ".b"] = (rng.standard_normal(cout, dtype=np.float32) * np.float32(0.05)).astype(np.float32)

    def ln(name, c):
        w[name + ".g"] = (1.0 + 0.1 * rng.standard_normal(c)).astype(np.float32)
        w[name + ".b"] = (0.05 * rng.standard_normal(c)).astype(np.float32)

    conv("svtr.pe1", dims[0] // 2, 3, 3, gain=1.3)
    conv("svtr.pe2", dims[0], 3, dims[0] // 2, gain=1.3)
    w["svtr.pos.w"] = bf16_round((0.5 * rng.standard_normal(((REC_H // 4) * (REC_W // 4), dims[0]))).astype(np.float32))
    for b in svtr_block_table(dict(cfg)):
        p, c = f"svtr.b{b['idx']}", b["dim"]
        conv(p + ".qkv", 3 * c, 1, c, gain=0.8)
        conv(p + ".proj", c, 1, c, gain=0.15)   # small residual branches: with untrained weights larger ones wash the token identity out
        ln(p + ".ln1", c)
        conv(p + ".fc1", 4 * c, 1, c, gain=1.0)
        conv(p + ".fc2", c, 1, 4 * c, gain=0.15)
        ln(p + ".ln2", c)
    for s in range(2):
        conv(f"svtr.sub{s}", dims[s + 1], 3, dims[s], gain=1.0)
        ln(f"svtr.sub{s}.ln", dims[s + 1])
    conv("svtr.last", cfg["out"], 1, dims[2], gain=1.4)
    w["svtr.ctc.fc.w"] = bf16_round(rng.standard_normal((num_classes, cfg["out"]), dtype=np.float32) * np.float32(12.0 / np.sqrt(cfg["out"])))
    w["svtr.ctc.fc.b"] = (rng.standard_normal(num_classes, dtype=np.float32) * np.float32(0.1)).astype(np.float32)
    return w


# --------------------------------------------------------------------------------------
# "LOCW" weight container
#   header : b"LOCW", u32 version(1), u32 n_tensors
#   tensor : u16 name_len, name, u8 dtype(0=f32,1=bf16), u8 ndim, u32 dims[ndim], u64 nbytes,
#            pad to 16-byte file offset, raw data
# --------------------------------------------------------------------------------------
BLOB_MAGIC = b"LOCW"


def write_blob(weights: Dict[str, np.ndarray]) -> bytes:
    out = bytearray()
    out += BLOB_MAGIC + struct.pack("<II", 1, len(weights))
    for name, arr in weights.items():
        nb = name.encode()
        as_bf16 = name.endswith(".w") or name.endswith(".w_ih") or name.endswith(".w_hh")
        data = f32_to_bf16_bits(arr).tobytes() if as_bf16 else np.ascontiguousarray(arr, np.float32).tobytes()
        out += struct.pack("<H", len(nb)) + nb + struct.pack("<BB", 1 if as_bf16 else 0, arr.ndim)
        out += struct.pack("<%dI" % arr.ndim, *arr.shape) + struct.pack("<Q", len(data))
        out += b"\x00" * ((-len(out)) % 16)
        out += data
    return bytes(out)


def read_blob(blob: bytes) -> Dict[str, np.ndarray]:
    assert blob[:4] == BLOB_MAGIC, "not a LOCW blob"
    ver, n = struct.unpack_from("<II", blob, 4)
    assert ver == 1
    off = 12
    out: Dict[str, np.ndarray] = {}
    for _ in range(n):
        (ln,) = struct.unpack_from("<H", blob, off); off += 2
        name = blob[off:off + ln].decode(); off += ln
        dt, nd = struct.unpack_from("<BB", blob, off); off += 2
        dims = struct.unpack_from("<%dI" % nd, blob, off); off += 4 * nd
        (nbytes,) = struct.unpack_from("<Q", blob, off); off += 8
        off += (-off) % 16
        raw = blob[off:off + nbytes]; off += nbytes
        if dt == 1:
            out[name] = bf16_bits_to_f32(np.frombuffer(raw, np.uint16).reshape(dims))
        else:
            out[name] = np.frombuffer(raw, np.float32).reshape(dims).copy()
    return out
