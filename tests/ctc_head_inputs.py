"""Inputs and the float64 reference of the CTC head tests (tests/test_gpu_ctc_head.py; self-checked on the CPU by
tests/test_ctc_head_inputs.py).  The head is ctc_fc_argmax_kernel: FC + arg-max + soft-max fused, the logits never in memory.  Every
construction here replaces only the FC of a seeded recogniser (`ctc.fc.*` of the CRNN, `svtr.ctc.fc.*` of SVTR); the reference is
computed from the sequence the head consumed and the weights as the loader stores them."""
from __future__ import annotations

import numpy as np

from lumina_ocr import arch

CLEAR_MARGIN = 1e-4      # top-1 / top-2 margin (float64 logits) from which fp32 accumulation cannot flip the arg-max
CLEAR_SHARE = 0.95       # at least this share of the rows is clear in every case
PROB_RTOL = 2e-4
K = 192                  # channels of the sequence of both recognisers (2 x arch.REC_HIDDEN, arch.SVTR_OUT)
FC = {"crnn": "ctc.fc", "svtr": "svtr.ctc.fc"}


def stored(w: np.ndarray, dtype: str = "bf16") -> np.ndarray:
    """FC weights as the engine multiplies them, float64: the blob carries bf16 bits (arch.write_blob); an fp16 model converts those
    to fp16 with one round-to-nearest-even (engine.hip bf16_bits_to: `(_Float16)f`, exact for bf16 values with |w| >= 2^-14)."""
    w = arch.bf16_round(np.asarray(w, np.float32))
    if dtype == "f16":
        w = w.astype(np.float16).astype(np.float32)
    assert np.isfinite(w).all()
    return w.astype(np.float64)


def reference(seq: np.ndarray, w: np.ndarray, b: np.ndarray, dtype: str = "bf16", distinct: int = None):
    """seq [M, K] (the tap the head consumed) -> dict(idx int64 [M], prob float64 [M], clear bool [M], logits float64 [M, C]).
    idx is np.argmax's: the LOWEST index among equal logits.  clear: top-1 / top-2 margin > CLEAR_MARGIN, over the first `distinct`
    classes when given (the periodic sets, whose other classes are exact copies: their logits are copied, not computed again, so
    that the ties are exact whatever order the host's matrix product sums in)."""
    ws, bs = stored(w, dtype), np.asarray(b, np.float32).astype(np.float64)
    if distinct is not None:
        sel = np.arange(len(ws)) % distinct
        assert np.array_equal(ws, ws[sel]) and np.array_equal(bs, bs[sel])
        logits = (np.asarray(seq, np.float64) @ ws[:distinct].T + bs[:distinct])[:, sel]
    else:
        logits = np.asarray(seq, np.float64) @ ws.T + bs
    idx = logits.argmax(1)
    mx = logits.max(1, keepdims=True)
    prob = 1.0 / np.exp(logits - mx).sum(1)
    d = logits if distinct is None else logits[:, :distinct]
    if d.shape[1] > 1:
        top2 = np.partition(d, -2, axis=1)[:, -2:]
        clear = (top2[:, 1] - top2[:, 0]) > CLEAR_MARGIN
    else:
        clear = np.ones(len(d), bool)
    return dict(idx=idx, prob=prob, clear=clear, logits=logits)


def with_fc(wd: dict, model: str, w: np.ndarray, b: np.ndarray) -> dict:
    """A copy of the weight dict with the head's FC replaced (the backbone's arrays are shared, not copied)."""
    out = dict(wd)
    assert w.ndim == 2 and w.shape[1] == wd[FC[model] + ".w"].shape[1] and b.shape == (w.shape[0],)
    out[FC[model] + ".w"] = np.ascontiguousarray(w, np.float32)
    out[FC[model] + ".b"] = np.ascontiguousarray(b, np.float32)
    return out


def seeded_fc(c: int, seed: int):
    """arch.make_rec_weights' FC distribution for c classes: weights bf16-exact N(0, (12 / sqrt K)^2), bias N(0, 0.1^2)."""
    rng = np.random.default_rng(seed)
    w = arch.bf16_round(rng.standard_normal((c, K), dtype=np.float32) * np.float32(12.0 / np.sqrt(K)))
    b = (rng.standard_normal(c, dtype=np.float32) * np.float32(0.1)).astype(np.float32)
    return w, b


# ---------------------------------------------------------------------------------------------------------------- class-count edges
# C < 64: one, mostly padded tile; 64 and 128: no padded class at all; 65: one real class in the last tile, 63 x -1e30 beside it.
EDGE_CLASSES = [3, 64, 65, 128]
EDGE_BOOST = 2.0


def edge_winners(c: int):
    """The classes that must win somewhere: the first, the last, and class 64 when it exists as the last tile's only class."""
    return sorted({0, c - 1} | ({64} if c == 65 else set()))


def class_edge_fc(c: int, seq: np.ndarray, seed: int = 97):
    """Seeded FC of c classes for the head input seq [M, K] (which does not depend on the FC: take it from a run with any FC).
    The seeded CRNN's sequence changes little from row to row (a class's logit varies by ~0.9 over the rows, the classes' means by
    ~1.8), so with a seeded bias the same one or two classes win every row.  The bias is therefore centred — every class's mean
    logit over the rows becomes 0, and the winners spread over the classes — and then raised by EDGE_BOOST (two of those standard
    deviations) for edge_winners(c): each of them is the arg-max of some rows, none of all."""
    w, b = seeded_fc(c, seed + c)
    mean = (np.asarray(seq, np.float64) @ stored(w).T).mean(0)
    b = (-mean).astype(np.float32)
    for k in edge_winners(c):
        b[k] += np.float32(EDGE_BOOST)
    return w, b


# ------------------------------------------------------------------------------------------------------------------------ tie rules
# W[c] = W[c % P], b[c] = b[c % P]: every logit has bit-identical copies (the same operands in the same K order, whatever the
# accumulation order is).  The kernel's lane (r, h) of a wave holds, of a 64-class tile, the classes nt * 32 + (j & 3) + 8 * (j >> 2)
# + 4 * h (nt < 2, j < 16); its partner lane r + 32 holds the other h.
#   P = 4 : class c and c + 4 lie in partner half-waves (and c + 8 in the same lane)      -> `om == tm && oi < ti`
#   P = 32: class c and c + 32 are the two 32-class sub-tiles of one lane                 -> the strict `v > tm` in j order
#   P = 64: the copies lie in later tiles                                                -> the strict `tm > run_m`
TIE_CLASSES = 200
TIE_PERIODS = [4, 32, 64]


def periodic_fc(w: np.ndarray, b: np.ndarray, period: int, c: int = TIE_CLASSES):
    """The first `period` rows of (w, b), repeated up to c classes."""
    sel = np.arange(c) % period
    return np.ascontiguousarray(np.asarray(w, np.float32)[sel]), np.ascontiguousarray(np.asarray(b, np.float32)[sel])


# ------------------------------------------------------------------------------------------------------------- saturated soft-max
SATURATE = 16.0          # 2^4: exact in bf16 and fp16; |w| stays below 2^7, far inside fp16's range; margins reach the hundreds


def saturated_fc(w: np.ndarray, b: np.ndarray):
    return np.asarray(w, np.float32) * np.float32(SATURATE), np.asarray(b, np.float32)
