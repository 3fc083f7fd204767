"""Batched device pipeline: pages -> (resize/enhance) -> DBNet -> DB post-process -> crops -> CRNN -> CTC.

This is the arithmetic that fills the reference's engine slot
(/root/reference/backend/services/ocr_service.py:420 `_analyze_with_azure`, :428 `_extract_layout_boxes`);
every stage is a C-ABI call into liblumina_ocr.so.  torch is used for buffers, the stream and two tiny
index-gather ops between stages; one host sync (box counts) separates det from rec.
"""
from __future__ import annotations

import logging
from dataclasses import dataclass, field
from typing import List, Optional, Sequence, Tuple

import numpy as np

from . import arch
from .engine import MAX_BOXES, Engine
from .utils import page_orient
from .utils.image_preprocessing import get_optimal_size

logger = logging.getLogger(__name__)


@dataclass
class PageDetections:
    quads: np.ndarray          # int32 [n, 8]  TL,TR,BR,BL in processed-image pixels
    texts: List[str]
    scores: np.ndarray         # float32 [n]  CTC mean max-prob
    det_scores: np.ndarray     # float32 [n]  DB box score
    width: int = 0             # processed image size
    height: int = 0
    text_ids: Optional[np.ndarray] = None   # int32 [n, 80] class ids (-1 padded): what travels in the multi-GPU gather
    lens: Optional[np.ndarray] = None       # int32 [n]
    cls_labels: Optional[np.ndarray] = None   # int32 [n] 0 / 1 (= "0" / "180"): OcrPipeline(angle_cls=True) only
    cls_scores: Optional[np.ndarray] = None   # float32 [n] probability of the label
    hrules: Optional[np.ndarray] = None       # int32 [nh, 5] x0, y0, x1, y1, area of the page's horizontal rules: OcrPipeline(tables=True) only
    vrules: Optional[np.ndarray] = None       # int32 [nv, 5] vertical rules (both empty when a list overflowed its capacity)
    marks: Optional[np.ndarray] = None        # int32 [m, 8] x0, y0, x1, y1, edge, ink_in, area_in, state of the page's checkboxes:
                                              # OcrPipeline(marks=True) only (empty when the list overflowed its capacity)
    round_marks: Optional[np.ndarray] = None  # int32 [m, 8] the same of the page's radio buttons: OcrPipeline(marks=True, round_marks=True) only
    barcodes: Optional[np.ndarray] = None     # int32 [m, 8] x0, y0, x1, y1, kind, nsym, rows, flags of the page's barcode strips:
                                              # OcrPipeline(barcodes=True) only (empty when the list overflowed its capacity)
    barcode_syms: Optional[np.ndarray] = None  # int32 [m, 64] their symbol values (utils/barcodes.py turns them into text)
    qrcodes: Optional[np.ndarray] = None      # int32 [m, 12] x0, y0, x1, y1, version, level, mask, ndata, errors, rotation, format distance,
                                              # timing mismatches of the page's QR symbols: OcrPipeline(qrcodes=True) only (empty on overflow)
    qr_data: Optional[np.ndarray] = None      # int32 [m, 288] their corrected data codewords (utils/qrcodes.py turns them into text);
                                              # uint8 [m, 2956] with OcrPipeline(qr_max_version > 10)
    datamatrix: Optional[np.ndarray] = None   # int32 [m, 12] x0, y0, x1, y1, rows, cols, ndata, errors, rotation, timing mismatches, L misses, 0
                                              # of the page's Data Matrix symbols: OcrPipeline(datamatrix=True) only (empty on overflow)
    dm_data: Optional[np.ndarray] = None      # int32 [m, 208] their corrected data codewords (utils/datamatrix.py turns them into text);
                                              # uint8 [m, 1560] with OcrPipeline(dm_max_size > 52)
    aztec: Optional[np.ndarray] = None        # int32 [m, 12] x0, y0, x1, y1, layers, compact, codeword width, ndata, errors, rotation, mode errors,
                                              # mismatches of the page's Aztec symbols: OcrPipeline(aztec=True) only (empty on overflow)
    az_data: Optional[np.ndarray] = None      # int32 [m, 320] their corrected data codewords (utils/aztec.py turns them into text);
                                              # uint16 [m, 1664] with OcrPipeline(aztec_max_layers > 11)
    word_quads: Optional[np.ndarray] = None   # int32 [n, 40, 8] the words of every line from the CTC alignment, each in its line's corner
                                              # order: OcrPipeline(word_boxes=True) only, like the three below
    word_spans: Optional[np.ndarray] = None   # int32 [n, 40, 2] first character in texts[i], character count
    word_scores: Optional[np.ndarray] = None  # float32 [n, 40] mean max-prob of the word's characters
    word_counts: Optional[np.ndarray] = None  # int32 [n] words of line i: the rows before it are valid
    turn: Optional[int] = None                # quarter turns that made the page upright, upright = np.rot90(input, turn); everything above
                                              # refers to the upright page: OcrPipeline(page_orient=True).run_oriented only

    def triples(self) -> List[Tuple[Sequence[int], str, float]]:
        return [(self.quads[i].tolist(), self.texts[i], float(self.scores[i])) for i in range(len(self.texts))]

    def line_words(self) -> Optional[List[List[Tuple[int, int, List[int], float]]]]:
        """Per line its words as (first character, count, quad 8 ints, score) in text order — utils/layout.build_layout_boxes' `words`;
        None without OcrPipeline(word_boxes=True)."""
        if self.word_counts is None:
            return None
        return [[(int(self.word_spans[i, k, 0]), int(self.word_spans[i, k, 1]), self.word_quads[i, k].tolist(), float(self.word_scores[i, k]))
                 for k in range(int(self.word_counts[i]))] for i in range(len(self.texts))]


@dataclass
class _Pending:
    """A batch whose device work is enqueued: pinned host copies of the outputs + the event that completes them."""
    b: int
    w: int
    h: int
    counts_h: np.ndarray
    n: int
    processed: object
    host: Optional[list] = None
    event: Optional[object] = None
    gathered: Optional[object] = None   # multi-GPU: handle of dist.PageGather.submit (the batch's results of ALL ranks)
    rules_host: Optional[list] = None   # tables: pinned copies of hrules, vrules, counts
    marks_host: Optional[list] = None   # marks: pinned copies of marks, counts (round_marks: and of round marks, round counts)
    codes_host: dict = field(default_factory=dict)   # per code pass that ran (_CODE_PASSES): pinned copies of codes, symbol values or data codewords, counts
    words_host: Optional[list] = None   # word_boxes: pinned copies of word quads, spans, scores, counts


# the code passes: the pipeline's switch (also the key of _Pending.codes_host), PageDetections' fields for the rows and their symbol
# values or data codewords, and what the overflow warning calls them
_CODE_PASSES = (("barcodes", ("barcodes", "barcode_syms"), "barcodes"),
                ("qrcodes", ("qrcodes", "qr_data"), "QR codes"),
                ("datamatrix", ("datamatrix", "dm_data"), "Data Matrix symbols"),
                ("aztec", ("aztec", "az_data"), "Aztec symbols"))


class OcrPipeline:
    def __init__(self, engine: Engine, charset: Optional[List[str]] = None, max_dimension: int = 2000, post: Optional[dict] = None,
                 recognizer: str = "crnn", gather=None, angle_cls: bool = False, cls_thresh: float = arch.CLS_THRESH,
                 tables: bool = False, table_params: Optional[dict] = None, marks: bool = False, mark_params: Optional[dict] = None,
                 page_orient: bool = False, page_orient_params: Optional[dict] = None, word_boxes: bool = False, round_marks: bool = False,
                 round_mark_params: Optional[dict] = None, barcodes: bool = False, barcode_params: Optional[dict] = None,
                 qrcodes: bool = False, qr_params: Optional[dict] = None, qr_max_version: int = 10, barcode_kinds=arch.BARCODE_KINDS_DEFAULT,
                 datamatrix: bool = False, dm_params: Optional[dict] = None, aztec: bool = False, aztec_params: Optional[dict] = None,
                 aztec_max_layers: int = 11, dm_max_size: int = 52):
        """recognizer: "crnn" (CRNN-MobileNetV3 + BiLSTM, engine.load_rec) or "svtr" (SVTR, engine.load_svtr).
        angle_cls: PaddleOCR's use_angle_cls — every line is classified 0 / 180 degrees (engine.load_cls) before recognition, and a line
        read as 180 with probability > cls_thresh is recognised turned; boxes and reading order are unchanged.  Per-line labels are
        not part of the multi-GPU gather.
        tables: the rules of ruled tables are extracted from the processed pages (engine.table_rules, parameters arch.TABLE_PARAMS or
        table_params) and come back as PageDetections.hrules / vrules; like the per-line labels they stay on their rank.
        marks: the checkboxes of the processed pages (engine.selection_marks, parameters arch.MARK_PARAMS or mark_params) come back as
        PageDetections.marks; they stay on their rank too.  With tables on as well and one threshold for both, the ink mask is
        computed once (engine.rules_and_marks).
        round_marks: with marks, the radio buttons as well (engine.selection_marks_round / rules_and_marks_round, parameters
        arch.ROUND_MARK_PARAMS or round_mark_params) as PageDetections.round_marks; the checkbox rows are the ones without it.  Without
        marks it is a ValueError.
        barcodes: the Code 128 and Code 39 strips of the processed pages (engine.barcodes, parameters arch.BARCODE_PARAMS or
        barcode_params) come back as PageDetections.barcodes / barcode_syms; like the marks they stay on their rank, and with a gather
        the pass is not run.  barcode_kinds: the kinds to read instead, names of arch.BARCODE_KINDS ("ean13", "ean8", "upce", "itf"
        beside the two) or "all"; an unknown name is a ValueError.
        qrcodes: the QR symbols (Model 2, versions 1-10) of the processed pages (engine.qrcodes, parameters arch.QR_PARAMS or qr_params)
        come back as PageDetections.qrcodes / qr_data; they stay on their rank too, and with a gather the pass is not run.
        qr_max_version (10..40): above 10 the pass is engine.qrcodes_versions, which reads versions 11 .. qr_max_version as well;
        qr_data is then uint8 [m, 2956].
        datamatrix: the Data Matrix symbols (ECC 200, up to 52 x 52) of the processed pages (engine.datamatrix, parameters arch.DM_PARAMS
        or dm_params) come back as PageDetections.datamatrix / dm_data; the pass runs behind the QR pass and takes the ink mask the
        earlier passes made at its threshold; with a gather it is not run.
        dm_max_size (52..144): above 52 the pass is engine.datamatrix_sizes, which reads the squares of 64 x 64 .. dm_max_size as well;
        dm_data is then uint8 [m, 1560].
        aztec: the Aztec symbols (compact 1-4 layers, full-range 1-11 layers) of the processed pages (engine.aztec, parameters
        arch.AZTEC_PARAMS or aztec_params; an unknown key is a ValueError) come back as PageDetections.aztec / az_data; the pass runs behind
        the Data Matrix pass and takes the ink mask an earlier pass made at its threshold; with a gather it is not run.
        aztec_max_layers (11..32): above 11 the pass is engine.aztec_layers, which reads full-range symbols of 12 .. aztec_max_layers
        layers as well; az_data is then uint16 [m, 1664].
        page_orient: run_oriented() finds for every page the quarter turns that make it upright (ink profiles for sideways pages,
        parameters arch.PAGE_ORIENT_PARAMS or page_orient_params; the line classifier's majority for upside-down ones, so it needs
        engine.load_cls like angle_cls), turns the raw page on the device and runs the stages below on the upright page.  run /
        run_many / submit_* are the same with it on or off.  Not with a gather.
        word_boxes: the words of every line come from the recogniser's CTC alignment (engine.ctc_decode_words instead of ctc_decode: same
        texts and scores, plus PageDetections.word_quads / word_spans / word_scores / word_counts); it works with both recognisers, with
        angle_cls and inside run_oriented, and adds no host synchronisation.  With a gather the words are not computed: like the table
        rules they are not part of what travels between the ranks.
        gather: a dist.PageGather — multi-GPU runs: every batch's results are all-gathered from the device tensors and
        finish() returns a GatheredPages over the pages of ALL ranks instead of this rank's PageDetections."""
        assert recognizer in ("crnn", "svtr")
        self.recognizer = recognizer
        self.gather = gather
        self.binarize = None     # None | "adaptive" (cv2.adaptiveThreshold semantics) | "simple" (L > 128: the reference without OpenCV)
        self.eng = engine
        self.charset = charset or arch.ctc_charset(engine.num_classes or 6625)
        self._decoder = arch.TextDecoder(self.charset)   # class ids -> strings (vectorised for single-code-point dictionaries)
        self.max_dimension = max_dimension
        self.post = dict(arch.DEFAULT_POST if post is None else post)
        self.angle_cls, self.cls_thresh = bool(angle_cls), float(cls_thresh)
        self.tables = bool(tables)
        self.table_params = dict(arch.TABLE_PARAMS if table_params is None else table_params)
        self.marks = bool(marks)
        self.mark_params = dict(arch.MARK_PARAMS if mark_params is None else mark_params)
        self.round_marks = bool(round_marks)
        self.round_mark_params = dict(arch.ROUND_MARK_PARAMS if round_mark_params is None else round_mark_params)
        if self.round_marks and not self.marks:
            raise ValueError("round_marks needs marks=True: the radio buttons are found in the checkboxes' pass")
        self.barcodes = bool(barcodes)
        self.barcode_params = dict(arch.BARCODE_PARAMS if barcode_params is None else barcode_params)
        self.barcode_kinds = arch.barcode_kinds_mask(barcode_kinds)
        # the default kinds go through lumina_ocr_barcodes, as before there were others
        self._barcode_kinds_arg = None if self.barcode_kinds == arch.barcode_kinds_mask(arch.BARCODE_KINDS_DEFAULT) else self.barcode_kinds
        self.qrcodes = bool(qrcodes)
        self.qr_params = dict(arch.QR_PARAMS if qr_params is None else qr_params)
        self.qr_max_version = int(qr_max_version)
        if not 10 <= self.qr_max_version <= 40:
            raise ValueError("qr_max_version must be 10..40, not %r" % (qr_max_version,))
        self.datamatrix = bool(datamatrix)
        self.dm_params = dict(arch.DM_PARAMS if dm_params is None else dm_params)
        self.dm_max_size = int(dm_max_size)
        if not 52 <= self.dm_max_size <= 144:
            raise ValueError("dm_max_size must be 52..144, not %r" % (dm_max_size,))
        self.aztec = bool(aztec)
        self.aztec_params = dict(arch.AZTEC_PARAMS if aztec_params is None else aztec_params)
        if set(self.aztec_params) - set(arch.AZTEC_PARAMS):
            raise ValueError("aztec_params: unknown keys %s" % sorted(set(self.aztec_params) - set(arch.AZTEC_PARAMS)))
        self.aztec_max_layers = int(aztec_max_layers)
        if not 11 <= self.aztec_max_layers <= 32:
            raise ValueError("aztec_max_layers must be 11..32, not %r" % (aztec_max_layers,))
        self.page_orient = bool(page_orient)
        self.word_boxes = bool(word_boxes)
        self.space_id = self.charset.index(" ") if " " in self.charset else -1   # the class words split on (-1: a line is one word)
        self.page_orient_params = dict(arch.PAGE_ORIENT_PARAMS if page_orient_params is None else page_orient_params)
        if self.angle_cls and not engine.cls_loaded:
            raise ValueError("angle_cls needs the orientation classifier's weights (Engine.load_cls)")
        if self.page_orient and not engine.cls_loaded:
            raise ValueError("page_orient needs the orientation classifier's weights (Engine.load_cls)")
        if self.page_orient and gather is not None:
            raise ValueError("page_orient does not run with a gather: a page's turn and its processed size stay on their rank")

    # ---- stages -------------------------------------------------------------------------
    def preprocess(self, pages, enhance: bool = True, deskew: bool = False):
        """uint8 [B,H,W,3] device -> processed uint8 [B,H',W',3]: the reference's order (image_preprocessing.py:559-628 /
        :191-242): resize -> [deskew] -> contrast 1.2 -> sharpness 1.1 (JPEG hand-off is the provider's)."""
        b, h, w, _ = pages.shape
        nw, nh = get_optimal_size(w, h, self.max_dimension)
        x = pages if (nw, nh) == (w, h) else self.eng.resize_lanczos(pages, nh, nw)
        if deskew:
            x, self.last_skew_angles = self.eng.deskew(x)
        if self.binarize:        # (:613-622) binarisation replaces contrast + sharpness
            return self.eng.binarize(x, adaptive=self.binarize == "adaptive")
        return self.eng.enhance(x, 1.2, 1.1) if enhance else x

    def detect(self, processed):
        b, h, w, _ = processed.shape
        prob = self.eng.det_forward(processed)
        return self.eng.det_postprocess(prob, h, w, **self.post)

    def recognize(self, processed, boxes, scores, counts) -> List[PageDetections]:
        return self.finish(self.submit_recognize(processed, boxes, scores, counts))[0]

    # ---- split submission: lets the host-side decode of batch k overlap the device work of batch k+1 ----------------
    def submit_detect(self, pages, enhance: bool = True, deskew: bool = False):
        """Enqueue resize/[deskew]/enhance + DBNet + DB post-process; no host synchronisation. -> handle for submit_recognize."""
        processed = self.preprocess(pages, enhance, deskew)
        return (processed,) + tuple(self.detect(processed))

    def submit_recognize(self, processed, boxes, scores, counts) -> "_Pending":
        """One host sync (box counts), then crop + CRNN + CTC and the device->pinned-host copies are enqueued. -> pending."""
        rules, marks, codes, qrs, dms, azs = self._submit_page_analysis(processed)   # enqueued before the sync below: it runs while the host waits for the box counts
        counts_h = counts.cpu().numpy()  # the one host sync of the pipeline
        return self._submit_lines(processed, boxes, scores, counts_h, rules, marks, barcodes=codes, qrcodes=qrs, datamatrix=dms, aztec=azs)

    def _submit_datamatrix(self, processed, mask, mask_at):
        """Enqueue the Data Matrix pass -> (codes, data codewords, counts) device tensors; mask: the ink mask an earlier pass made at the
        threshold mask_at, or None."""
        dp = self.dm_params
        mask_in = mask if mask is not None and mask_at == dp["threshold"] else None
        if self.dm_max_size == 52:
            return self.eng.datamatrix(processed, mask_in=mask_in, **dp)
        return self.eng.datamatrix_sizes(processed, self.dm_max_size, mask_in=mask_in, **dp)

    def _submit_page_analysis(self, processed):
        """_submit_passes, then the Aztec pass behind them -> (rules, marks, codes, qr codes, data matrix symbols, aztec symbols), None
        where a pass is off.  With the Aztec pass off this is _submit_passes as it ever was."""
        if not (self.aztec and self.gather is None):
            return self._submit_passes(processed) + (None,)
        ap = self.aztec_params
        handed = []
        out = self._submit_passes(processed, handed)
        mask = handed[0][0] if handed and handed[0][1] == ap["threshold"] else None
        if self.aztec_max_layers == 11:
            return out + (self.eng.aztec(processed, mask_in=mask, **ap),)
        return out + (self.eng.aztec_layers(processed, self.aztec_max_layers, mask_in=mask, **ap),)

    def _submit_passes(self, processed, handed: Optional[list] = None):
        """Enqueue the table rules, selection marks, barcodes, QR codes and Data Matrix symbols of the processed pages -> (rules, marks,
        codes, qr codes, data matrix symbols), None where a pass is off.  The barcode pass takes the ink mask from the marks or the tables
        call when that call ran on its own at the barcodes' threshold; the joint rules-and-marks call hands no mask out, so behind it the barcode pass computes its own.  The QR
        pass takes the mask the same way, or from the barcode pass when that one computed it at the QR threshold.  The Data Matrix pass
        runs last, on the mask of whichever earlier pass made one at its threshold (the barcode or the QR pass hands its own out).
        handed: a list that receives (mask, threshold) when an earlier pass made a mask (the Aztec pass asks, and the passes then hand
        their mask on as they do for the Data Matrix pass); without it nothing runs differently."""
        on = self.gather is None
        if (self.datamatrix or handed is not None) and on:   # behind the other passes, with the mask they made when it is the last pass's threshold too
            last = self.dm_params if self.datamatrix else self.aztec_params
            want = (self.barcode_params["threshold"] if self.barcodes else self.qr_params["threshold"] if self.qrcodes else last["threshold"])
            rules, marks, mask = self._submit_rules_marks(processed, mask_at=want)
            codes = qrs = None
            if self.barcodes:
                codes = self._submit_barcodes(processed, mask, mask_out=mask is None)
                if mask is None:
                    codes, mask = codes[:3], codes[3]
            if self.qrcodes:
                qmask = mask if self.qr_params["threshold"] == want else None
                qrs = self._submit_qrcodes(processed, qmask, debug=mask is None)
                if mask is None:
                    qrs, mask, want = qrs[:3], qrs[3], self.qr_params["threshold"]
            if handed is not None and mask is not None:
                handed.append((mask, want))
            return rules, marks, codes, qrs, self._submit_datamatrix(processed, mask, want) if self.datamatrix else None
        want = self.barcode_params["threshold"] if self.barcodes and on else (self.qr_params["threshold"] if self.qrcodes and on else None)
        rules, marks, mask = self._submit_rules_marks(processed, mask_at=want)
        if not (self.qrcodes and on):
            return rules, marks, self._submit_barcodes(processed, mask), None, None
        if self.barcodes and self.qr_params["threshold"] == want:
            codes = self._submit_barcodes(processed, mask, mask_out=mask is None)
            if mask is None:
                codes, mask = codes[:3], codes[3]
        else:
            codes = self._submit_barcodes(processed, mask)
            mask = mask if self.qr_params["threshold"] == want else None
        return rules, marks, codes, self._submit_qrcodes(processed, mask), None

    def _submit_qrcodes(self, processed, mask_in=None, debug: bool = False):
        """Enqueue the QR pass: today's call at qr_max_version = 10, the all-versions call (byte data rows of 2956) above it."""
        if self.qr_max_version == 10:
            return self.eng.qrcodes(processed, mask_in=mask_in, debug=debug, **self.qr_params)
        return self.eng.qrcodes_versions(processed, self.qr_max_version, mask_in=mask_in, debug=debug, **self.qr_params)

    def _submit_barcodes(self, processed, mask_in=None, mask_out: bool = False):
        """Enqueue the barcode pass of the processed pages -> (codes, symbol values, counts) device tensors, or None; with mask_out the
        ink mask the pass computed comes fourth."""
        if not self.barcodes or self.gather is not None:
            return None
        bp = self.barcode_params
        return self.eng.barcodes(processed, bp["threshold"], bp["quiet"], bp["max_dist"], bp["min_rows"], bp["row_gap"], bp["max_codes"],
                                 mask_in=mask_in, debug=mask_out, kinds=self._barcode_kinds_arg)

    def _submit_rules_marks(self, processed, mask_at: Optional[int] = None):
        """Enqueue the table rules and / or selection marks of the processed pages -> (rules, marks, mask): device tensors, or None each; with
        round_marks the marks are four tensors: marks, counts, round marks, round counts.  mask: the ink mask int64 [b,H,ceil(W/64)] of a
        call made here on its own at the threshold mask_at, else None."""
        rules = marks = mask = None
        if self.gather is None and (self.tables or self.marks):
            tp, mp = self.table_params, self.mark_params
            if self.tables and self.marks and tp["threshold"] == mp["threshold"]:
                if self.round_marks:
                    both = self.eng.rules_and_marks_round(processed, tp["threshold"], tp["gap"], tp["min_len"], tp["max_thick"], tp["max_rules"],
                                                          mp["min_side"], mp["max_side"], mp["max_marks"], self.round_mark_params)
                else:
                    both = self.eng.rules_and_marks(processed, tp["threshold"], tp["gap"], tp["min_len"], tp["max_thick"], tp["max_rules"],
                                                    mp["min_side"], mp["max_side"], mp["max_marks"])
                rules, marks = both[:3], both[3:]
            else:
                if self.tables:
                    share = mask_at is not None and tp["threshold"] == mask_at
                    rules = self.eng.table_rules(processed, tp["threshold"], tp["gap"], tp["min_len"], tp["max_thick"], tp["max_rules"], debug=share)
                    if share:
                        rules, mask = rules[:3], rules[3]
                share = mask is None and mask_at is not None and mp["threshold"] == mask_at
                if self.marks and self.round_marks:
                    marks = self.eng.selection_marks_round(processed, mp["threshold"], mp["min_side"], mp["max_side"], mp["max_marks"],
                                                           self.round_mark_params, debug=share)
                elif self.marks:
                    marks = self.eng.selection_marks(processed, mp["threshold"], mp["min_side"], mp["max_side"], mp["max_marks"], debug=share)
                if self.marks and share:
                    marks, mask = marks[:-1], marks[-1]
        return rules, marks, mask

    @staticmethod
    def _select_lines(boxes, scores, counts_h, b: int):
        """The valid (page, slot) pairs are known on the host (counts): one small index upload + two gathers, instead of boolean-mask
        indexing (each of those runs a nonzero kernel and synchronises to learn its output size). -> quads, det scores, page index"""
        import torch
        n = int(counts_h.sum())
        cap = boxes.shape[1]
        page_h = np.repeat(np.arange(b, dtype=np.int64), counts_h)
        slot_h = np.arange(n, dtype=np.int64) - np.repeat(np.cumsum(counts_h) - counts_h, counts_h)
        flat = torch.from_numpy(page_h * cap + slot_h).to(boxes.device, non_blocking=True)
        quads = boxes.view(-1, 8).index_select(0, flat)
        det_sc = scores.view(-1).index_select(0, flat)
        page_idx = torch.from_numpy(page_h.astype(np.int32)).to(boxes.device, non_blocking=True)
        return quads, det_sc, page_idx

    def _submit_lines(self, processed, boxes, scores, counts_h, rules, marks, lines=None, barcodes=None, qrcodes=None, datamatrix=None, aztec=None) -> "_Pending":
        """submit_recognize after its sync.  lines: (quads, det scores, page index, cls_forward's outputs or None) of the counted lines when
        the caller has them already (run_oriented: the vote needed them), else they are selected and classified here."""
        import torch
        b, h, w, _ = processed.shape
        n = int(counts_h.sum())
        pend = _Pending(b=b, w=w, h=h, counts_h=counts_h, n=n, processed=processed)
        if rules is not None:
            pend.rules_host = [torch.empty(t.shape, dtype=t.dtype, pin_memory=True).copy_(t, non_blocking=True) for t in rules]
        if marks is not None:
            pend.marks_host = [torch.empty(t.shape, dtype=t.dtype, pin_memory=True).copy_(t, non_blocking=True) for t in marks]
        for kind, tensors in (("barcodes", barcodes), ("qrcodes", qrcodes), ("datamatrix", datamatrix), ("aztec", aztec)):
            if tensors is not None:
                pend.codes_host[kind] = [torch.empty(t.shape, dtype=t.dtype, pin_memory=True).copy_(t, non_blocking=True) for t in tensors]
        if self.gather is not None:
            self.gather.begin(counts_h)          # capacity all-reduce runs beside the recogniser
        if n == 0:
            if self.gather is not None:          # every rank takes part in the collective, with or without lines
                e = lambda *shape, dt=torch.int32: torch.empty(shape, dtype=dt, device=boxes.device)
                pend.gathered = self.gather.submit(counts_h, e(0, 8), e(0, dt=torch.float32), e(0, 80), e(0), e(0, dt=torch.float32))
            elif pend.rules_host is not None or pend.marks_host is not None or pend.codes_host:
                pend.event = torch.cuda.Event()
                pend.event.record(torch.cuda.current_stream(processed.device))
            return pend
        if lines is None:
            quads, det_sc, page_idx = self._select_lines(boxes, scores, counts_h, b)
            cls = None
            if self.angle_cls:   # classifier crops -> labels and flip flags -> turned recognition crops, all on the device
                ccrops, cwidths = self.eng.cls_crop(processed, quads, page_idx)
                cls = self.eng.cls_forward(ccrops, cwidths, self.cls_thresh)
        else:
            quads, det_sc, page_idx, cls = lines
        crops, widths = self.eng.rec_crop(processed, quads, page_idx, flip=None if cls is None else cls[2])
        idx, prob = (self.eng.svtr_forward if self.recognizer == "svtr" else self.eng.rec_forward)(crops, widths)
        words = None
        if self.word_boxes and self.gather is None:
            text, length, score, *words = self.eng.ctc_decode_words(idx, prob, quads, widths, None if cls is None else cls[2], self.space_id)
        else:
            text, length, score = self.eng.ctc_decode(idx, prob)
        if self.gather is not None:
            pend.gathered = self.gather.submit(counts_h, quads, det_sc, text, length, score)
            return pend
        outs = (text, length, score, quads, det_sc) + (() if cls is None else cls[:2])
        pend.host = [torch.empty(t.shape, dtype=t.dtype, pin_memory=True).copy_(t, non_blocking=True) for t in outs]
        if words is not None:
            pend.words_host = [torch.empty(t.shape, dtype=t.dtype, pin_memory=True).copy_(t, non_blocking=True) for t in words]
        pend.event = torch.cuda.Event()
        pend.event.record(torch.cuda.current_stream(processed.device))
        return pend

    def finish(self, pend: "_Pending") -> Tuple[List[PageDetections], "object"]:
        """Wait for the pending batch's copies and build the per-page results (string decode on the host)."""
        b, w, h = pend.b, pend.w, pend.h
        if pend.gathered is not None:
            return self.gather.finish(pend.gathered), pend.processed
        if pend.event is not None:
            pend.event.synchronize()
        rules = self._page_rules(pend)
        marks = self._page_marks(pend)
        rounds = self._page_marks(pend, 2)
        codes = [{} for _ in range(b)]   # per page: PageDetections' fields of the four code passes
        for kind, fields, _ in _CODE_PASSES:
            for p, pair in enumerate(self._page_barcodes(pend, kind)):
                codes[p].update(zip(fields, pair))
        if pend.n == 0:
            nw = self._empty_words() if self.word_boxes else {}
            return [PageDetections(np.zeros((0, 8), np.int32), [], np.zeros(0, np.float32), np.zeros(0, np.float32), w, h,
                                   hrules=rules[p][0], vrules=rules[p][1], marks=marks[p], round_marks=rounds[p], **codes[p], **nw)
                    for p in range(b)], pend.processed
        text_h, len_h, score_h, quads_h, det_h, *cls_h = (t.numpy() for t in pend.host)
        all_texts = self._decoder.decode(text_h, len_h)
        words_h = None
        if pend.words_host is not None:
            words_h = [t.numpy() for t in pend.words_host]
            words_h[1] = self._string_spans(words_h[1], words_h[3], text_h)
        out, off = [], 0
        for p in range(b):
            c = int(pend.counts_h[p])
            texts = all_texts[off:off + c]
            out.append(PageDetections(quads_h[off:off + c], texts, score_h[off:off + c], det_h[off:off + c], w, h,
                                      text_h[off:off + c], len_h[off:off + c],
                                      *((cls_h[0][off:off + c], cls_h[1][off:off + c]) if cls_h else ()),
                                      hrules=rules[p][0], vrules=rules[p][1], marks=marks[p], round_marks=rounds[p], **codes[p],
                                      **({} if words_h is None else dict(zip(self._WORD_FIELDS, (t[off:off + c] for t in words_h))))))
            off += c
        return out, pend.processed

    _WORD_FIELDS = ("word_quads", "word_spans", "word_scores", "word_counts")

    @staticmethod
    def _empty_words() -> dict:
        from .engine import MAX_WORDS
        return dict(word_quads=np.zeros((0, MAX_WORDS, 8), np.int32), word_spans=np.zeros((0, MAX_WORDS, 2), np.int32),
                    word_scores=np.zeros((0, MAX_WORDS), np.float32), word_counts=np.zeros(0, np.int32))

    def _string_spans(self, spans: np.ndarray, counts: np.ndarray, text_ids: np.ndarray) -> np.ndarray:
        """The device counts a word's span in classes; texts[i] is indexed in code points.  They are the same for a dictionary of single
        code points (every PP-OCR key file); otherwise the spans are moved to code points here."""
        if self._decoder.single:
            return spans
        width = np.array([len(c) for c in self.charset], np.int64)
        out = spans.copy()
        for i in np.nonzero(counts)[0]:
            cum = np.concatenate([[0], np.cumsum(width[np.maximum(text_ids[i], 0)])])
            for k in range(int(counts[i])):
                a, n = int(spans[i, k, 0]), int(spans[i, k, 1])
                out[i, k] = (cum[a], cum[a + n] - cum[a])
        return out

    def _page_rules(self, pend: "_Pending"):
        """-> per page (hrules [nh,5], vrules [nv,5]) from the pending batch's host copies, or (None, None) without tables.  A page whose
        true count exceeds the capacity of a list has no guaranteed rules: it is treated as having none."""
        if pend.rules_host is None:
            return [(None, None)] * pend.b
        hr, vr, cnt = (t.numpy() for t in pend.rules_host)
        cap = hr.shape[1]
        out = []
        for p in range(pend.b):
            nh, nv = int(cnt[p, 0]), int(cnt[p, 1])
            if nh > cap or nv > cap:
                logger.warning("page %d of the batch has %d horizontal / %d vertical rules, more than max_rules = %d: no tables are built for it", p, nh, nv, cap)
                nh = nv = 0
            out.append((hr[p, :nh].copy(), vr[p, :nv].copy()))
        return out

    def _page_marks(self, pend: "_Pending", first: int = 0):
        """-> per page marks [m,8] from the pending batch's host copies, or None without marks.  A page whose true count exceeds the
        capacity has no rows: it is treated as having no marks.  first = 2: the same for the round marks."""
        if pend.marks_host is None or len(pend.marks_host) < first + 2:
            return [None] * pend.b
        rows, cnt = (t.numpy() for t in pend.marks_host[first:first + 2])
        cap = rows.shape[1]
        out = []
        for p in range(pend.b):
            m = int(cnt[p])
            if m > cap:
                logger.warning("page %d of the batch has %d %sselection marks, more than max_marks = %d: none are reported for it", p, m, "round " if first else "", cap)
                m = 0
            out.append(rows[p, :m].copy())
        return out

    def _page_barcodes(self, pend: "_Pending", kind: str = "barcodes"):
        """-> per page (codes [m,8], symbol values [m,64]) from the pending batch's host copies, or (None, None) without barcodes.  A
        page whose true count exceeds the capacity has no rows: it is treated as having no barcodes.  kind: another row of _CODE_PASSES
        for the same of that pass's copies, "qrcodes": (codes [m,12], data codewords [m,288], or bytes [m,2956] above qr_max_version 10);
        "datamatrix": (codes [m,12], data codewords [m,208], or uint8 [m,1560] above dm_max_size 52); "aztec": (codes [m,12], data codewords [m,320], or uint16 [m,1664] above
        aztec_max_layers 11)."""
        host = pend.codes_host.get(kind)
        if host is None:
            return [(None, None)] * pend.b
        noun = next(noun for k, _, noun in _CODE_PASSES if k == kind)
        rows, syms, cnt = (t.numpy() for t in host)
        cap = rows.shape[1]
        out = []
        for p in range(pend.b):
            m = int(cnt[p])
            if m > cap:
                logger.warning("page %d of the batch has %d %s, more than max_codes = %d: none are reported for it", p, m, noun, cap)
                m = 0
            out.append((rows[p, :m].copy(), syms[p, :m].copy()))
        return out

    def run_many(self, batches, enhance: bool = True, deskew: bool = False):
        """Generator over batches: yields (detections, processed) per batch, in order, with batch k's host decode running
        while the device works on batch k+1's detection half."""
        pending = None
        for pages in batches:
            h = self.submit_detect(pages, enhance, deskew)
            if pending is not None:
                yield self.finish(pending)
            pending = self.submit_recognize(*h)
        if pending is not None:
            yield self.finish(pending)

    def run(self, pages, enhance: bool = True, deskew: bool = False) -> Tuple[List[PageDetections], "object"]:
        """-> (per-page detections, processed pages on device)."""
        return self.finish(self.submit_recognize(*self.submit_detect(pages, enhance, deskew)))

    # ---- page orientation -----------------------------------------------------------------------------------------------
    def _submit_first_pass(self, pages, enhance: bool, deskew: bool):
        """The stages up to the classifier on pages that are upright or upside-down, the vote, then recognition of the pages voted
        upright from the detections they have. -> (pending, bool [b]: voted upside-down; those pages have no lines in the pending)"""
        import torch
        processed, boxes, scores, counts = self.submit_detect(pages, enhance, deskew)
        b = processed.shape[0]
        rules, marks, codes, qrs, dms, azs = self._submit_page_analysis(processed)
        counts_h = counts.cpu().numpy()
        if int(counts_h.sum()) == 0:
            return self._submit_lines(processed, boxes, scores, counts_h, rules, marks, barcodes=codes, qrcodes=qrs, datamatrix=dms, aztec=azs), np.zeros(b, bool)
        quads, det_sc, page_idx = self._select_lines(boxes, scores, counts_h, b)
        ccrops, cwidths = self.eng.cls_crop(processed, quads, page_idx)
        cls = self.eng.cls_forward(ccrops, cwidths, self.cls_thresh)
        votes = self.eng.page_vote(cls[2], page_idx, b).cpu().numpy()   # the second small read: b x 2 integers
        flipped = page_orient.upside_down(votes, self.page_orient_params["min_lines"])
        if flipped.any():   # their lines leave the first pass: the second one reads the turned raw page
            keep_h = np.nonzero(~flipped[np.repeat(np.arange(b), counts_h)])[0]
            keep = torch.from_numpy(keep_h).to(boxes.device, non_blocking=True)
            quads, det_sc, page_idx = (t.index_select(0, keep) for t in (quads, det_sc, page_idx))
            cls = tuple(t.index_select(0, keep) for t in cls)
            counts_h = np.where(flipped, 0, counts_h).astype(counts_h.dtype)
        lines = (quads, det_sc, page_idx, cls if self.angle_cls else None)
        return self._submit_lines(processed, boxes, scores, counts_h, rules, marks, lines=lines, barcodes=codes, qrcodes=qrs, datamatrix=dms, aztec=azs), flipped

    def run_oriented_groups(self, pages, enhance: bool = True, deskew: bool = False):
        """run_oriented's work, as the passes made it: -> [(input indices, detections, processed pages [m,H',W',3] on the device)], every
        input page in exactly one entry; detections carry `turn`."""
        import torch
        if not self.page_orient:
            raise ValueError("run_oriented needs OcrPipeline(page_orient=True)")
        pp = self.page_orient_params
        dev = pages.device
        n = pages.shape[0]
        _, sideways = self.eng.page_quarter(pages, pp["threshold"], pp["ratio"])
        sideways_h = sideways.cpu().numpy()   # the first small read: which pages make the W x H group
        index = lambda idxs: torch.tensor(idxs, dtype=torch.int32, device=dev)
        first = []
        for quarter, idxs in page_orient.first_pass_groups(sideways_h):
            sub = pages if quarter == 0 and len(idxs) == n else self.eng.page_turn(pages, index(idxs), quarter)
            first.append((quarter, idxs) + self._submit_first_pass(sub, enhance, deskew))
        second = []
        for quarter, idxs, _, flipped in first:
            turn, again, _ = page_orient.second_pass(quarter, idxs, flipped)
            if again:
                turned = self.eng.page_turn(pages, index(again), turn)
                second.append((turn, again, self.submit_recognize(*self.submit_detect(turned, enhance, deskew))))
        out = []
        for quarter, idxs, pend, flipped in first:
            dets, processed = self.finish(pend)
            keep = np.nonzero(~flipped)[0].tolist()
            if not keep:
                continue
            for k in keep:
                dets[k].turn = quarter
            whole = len(keep) == len(idxs)
            out.append(([idxs[k] for k in keep], dets if whole else [dets[k] for k in keep],
                        processed if whole else processed.index_select(0, torch.tensor(keep, dtype=torch.int64, device=dev))))
        for turn, idxs, pend in second:
            dets, processed = self.finish(pend)
            for d in dets:
                d.turn = turn
            out.append((idxs, dets, processed))
        return out

    def run_oriented(self, pages, enhance: bool = True, deskew: bool = False) -> Tuple[List[PageDetections], list]:
        """pages uint8 [B,H,W,3] on the device, each lying any of the four ways -> (per-page detections in input order, each of the upright
        page and with its `turn`; per-page processed page uint8 [H',W',3] on the device, upright).  Two small host reads more than run()
        (the sideways flags, the votes), and a second pass over the pages found upside-down."""
        groups = self.run_oriented_groups(pages, enhance, deskew)
        dets = page_orient.reassemble(pages.shape[0], [(idxs, d) for idxs, d, _ in groups])
        processed = page_orient.reassemble(pages.shape[0], [(idxs, list(p.unbind(0))) for idxs, _, p in groups])
        return dets, processed
