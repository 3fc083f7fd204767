"""OCR provider backed by the MI355X det+rec engine — a drop-in for the reference's provider module.

Replace /root/reference/backend/services/ocr_service.py with this module: callers do
`from services.ocr_service import OCRService, DocumentOCRResult` and `OCRService()`
(/root/reference/backend/services/extraction_service.py:46, :207).  Mirrored surface (reference file:line):
  OCROutput :48-79, DocumentOCRResult :82-104 (same fields, same to_dict keys; processed_image_bytes excluded)
  OCRService: singleton :126-135, process_image_sync :477-502, _process_single_image_sync :398-475,
    process_pdf_sync :508-602, process_pdf_as_images_sync :604-660, process_image/process_pdf (async) :666-693,
    process_document :695-731, get_status :759-771, preload_model :773-775, is_model_loaded :777-780, cleanup :782-795
  module level: ocr_service :802, ocr_node :805-829, preload_ocr_model :832-837, get_ocr_status :840-842
Errors are data, never exceptions (:464-475, :653-660).  Box coordinates, page_width_inches/page_height_inches
and processed_image_bytes (JPEG) all refer to the processed image's pixel grid.
There is no CPU fallback: without the HIP library / a GPU every call returns success=False with the reason.
"""
from __future__ import annotations

import asyncio
import io
import logging
import os
import threading
import time
from dataclasses import dataclass, field
from pathlib import Path
from typing import Any, Dict, List, Optional, Union

import numpy as np
from PIL import Image

from .. import arch
from ..utils import layout
from ..utils import barcodes as barcode_layout
from ..utils import marks as mark_layout
from ..utils import page_orient
from ..utils import qrcodes as qr_layout
from ..utils import datamatrix as dm_layout
from ..utils import aztec as aztec_layout
from ..utils import pdf_pages, tiff_pages
from ..utils import tables as table_layout
from ..utils.image_preprocessing import ImagePreprocessor, get_optimal_size

logger = logging.getLogger(__name__)

SUPPORTED_IMAGE_TYPES = ("png", "jpg", "jpeg", "webp", "bmp", "tiff")
PNG_SIGNATURE = b"\x89PNG\r\n\x1a\n"
JP2_SIGNATURE = b"\x00\x00\x00\x0cjP  \r\n\x87\n"   # the signature box of a JP2 / JPX file
J2K_SIGNATURE = b"\xff\x4f\xff\x51"                 # SOC + SIZ: a raw JPEG 2000 codestream
JP2_FILE_TYPES = ("jp2", "j2k", "jpx")                # process_document sends these to the image path with LUMINA_OCR_DEVICE_JP2=1


@dataclass
class OCROutput:
    markdown: str = ""
    html: str = ""
    json_output: Dict[str, Any] = field(default_factory=dict)
    processing_time_ms: int = 0
    success: bool = True
    error: Optional[str] = None
    page_number: int = 1
    image_width: int = 0
    image_height: int = 0
    layout_boxes: List[Dict[str, Any]] = field(default_factory=list)
    processed_image_bytes: Optional[bytes] = None
    page_width_inches: float = 0.0
    page_height_inches: float = 0.0

    def to_dict(self) -> Dict[str, Any]:
        keys = ("markdown", "html", "json_output", "processing_time_ms", "success", "error", "page_number", "image_width",
                "image_height", "layout_boxes", "page_width_inches", "page_height_inches")
        return {k: getattr(self, k) for k in keys}


@dataclass
class DocumentOCRResult:
    pages: List[OCROutput] = field(default_factory=list)
    total_pages: int = 0
    total_processing_time_ms: int = 0
    success: bool = True
    error: Optional[str] = None
    combined_markdown: str = ""
    combined_html: str = ""
    combined_layout_boxes: List[Dict[str, Any]] = field(default_factory=list)

    def to_dict(self) -> Dict[str, Any]:
        d = {k: getattr(self, k) for k in ("total_pages", "total_processing_time_ms", "success", "error", "combined_markdown",
                                           "combined_html", "combined_layout_boxes")}
        return {"pages": [p.to_dict() for p in self.pages], **d}


def _ms_since(t0: float) -> int:
    return int((time.time() - t0) * 1000)


class OCRService:
    """Process-wide singleton; pages are serialised by a semaphore exactly like the reference (:157, :404)."""

    _instance = None
    _lock = threading.Lock()

    def __new__(cls):
        if cls._instance is None:
            with cls._lock:
                if cls._instance is None:
                    cls._instance = super().__new__(cls)
                    cls._instance._initialized = False
        return cls._instance

    def __init__(self):
        if getattr(self, "_initialized", False):
            return
        self._engine = None
        self._pipeline = None
        self._engine_lock = threading.Lock()
        self._semaphore = threading.Semaphore(1)
        self.max_dimension = int(os.environ.get("OCR_MAX_IMAGE_DIMENSION", 2000))
        # settings.OCR_APPLY_DESKEW (/root/reference/backend/config.py:85, default True; used at ocr_service.py:150, :412-417)
        self.apply_deskew = os.environ.get("OCR_APPLY_DESKEW", "true").lower() not in ("0", "false", "no")
        # settings.PREPROCESSING_APPLY_BINARIZE (ocr_service.py:151, default False): "true" / "adaptive" = cv2.adaptiveThreshold semantics,
        # "simple" = the L > 128 threshold the reference falls back to without OpenCV (image_preprocessing.py:473-475)
        b = os.environ.get("PREPROCESSING_APPLY_BINARIZE", "false").lower()
        self.device_jpeg = os.environ.get("LUMINA_OCR_DEVICE_JPEG", "1").lower() not in ("0", "false", "no")   # baseline JPEG inputs are decoded on the device
        # LUMINA_OCR_PROGRESSIVE_JPEG=1: progressive JPEG files (SOF2) of the device subset, and progressive /DCTDecode pages of
        # LUMINA_OCR_PDF_SCANS, are decoded on the device as well (lumina_ocr_jpeg_decode_progressive).  Off by default: a progressive
        # file is then decoded by Pillow, and exactly the calls made without the option are made.
        self.progressive_jpeg = os.environ.get("LUMINA_OCR_PROGRESSIVE_JPEG", "0").lower() not in ("", "0", "false", "no")
        # LUMINA_OCR_DEVICE_PNG=1: non-interlaced PNG inputs of 8 bits or less and lazily opened PNG pages (pdf2image) are decoded on the
        # device.  Off by default: measured slower than Pillow for single pages and for 300 dpi batches
        self.device_png = os.environ.get("LUMINA_OCR_DEVICE_PNG", "0").lower() not in ("0", "false", "no")
        # LUMINA_OCR_DEVICE_WEBP=1: lossless WebP inputs (one VP8L chunk, bare or inside VP8X; recognised by magic) are decoded on the device
        # (lumina_ocr_webp_decode); lossy and animated files, and files with an XMP chunk, still go to Pillow.  Off by default: exactly
        # the calls made without the option are made (the measurements are in DESIGN.md §8.3)
        self.device_webp = os.environ.get("LUMINA_OCR_DEVICE_WEBP", "0").lower() not in ("", "0", "false", "no")
        self._webp_reasons_logged = set()
        # LUMINA_OCR_WEBP_LOSSY=1 (takes effect only together with LUMINA_OCR_DEVICE_WEBP, ignored without it): lossy WebP files (one VP8
        # key frame without ALPH) are decoded on the device as well; the provider then calls lumina_ocr_webp_probe_lossy /
        # _decode_lossy for every WebP input, lossless ones included.  Off by default.
        self.webp_lossy = os.environ.get("LUMINA_OCR_WEBP_LOSSY", "0").lower() not in ("", "0", "false", "no")
        # LUMINA_OCR_PDF_SCANS=1: a PDF page that is one image over the whole MediaBox (a scan: DCT, Flate or CCITT of any /K) is decoded
        # on the device from its embedded stream, at the image's own sample grid, instead of being rasterised by pdf2image / poppler; other
        # pages still go to pdf_to_images.  Off by default: process_pdf_sync is then the rasterise-and-batch path alone.
        self.device_pdf = os.environ.get("LUMINA_OCR_PDF_SCANS", "0").lower() not in ("", "0", "false", "no")
        # LUMINA_OCR_PDF_LAYERS=1 (with LUMINA_OCR_PDF_SCANS=1; ignored without it): pages painted from several images (strips, a
        # stencil over a background, images with /SMask or a /Mask stream) and pages with an invisible text layer are read as well:
        # their layers join the decode groups and lumina_ocr_page_compose puts them together.  Off by default: exactly the calls made
        # without the option are made.
        self.pdf_layers = os.environ.get("LUMINA_OCR_PDF_LAYERS", "0").lower() not in ("", "0", "false", "no")
        # LUMINA_OCR_PDF_JBIG2=1 (with LUMINA_OCR_PDF_SCANS=1; ignored without it): /JBIG2Decode page images, and with
        # LUMINA_OCR_PDF_LAYERS the JBIG2 stencils and masks of layered pages, are decoded on the device where they are made of generic
        # regions (lumina_ocr_jbig2_decode); a symbol-coded or damaged stream goes where a refused page goes.  Off by default: exactly
        # the calls made without the option are made.
        self.pdf_jbig2 = os.environ.get("LUMINA_OCR_PDF_JBIG2", "0").lower() not in ("", "0", "false", "no")
        # LUMINA_OCR_DEVICE_TIFF=1: stripped TIFF inputs (LZW, PackBits, Deflate, Group 4, Group 3, CCITT RLE, uncompressed; utils/tiff_pages.py) are decoded on
        # the device, process_tiff_sync reads every page of a multi-page TIFF, and process_document sends "tiff" and "tif" there.  Off by
        # default: a TIFF is then decoded by Pillow, first frame only, and every output is exactly the one without the option.
        self.device_tiff = os.environ.get("LUMINA_OCR_DEVICE_TIFF", "0").lower() not in ("", "0", "false", "no")
        # LUMINA_OCR_DEVICE_JP2=1: JPEG 2000 inputs (JP2 / JPX-baseline files and raw codestreams, recognised by their magic) of the
        # device subset (5/3 reversible, one tile ...: lumina_ocr_jp2_decode) are decoded on the device, lazily opened JPEG 2000 pages
        # of a batch are grouped by size, process_document takes "jp2", "j2k" and "jpx", and with LUMINA_OCR_PDF_SCANS=1 the /JPXDecode
        # pages of a scanned PDF are read as well.  Off by default: exactly the calls made without the option are made.
        self.device_jp2 = os.environ.get("LUMINA_OCR_DEVICE_JP2", "0").lower() not in ("", "0", "false", "no")
        # LUMINA_OCR_JP2_IRREVERSIBLE=1: with LUMINA_OCR_DEVICE_JP2, files of the 9/7 irreversible transform (what lossy JPEG 2000 is in
        # practice) are decoded on the device as well (lumina_ocr_jp2_decode_irreversible), wherever a 5/3 file is.  Off by default, and
        # ignored without LUMINA_OCR_DEVICE_JP2: exactly the calls made without the option are made.
        self.jp2_irreversible = os.environ.get("LUMINA_OCR_JP2_IRREVERSIBLE", "0").lower() not in ("", "0", "false", "no")
        # LUMINA_OCR_JP2_TILES=1: with LUMINA_OCR_DEVICE_JP2, tiled JPEG 2000 files (tiles, image and tile origins, user precincts: what
        # scanners and Acrobat's scan profiles write) are decoded on the device as well (lumina_ocr_jp2_decode_ex), wherever a one-tile
        # file is; it combines with LUMINA_OCR_JP2_IRREVERSIBLE.  Off by default, and ignored without LUMINA_OCR_DEVICE_JP2: exactly the
        # calls made without the option are made.
        self.jp2_tiles = os.environ.get("LUMINA_OCR_JP2_TILES", "0").lower() not in ("", "0", "false", "no")
        self._jp2_reasons_logged: set = set()
        self.apply_binarize = "adaptive" if b in ("1", "true", "yes", "adaptive") else ("simple" if b == "simple" else None)
        self._device = int(os.environ.get("LUMINA_OCR_DEVICE", os.environ.get("LOCAL_RANK", 0)))
        self._det_weights = os.environ.get("LUMINA_OCR_DET_WEIGHTS", "")
        self._rec_weights = os.environ.get("LUMINA_OCR_REC_WEIGHTS", "")
        self._recognizer = os.environ.get("LUMINA_OCR_RECOGNIZER", "crnn")        # "crnn" | "svtr" (BASELINE configs[4] family)
        self._svtr_weights = os.environ.get("LUMINA_OCR_SVTR_WEIGHTS", "")
        self._rec_dict = os.environ.get("LUMINA_OCR_REC_DICT", "")               # dictionary file: one symbol per line (PP-OCR key-file format)
        self._allow_synthetic = os.environ.get("LUMINA_OCR_ALLOW_SYNTHETIC", "") == "1"
        # PaddleOCR's use_angle_cls: lines read upside down (0/180-degree classifier, LOCW blob with the cls.* tensors) are recognised
        # turned.  Off by default: every code path is then the one without the classifier.
        self._use_angle_cls = os.environ.get("LUMINA_OCR_USE_ANGLE_CLS", "0").lower() not in ("", "0", "false", "no")
        self._cls_weights = os.environ.get("LUMINA_OCR_CLS_WEIGHTS", "")
        # LUMINA_OCR_TABLES=1: ruled tables become `table` / `table_cell` entries and <table> blocks of the Markdown (the reference gets them
        # from Azure's layout model, :324-352).  Off by default: every output is then the one without them and tables_count stays 0.
        self._use_tables = os.environ.get("LUMINA_OCR_TABLES", "0").lower() not in ("", "0", "false", "no")
        # LUMINA_OCR_SELECTION_MARKS=1: checkboxes become `selection_mark` entries and :selected: / :unselected: tokens of the Markdown (the
        # reference gets them from Azure's layout model, :313-322).  Off by default: every output is then the one without them.
        self._use_marks = os.environ.get("LUMINA_OCR_SELECTION_MARKS", "0").lower() not in ("", "0", "false", "no")
        # LUMINA_OCR_RADIO_BUTTONS=1 (with LUMINA_OCR_SELECTION_MARKS=1; alone it is an error): radio buttons become `selection_mark` entries
        # and tokens exactly as checkboxes do (Azure's selection marks cover both).  Off by default: every output is then the one without it.
        self._use_round_marks = os.environ.get("LUMINA_OCR_RADIO_BUTTONS", "0").lower() not in ("", "0", "false", "no")
        # LUMINA_OCR_BARCODES=1: Code 128 and Code 39 strips become `barcode` entries with their decoded content and a `:barcode: <content>`
        # line of the Markdown; the text lines the detector found on a strip are dropped.  Off by default: every output is then the one without it.
        self._use_barcodes = os.environ.get("LUMINA_OCR_BARCODES", "0").lower() not in ("", "0", "false", "no")
        # LUMINA_OCR_BARCODE_KINDS (with LUMINA_OCR_BARCODES=1; alone it has no effect): the kinds to read, a comma list of code128, code39,
        # ean13 (UPC-A with it), ean8, upce, itf, or all.  Default code128,code39: every output is then the one without the variable.  An
        # unknown name is an error result.
        self._barcode_kinds = os.environ.get("LUMINA_OCR_BARCODE_KINDS", "") or ",".join(arch.BARCODE_KINDS_DEFAULT)
        # LUMINA_OCR_QRCODES=1: QR symbols (Model 2, versions 1-10) become `barcode` entries of kind "QRCode" with their decoded content and a
        # `:barcode: <content>` line of the Markdown, behind the 1-D codes of the page when LUMINA_OCR_BARCODES is on as well; the text lines the
        # detector found inside a symbol are dropped.  Off by default: every output is then the one without it.
        self._use_qrcodes = os.environ.get("LUMINA_OCR_QRCODES", "0").lower() not in ("", "0", "false", "no")
        # LUMINA_OCR_QR_MAX_VERSION (with LUMINA_OCR_QRCODES=1; alone it has no effect): the largest QR version to read, 10..40.  Default 10:
        # every output is then the one without the variable.  Above 10 the symbols of versions 11 and up (e-invoice, payment and
        # certificate codes) are read too, on the affine grid through the three finders.  A value outside 10..40 is an error result.
        self._qr_max_version = os.environ.get("LUMINA_OCR_QR_MAX_VERSION", "") or "10"
        # LUMINA_OCR_DATAMATRIX=1: Data Matrix symbols (ECC 200, 10 x 10 .. 52 x 52 and the six rectangles) become `barcode` entries of kind
        # "DataMatrix" with their decoded content and a `:barcode: <content>` line of the Markdown, behind the 1-D and QR codes of the page;
        # the text lines the detector found inside a symbol are dropped.  Off by default: every output is then the one without it.
        self._use_datamatrix = os.environ.get("LUMINA_OCR_DATAMATRIX", "0").lower() not in ("", "0", "false", "no")
        # LUMINA_OCR_DATAMATRIX_MAX_SIZE=52..144 (with LUMINA_OCR_DATAMATRIX=1; alone it has no effect; default 52: the pass above and nothing
        # else): the squares of 64 x 64 up to that many modules a side are read as well (lumina_ocr_datamatrix_sizes).  Checked when the
        # engine starts: another value is an error result.
        self._dm_max_size = os.environ.get("LUMINA_OCR_DATAMATRIX_MAX_SIZE", "") or "52"
        # LUMINA_OCR_AZTEC=1: Aztec symbols (compact 1-4 layers, full-range 1-11 layers) become `barcode` entries of kind "Aztec" with their
        # decoded content and a `:barcode: <content>` line of the Markdown, behind the 1-D, QR and Data Matrix codes of the page; the text
        # lines the detector found inside a symbol are dropped.  Off by default: every output is then the one without it.
        self._use_aztec = os.environ.get("LUMINA_OCR_AZTEC", "0").lower() not in ("", "0", "false", "no")
        # LUMINA_OCR_AZTEC_MAX_LAYERS=11..32 (with LUMINA_OCR_AZTEC=1; default 11: the pass above and nothing else): full-range symbols of up
        # to that many layers are read as well (lumina_ocr_aztec_layers).  Checked when the engine starts: another value is an error result.
        self._aztec_max_layers = os.environ.get("LUMINA_OCR_AZTEC_MAX_LAYERS", "") or "11"
        # LUMINA_OCR_PAGE_ORIENTATION=1: pages lying sideways or upside-down are turned upright on the device before anything else reads
        # them (after decode and EXIF orientation, before the resize), and json_output reports page_rotation.  It uses the classifier
        # (LUMINA_OCR_CLS_WEIGHTS) whether or not LUMINA_OCR_USE_ANGLE_CLS is set.  Off by default: every output is then the one without it.
        self._use_page_orient = os.environ.get("LUMINA_OCR_PAGE_ORIENTATION", "0").lower() not in ("", "0", "false", "no")
        # LUMINA_OCR_WORD_BOXES=1: every `word` entry takes its polygon and confidence from the recogniser's CTC alignment
        # (lumina_ocr_ctc_decode_words) instead of a proportional split of its line and the line's score.  Contents, order and every other
        # entry are the same.  Off by default: every output is then the one without it.
        self._use_word_boxes = os.environ.get("LUMINA_OCR_WORD_BOXES", "0").lower() not in ("", "0", "false", "no")
        self._weights_kind = "unloaded"
        self._pre = ImagePreprocessor(self.max_dimension)
        self._initialized = True

    # ---- engine management (reference: _ensure_client_initialized :166-207) ----
    def _ensure_engine(self) -> None:
        """Builds the engine once.  Like the reference without Azure credentials (:175-195), a provider without its weights is
        an ERROR, returned as data by the callers: seeded synthetic networks are only used when LUMINA_OCR_ALLOW_SYNTHETIC=1
        says so (tests, demos, the benchmark), never silently."""
        if self._pipeline is not None:
            return
        with self._engine_lock:
            if self._pipeline is not None:
                return
            import torch
            from ..engine import Engine
            from ..pipeline import OcrPipeline
            svtr = self._recognizer == "svtr"
            have_files = bool(self._det_weights) and bool(self._svtr_weights if svtr else self._rec_weights)
            if not have_files and not self._allow_synthetic:
                missing = [k for k, v in (("LUMINA_OCR_DET_WEIGHTS", self._det_weights),
                                          ("LUMINA_OCR_SVTR_WEIGHTS" if svtr else "LUMINA_OCR_REC_WEIGHTS", self._svtr_weights if svtr else self._rec_weights)) if not v]
                raise RuntimeError("OCR weights not configured: set %s (LOCW blobs) and LUMINA_OCR_REC_DICT, or LUMINA_OCR_ALLOW_SYNTHETIC=1 "
                                   "for seeded synthetic networks" % " and ".join(missing))
            use_cls = self._use_angle_cls or self._use_page_orient
            if use_cls and not self._cls_weights and not self._allow_synthetic:
                raise RuntimeError("orientation classifier weights not configured: set LUMINA_OCR_CLS_WEIGHTS (LOCW blob) with "
                                   "%s=1, or LUMINA_OCR_ALLOW_SYNTHETIC=1 for a seeded synthetic classifier"
                                   % ("LUMINA_OCR_USE_ANGLE_CLS" if self._use_angle_cls else "LUMINA_OCR_PAGE_ORIENTATION"))
            if self._use_round_marks and not self._use_marks:
                raise RuntimeError("LUMINA_OCR_RADIO_BUTTONS=1 needs LUMINA_OCR_SELECTION_MARKS=1: radio buttons are found in the checkboxes' pass")
            qr_max_version = 10
            if self._use_qrcodes:
                if not (self._qr_max_version.strip().isdigit() and 10 <= int(self._qr_max_version) <= 40):
                    raise RuntimeError("LUMINA_OCR_QR_MAX_VERSION: %r is not a version 10..40" % self._qr_max_version)
                qr_max_version = int(self._qr_max_version)
            dm_max_size = 52
            if self._use_datamatrix:
                if not (self._dm_max_size.strip().isdigit() and 52 <= int(self._dm_max_size) <= 144):
                    raise RuntimeError("LUMINA_OCR_DATAMATRIX_MAX_SIZE: %r is not a number of modules 52..144" % self._dm_max_size)
                dm_max_size = int(self._dm_max_size)
            aztec_max_layers = 11
            if self._use_aztec:
                if not (self._aztec_max_layers.strip().isdigit() and 11 <= int(self._aztec_max_layers) <= 32):
                    raise RuntimeError("LUMINA_OCR_AZTEC_MAX_LAYERS: %r is not a number of layers 11..32" % self._aztec_max_layers)
                aztec_max_layers = int(self._aztec_max_layers)
            if self._use_barcodes:
                try:
                    arch.barcode_kinds_mask(self._barcode_kinds)
                except ValueError as e:
                    raise RuntimeError("LUMINA_OCR_BARCODE_KINDS: %s" % e)
            if have_files and not self._rec_dict:
                raise RuntimeError("LUMINA_OCR_REC_DICT (the dictionary file the recogniser was trained with) is required with weight files")
            eng = Engine(self._device)  # raises EngineUnavailable without the HIP library / a GPU
            try:
                with torch.cuda.device(self._device):
                    if have_files:
                        eng.load_det(Path(self._det_weights).read_bytes())
                        if svtr:
                            eng.load_svtr(Path(self._svtr_weights).read_bytes())
                        else:
                            eng.load_rec(Path(self._rec_weights).read_bytes())
                        charset = arch.load_charset(self._rec_dict)
                        kind, post = "files", arch.DEFAULT_POST
                    else:  # no trained weights ship offline: deterministic seeded networks, on request only
                        logger.warning("OCR provider is running SEEDED SYNTHETIC networks (LUMINA_OCR_ALLOW_SYNTHETIC=1): recognised text is not meaningful")
                        eng.load_det(arch.make_det_weights())
                        charset = arch.load_charset(self._rec_dict) if self._rec_dict else arch.ctc_charset()
                        if svtr:
                            eng.load_svtr(arch.make_svtr_weights(num_classes=len(charset)))
                        else:
                            eng.load_rec(arch.make_rec_weights(num_classes=len(charset), code_path=True))
                        kind, post = "seeded-synthetic", arch.TEXT_PATH_POST
                    if use_cls:
                        if self._cls_weights:
                            eng.load_cls(Path(self._cls_weights).read_bytes())
                        else:
                            logger.warning("OCR provider is running a SEEDED SYNTHETIC orientation classifier (LUMINA_OCR_ALLOW_SYNTHETIC=1)")
                            eng.load_cls(arch.make_cls_weights(orientation_path=True))
                    n_cls = eng.svtr_num_classes if svtr else eng.num_classes
                    if len(charset) != n_cls:
                        raise RuntimeError("dictionary has %d classes (blank + symbols + space) but the %s head has %d"
                                           % (len(charset), "SVTR" if svtr else "CRNN", n_cls))
                    pipeline = OcrPipeline(eng, charset=charset, max_dimension=self.max_dimension, post=post, recognizer=self._recognizer,
                                           angle_cls=self._use_angle_cls, tables=self._use_tables, marks=self._use_marks,
                                           page_orient=self._use_page_orient, word_boxes=self._use_word_boxes, round_marks=self._use_round_marks,
                                           barcodes=self._use_barcodes, qrcodes=self._use_qrcodes, qr_max_version=qr_max_version, datamatrix=self._use_datamatrix, aztec=self._use_aztec,
                                           aztec_max_layers=aztec_max_layers, dm_max_size=dm_max_size, barcode_kinds=self._barcode_kinds if self._use_barcodes else arch.BARCODE_KINDS_DEFAULT)
            except Exception:
                eng.close()
                raise
            self._weights_kind = kind
            self._engine = eng
            self._pre._engine = eng
            pipeline.binarize = self.apply_binarize
            self._pipeline = pipeline

    def _qr_max_version_status(self):
        """The largest QR version the provider reads (None with QR codes off; the variable's text when it is no version 10..40)."""
        if not self._use_qrcodes:
            return None
        text = self._qr_max_version.strip()
        return int(text) if text.isdigit() and 10 <= int(text) <= 40 else self._qr_max_version

    def _dm_max_size_status(self):
        """The largest Data Matrix side the provider reads (None with Data Matrix off; the variable's text when it is no number 52..144)."""
        if not self._use_datamatrix:
            return None
        text = self._dm_max_size.strip()
        return int(text) if text.isdigit() and 52 <= int(text) <= 144 else self._dm_max_size

    def _aztec_max_layers_status(self):
        """The most layers of a full-range Aztec symbol the provider reads (None with Aztec off; the variable's text when it is no number 11..32)."""
        if not self._use_aztec:
            return None
        text = self._aztec_max_layers.strip()
        return int(text) if text.isdigit() and 11 <= int(text) <= 32 else self._aztec_max_layers

    def _barcode_kinds_names(self):
        """The kinds the provider reads, by name ([] with barcodes off; the variable's text when it names an unknown kind)."""
        if not self._use_barcodes:
            return []
        try:
            mask = arch.barcode_kinds_mask(self._barcode_kinds)
        except ValueError:
            return [self._barcode_kinds]
        return [k for k, bit in arch.BARCODE_KINDS.items() if mask & bit]

    def _device_ctx(self):
        """Binds the calling thread (possibly an asyncio.to_thread worker, which starts on device 0) to the engine's GPU."""
        import torch
        return torch.cuda.device(self._device)

    # ---- single image (:398-475) ----
    def _prepare(self, image: Image.Image) -> Image.Image:
        """EXIF orientation, RGB, size check (optimize_for_ocr's first steps, image_preprocessing.py:206-215) -> PIL RGB image."""
        image = self._pre.auto_orient(image)
        if image.mode != "RGB":
            image = image.convert("RGB")
        w, h = image.size
        nw, nh = get_optimal_size(w, h, self.max_dimension)
        if nw <= 0 or nh <= 0:
            raise ValueError("height and width must be > 0")
        return image

    def _stage_pages(self, images: List[Image.Image]):
        """Same-size PIL RGB pages -> one host uint8 tensor [n,H,W,3] (pinned when there is a GPU).  The pixels go from Pillow's raw
        encoder straight into the staging buffer: np.asarray(image) + np.stack + a pageable upload were 5 ms of the 7.5 ms host
        time per A4 page (tobytes() joins 64 KB chunks, stack copies them again)."""
        import torch
        w, h = images[0].size
        n = len(images)
        key = (n, h, w)
        if getattr(self, "_stage_key", None) != key:
            self._stage = torch.empty((n, h, w, 3), dtype=torch.uint8)
            if torch.cuda.is_available():
                self._stage = self._stage.pin_memory()
            self._stage_key = key
        flat = self._stage.view(n, -1).numpy()
        row_bytes = w * 3
        chunk = max(row_bytes, (4 << 20) // row_bytes * row_bytes)   # whole rows, ~4 MB per encoder call
        for i, im in enumerate(images):
            if not self._raw_copy(im, flat[i], h * row_bytes, chunk):
                self._stage[i] = torch.from_numpy(np.asarray(im, np.uint8))   # any Pillow whose raw encoder is not driven this way
        return self._stage

    @staticmethod
    def _raw_copy(im: Image.Image, dst: np.ndarray, nbytes: int, chunk: int) -> bool:
        """What Image.tobytes() does, minus the join: the raw encoder's chunks are written where they are wanted."""
        try:
            im.load()
            enc = Image._getencoder("RGB", "raw", "RGB")
            try:
                enc.setimage(im.im, (0, 0) + im.size)
            except TypeError:   # Pillow < 10: setimage(im)
                enc.setimage(im.im)
            off = 0
            while True:
                _, status, data = enc.encode(chunk)
                dst[off:off + len(data)] = np.frombuffer(data, np.uint8)
                off += len(data)
                if status:
                    break
            return status > 0 and off == nbytes
        except Exception:
            return False

    def _upload(self, staged):
        """Staging buffer -> the engine's device (worker threads start on device 0 whatever LUMINA_OCR_DEVICE says)."""
        import torch
        dev = torch.device("cuda", self._device)
        out = staged.to(dev, non_blocking=True)
        torch.cuda.current_stream(dev).synchronize()   # the staging buffer is reused by the next call
        return out

    def _finish_page(self, det, jpeg: bytes, processed_hw, page_number: int, original_size, t0: float) -> OCROutput:
        triples = det.triples()
        line_words = det.line_words() if getattr(det, "word_counts", None) is not None else None   # LUMINA_OCR_WORD_BOXES=1
        codes = strips = squares = matrices = aztecs = None
        if getattr(det, "barcodes", None) is not None:   # LUMINA_OCR_BARCODES=1: what the recogniser made of the bars is no text
            strips = barcode_layout.read_barcodes(det.barcodes, det.barcode_syms)
        if getattr(det, "qrcodes", None) is not None:    # LUMINA_OCR_QRCODES=1: the same for the modules of a QR symbol
            squares = qr_layout.read_qrcodes(det.qrcodes, det.qr_data)
        if getattr(det, "datamatrix", None) is not None:   # LUMINA_OCR_DATAMATRIX=1: and of a Data Matrix symbol
            matrices = dm_layout.read_datamatrix(det.datamatrix, det.dm_data)
        if getattr(det, "aztec", None) is not None:   # LUMINA_OCR_AZTEC=1: and of an Aztec symbol
            aztecs = aztec_layout.read_aztec(det.aztec, det.az_data, max_layers=self._pipeline.aztec_max_layers if self._pipeline is not None else 11)
        if strips is not None or squares is not None or matrices is not None or aztecs is not None:
            codes = (strips or []) + (squares or []) + (matrices or []) + (aztecs or [])
            keep = [i for i, t in enumerate(triples) if not barcode_layout.inside_any(t[0], codes)]
            if len(keep) < len(triples):
                triples = [triples[i] for i in keep]
                line_words = None if line_words is None else [line_words[i] for i in keep]
        merged, ordered = layout.reading_order(triples)
        words = None
        if line_words is not None:   # reading_order hands the same tuples back in another order: the words follow their lines
            at = {id(t): i for i, t in enumerate(triples)}
            words = [line_words[at[id(t)]] for t in ordered]
        tabs = []
        if det.hrules is not None:   # LUMINA_OCR_TABLES=1; table_index counts from 0 here, _number_tables makes it run over a document
            tabs = table_layout.find_tables(det.hrules, det.vrules, arch.TABLE_PARAMS["snap"])
            table_layout.fill_cells(tabs, ordered)
        found = None
        if getattr(det, "marks", None) is not None:   # LUMINA_OCR_SELECTION_MARKS=1 [+ LUMINA_OCR_RADIO_BUTTONS=1]
            rounds = getattr(det, "round_marks", None)
            found = mark_layout.select_marks(det.marks) if rounds is None else mark_layout.select_marks(det.marks, rounds)
        if codes:
            md = layout.page_markdown(merged, tabs, marks=found or None, barcodes=codes)
        elif found:
            md = layout.page_markdown(merged, tabs, marks=found)
        else:
            md = layout.page_markdown(merged, tabs) if tabs else layout.page_markdown(merged)
        paragraphs = layout.build_paragraph_boxes(merged, page_number)
        # words, lines, selection marks, tables with their cells, paragraphs: the order of ocr_service.py:285-367
        boxes = ((layout.build_layout_boxes(ordered, page_number) if words is None else layout.build_layout_boxes(ordered, page_number, words=words))
                 + layout.build_mark_boxes(found or [], page_number) + layout.build_barcode_boxes(codes or [], page_number)
                 + layout.build_table_boxes(tabs, page_number) + paragraphs)
        counts = {"page_count": 1, "words_count": sum(1 for b in boxes if b["type"] == "word"), "lines_count": len(ordered),
                  "tables_count": len(tabs), "paragraphs_count": len(paragraphs)}
        if found is not None:
            counts["selection_marks_count"] = len(found)
        if strips is not None:
            counts["barcodes_count"] = len(strips)
        if squares is not None:
            counts["qrcodes_count"] = len(squares)
        if matrices is not None:
            counts["datamatrix_count"] = len(matrices)
        if aztecs is not None:
            counts["aztec_count"] = len(aztecs)
        if getattr(det, "turn", None) is not None:   # LUMINA_OCR_PAGE_ORIENTATION=1
            counts["page_rotation"] = page_orient.page_rotation(det.turn)
        ph, pw = processed_hw
        return OCROutput(markdown=md, html=layout.html_from_markdown(md),
                         json_output=counts,
                         processing_time_ms=_ms_since(t0), success=True, page_number=page_number, image_width=original_size[0],
                         image_height=original_size[1], layout_boxes=boxes, processed_image_bytes=jpeg,
                         page_width_inches=float(pw), page_height_inches=float(ph))

    def _run_pages(self, pages):
        """Same-size pages on the device -> per page (detections, processed_image_bytes, processed (height, width)), in order.  With
        LUMINA_OCR_PAGE_ORIENTATION=1 the pages come back upright: a batch may leave in several groups of two sizes."""
        if not self._use_page_orient:
            dets, processed = self._pipeline.run(pages, deskew=self.apply_deskew)
            jpegs = self._pre.compress_for_azure_device(processed)   # processed_image_bytes: encoded on the device
            hw = tuple(processed.shape[1:3])
            return [(d, j, hw) for d, j in zip(dets, jpegs)]
        parts = []
        for idxs, dets, processed in self._pipeline.run_oriented_groups(pages, deskew=self.apply_deskew):
            jpegs = self._pre.compress_for_azure_device(processed)
            hw = tuple(processed.shape[1:3])
            parts.append((idxs, [(d, j, hw) for d, j in zip(dets, jpegs)]))
        return page_orient.reassemble(pages.shape[0], parts)

    def _process_single_image_sync(self, image: Image.Image, page_number: int = 1, decoded=None) -> OCROutput:
        """decoded: the page already on the device (uint8 [1,H,W,3], from the device JPEG decoder) — `image` is then only consulted
        for its size."""
        with self._semaphore:
            t0 = time.time()
            original_size = image.size
            try:
                import torch
                self._ensure_engine()
                with self._device_ctx():
                    if decoded is None:
                        decoded = self._upload(self._stage_pages([self._prepare(image)]))
                    else:
                        w, h = original_size
                        nw, nh = get_optimal_size(w, h, self.max_dimension)
                        if nw <= 0 or nh <= 0:
                            raise ValueError("height and width must be > 0")
                    det, jpeg, processed_hw = self._run_pages(decoded)[0]
                return self._finish_page(det, jpeg, processed_hw, page_number, original_size, t0)
            except Exception as e:  # errors are data (:464-475)
                logger.error("OCR failed: %s", e)
                return OCROutput(success=False, error=str(e), processing_time_ms=_ms_since(t0), page_number=page_number,
                                 image_width=original_size[0], image_height=original_size[1])

    def _decode_jpeg_on_device(self, data: bytes, image: Image.Image):
        """The reference decodes every input with Image.open (image_preprocessing.py:57-75).  For a baseline JPEG
        the pixels are produced on the device instead (lumina_ocr_jpeg_decode: byte-identical to Pillow's decode; grey files arrive with
        their value on all three channels, which is what convert('RGB') gives): nothing is decoded on the host, the file's
        entropy-coded bytes are what crosses PCIe (~10x less than the pixels).  -> device tensor [1,H,W,3], or None: Pillow decodes."""
        if not self.device_jpeg or image.format != "JPEG" or data[:2] != b"\xff\xd8":
            return None
        try:
            orientation = image.getexif().get(0x0112, 1)
            if orientation not in range(0, 9):
                return None
            from ..engine import Engine
            rc, info = Engine.jpeg_probe_progressive(data) if self.progressive_jpeg else Engine.jpeg_probe(data)
            if rc != 0 or (info["width"], info["height"]) != image.size:
                return None
            self._ensure_engine()
            with self._device_ctx():
                decode = self._engine.jpeg_decode_progressive if self.progressive_jpeg else self._engine.jpeg_decode
                out, status = decode([data], info["height"], info["width"])
                if status != [0]:
                    return None
                return self._engine.exif_transpose(out, orientation)     # auto_orient (image_preprocessing.py:213), on the device as well
        except Exception as e:       # any doubt: the reference's own path
            logger.warning("device JPEG decode not used: %s", e)
            return None

    @staticmethod
    def _png_orientation(image: Image.Image) -> Optional[int]:
        """The EXIF orientation auto_orient would apply, read without decoding, or None: leave the file to the host path.  Pillow's PNG
        getexif() loads the pixels when the eXIf chunk was not among the chunks read at open (a file with chunks after IDAT is refused by
        the device decoder anyway), and Pillow also takes the orientation from a "Raw profile type exif" text chunk or an XMP
        tiff:Orientation ("XML:com.adobe.xmp"): files carrying either are left to the host path, so that no orientation source is missed."""
        if "Raw profile type exif" in image.info or "XML:com.adobe.xmp" in image.info:
            return None
        return image.getexif().get(0x0112, 1) if "exif" in image.info else 1

    def _decode_png_on_device(self, data: bytes, image: Image.Image):
        """The reference decodes every input with Image.open + convert('RGB') (image_preprocessing.py:57-75).  For a PNG in the device
        subset the pixels are produced on the device instead (lumina_ocr_png_decode: byte-identical to Pillow); `image` must be the
        lazily opened file (nothing decoded yet).  -> device tensor [1,H,W,3] with the EXIF orientation applied, or None: Pillow decodes."""
        if not self.device_png or image.format != "PNG" or data[:8] != PNG_SIGNATURE:
            return None
        try:
            orientation = self._png_orientation(image)
            if orientation is None or orientation not in range(0, 9):
                return None
            # the engine first: it brings up torch's HIP runtime before the probe loads the engine library (loaded the other way round,
            # the library's own runtime was the first in the process and torch's saw no device)
            self._ensure_engine()
            from ..engine import Engine
            rc, info = Engine.png_probe(data)
            if rc != 0 or (info["width"], info["height"]) != image.size:
                return None
            with self._device_ctx():
                out, status = self._engine.png_decode([data], info["height"], info["width"])
                if status != [0]:
                    return None
                return self._engine.exif_transpose(out, orientation)
        except Exception as e:       # any doubt: the reference's own path
            logger.warning("device PNG decode not used: %s", e)
            return None

    def _process_png_on_device(self, image_source: Union[str, Path, bytes], page_number: int) -> Optional[OCROutput]:
        """A PNG path / bytes whose pixels the device decodes -> its result; None: today's path (load_image converts P / RGBA / LA / 1
        files at once, so the lazily opened file is looked at before that)."""
        try:
            data = image_source if isinstance(image_source, bytes) else Path(image_source).read_bytes()
        except OSError:
            return None
        if data[:8] != PNG_SIGNATURE:
            return None
        try:
            image = Image.open(io.BytesIO(data))
        except Exception:
            return None
        decoded = self._decode_png_on_device(data, image)
        if decoded is None:
            return None
        return self._process_single_image_sync(image, page_number, decoded=decoded)

    @staticmethod
    def _is_webp(head: bytes) -> bool:
        return head[:4] == b"RIFF" and head[8:12] == b"WEBP"

    def _decode_webp_on_device(self, data: bytes, image: Image.Image):
        """A WebP file the device reads (lossless; lossy as well with webp_lossy) -> device tensor [1,H,W,3] with the EXIF orientation
        applied (lumina_ocr_webp_decode / _decode_lossy: byte-identical to Pillow), or None: Pillow decodes.  `image` is the lazily opened file (nothing decoded yet): its info carries
        the EXIF chunk, read here as _png_orientation reads a PNG's; a file with XMP is left to the host path and its auto_orient."""
        try:
            if image.format != "WEBP" or "xmp" in image.info or "XML:com.adobe.xmp" in image.info:
                return None
            orientation = image.getexif().get(0x0112, 1) if "exif" in image.info else 1
            if orientation not in range(0, 9):
                return None
            self._ensure_engine()   # (before the probe loads the engine library: see _decode_png_on_device)
            from ..engine import Engine
            rc, info = Engine.webp_probe_lossy(data) if self.webp_lossy else Engine.webp_probe(data)
            if rc != 0 or info["xmp"] or (info["width"], info["height"]) != image.size:
                reason = info["reason"] if rc else "XMP chunk, or a size that differs from the opened image's"
                if reason not in self._webp_reasons_logged:
                    self._webp_reasons_logged.add(reason)
                    logger.info("WebP input left to Pillow (status %d): %s", rc, reason)
                return None
            with self._device_ctx():
                decode = self._engine.webp_decode_lossy if self.webp_lossy else self._engine.webp_decode
                out, status = decode([data], info["height"], info["width"])
                if status != [0]:
                    return None
                return self._engine.exif_transpose(out, orientation)     # auto_orient (image_preprocessing.py:213), on the device as well
        except Exception as e:       # any doubt: the reference's own path
            logger.warning("device WebP decode not used: %s", e)
            return None

    def _process_webp_on_device(self, image_source: Union[str, Path, bytes], page_number: int) -> Optional[OCROutput]:
        """A WebP path / bytes (recognised by magic, never by extension) whose pixels the device decodes -> its result; None: today's path."""
        try:
            if isinstance(image_source, bytes):
                data = image_source
            else:
                with open(image_source, "rb") as f:
                    if not self._is_webp(f.read(12)):
                        return None
                data = Path(image_source).read_bytes()
        except OSError:
            return None
        if not self._is_webp(data[:12]):
            return None
        try:
            image = Image.open(io.BytesIO(data))
        except Exception:
            return None
        decoded = self._decode_webp_on_device(data, image)
        if decoded is None:
            return None
        return self._process_single_image_sync(image, page_number, decoded=decoded)

    @staticmethod
    def _is_jp2(head: bytes) -> bool:
        return head[:12] == JP2_SIGNATURE or head[:4] == J2K_SIGNATURE

    def _jp2_probe(self, data: bytes, size) -> Optional[Dict[str, Any]]:
        """The probe's info when the device decodes this JPEG 2000 file and its size is `size`, else None, the reason logged once."""
        from ..engine import Engine
        if self.jp2_tiles:
            rc, info = Engine.jp2_probe_ex(data, self._jp2_flags())
        else:
            rc, info = Engine.jp2_probe_irreversible(data) if self.jp2_irreversible else Engine.jp2_probe(data)
        if rc == 0 and (info["width"], info["height"]) == tuple(size):
            return info
        reason = info["reason"] if rc else "size differs from the opened image's"
        if reason not in self._jp2_reasons_logged:
            self._jp2_reasons_logged.add(reason)
            logger.info("JPEG 2000 input left to Pillow (status %d): %s", rc, reason)
        return None

    def _jp2_flags(self) -> int:
        from ..engine import Engine
        return Engine.JP2_F_TILES | (Engine.JP2_F_IRREVERSIBLE if self.jp2_irreversible else 0)

    def _jp2_decoder(self):
        if self.jp2_tiles:
            flags = self._jp2_flags()
            return lambda files, height, width: self._engine.jp2_decode_ex(files, height, width, flags)
        return self._engine.jp2_decode_irreversible if self.jp2_irreversible else self._engine.jp2_decode

    def _decode_jp2_on_device(self, data: bytes, image: Image.Image):
        """A JPEG 2000 file of the device subset -> device tensor [1,H,W,3] (lumina_ocr_jp2_decode: byte-identical to Pillow), or None:
        Pillow decodes.  `image` is the lazily opened file; one that carries EXIF or XMP is left to the host path and its auto_orient."""
        try:
            if image.format != "JPEG2000" or "exif" in image.info or "XML:com.adobe.xmp" in image.info or "xmp" in image.info:
                return None
            self._ensure_engine()   # (before the probe loads the engine library: see _decode_png_on_device)
            info = self._jp2_probe(data, image.size)
            if info is None:
                return None
            with self._device_ctx():
                out, status = self._jp2_decoder()([data], info["height"], info["width"])
                return out if status == [0] else None
        except Exception as e:       # any doubt: the reference's own path
            logger.warning("device JPEG 2000 decode not used: %s", e)
            return None

    def _process_jp2_on_device(self, image_source: Union[str, Path, bytes], page_number: int) -> Optional[OCROutput]:
        """A JPEG 2000 path / bytes (recognised by magic, never by extension) whose pixels the device decodes -> its result; None: today's path."""
        try:
            if isinstance(image_source, bytes):
                data = image_source
            else:
                with open(image_source, "rb") as f:
                    if not self._is_jp2(f.read(12)):
                        return None
                data = Path(image_source).read_bytes()
        except OSError:
            return None
        if not self._is_jp2(data[:12]):
            return None
        try:
            image = Image.open(io.BytesIO(data))
        except Exception:
            return None
        decoded = self._decode_jp2_on_device(data, image)
        if decoded is None:
            return None
        return self._process_single_image_sync(image, page_number, decoded=decoded)

    def process_image_sync(self, image_source: Union[str, Path, Image.Image, bytes], page_number: int = 1) -> OCROutput:
        data = None
        if self.device_jp2 and isinstance(image_source, (bytes, str, Path)):
            r = self._process_jp2_on_device(image_source, page_number)
            if r is not None:
                return r
        if self.device_tiff and isinstance(image_source, (bytes, str, Path)):
            r = self._process_tiff_on_device(image_source, page_number)
            if r is not None:
                return r
        if self.device_png and isinstance(image_source, (bytes, str, Path)):
            r = self._process_png_on_device(image_source, page_number)
            if r is not None:
                return r
        if self.device_webp and isinstance(image_source, (bytes, str, Path)):
            r = self._process_webp_on_device(image_source, page_number)
            if r is not None:
                return r
        if isinstance(image_source, bytes):
            data = image_source
            image = self._pre.load_image_bytes(image_source)
        elif isinstance(image_source, (str, Path)):
            image = self._pre.load_image(image_source)
            if getattr(image, "format", None) == "JPEG" and self.device_jpeg:
                try:
                    data = Path(image_source).read_bytes()
                except OSError:
                    data = None
        elif isinstance(image_source, Image.Image):
            image = image_source
        else:
            raise ValueError(f"Unsupported image type: {type(image_source)}")
        decoded = self._decode_jpeg_on_device(data, image) if data is not None else None      # (Image.open is lazy: no pixel was decoded yet)
        return self._process_single_image_sync(image, page_number, decoded=decoded)

    # ---- page batches: the data-parallel unit (reference loops pages serially, :620-627) ----
    @staticmethod
    def _lazy_png_bytes(im: Image.Image) -> Optional[bytes]:
        """The file bytes of a PNG page Pillow has not decoded yet (pdf2image's pages: Image.open over a BytesIO, or a file), else None."""
        if getattr(im, "format", None) != "PNG" or getattr(im, "_im", 0) is not None:   # (Pillow 12: _im is None until load())
            return None
        try:
            fp = getattr(im, "fp", None)
            if isinstance(fp, io.BytesIO):
                data = fp.getvalue()
            elif getattr(im, "filename", None):
                data = Path(im.filename).read_bytes()
            else:
                return None
        except (OSError, ValueError):
            return None
        return data if data[:8] == PNG_SIGNATURE else None

    def _decode_png_pages(self, images: List[Image.Image]) -> Dict[int, Any]:
        """Lazily opened PNG pages -> {page index: device tensor [1,H,W,3], EXIF orientation applied}, one png_decode per size group.
        Pages the decoder refuses, and everything else, are absent: they take the host path."""
        try:
            if not any(self._lazy_png_bytes(im) is not None for im in images):
                return {}
            self._ensure_engine()   # (before the probe loads the engine library: see _decode_png_on_device)
            from ..engine import Engine
            cand: Dict[Any, list] = {}
            for i, im in enumerate(images):
                data = self._lazy_png_bytes(im)
                if data is None:
                    continue
                rc, info = Engine.png_probe(data)
                if rc != 0 or (info["width"], info["height"]) != im.size:
                    continue
                # (only now: getexif() caches on the image, and a refused page keeps its host path exactly as it was)
                orientation = self._png_orientation(im)
                if orientation is None or orientation not in range(0, 9):
                    continue
                cand.setdefault(im.size, []).append((i, data, orientation))
            if not cand:
                return {}
            res: Dict[int, Any] = {}
            with self._device_ctx():
                for (w, h), items in cand.items():
                    out, status = self._engine.png_decode([d for _, d, _ in items], h, w)
                    for k, (i, _, orientation) in enumerate(items):
                        if status[k] == 0:
                            res[i] = self._engine.exif_transpose(out[k:k + 1], orientation)
            return res
        except Exception as e:       # any doubt: the reference's own path for every page
            logger.warning("device PNG decode not used: %s", e)
            return {}

    def _decode_jp2_pages(self, images: List[Image.Image]) -> Dict[int, Any]:
        """Lazily opened JPEG 2000 pages -> {page index: device tensor [1,H,W,3]}, one jp2_decode per size group.  Pages the decoder
        refuses, and everything else, are absent: they take the host path."""
        try:
            cand: Dict[Any, list] = {}
            for i, im in enumerate(images):
                if getattr(im, "format", None) != "JPEG2000" or getattr(im, "_im", 0) is not None:
                    continue
                if "exif" in im.info or "XML:com.adobe.xmp" in im.info or "xmp" in im.info:
                    continue
                fp = getattr(im, "fp", None)
                try:
                    data = fp.getvalue() if isinstance(fp, io.BytesIO) else Path(im.filename).read_bytes() if getattr(im, "filename", None) else None
                except (OSError, ValueError):
                    data = None
                if data is None or not self._is_jp2(data[:12]):
                    continue
                self._ensure_engine()
                if self._jp2_probe(data, im.size) is not None:
                    cand.setdefault(im.size, []).append((i, data))
            res: Dict[int, Any] = {}
            if cand:
                with self._device_ctx():
                    for (w, h), items in cand.items():
                        out, status = self._jp2_decoder()([d for _, d in items], h, w)
                        for k, (i, _) in enumerate(items):
                            if status[k] == 0:
                                res[i] = out[k:k + 1]
            return res
        except Exception as e:       # any doubt: the reference's own path for every page
            logger.warning("device JPEG 2000 decode not used: %s", e)
            return {}

    def process_pages_sync(self, images: List[Image.Image], first_page_number: int = 1) -> List[OCROutput]:
        """Same-size pages go through the engine as one batch; results are identical to the per-page path."""
        out: List[Optional[OCROutput]] = [None] * len(images)
        with self._semaphore:
            groups: Dict[Any, List[int]] = {}
            prepared: List[Optional[Image.Image]] = [None] * len(images)
            on_device = self._decode_png_pages(images) if self.device_png else {}
            if self.device_jp2:
                on_device.update(self._decode_jp2_pages(images))
            for i, im in enumerate(images):
                if i in on_device:   # decoded (and oriented) on the device: grouped by its oriented size, apart from host pages
                    groups.setdefault(("device", on_device[i].shape[2], on_device[i].shape[1]), []).append(i)
                    continue
                try:
                    prepared[i] = self._prepare(im)   # (EXIF orientation may swap width and height: group by the prepared size)
                    groups.setdefault(prepared[i].size, []).append(i)
                except Exception as e:
                    out[i] = OCROutput(success=False, error=str(e), page_number=first_page_number + i, image_width=im.size[0], image_height=im.size[1])
            sizes = [im.size for im in images]
            for size, idxs in groups.items():
                self._run_group(idxs, on_device if size[0] == "device" else None, prepared, sizes, first_page_number, out)
        self._number_tables(out)
        return out  # type: ignore[return-value]

    def _run_group(self, idxs: List[int], on_device, prepared, sizes, first_page_number: int, out: List[Optional[OCROutput]]) -> None:
        """One same-size group of a page batch through the engine (the caller holds the semaphore): pages idxs, either already on the
        device (on_device[i]: uint8 [1,H,W,3]) or prepared PIL images; sizes[i]: the page's own (width, height).  Fills out[i]."""
        t0 = time.time()
        try:
            import torch
            self._ensure_engine()
            with self._device_ctx():
                if on_device is not None:
                    pages = torch.cat([on_device[i] for i in idxs]) if len(idxs) > 1 else on_device[idxs[0]]
                else:
                    pages = self._upload(self._stage_pages([prepared[i] for i in idxs]))
                results = self._run_pages(pages)
            for (det, jpeg, processed_hw), i in zip(results, idxs):
                out[i] = self._finish_page(det, jpeg, processed_hw, first_page_number + i, sizes[i], t0)
        except Exception as e:
            for i in idxs:
                out[i] = OCROutput(success=False, error=str(e), processing_time_ms=_ms_since(t0),
                                   page_number=first_page_number + i, image_width=sizes[i][0], image_height=sizes[i][1])

    @staticmethod
    def _number_tables(pages) -> None:
        """table_index runs over the document's tables in page order, as the index of Azure's result.tables does (:326)."""
        seen = 0
        for p in pages:
            if p is None or not p.success:
                continue
            for b in p.layout_boxes:
                if b["type"] == "table":
                    b["table_index"] += seen
            seen += int((p.json_output or {}).get("tables_count", 0))

    def _document_from_pages(self, pages: List[OCROutput], t0: float) -> DocumentOCRResult:
        ok = all(p.success for p in pages)
        boxes: List[Dict[str, Any]] = []
        for p in pages:
            boxes.extend(p.layout_boxes)
        return DocumentOCRResult(pages=pages, total_pages=len(pages), total_processing_time_ms=_ms_since(t0), success=ok,
                                 error=None if ok else "Some pages failed", combined_markdown=layout.combine_markdown(pages),
                                 combined_html=layout.combine_html(pages), combined_layout_boxes=boxes)

    # ---- PDF (:508-660): every PDF goes through the rasterise-and-batch path ----
    def process_pdf_as_images_sync(self, pdf_path: Union[str, Path]) -> DocumentOCRResult:
        t0 = time.time()
        try:
            images = self._pre.pdf_to_images(pdf_path)
            if not images:
                return DocumentOCRResult(success=False, error="No pages found in PDF")
            return self._document_from_pages(self.process_pages_sync(images), t0)
        except Exception as e:
            return DocumentOCRResult(success=False, error=str(e), total_processing_time_ms=_ms_since(t0))

    def process_pdf_sync(self, pdf_path: Union[str, Path]) -> DocumentOCRResult:
        if not Path(pdf_path).exists():
            return DocumentOCRResult(success=False, error=f"File not found: {Path(pdf_path)}")
        if self.device_pdf:
            return self._process_pdf_scans_sync(pdf_path)
        return self.process_pdf_as_images_sync(pdf_path)

    # ---- scanned PDFs (LUMINA_OCR_PDF_SCANS=1): the pages' embedded images, decoded on the device ----
    ROTATE_TO_EXIF = {0: 1, 90: 6, 180: 3, 270: 8}   # /Rotate turns the page clockwise, as these EXIF orientations do

    def _decode_pdf_pages(self, entries, reasons: Dict[int, str]) -> Dict[int, Any]:
        """The accepted pages of pdf_pages.read_pages -> {page index: device tensor [1,H,W,3], /Rotate applied}: grouped by filter and
        size, one decoder call per group.  A page a decoder refuses gets its reason in `reasons` (it goes to the rasteriser); a DCT page
        the device JPEG decoder does not take is decoded by Pillow, as JPEG files are.  The images and masks of a layered page
        (pdf_pages.PageLayers, LUMINA_OCR_PDF_LAYERS=1) join the same groups; such pages are then put together per canvas size by
        page_compose.  A layered page one of whose layers is not decoded gets that layer's reason and goes to the rasteriser whole."""
        # what is decoded: (page index, None) for a one-image page, (page index, (layer, 0 image | 1 mask)) for a layer of a layered one
        groups: Dict[Any, List[Any]] = {}
        for i, e in enumerate(entries):
            if isinstance(e, pdf_pages.PageImage):
                groups.setdefault((e.filter, e.width, e.height), []).append(((i, None), e))
            elif isinstance(e, pdf_pages.PageLayers):
                for k, layer in enumerate(e.layers):
                    for which, r in enumerate((layer.image, layer.mask)):
                        if r is not None:
                            groups.setdefault((r.filter, r.width, r.height), []).append(((i, (k, which)), r))
        res: Dict[int, Any] = {}
        parts: Dict[Any, Any] = {}   # the decoded layers of layered pages
        self._ensure_engine()
        eng = self._engine
        with self._device_ctx():
            for (filt, w, h), items in groups.items():
                idxs = [key[0] for key, _ in items]
                recs = [r for _, r in items]
                streams = [bytes(r.stream) for r in recs]
                try:
                    if filt == "DCTDecode":
                        decode = eng.jpeg_decode_progressive if self.progressive_jpeg else eng.jpeg_decode
                        out, status = decode(streams, h, w) if self.device_jpeg else (None, [-2] * len(idxs))
                    elif filt == "JPXDecode":   # (only with LUMINA_OCR_DEVICE_JP2: read_pages returns none otherwise)
                        out, status = self._jp2_decoder()(streams, h, w)
                    elif filt == "JBIG2Decode":   # (only with LUMINA_OCR_PDF_JBIG2: read_pages returns none otherwise)
                        out, status = eng.jbig2_decode(streams, h, w, [r.params["globals"] for r in recs], [int(r.params["invert"]) for r in recs])
                    elif filt in ("LZWDecode", "RunLengthDecode"):   # one-strip pages of the strip decoders
                        codec = 5 if filt == "LZWDecode" else 32773
                        params = [(codec, r.params["predictor"], r.params["components"], r.params["bits"], int(r.params["indexed"]),
                                   int(r.params["invert"]), int(filt == "RunLengthDecode")) for r in recs]
                        out, status = eng.strip_image_decode([[s] for s in streams], h, w, h, params, [r.params["palette"] for r in recs])
                    elif filt == "FlateDecode":
                        params = [(r.params["predictor"], r.params["components"], r.params["bits"], int(r.params["indexed"]), int(r.params["invert"]))
                                  for r in recs]
                        out, status = eng.flate_image_decode(streams, h, w, params, [r.params["palette"] for r in recs])
                    else:
                        params = [(r.params["K"], int(r.params["EncodedByteAlign"]), int(r.params["BlackIs1"]), int(r.params["invert"])) for r in recs]
                        out, status = eng.fax_decode(streams, h, w, [q + (0,) for q in params])
                except Exception as e:   # the engine's own failure: these pages go to the rasteriser
                    for i in idxs:
                        reasons.setdefault(i, "%s decode failed: %s" % (filt, e))
                    continue
                for k, (i, slot) in enumerate(key for key, _ in items):
                    page = None
                    if status[k] == 0:
                        page = out[k:k + 1]
                    elif filt == "DCTDecode":   # progressive, CMYK, Adobe transforms ...: the fallback JPEG files have
                        try:
                            im = Image.open(io.BytesIO(streams[k])).convert("RGB")
                            if im.size == (w, h):
                                page = self._upload(self._stage_pages([im]))
                        except Exception as e:
                            reasons.setdefault(i, "embedded JPEG not decodable: %s" % e)
                            continue
                    if page is None:
                        reasons.setdefault(i, "%s stream %s (status %d)" % (filt, "corrupt" if status[k] == -1 else "outside the device subset", status[k]))
                        continue
                    if slot is None:
                        res[i] = eng.exif_transpose(page, self.ROTATE_TO_EXIF[recs[k].rotate])
                    else:
                        parts[(i, slot)] = page[0]
            # layered pages: one page_compose per canvas size, then /Rotate; from here on they are ordinary pages
            canvases: Dict[Any, List[int]] = {}
            for i, e in enumerate(entries):
                if isinstance(e, pdf_pages.PageLayers) and i not in reasons:
                    canvases.setdefault((e.height, e.width), []).append(i)
            for hw, idxs in canvases.items():
                table = [(j, l.kind, l.rect, l.flip, l.fill, parts.get((i, (k, 0))), parts.get((i, (k, 1))))
                         for j, i in enumerate(idxs) for k, l in enumerate(entries[i].layers)]
                try:
                    pages = eng.page_compose(hw, len(idxs), table)
                except Exception as e:
                    for i in idxs:
                        reasons[i] = "page composition failed: %s" % e
                    continue
                for j, i in enumerate(idxs):
                    res[i] = eng.exif_transpose(pages[j:j + 1], self.ROTATE_TO_EXIF[entries[i].rotate])
        return res

    def _process_pdf_scans_sync(self, pdf_path: Union[str, Path]) -> DocumentOCRResult:
        t0 = time.time()
        try:
            data = Path(pdf_path).read_bytes()
            try:
                entries = pdf_pages.read_pages(data, strip_filters=self.device_tiff, **({"jpx": True} if self.device_jp2 else {}),
                                               **({"layers": True} if self.pdf_layers else {}), **({"jbig2": True} if self.pdf_jbig2 else {}))
            except pdf_pages.PdfRefused as e:   # not a file the reader takes: the rasterise-and-batch path, whole
                r = self.process_pdf_as_images_sync(pdf_path)
                if not r.success and r.error and not r.pages:
                    r.error = "%s (scanned-page reader: %s)" % (r.error, e.reason)
                return r
            n = len(entries)
            reasons: Dict[int, str] = {i: e.reason for i, e in enumerate(entries) if isinstance(e, pdf_pages.PdfRefused)}
            out: List[Optional[OCROutput]] = [None] * n
            with self._semaphore:
                try:
                    on_device = self._decode_pdf_pages(entries, reasons)
                except Exception as e:   # no engine: errors are data
                    return DocumentOCRResult(success=False, error=str(e), total_processing_time_ms=_ms_since(t0))
                groups: Dict[Any, List[int]] = {}
                sizes: List[Any] = [None] * n
                for i, page in on_device.items():
                    sizes[i] = (int(page.shape[2]), int(page.shape[1]))   # the size the page has after /Rotate
                    groups.setdefault(sizes[i], []).append(i)
                for idxs in groups.values():
                    self._run_group(sorted(idxs), on_device, None, sizes, 1, out)
            for i in range(n):
                if out[i] is not None:
                    continue
                why = reasons.get(i, "not decoded")
                try:   # a page that is no scan: rasterised, as every page is with the option off
                    images = self._pre.pdf_to_images(pdf_path, first_page=i + 1, last_page=i + 1)
                    if not images:
                        raise ValueError("the rasteriser returned no page")
                    out[i] = self.process_pages_sync(images[:1], first_page_number=i + 1)[0]
                except Exception as e:
                    out[i] = OCROutput(success=False, error="page %d is not a scanned page the device decodes (%s) and could not be rasterised: %s"
                                       % (i + 1, why, e), page_number=i + 1)
            self._number_tables(out)
            return self._document_from_pages(out, t0)  # type: ignore[arg-type]
        except Exception as e:
            return DocumentOCRResult(success=False, error=str(e), total_processing_time_ms=_ms_since(t0))

    # ---- scanned TIFFs (LUMINA_OCR_DEVICE_TIFF=1): the pages' strips, decoded on the device ----
    def _decode_tiff_strips_in_place(self, eng, recs, w: int, h: int, rps: int, fax: bool):
        """Fax-coded (Group 4, Group 3, CCITT RLE: every strip restarts the coder) and Deflate pages of one shape through the existing one-image decoders: a strip is an image of rps rows, and the strips
        of a page are contiguous rows of its output.  The full strips of all pages decode in one call (in place as a [n * k, rps, W, 3] view
        when the height is a multiple of rps, else into a temporary that is copied); the shorter last strips of all pages go in one more.  -> (pages uint8 [n,H,W,3], status per page = the lowest of its strips')."""
        import torch
        n = len(recs)
        out = torch.empty((n, h, w, 3), dtype=torch.uint8, device=torch.device("cuda", self._device))
        full, rem = h // rps, h % rps
        status = [0] * n

        def run(strips, owners, rows, view):
            if fax:
                _, st = eng.fax_decode(strips, rows, w, [recs[o].ccitt_params() + (0,) for o in owners], out=view)
            else:
                _, st = eng.flate_image_decode(strips, rows, w, [recs[o].flate_params() for o in owners], [recs[o].palette for o in owners], out=view)
            for o, v in zip(owners, st):
                status[o] = min(status[o], v)

        if full and rem == 0:     # the pages follow each other without a gap: every strip of the group in one call, in place
            run([s for r in recs for s in r.strips], [k for k in range(n) for _ in range(full)], rps, out.view(n * full, rps, w, 3))
        elif full:                # a shorter last strip separates the pages: all full strips in one call into a temporary, then copied
            body = torch.empty((n * full, rps, w, 3), dtype=torch.uint8, device=out.device)
            run([s for r in recs for s in r.strips[:full]], [k for k in range(n) for _ in range(full)], rps, body)
            out[:, :full * rps] = body.view(n, full * rps, w, 3)
        if rem:
            last = torch.empty((n, rem, w, 3), dtype=torch.uint8, device=out.device)
            run([r.strips[full] for r in recs], list(range(n)), rem, last)
            out[:, full * rps:] = last
        return out, status

    def _decode_tiff_pages(self, entries, reasons: Dict[int, str]) -> Dict[int, Any]:
        """The accepted pages of tiff_pages.read_pages -> {page index: device tensor [1,H,W,3], Orientation applied}: grouped by codec
        and shape, one decoder call per group (the fax codings and Deflate: see _decode_tiff_strips_in_place).  A page a decoder refuses gets its
        reason in `reasons` (it goes to Pillow)."""
        groups: Dict[Any, List[int]] = {}
        for i, e in enumerate(entries):
            if isinstance(e, tiff_pages.PageImage):
                kind = "fax" if e.codec in tiff_pages.FAX_CODECS else e.codec if e.codec == "deflate" else "strips"
                groups.setdefault((kind, e.width, e.height, e.rows_per_strip), []).append(i)
        res: Dict[int, Any] = {}
        if not groups:
            return res
        self._ensure_engine()
        eng = self._engine
        with self._device_ctx():
            for (kind, w, h, rps), idxs in groups.items():
                recs = [entries[i] for i in idxs]
                try:
                    if kind == "strips":
                        out, status = eng.strip_image_decode([r.strips for r in recs], h, w, rps, [r.strip_params() for r in recs],
                                                             [r.palette for r in recs])
                    else:
                        out, status = self._decode_tiff_strips_in_place(eng, recs, w, h, rps, kind == "fax")
                except Exception as e:   # the engine's own failure: these pages go to Pillow
                    for i in idxs:
                        reasons[i] = "%s decode failed: %s" % (kind, e)
                    continue
                for k, i in enumerate(idxs):
                    if status[k] != 0:
                        reasons[i] = "%s strips %s (status %d)" % (recs[k].codec, "corrupt" if status[k] == -1 else "outside the device subset", status[k])
                        continue
                    res[i] = eng.exif_transpose(out[k:k + 1], recs[k].orientation)
        return res

    def _process_tiff_on_device(self, image_source: Union[str, Path, bytes], page_number: int) -> Optional[OCROutput]:
        """A TIFF path / bytes whose first page the device decodes -> its result; None: today's path."""
        try:
            if isinstance(image_source, bytes):
                data = image_source
            else:
                with open(image_source, "rb") as f:
                    if not tiff_pages.is_tiff(f.read(4)):
                        return None
                data = Path(image_source).read_bytes()
        except OSError:
            return None
        if not tiff_pages.is_tiff(data[:4]):
            return None
        try:
            first = tiff_pages.read_pages(data, max_pages=1)[0]
            if not isinstance(first, tiff_pages.PageImage):
                return None
            image = Image.open(io.BytesIO(data))      # lazily opened: consulted for its size only
            reasons: Dict[int, str] = {}
            decoded = self._decode_tiff_pages([first], reasons).get(0)
            if decoded is None or (int(decoded.shape[2]), int(decoded.shape[1])) != image.size:
                return None
        except Exception as e:       # any doubt: the reference's own path
            logger.warning("device TIFF decode not used: %s", e)
            return None
        return self._process_single_image_sync(image, page_number, decoded=decoded)

    def process_tiff_sync(self, tiff_path: Union[str, Path]) -> DocumentOCRResult:
        """Every page (IFD) of a TIFF: decoded on the device where the reader and the decoders take it, by Pillow (Image.open; seek(k))
        where they do not; same-size pages run through the engine as one batch; tables are numbered over the document."""
        t0 = time.time()
        path = Path(tiff_path)
        if not path.exists():
            return DocumentOCRResult(success=False, error=f"File not found: {path}")
        try:
            data = path.read_bytes()
            entries = tiff_pages.read_pages(data)
            reasons: Dict[int, str] = {}
            if isinstance(entries[0], tiff_pages.TiffRefused) and entries[0].whole_file:
                # not a file the reader takes: every frame Pillow finds is Pillow's
                try:
                    with Image.open(io.BytesIO(data)) as probe:
                        n = int(getattr(probe, "n_frames", 1))
                except Exception as e:
                    return DocumentOCRResult(success=False, error="%s (TIFF reader: %s)" % (e, entries[0].reason), total_processing_time_ms=_ms_since(t0))
                reasons = {i: entries[0].reason for i in range(n)}
                entries = [entries[0]] * n
            n = len(entries)
            for i, e in enumerate(entries):
                if isinstance(e, tiff_pages.TiffRefused):
                    reasons.setdefault(i, e.reason)
            out: List[Optional[OCROutput]] = [None] * n
            with self._semaphore:
                try:
                    on_device = self._decode_tiff_pages(entries, reasons)
                except Exception as e:   # no engine: errors are data
                    return DocumentOCRResult(success=False, error=str(e), total_processing_time_ms=_ms_since(t0))
                for i in range(n):
                    if i in on_device:
                        continue
                    why = reasons.get(i, "not decoded")
                    try:   # Pillow's frame, as every TIFF is read with the option off; it joins the group of its size
                        im = Image.open(io.BytesIO(data))
                        im.seek(i)
                        prepared = self._prepare(self._pre._normalise_mode(im))
                        with self._device_ctx():
                            on_device[i] = self._upload(self._stage_pages([prepared]))
                    except Exception as e:
                        out[i] = OCROutput(success=False, error="page %d is not a page the device decodes (%s) and Pillow could not decode it: %s"
                                           % (i + 1, why, e), page_number=i + 1)
                groups: Dict[Any, List[int]] = {}
                sizes: List[Any] = [None] * n
                for i, page in on_device.items():
                    sizes[i] = (int(page.shape[2]), int(page.shape[1]))   # the size the page has after Orientation
                    groups.setdefault(sizes[i], []).append(i)
                for idxs in groups.values():
                    self._run_group(sorted(idxs), on_device, None, sizes, 1, out)
            self._number_tables(out)
            return self._document_from_pages(out, t0)  # type: ignore[arg-type]
        except Exception as e:
            return DocumentOCRResult(success=False, error=str(e), total_processing_time_ms=_ms_since(t0))

    # ---- async wrappers (:666-731) ----
    async def process_image(self, image_source, page_number: int = 1, timeout: float = 120.0) -> OCROutput:
        try:
            return await asyncio.wait_for(asyncio.to_thread(self.process_image_sync, image_source, page_number), timeout=timeout)
        except asyncio.TimeoutError:
            return OCROutput(success=False, error=f"Timed out after {timeout}s")

    async def process_pdf(self, pdf_path, timeout: float = 600.0) -> DocumentOCRResult:
        try:
            return await asyncio.wait_for(asyncio.to_thread(self.process_pdf_sync, pdf_path), timeout=timeout)
        except asyncio.TimeoutError:
            return DocumentOCRResult(success=False, error=f"Timed out after {timeout}s")

    async def process_document(self, file_path: Union[str, Path], file_type: str) -> DocumentOCRResult:
        file_type = file_type.lower().strip(".")
        path = Path(file_path)
        if not path.exists():
            return DocumentOCRResult(success=False, error=f"File not found: {path}")
        if file_type == "pdf":
            return await self.process_pdf(path)
        if self.device_tiff and file_type in ("tiff", "tif"):
            try:
                return await asyncio.wait_for(asyncio.to_thread(self.process_tiff_sync, path), timeout=600.0)
            except asyncio.TimeoutError:
                return DocumentOCRResult(success=False, error="Timed out after 600.0s")
        if file_type in SUPPORTED_IMAGE_TYPES or (self.device_jp2 and file_type in JP2_FILE_TYPES):
            r = await self.process_image(path)
            return DocumentOCRResult(pages=[r], total_pages=1, total_processing_time_ms=r.processing_time_ms, success=r.success,
                                     error=r.error, combined_markdown=r.markdown, combined_html=r.html, combined_layout_boxes=r.layout_boxes)
        return DocumentOCRResult(success=False, error=f"Unsupported file type: {file_type}")

    # ---- status (:759-795) ----
    def get_status(self) -> Dict[str, Any]:
        st = {"client_initialized": self._pipeline is not None, "model_id": "dbnet-r18vd+crnn-mv3", "max_dimension": self.max_dimension,
              "device": self._device, "weights": self._weights_kind, "recognizer": self._recognizer, "apply_deskew": self.apply_deskew, "apply_binarize": bool(self.apply_binarize), "word_boxes": self._use_word_boxes, "barcodes": self._use_barcodes, "barcode_kinds": self._barcode_kinds_names(), "qrcodes": self._use_qrcodes, "qr_max_version": self._qr_max_version_status(), "datamatrix": self._use_datamatrix, "datamatrix_max_size": self._dm_max_size_status(), "aztec": self._use_aztec, "aztec_max_layers": self._aztec_max_layers_status(), "device_pdf": self.device_pdf, "pdf_layers": self.pdf_layers, "pdf_jbig2": self.pdf_jbig2, "progressive_jpeg": self.progressive_jpeg, "device_tiff": self.device_tiff, "device_jp2": self.device_jp2, "jp2_irreversible": self.jp2_irreversible, "jp2_tiles": self.jp2_tiles, "engine": "Lumina MI355X det+rec (HIP, gfx950)"}
        if self._engine is not None:
            st["engine_version"] = self._engine.version()
            st["num_classes"] = self._engine.num_classes
        return st

    def preload_model(self) -> None:
        self._ensure_engine()

    @property
    def is_model_loaded(self) -> bool:
        return self._pipeline is not None

    def cleanup(self) -> None:
        with self._engine_lock:
            if self._engine is not None:
                self._engine.close()
            self._engine = self._pipeline = None


ocr_service = OCRService()


async def ocr_node(state: Dict[str, Any]) -> Dict[str, Any]:
    """LangGraph node (:805-829)."""
    path = state.get("document_path")
    if not path:
        return {**state, "ocr_result": None, "ocr_markdown": "", "ocr_success": False, "ocr_error": "No document_path in state", "ocr_time_ms": 0}
    r = await ocr_service.process_document(path, state.get("file_type", ""))
    return {**state, "ocr_result": r.to_dict(), "ocr_markdown": r.combined_markdown, "ocr_success": r.success, "ocr_error": r.error,
            "ocr_time_ms": r.total_processing_time_ms}


def preload_ocr_model() -> None:
    try:
        ocr_service.preload_model()
    except Exception as e:
        logger.warning("OCR preload failed: %s", e)


async def get_ocr_status() -> Dict[str, Any]:
    return ocr_service.get_status()
