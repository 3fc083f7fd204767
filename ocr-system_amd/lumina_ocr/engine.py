"""ctypes binding of liblumina_ocr.so (include/lumina_ocr.h) — the only way the host reaches the GPU.

PyTorch-ROCm is used for device memory and streams only (tensor.data_ptr(), current stream);
no torch op runs on the hot path.  There is NO CPU fallback: a missing library or device raises
EngineUnavailable, which the provider turns into an error *result* (the reference's convention,
/root/reference/backend/services/ocr_service.py:464-475).
"""
from __future__ import annotations

import ctypes
import os
from pathlib import Path
from typing import Dict, Optional, Tuple

import numpy as np

from . import arch

_LIB_PATH = Path(__file__).resolve().parent.parent / "lib" / "liblumina_ocr.so"

REC_H, REC_W, REC_T = 32, 320, 80
MAX_WORDS = 40
MAX_BOXES = 1000


class EngineUnavailable(RuntimeError):
    pass


_MODEL_KINDS = ("det", "rec", "cls", "svtr")   # lumina_ocr_model_loaded's kind


class EngineError(RuntimeError):
    pass


_lib = None


def load_library() -> ctypes.CDLL:
    """Load the HIP engine; fails loudly when it has not been built (no fallback path exists)."""
    global _lib
    if _lib is not None:
        return _lib
    path = Path(os.environ.get("LUMINA_OCR_LIB", str(_LIB_PATH)))
    if not path.exists():
        raise EngineUnavailable(f"{path} not found: build it with `make -C ocr-system_amd` (hipcc, gfx950)")
    lib = ctypes.CDLL(str(path))
    c = ctypes
    vp, i32, f32, sz = c.c_void_p, c.c_int, c.c_float, c.c_size_t
    sig = {
        "lumina_ocr_create": (i32, [i32, c.POINTER(vp)]),
        "lumina_ocr_destroy": (None, [vp]),
        "lumina_ocr_last_error": (c.c_char_p, [vp]),
        "lumina_ocr_version": (c.c_char_p, []),
        "lumina_ocr_set_option": (i32, [vp, c.c_char_p, i32]),
        "lumina_ocr_load_det_weights": (i32, [vp, vp, sz]),
        "lumina_ocr_load_rec_weights": (i32, [vp, vp, sz]),
        "lumina_ocr_num_classes": (i32, [vp]),
        "lumina_ocr_model_loaded": (i32, [vp, i32]),
        "lumina_ocr_normalize": (i32, [vp, vp, i32, i32, i32, i32, i32, c.POINTER(f32), c.POINTER(f32), i32, vp, vp]),
        "lumina_ocr_det_forward": (i32, [vp, vp, i32, i32, i32, i32, i32, vp, vp]),
        "lumina_ocr_det_postprocess": (i32, [vp, vp, i32, i32, i32, i32, i32, f32, f32, f32, i32, i32, vp, vp, vp, vp]),
        "lumina_ocr_rec_crop": (i32, [vp, vp, i32, i32, i32, vp, vp, i32, vp, vp, vp]),
        "lumina_ocr_rec_crop_oriented": (i32, [vp, vp, i32, i32, i32, vp, vp, i32, vp, vp, vp, vp]),
        "lumina_ocr_cls_crop": (i32, [vp, vp, i32, i32, i32, vp, vp, i32, vp, vp, vp]),
        "lumina_ocr_load_cls_weights": (i32, [vp, vp, sz]),
        "lumina_ocr_cls_forward": (i32, [vp, vp, vp, i32, f32, vp, vp, vp, vp]),
        "lumina_ocr_rec_forward": (i32, [vp, vp, vp, i32, vp, vp, vp]),
        "lumina_ocr_ctc_decode": (i32, [vp, vp, vp, i32, vp, vp, vp, vp]),
        "lumina_ocr_ctc_decode_words": (i32, [vp, vp, vp, i32, vp, vp, vp, i32, vp, vp, vp, vp, vp, vp, vp, vp]),
        "lumina_ocr_conv2d": (i32, [vp, vp, i32, i32, i32, i32, vp, vp, i32, i32, i32, i32, vp, vp, vp]),
        "lumina_ocr_read_tap": (i32, [vp, c.c_char_p, vp, sz, c.POINTER(i32)]),
        "lumina_ocr_conv_timing": (i32, [vp, c.POINTER(c.c_double), c.POINTER(c.c_double), c.POINTER(i32)]),
        "lumina_ocr_conv_timing_detail": (i32, [vp, c.c_char_p, sz]),
        "lumina_ocr_resize_lanczos": (i32, [vp, vp, i32, i32, i32, i32, vp, i32, i32, vp]),
        "lumina_ocr_enhance": (i32, [vp, vp, i32, i32, i32, f32, f32, vp, vp, vp]),
        "lumina_ocr_jpeg_encode": (i32, [vp, vp, i32, i32, i32, i32, i32, vp, sz, vp, vp]),
        "lumina_ocr_jpeg_probe": (i32, [vp, sz, vp]),
        "lumina_ocr_jpeg_last_passes": (i32, [vp]),
        "lumina_ocr_jpeg_decode_async": (i32, [vp, vp, vp, i32, i32, i32, vp, vp, i32, vp]),
        "lumina_ocr_jpeg_decode": (i32, [vp, vp, vp, i32, i32, i32, vp, vp, vp]),
        "lumina_ocr_jpeg_probe_progressive": (i32, [vp, sz, vp]),
        "lumina_ocr_jpeg_decode_progressive": (i32, [vp, vp, vp, i32, i32, i32, vp, vp, vp]),
        "lumina_ocr_jpeg_coefficients": (i32, [vp, vp, i32, i32, i32, i32, vp, vp]),
        "lumina_ocr_png_probe": (i32, [vp, sz, vp]),
        "lumina_ocr_png_decode": (i32, [vp, vp, vp, i32, i32, i32, vp, vp, vp]),
        "lumina_ocr_webp_probe": (i32, [vp, sz, vp]),
        "lumina_ocr_webp_reason": (c.c_char_p, [i32]),
        "lumina_ocr_webp_decode": (i32, [vp, vp, vp, i32, i32, i32, vp, vp, vp]),
        "lumina_ocr_webp_probe_lossy": (i32, [vp, sz, vp]),
        "lumina_ocr_webp_decode_lossy": (i32, [vp, vp, vp, i32, i32, i32, vp, vp, vp]),
        "lumina_ocr_jp2_probe": (i32, [vp, sz, vp]),
        "lumina_ocr_jp2_reason": (c.c_char_p, [i32]),
        "lumina_ocr_jp2_decode": (i32, [vp, vp, vp, i32, i32, i32, vp, vp, vp]),
        "lumina_ocr_jp2_probe_irreversible": (i32, [vp, sz, vp]),
        "lumina_ocr_jp2_decode_irreversible": (i32, [vp, vp, vp, i32, i32, i32, vp, vp, vp]),
        "lumina_ocr_jp2_probe_ex": (i32, [vp, sz, c.c_uint, vp]),
        "lumina_ocr_jp2_decode_ex": (i32, [vp, vp, vp, i32, i32, i32, vp, vp, c.c_uint, vp]),
        "lumina_ocr_flate_image_decode": (i32, [vp, vp, vp, i32, i32, i32, vp, vp, vp, vp, vp]),
        "lumina_ocr_ccitt_decode": (i32, [vp, vp, vp, i32, i32, i32, vp, vp, vp, vp]),
        "lumina_ocr_fax_decode": (i32, [vp, vp, vp, i32, i32, i32, vp, vp, vp, vp]),
        "lumina_ocr_jbig2_probe": (i32, [vp, sz, vp, sz, vp]),
        "lumina_ocr_jbig2_reason": (c.c_char_p, [i32]),
        "lumina_ocr_jbig2_decode": (i32, [vp, vp, vp, vp, vp, i32, i32, i32, vp, vp, vp, vp]),
        "lumina_ocr_strip_image_decode": (i32, [vp, vp, vp, i32, vp, i32, i32, i32, i32, vp, vp, vp, vp, vp]),
        "lumina_ocr_load_svtr_weights": (i32, [vp, vp, sz]),
        "lumina_ocr_svtr_forward": (i32, [vp, vp, vp, i32, vp, vp, vp]),
        "lumina_ocr_svtr_num_classes": (i32, [vp]),
        "lumina_ocr_svtr_dtype": (i32, [vp]),
        "lumina_ocr_binarize": (i32, [vp, vp, i32, i32, i32, i32, i32, vp, vp]),
        "lumina_ocr_grayscale": (i32, [vp, vp, i32, i32, i32, vp, vp]),
        "lumina_ocr_exif_transpose": (i32, [vp, vp, i32, i32, i32, i32, vp, vp]),
        "lumina_ocr_denoise": (i32, [vp, vp, i32, i32, i32, vp, vp]),
        "lumina_ocr_deskew": (i32, [vp, vp, i32, i32, i32, vp, vp, vp, vp, vp, vp, vp]),
        "lumina_ocr_deskew_warp": (i32, [vp, vp, i32, i32, i32, vp, vp, vp]),
        "lumina_ocr_table_rules": (i32, [vp, vp, i32, i32, i32, i32, i32, i32, i32, i32, vp, vp, vp, vp, vp]),
        "lumina_ocr_selection_marks": (i32, [vp, vp, i32, i32, i32, i32, i32, i32, i32, vp, vp, vp, vp]),
        "lumina_ocr_barcodes": (i32, [vp, vp, i32, i32, i32, i32, i32, i32, i32, i32, i32, vp, vp, vp, vp, vp, vp]),
        "lumina_ocr_barcodes_kinds": (i32, [vp, vp, i32, i32, i32, i32, i32, i32, i32, i32, i32, vp, vp, vp, vp, vp, vp, i32]),
        "lumina_ocr_qrcodes": (i32, [vp, vp, i32, i32, i32] + [i32] * 9 + [vp] * 7),
        "lumina_ocr_qrcodes_versions": (i32, [vp, vp, i32, i32, i32] + [i32] * 10 + [vp] * 7),
        "lumina_ocr_datamatrix": (i32, [vp, vp, i32, i32, i32] + [i32] * 8 + [vp] * 7),
        "lumina_ocr_datamatrix_sizes": (i32, [vp, vp, i32, i32, i32] + [i32] * 9 + [vp] * 7),
        "lumina_ocr_datamatrix_sizes_workspace_bytes": (sz, [i32, i32, i32, i32, i32]),
        "lumina_ocr_datamatrix_placement": (i32, [i32, vp, i32]),
        "lumina_ocr_aztec": (i32, [vp, vp, i32, i32, i32] + [i32] * 9 + [vp] * 7),
        "lumina_ocr_aztec_layers": (i32, [vp, vp, i32, i32, i32] + [i32] * 10 + [vp] * 7),
        "lumina_ocr_rules_and_marks": (i32, [vp, vp, i32, i32, i32, i32, i32, i32, i32, i32, vp, vp, vp, i32, i32, i32, vp, vp, vp]),
        "lumina_ocr_selection_marks_round": (i32, [vp, vp, i32, i32, i32, i32, i32, i32, i32, vp, vp, vp, i32, i32, i32, i32, vp, vp, vp]),
        "lumina_ocr_rules_and_marks_round": (i32, [vp, vp, i32, i32, i32, i32, i32, i32, i32, i32, vp, vp, vp, i32, i32, i32, vp, vp,
                                                   i32, i32, i32, i32, vp, vp, vp]),
        "lumina_ocr_page_quarter_workspace_bytes": (sz, [i32, i32, i32]),
        "lumina_ocr_aztec_workspace_bytes": (sz, [i32, i32, i32, i32, i32]),
        "lumina_ocr_aztec_layers_workspace_bytes": (sz, [i32, i32, i32, i32, i32]),
        "lumina_ocr_page_quarter": (i32, [vp, vp, i32, i32, i32, i32, i32, vp, vp, vp]),
        "lumina_ocr_page_turn": (i32, [vp, vp, i32, i32, i32, vp, i32, i32, vp, vp]),
        "lumina_ocr_page_vote": (i32, [vp, vp, vp, i32, i32, vp, vp]),
        "lumina_ocr_page_compose": (i32, [vp, vp, i32, i32, i32, i32, vp, vp]),
    }
    missing = []
    for name, (res, args) in sig.items():
        try:
            fn = getattr(lib, name)
        except AttributeError:
            missing.append(name)
            continue
        fn.restype = res
        fn.argtypes = args
    lib._missing = missing  # exported-symbol check lives in tests/test_abi.py
    _lib = lib
    return lib


EXPORTED_SYMBOLS = [
    "lumina_ocr_create", "lumina_ocr_destroy", "lumina_ocr_last_error", "lumina_ocr_version", "lumina_ocr_set_option",
    "lumina_ocr_load_det_weights", "lumina_ocr_load_rec_weights", "lumina_ocr_num_classes", "lumina_ocr_model_loaded", "lumina_ocr_normalize",
    "lumina_ocr_det_forward", "lumina_ocr_det_postprocess", "lumina_ocr_rec_crop", "lumina_ocr_rec_crop_oriented", "lumina_ocr_cls_crop",
    "lumina_ocr_load_cls_weights", "lumina_ocr_cls_forward", "lumina_ocr_rec_forward",
    "lumina_ocr_ctc_decode", "lumina_ocr_ctc_decode_words", "lumina_ocr_conv2d", "lumina_ocr_read_tap", "lumina_ocr_conv_timing", "lumina_ocr_conv_timing_detail",
    "lumina_ocr_resize_lanczos", "lumina_ocr_enhance", "lumina_ocr_jpeg_encode", "lumina_ocr_jpeg_coefficients", "lumina_ocr_jpeg_probe", "lumina_ocr_jpeg_decode", "lumina_ocr_jpeg_decode_async", "lumina_ocr_jpeg_last_passes",
    "lumina_ocr_jpeg_probe_progressive", "lumina_ocr_jpeg_decode_progressive",
    "lumina_ocr_jp2_probe", "lumina_ocr_jp2_reason", "lumina_ocr_jp2_decode",
    "lumina_ocr_jp2_probe_irreversible", "lumina_ocr_jp2_decode_irreversible", "lumina_ocr_jp2_probe_ex", "lumina_ocr_jp2_decode_ex",
    "lumina_ocr_webp_probe", "lumina_ocr_webp_reason", "lumina_ocr_webp_decode", "lumina_ocr_webp_probe_lossy", "lumina_ocr_webp_decode_lossy",
    "lumina_ocr_png_probe", "lumina_ocr_png_decode", "lumina_ocr_flate_image_decode", "lumina_ocr_ccitt_decode", "lumina_ocr_fax_decode", "lumina_ocr_strip_image_decode",
    "lumina_ocr_jbig2_probe", "lumina_ocr_jbig2_reason", "lumina_ocr_jbig2_decode",
    "lumina_ocr_load_svtr_weights", "lumina_ocr_svtr_forward", "lumina_ocr_svtr_num_classes", "lumina_ocr_svtr_dtype", "lumina_ocr_binarize", "lumina_ocr_exif_transpose", "lumina_ocr_grayscale", "lumina_ocr_denoise", "lumina_ocr_deskew", "lumina_ocr_deskew_warp",
    "lumina_ocr_table_rules", "lumina_ocr_selection_marks", "lumina_ocr_rules_and_marks", "lumina_ocr_selection_marks_round",
    "lumina_ocr_rules_and_marks_round", "lumina_ocr_barcodes", "lumina_ocr_barcodes_kinds", "lumina_ocr_qrcodes", "lumina_ocr_qrcodes_versions", "lumina_ocr_datamatrix", "lumina_ocr_datamatrix_sizes", "lumina_ocr_datamatrix_sizes_workspace_bytes", "lumina_ocr_datamatrix_placement", "lumina_ocr_aztec", "lumina_ocr_aztec_workspace_bytes", "lumina_ocr_aztec_layers", "lumina_ocr_aztec_layers_workspace_bytes",
    "lumina_ocr_page_quarter_workspace_bytes", "lumina_ocr_page_quarter", "lumina_ocr_page_turn", "lumina_ocr_page_vote",
    "lumina_ocr_page_compose",
]


class ComposeLayer(ctypes.Structure):
    """lumina_ocr_compose_layer (include/lumina_ocr.h): one layer of a composed page"""
    _fields_ = [("page", ctypes.c_int32), ("kind", ctypes.c_int32), ("x0", ctypes.c_int32), ("y0", ctypes.c_int32), ("x1", ctypes.c_int32),
                ("y1", ctypes.c_int32), ("flip", ctypes.c_int32), ("fill", ctypes.c_int32), ("src", ctypes.c_void_p), ("w", ctypes.c_int32),
                ("h", ctypes.c_int32), ("mask", ctypes.c_void_p), ("mw", ctypes.c_int32), ("mh", ctypes.c_int32)]


def _torch():
    import torch
    return torch


def _ptr(t) -> int:
    return 0 if t is None else t.data_ptr()


class Engine:
    """One engine handle == one GPU.  Not re-entrant (the reference serialises pages the same way)."""

    def __init__(self, device: int = 0):
        torch = _torch()
        if not torch.cuda.is_available():
            raise EngineUnavailable("no ROCm device visible to torch (torch.cuda.is_available() is False)")
        self.lib = load_library()
        self.device = device
        torch.cuda.set_device(device)
        h = ctypes.c_void_p()
        rc = self.lib.lumina_ocr_create(device, ctypes.byref(h))
        self._h = h
        if rc != 0:
            msg = self.lib.lumina_ocr_last_error(h).decode() if h else "create failed"
            raise EngineUnavailable(msg)
        self.num_classes = self.svtr_num_classes = 0
        self.det_loaded = self.rec_loaded = self.svtr_loaded = self.cls_loaded = False

    # -- plumbing -------------------------------------------------------------------------
    def close(self):
        if getattr(self, "_h", None):
            self.lib.lumina_ocr_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _chk(self, rc: int):
        if rc != 0:
            raise EngineError(self.lib.lumina_ocr_last_error(self._h).decode())

    def _stream(self) -> int:
        return _torch().cuda.current_stream().cuda_stream

    def jpeg_encode(self, pages, quality: int = 95, max_bytes: int = 2 * 1024 * 1024, optimize: bool = True):
        """uint8 [n,H,W,3] device -> (files uint8 [n, stride] device, sizes int32 [n] device); sizes[i] < 0: file i needs more than
        max_bytes (the reference's cue to lower the quality).  Asynchronous; byte-identical to PIL save(JPEG, quality, optimize=True)."""
        torch = _torch()
        n, h, w, c = pages.shape
        assert c == 3 and pages.dtype == torch.uint8
        stride = (int(max_bytes) + 1023) // 1024 * 1024
        out = torch.empty((n, stride), dtype=torch.uint8, device=pages.device)
        sizes = torch.empty((n,), dtype=torch.int32, device=pages.device)
        self._chk(self.lib.lumina_ocr_jpeg_encode(self._h, _ptr(pages), n, h, w, int(quality), int(bool(optimize)), _ptr(out), stride, _ptr(sizes),
                                                  self._stream()))
        return out, sizes

    @staticmethod
    def jpeg_probe(data: bytes):
        """Host only. -> (rc, dict(width, height, ncomp, h, v, restart)); rc 0: the device decodes this file, -2: valid JPEG outside the
        subset (progressive, CMYK ...: decode with Pillow as the reference does), -1: corrupt / not a JPEG."""
        lib = load_library()
        info = (ctypes.c_int * 6)()
        buf = ctypes.c_char_p(data)
        rc = lib.lumina_ocr_jpeg_probe(buf, len(data), info)
        return rc, dict(width=info[0], height=info[1], ncomp=info[2], h=info[3], v=info[4], restart=info[5])

    def jpeg_decode(self, files, height: int, width: int, out=None):
        """JPEG file images (a sequence of bytes objects, all height x width) -> (uint8 [n,H,W,3] device, status list): the pixel work of
        the reference's Image.open for .jpg inputs (image_preprocessing.py:57-75), byte-identical to Pillow's decode.  status[i] != 0:
        page i was not decoded (-1 corrupt, -2 outside the device subset, -4 another size): the caller falls back to Pillow for it."""
        torch = _torch()
        n = len(files)
        if out is None:
            out = torch.empty((n, height, width, 3), dtype=torch.uint8, device=torch.device("cuda", self.device))
        ptrs = (ctypes.c_char_p * n)(*files)
        sizes = (ctypes.c_size_t * n)(*[len(f) for f in files])
        status = (ctypes.c_int * n)()
        self._chk(self.lib.lumina_ocr_jpeg_decode(self._h, ptrs, sizes, n, int(height), int(width), _ptr(out), status, self._stream()))
        return out, list(status)

    def jpeg_decode_async(self, files, height: int, width: int, out=None, passes: int = 12):
        """jpeg_decode without host synchronisation: -> (pages uint8 [n,H,W,3] device, status int32 [n] PINNED host tensor).  The status is
        valid once the current stream has run (e.g. after the event of the results that depend on the pages): 0 ok, -1 / -2 / -4 as
        jpeg_decode, -5 = `passes` synchronisation passes were not enough for that file (decode the batch again with jpeg_decode)."""
        torch = _torch()
        n = len(files)
        if out is None:
            out = torch.empty((n, height, width, 3), dtype=torch.uint8, device=torch.device("cuda", self.device))
        status = torch.zeros((n,), dtype=torch.int32).pin_memory()
        ptrs = (ctypes.c_char_p * n)(*files)
        sizes = (ctypes.c_size_t * n)(*[len(f) for f in files])
        self._chk(self.lib.lumina_ocr_jpeg_decode_async(self._h, ptrs, sizes, n, int(height), int(width), _ptr(out), status.data_ptr(), int(passes), self._stream()))
        return out, status

    @staticmethod
    def jpeg_probe_progressive(data: bytes):
        """Host only. jpeg_probe that also takes progressive files (SOF2) of the device subset -> (rc, dict(width, height, ncomp, h, v,
        restart, progressive, scans)); rc as jpeg_probe (-2: arithmetic, 12 bit, CMYK, more than 32 scans, scans short of full precision)."""
        lib = load_library()
        info = (ctypes.c_int * 8)()
        rc = lib.lumina_ocr_jpeg_probe_progressive(ctypes.c_char_p(data), len(data), info)
        return rc, dict(width=info[0], height=info[1], ncomp=info[2], h=info[3], v=info[4], restart=info[5], progressive=bool(info[6]), scans=info[7])

    def jpeg_decode_progressive(self, files, height: int, width: int, out=None):
        """jpeg_decode for batches that may hold progressive files: the same result and status codes, status 0 => byte-identical to
        Pillow's decode.  A sequential file takes jpeg_decode's kernels."""
        torch = _torch()
        n = len(files)
        if out is None:
            out = torch.empty((n, height, width, 3), dtype=torch.uint8, device=torch.device("cuda", self.device))
        ptrs = (ctypes.c_char_p * n)(*files)
        sizes = (ctypes.c_size_t * n)(*[len(f) for f in files])
        status = (ctypes.c_int * n)()
        self._chk(self.lib.lumina_ocr_jpeg_decode_progressive(self._h, ptrs, sizes, n, int(height), int(width), _ptr(out), status, self._stream()))
        return out, list(status)

    @staticmethod
    def png_probe(data: bytes):
        """Host only, the chunks before the first IDAT. -> (rc, dict(width, height, color_type, bit_depth, interlace, palette_size,
        orientation)); rc 0: the device decodes this file, -2: valid PNG outside the subset (Adam7, 16 bit ...: decode with Pillow as the
        reference does), -1: corrupt / not a PNG.  orientation: EXIF Orientation of an eXIf chunk before IDAT, 0 without one."""
        lib = load_library()
        info = (ctypes.c_int * 8)()
        rc = lib.lumina_ocr_png_probe(ctypes.c_char_p(data), len(data), info)
        return rc, dict(width=info[0], height=info[1], color_type=info[2], bit_depth=info[3], interlace=info[4], palette_size=info[5],
                        orientation=info[6])

    def png_decode(self, files, height: int, width: int, out=None):
        """PNG file images (a sequence of bytes objects, all height x width) -> (uint8 [n,H,W,3] device, status list): the pixels of the
        reference's Image.open(...).convert('RGB') for .png inputs (image_preprocessing.py:57-75), byte-identical to Pillow.  status[i] != 0:
        page i was not decoded (-1 corrupt, -2 outside the device subset, -4 another size) and is left to Pillow."""
        torch = _torch()
        n = len(files)
        if out is None:
            out = torch.empty((n, height, width, 3), dtype=torch.uint8, device=torch.device("cuda", self.device))
        ptrs = (ctypes.c_char_p * n)(*files)
        sizes = (ctypes.c_size_t * n)(*[len(f) for f in files])
        status = (ctypes.c_int * n)()
        self._chk(self.lib.lumina_ocr_png_decode(self._h, ptrs, sizes, n, int(height), int(width), _ptr(out), status, self._stream()))
        return out, list(status)

    @staticmethod
    def webp_probe(data: bytes):
        """Host only, the RIFF chunk headers and the VP8L header. -> (rc, dict(width, height, alpha, vp8x, exif, xmp, reason)); rc 0: the
        device decodes this file (lossless, one VP8L chunk, bare or inside VP8X), -2: valid WebP that is not read (lossy, ALPH, animated,
        more than 2^26 pixels: decode with Pillow as the reference does), -1: corrupt or irregular.  exif / xmp: the file has such a chunk."""
        lib = load_library()
        info = (ctypes.c_int * 8)()
        data = data if isinstance(data, bytes) else bytes(data)
        rc = lib.lumina_ocr_webp_probe(ctypes.c_char_p(data), len(data), info)
        return rc, dict(width=info[0], height=info[1], alpha=info[2], vp8x=info[3], exif=info[4], xmp=info[5],
                        reason=lib.lumina_ocr_webp_reason(rc).decode() if rc else "")

    def webp_decode(self, files, height: int, width: int, out=None):
        """Lossless WebP file images (a sequence of bytes objects, all height x width) -> (uint8 [n,H,W,3] device, status list): the pixels
        of the reference's Image.open(...).convert('RGB') for .webp inputs (image_preprocessing.py:57-75), byte-identical to Pillow.
        status[i] != 0: page i was not decoded (-1 corrupt, -2 not read by the device, -4 another size) and is left to Pillow."""
        torch = _torch()
        n = len(files)
        if out is None:
            out = torch.empty((n, height, width, 3), dtype=torch.uint8, device=torch.device("cuda", self.device))
        ptrs = (ctypes.c_char_p * n)(*files)
        sizes = (ctypes.c_size_t * n)(*[len(f) for f in files])
        status = (ctypes.c_int * n)()
        self._chk(self.lib.lumina_ocr_webp_decode(self._h, ptrs, sizes, n, int(height), int(width), _ptr(out), status, self._stream()))
        return out, list(status)

    @staticmethod
    def webp_probe_lossy(data: bytes):
        """Host only, as webp_probe, and rc 0 also for a still lossy file (one `VP8 ` chunk without ALPH, a key frame): the chunk headers
        and the boolean-coded frame header, no macroblock. -> (rc, dict(width, height, alpha, vp8x, exif, xmp, lossy, partitions,
        reason)); -2: lossy with ALPH, animated, more than 2^26 pixels; -1: corrupt or irregular."""
        lib = load_library()
        info = (ctypes.c_int * 8)()
        data = data if isinstance(data, bytes) else bytes(data)
        rc = lib.lumina_ocr_webp_probe_lossy(ctypes.c_char_p(data), len(data), info)
        return rc, dict(width=info[0], height=info[1], alpha=info[2], vp8x=info[3], exif=info[4], xmp=info[5], lossy=info[6],
                        partitions=info[7], reason=lib.lumina_ocr_webp_reason(rc).decode() if rc else "")

    def webp_decode_lossy(self, files, height: int, width: int, out=None):
        """WebP file images, lossy (VP8 key frames) and lossless in one batch (a sequence of bytes objects, all height x width) ->
        (uint8 [n,H,W,3] device, status list), byte-identical to Pillow's Image.open(...).convert('RGB').  The lossless files give
        webp_decode's bytes.  status[i] != 0: page i was not decoded (-1 corrupt, -2 not read by the device, -4 another size)."""
        torch = _torch()
        n = len(files)
        if out is None:
            out = torch.empty((n, height, width, 3), dtype=torch.uint8, device=torch.device("cuda", self.device))
        ptrs = (ctypes.c_char_p * n)(*files)
        sizes = (ctypes.c_size_t * n)(*[len(f) for f in files])
        status = (ctypes.c_int * n)()
        self._chk(self.lib.lumina_ocr_webp_decode_lossy(self._h, ptrs, sizes, n, int(height), int(width), _ptr(out), status, self._stream()))
        return out, list(status)

    JP2_ORDERS = ("LRCP", "RLCP", "RPCL", "PCRL", "CPRL")

    @staticmethod
    def jp2_probe(data: bytes):
        """Host only: the boxes, the headers and every packet header of a JPEG 2000 file (JP2 / JPX-baseline or a raw codestream); no
        pixel is decoded. -> (rc, dict(width, height, components, levels, layers, progression, codeblock_width, codeblock_height,
        reason)); rc 0: the device decodes this file, -2: valid outside the subset (9/7, tiles, precincts ...: decode with Pillow as the
        reference does), -1: corrupt or irregular.  reason: why a non-zero rc was given, for logs."""
        return Engine._jp2_probe(data, "lumina_ocr_jp2_probe")

    @staticmethod
    def jp2_probe_irreversible(data: bytes):
        """Host only. jp2_probe that also takes files of the 9/7 irreversible transform (expounded step sizes, at most 15 magnitude
        bit-planes a sub-band: OpenJPEG's files of up to 5 levels) -> (rc, dict) as jp2_probe."""
        return Engine._jp2_probe(data, "lumina_ocr_jp2_probe_irreversible")

    JP2_F_IRREVERSIBLE, JP2_F_TILES = 1, 2   # LUMINA_OCR_JP2_F_*

    @staticmethod
    def jp2_probe_ex(data: bytes, flags: int):
        """Host only. jp2_probe with `flags` naming what is read beyond the first subset: JP2_F_IRREVERSIBLE (9/7 files) and
        JP2_F_TILES (tiles, image and tile origins, user precincts) -> (rc, dict) as jp2_probe; with JP2_F_TILES width and height
        are those of the image area."""
        return Engine._jp2_probe(data, "lumina_ocr_jp2_probe_ex", int(flags))

    @staticmethod
    def _jp2_probe(data: bytes, entry: str, flags=None):
        lib = load_library()
        info = (ctypes.c_int * 8)()
        args = (ctypes.c_char_p(data), len(data)) + (() if flags is None else (flags,)) + (info,)
        rc = getattr(lib, entry)(*args)
        return rc, dict(width=info[0], height=info[1], components=info[2], levels=info[3], layers=info[4], progression=info[5],
                        codeblock_width=info[6], codeblock_height=info[7], reason=lib.lumina_ocr_jp2_reason(rc).decode() if rc else "")

    def jp2_decode(self, files, height: int, width: int, out=None):
        """JPEG 2000 file images (a sequence of bytes objects, all height x width) -> (uint8 [n,H,W,3] device, status list): the pixels of
        the reference's Image.open(...).convert('RGB') for .jp2 / .j2k inputs, byte-identical to Pillow.  status[i] != 0: page i was not
        decoded (-1 corrupt, -2 outside the device subset, -4 another size) and is left to Pillow."""
        return self._jp2_decode(self.lib.lumina_ocr_jp2_decode, files, height, width, out)

    def jp2_decode_irreversible(self, files, height: int, width: int, out=None):
        """jp2_decode for batches that may hold 9/7 (irreversible) files: the same result and status codes, status 0 => byte-identical
        to Pillow; a 5/3 file gives the bytes of jp2_decode."""
        return self._jp2_decode(self.lib.lumina_ocr_jp2_decode_irreversible, files, height, width, out)

    def jp2_decode_ex(self, files, height: int, width: int, flags: int, out=None):
        """jp2_decode with `flags` (JP2_F_IRREVERSIBLE | JP2_F_TILES): the same result and status codes, status 0 => byte-identical to
        Pillow; height and width are those of the image area.  A file the other entries take gives their bytes."""
        return self._jp2_decode(self.lib.lumina_ocr_jp2_decode_ex, files, height, width, out, int(flags))

    def _jp2_decode(self, entry, files, height: int, width: int, out, flags=None):
        torch = _torch()
        n = len(files)
        if out is None:
            out = torch.empty((n, height, width, 3), dtype=torch.uint8, device=torch.device("cuda", self.device))
        files = [f if isinstance(f, bytes) else bytes(f) for f in files]
        ptrs = (ctypes.c_char_p * n)(*files)
        sizes = (ctypes.c_size_t * n)(*[len(f) for f in files])
        status = (ctypes.c_int * n)()
        self._chk(entry(self._h, ptrs, sizes, n, int(height), int(width), _ptr(out), status, *(() if flags is None else (flags,)), self._stream()))
        return out, list(status)

    def _stream_batch(self, streams, height: int, width: int, out):
        torch = _torch()
        n = len(streams)
        if out is None:
            out = torch.empty((n, height, width, 3), dtype=torch.uint8, device=torch.device("cuda", self.device))
        streams = [s if isinstance(s, bytes) else bytes(s) for s in streams]   # (the records of utils/pdf_pages.py carry memoryviews)
        ptrs = (ctypes.c_char_p * n)(*streams)
        sizes = (ctypes.c_size_t * n)(*[len(s) for s in streams])
        return n, out, streams, ptrs, sizes, (ctypes.c_int * n)()

    def flate_image_decode(self, streams, height: int, width: int, params, palettes=None, out=None):
        """The /FlateDecode image streams of scanned PDF pages (all height x width) -> (uint8 [n,H,W,3] device, status list).  params: per
        stream (predictor, components, bits, indexed, invert); palettes: per stream None or 768 bytes of RGB (see lumina_ocr.h).
        status 0: exact pixels, -1 corrupt, -2 outside the supported combinations."""
        n, out, streams, ptrs, sizes, status = self._stream_batch(streams, height, width, out)
        flat = (ctypes.c_int32 * (5 * n))(*[int(v) for p in params for v in p])
        pals = None
        if palettes is not None and any(p is not None for p in palettes):
            keep = [None if p is None else bytes(p) for p in palettes]
            assert all(p is None or len(p) == 768 for p in keep)
            pals = (ctypes.c_char_p * n)(*keep)
        self._chk(self.lib.lumina_ocr_flate_image_decode(self._h, ptrs, sizes, n, int(height), int(width), flat, pals, _ptr(out), status, self._stream()))
        return out, list(status)

    def ccitt_decode(self, streams, rows: int, columns: int, params, out=None):
        """The /CCITTFaxDecode (Group 4, K < 0) streams of scanned PDF pages (all rows x columns) -> (uint8 [n,rows,columns,3] device,
        status list).  params: per stream (K, EncodedByteAlign, BlackIs1, invert).  status 0: exact pixels, -1 corrupt, -2 unsupported
        (K >= 0, EncodedByteAlign, columns > 8192)."""
        n, out, streams, ptrs, sizes, status = self._stream_batch(streams, rows, columns, out)
        flat = (ctypes.c_int32 * (4 * n))(*[int(v) for p in params for v in p])
        self._chk(self.lib.lumina_ocr_ccitt_decode(self._h, ptrs, sizes, n, int(rows), int(columns), flat, _ptr(out), status, self._stream()))
        return out, list(status)

    def fax_decode(self, streams, rows: int, columns: int, params, out=None):
        """Fax-coded streams (all rows x columns): /CCITTFaxDecode of any K, and the strips of TIFF Compression 2 / 3 / 4 -> (uint8
        [n,rows,columns,3] device, status list).  params: per stream (K, EncodedByteAlign, BlackIs1, invert, path); K < 0 is
        ccitt_decode's Group 4, K = 0 one-dimensional T.4, K > 0 two-dimensional T.4; path 0 automatic, 1 the serial walk.  status 0:
        exact pixels, -1 anything irregular (see lumina_ocr.h), -2 unsupported (K > 0 without EOLs, EncodedByteAlign with EOLs, path 2,
        columns > 8192)."""
        n, out, streams, ptrs, sizes, status = self._stream_batch(streams, rows, columns, out)
        flat = (ctypes.c_int32 * (5 * n))(*[int(v) for p in params for v in p])
        assert len(flat) == 5 * n
        self._chk(self.lib.lumina_ocr_fax_decode(self._h, ptrs, sizes, n, int(rows), int(columns), flat, _ptr(out), status, self._stream()))
        return out, list(status)

    @staticmethod
    def jbig2_probe(data: bytes, globals_data: bytes = None):
        """Host only: the segments of one page's /JBIG2Decode stream behind those of its /JBIG2Globals stream (or None); no pixel is
        decoded. -> (rc, dict(width, height, regions, arithmetic_regions, mmr_regions, highest_template, tpgdon, striped, reason)); rc 0:
        the device decodes this page (generic regions), -2: valid JBIG2 outside the subset (symbol dictionaries, text, halftone and
        refinement regions ...), -1: corrupt or irregular.  reason: why a non-zero rc was given, for logs."""
        lib = load_library()
        info = (ctypes.c_int * 8)()
        data = data if isinstance(data, bytes) else bytes(data)
        g = None if globals_data is None else (globals_data if isinstance(globals_data, bytes) else bytes(globals_data))
        rc = lib.lumina_ocr_jbig2_probe(ctypes.c_char_p(data), len(data), ctypes.c_char_p(g), len(g) if g else 0, info)
        return rc, dict(width=info[0], height=info[1], regions=info[2], arithmetic_regions=info[3], mmr_regions=info[4], highest_template=info[5],
                        tpgdon=info[6], striped=info[7], reason=lib.lumina_ocr_jbig2_reason(rc).decode() if rc else "")

    def jbig2_decode(self, streams, height: int, width: int, globals_list=None, invert=None, out=None):
        """/JBIG2Decode page or mask streams (all height x width) -> (uint8 [n,H,W,3] device, status list).  globals_list: per stream its
        /JBIG2Globals bytes or None; invert: per stream 0 | 1 (/Decode [1 0]; default 0: bit 1 is black).  status 0: exact pixels, -1
        corrupt, -2 outside the generic-region subset, -4 another size; a page with a non-zero status is not written."""
        n, out, streams, ptrs, sizes, status = self._stream_batch(streams, height, width, out)   # (n == 0: the call does nothing)
        keep = [None] * n if globals_list is None else [None if g is None else (g if isinstance(g, bytes) else bytes(g)) for g in globals_list]
        assert len(keep) == n
        gptrs = (ctypes.c_char_p * n)(*keep)
        gsizes = (ctypes.c_size_t * n)(*[len(g) if g else 0 for g in keep])
        flat = (ctypes.c_int32 * n)(*[int(v) for v in (invert if invert is not None else [0] * n)])
        self._chk(self.lib.lumina_ocr_jbig2_decode(self._h, ptrs, sizes, gptrs, gsizes, n, int(height), int(width), flat, _ptr(out), status, self._stream()))
        return out, list(status)

    def strip_image_decode(self, pages, height: int, width: int, rows_per_strip: int, params, palettes=None, out=None):
        """Strip-coded page images (the strips of scanned TIFF pages; PDF /LZWDecode and /RunLengthDecode streams as one-strip pages), all
        height x width with rows_per_strip rows a strip -> (uint8 [n,H,W,3] device, status list).  pages: per page the sequence of its
        strips (bytes or memoryviews) in row order; params: per page (codec 1 none | 5 LZW | 32773 PackBits, predictor, components, bits,
        indexed, invert, rle_eod); palettes: per page None or 768 bytes of RGB (see lumina_ocr.h).  status 0: exact pixels, -1 corrupt,
        -2 outside the supported combinations (a strip count other than ceil(height / rows_per_strip) among them)."""
        torch = _torch()
        n = len(pages)
        if out is None:
            out = torch.empty((n, height, width, 3), dtype=torch.uint8, device=torch.device("cuda", self.device))
        strips = [s if isinstance(s, bytes) else bytes(s) for p in pages for s in p]
        m = len(strips)
        ptrs = (ctypes.c_char_p * max(m, 1))(*strips)
        sizes = (ctypes.c_size_t * max(m, 1))(*[len(s) for s in strips])
        counts = (ctypes.c_int32 * n)(*[len(p) for p in pages])
        flat = (ctypes.c_int32 * (7 * n))(*[int(v) for p in params for v in p])
        assert len(flat) == 7 * n
        pals = None
        if palettes is not None and any(p is not None for p in palettes):
            keep = [None if p is None else bytes(p) for p in palettes]
            assert all(p is None or len(p) == 768 for p in keep)
            pals = (ctypes.c_char_p * n)(*keep)
        status = (ctypes.c_int * n)()
        self._chk(self.lib.lumina_ocr_strip_image_decode(self._h, ptrs, sizes, m, counts, n, int(height), int(width), int(rows_per_strip), flat, pals,
                                                         _ptr(out), status, self._stream()))
        return out, list(status)

    @property
    def jpeg_last_passes(self) -> int:
        return int(self.lib.lumina_ocr_jpeg_last_passes(self._h))

    def jpeg_coefficients(self, pages, quality: int = 95):
        torch = _torch()
        n, h, w, _ = pages.shape
        mcus = ((w + 15) // 16) * ((h + 15) // 16)
        coefs = torch.empty((n, mcus, 6, 64), dtype=torch.int16, device=pages.device)
        self._chk(self.lib.lumina_ocr_jpeg_coefficients(self._h, _ptr(pages), n, h, w, int(quality), _ptr(coefs), self._stream()))
        return coefs

    def set_option(self, key: str, value: int):
        self._chk(self.lib.lumina_ocr_set_option(self._h, key.encode(), int(value)))

    def version(self) -> str:
        return self.lib.lumina_ocr_version().decode()

    # -- weights --------------------------------------------------------------------------
    def _load(self, kind: str, weights, _offset: int = 0):
        """One LOCW blob (or a weight dict, written as one) into the model `kind`.  The engine checks every tensor before it touches the
        model (csrc/blob_check.h): a refused blob raises EngineError naming the reason and the tensor and leaves the model loaded
        before intact.  The Python-side flags follow the engine's, whatever the outcome.  _offset: bytes the blob is shifted from an
        aligned address (tests)."""
        blob = weights if isinstance(weights, (bytes, bytearray)) else arch.write_blob(weights)
        buf = ctypes.create_string_buffer(len(blob) + _offset)
        ctypes.memmove(ctypes.addressof(buf) + _offset, bytes(blob), len(blob))
        setattr(self, kind + "_loaded", False)
        try:
            self._chk(getattr(self.lib, "lumina_ocr_load_%s_weights" % kind)(self._h, ctypes.c_void_p(ctypes.addressof(buf) + _offset), len(blob)))
        finally:
            setattr(self, kind + "_loaded", bool(self.lib.lumina_ocr_model_loaded(self._h, _MODEL_KINDS.index(kind))))
            self.num_classes = self.lib.lumina_ocr_num_classes(self._h)
            self.svtr_num_classes = self.lib.lumina_ocr_svtr_num_classes(self._h)
            self.svtr_dtype = "f16" if self.lib.lumina_ocr_svtr_dtype(self._h) else "bf16"

    def load_det(self, weights, _offset: int = 0):
        self._load("det", weights, _offset)

    def load_rec(self, weights, _offset: int = 0):
        self._load("rec", weights, _offset)

    def load_cls(self, weights, _offset: int = 0):
        """Orientation-classifier weights (arch.make_cls_weights or a LOCW blob with the cls.* tensors)."""
        self._load("cls", weights, _offset)

    def load_svtr(self, weights, f16=None, _offset: int = 0):
        """SVTR recogniser weights (arch.make_svtr_weights or a LOCW blob with the svtr.* tensors): Tiny or Base, bf16 or fp16 as the
        blob's svtr.config says; f16 = True / False overrides the storage / MFMA type."""
        self.set_option("svtr_f16", -1 if f16 is None else int(bool(f16)))
        self._load("svtr", weights, _offset)

    # -- hot path -------------------------------------------------------------------------
    def normalize(self, img, hp: int, wp: int, scale, shift, nchw: bool = False):
        torch = _torch()
        n, h, w, _ = img.shape
        out = torch.empty((n, 3, hp, wp) if nchw else (n, hp, wp, 3), dtype=torch.bfloat16, device=img.device)
        sc = (ctypes.c_float * 3)(*scale)
        sh = (ctypes.c_float * 3)(*shift)
        self._chk(self.lib.lumina_ocr_normalize(self._h, _ptr(img), n, h, w, hp, wp, sc, sh, int(nchw), _ptr(out), self._stream()))
        return out

    def det_forward(self, pages, hp: Optional[int] = None, wp: Optional[int] = None, out=None):
        """pages uint8 [B,H,W,3] (device) -> probability map bf16 [B,Hp,Wp]."""
        torch = _torch()
        assert pages.dtype == torch.uint8 and pages.is_cuda and pages.is_contiguous() and pages.shape[-1] == 3
        b, h, w, _ = pages.shape
        hp = hp or (h + 31) // 32 * 32
        wp = wp or (w + 31) // 32 * 32
        if out is None:
            out = torch.empty((b, hp, wp), dtype=torch.bfloat16, device=pages.device)
        self._chk(self.lib.lumina_ocr_det_forward(self._h, _ptr(pages), b, h, w, hp, wp, _ptr(out), self._stream()))
        return out

    def det_postprocess(self, prob, valid_h: int, valid_w: int, thresh=arch.DET_THRESH, box_thresh=arch.DET_BOX_THRESH,
                        unclip_ratio=arch.DET_UNCLIP_RATIO, min_size=arch.DET_MIN_SIZE, max_boxes=MAX_BOXES):
        torch = _torch()
        b, hp, wp = prob.shape
        boxes = torch.zeros((b, max_boxes, 8), dtype=torch.int32, device=prob.device)
        scores = torch.zeros((b, max_boxes), dtype=torch.float32, device=prob.device)
        counts = torch.zeros((b,), dtype=torch.int32, device=prob.device)
        self._chk(self.lib.lumina_ocr_det_postprocess(self._h, _ptr(prob), b, hp, wp, valid_h, valid_w, thresh, box_thresh,
                                                      unclip_ratio, min_size, max_boxes, _ptr(boxes), _ptr(scores), _ptr(counts),
                                                      self._stream()))
        return boxes, scores, counts

    def rec_crop(self, pages, quads, page_idx, flip=None):
        """flip: None, or int32 [n] device flags (cls_forward's): a flagged crop is turned by 180 degrees within its valid width."""
        torch = _torch()
        b, h, w, _ = pages.shape
        n = quads.shape[0]
        crops = torch.empty((n, REC_H, REC_W, 3), dtype=torch.uint8, device=pages.device)
        widths = torch.empty((n,), dtype=torch.int32, device=pages.device)
        if n and flip is None:
            self._chk(self.lib.lumina_ocr_rec_crop(self._h, _ptr(pages), b, h, w, _ptr(quads), _ptr(page_idx), n, _ptr(crops),
                                                   _ptr(widths), self._stream()))
        elif n:
            if flip.dtype != torch.int32 or flip.device != pages.device or tuple(flip.shape) != (n,):
                raise ValueError("flip must be int32 [%d] on %s" % (n, pages.device))
            flip = flip.contiguous()
            self._chk(self.lib.lumina_ocr_rec_crop_oriented(self._h, _ptr(pages), b, h, w, _ptr(quads), _ptr(page_idx), n, _ptr(flip),
                                                            _ptr(crops), _ptr(widths), self._stream()))
        return crops, widths

    def cls_crop(self, pages, quads, page_idx):
        """The orientation classifier's crops: uint8 [n, 48, 192, 3] device + valid widths int32 [n] (min(192, ceil(48 * ratio)))."""
        torch = _torch()
        b, h, w, _ = pages.shape
        n = quads.shape[0]
        crops = torch.empty((n, arch.CLS_H, arch.CLS_W, 3), dtype=torch.uint8, device=pages.device)
        widths = torch.empty((n,), dtype=torch.int32, device=pages.device)
        if n:
            self._chk(self.lib.lumina_ocr_cls_crop(self._h, _ptr(pages), b, h, w, _ptr(quads), _ptr(page_idx), n, _ptr(crops),
                                                   _ptr(widths), self._stream()))
        return crops, widths

    def cls_forward(self, crops, widths=None, thresh: float = arch.CLS_THRESH):
        """cls_crop's crops uint8 [n, 48, 192, 3] device -> (label int32 [n]: 0 = "0", 1 = "180"; score float32 [n]: probability of the
        label; flip int32 [n]: label == 1 and score > thresh, rec_crop's flip argument).  Asynchronous."""
        torch = _torch()
        n = crops.shape[0]
        label = torch.empty((n,), dtype=torch.int32, device=crops.device)
        score = torch.empty((n,), dtype=torch.float32, device=crops.device)
        flip = torch.empty((n,), dtype=torch.int32, device=crops.device)
        if n:
            if crops.dtype != torch.uint8 or tuple(crops.shape[1:]) != (arch.CLS_H, arch.CLS_W, 3) or not crops.is_contiguous():
                raise ValueError("crops must be contiguous uint8 [n, %d, %d, 3]" % (arch.CLS_H, arch.CLS_W))
            self._chk(self.lib.lumina_ocr_cls_forward(self._h, _ptr(crops), _ptr(widths), n, float(thresh), _ptr(label), _ptr(score), _ptr(flip),
                                                      self._stream()))
        return label, score, flip

    def rec_forward(self, crops, widths=None):
        torch = _torch()
        n = crops.shape[0]
        idx = torch.empty((n, REC_T), dtype=torch.int32, device=crops.device)
        prob = torch.empty((n, REC_T), dtype=torch.float32, device=crops.device)
        if n:
            self._chk(self.lib.lumina_ocr_rec_forward(self._h, _ptr(crops), _ptr(widths), n, _ptr(idx), _ptr(prob), self._stream()))
        return idx, prob

    def svtr_forward(self, crops, widths=None):
        """Same contract as rec_forward, SVTR-Tiny backbone."""
        torch = _torch()
        n = crops.shape[0]
        idx = torch.empty((n, REC_T), dtype=torch.int32, device=crops.device)
        prob = torch.empty((n, REC_T), dtype=torch.float32, device=crops.device)
        if n:
            self._chk(self.lib.lumina_ocr_svtr_forward(self._h, _ptr(crops), _ptr(widths), n, _ptr(idx), _ptr(prob), self._stream()))
        return idx, prob

    def ctc_decode(self, idx, prob):
        torch = _torch()
        n = idx.shape[0]
        text = torch.empty((n, REC_T), dtype=torch.int32, device=idx.device)
        length = torch.empty((n,), dtype=torch.int32, device=idx.device)
        score = torch.empty((n,), dtype=torch.float32, device=idx.device)
        if n:
            self._chk(self.lib.lumina_ocr_ctc_decode(self._h, _ptr(idx), _ptr(prob), n, _ptr(text), _ptr(length), _ptr(score),
                                                     self._stream()))
        return text, length, score

    def ctc_decode_words(self, idx, prob, quads, widths, flip=None, space_id: int = -1):
        """ctc_decode + the words of every line from the CTC alignment (lumina_ocr_ctc_decode_words; the definition is in the header).
        quads int32 [n, 8] and widths int32 [n] are rec_crop's input and output, flip the flags it was given (or None), space_id the
        class of " " (-1: none, every line is one word).  -> (text, length, score) exactly as ctc_decode, then word_quads int32
        [n, 40, 8], word_spans int32 [n, 40, 2] (first character in text, count), word_scores float32 [n, 40], word_counts int32 [n];
        rows past a line's count are zero.  Asynchronous."""
        torch = _torch()
        n = idx.shape[0]
        dev = idx.device
        for name, t, shape in (("quads", quads, (n, 8)), ("widths", widths, (n,))) + ((("flip", flip, (n,)),) if flip is not None else ()):
            if t.dtype != torch.int32 or t.device != dev or tuple(t.shape) != shape:
                raise ValueError("%s must be int32 %s on %s" % (name, list(shape), dev))
        text = torch.empty((n, REC_T), dtype=torch.int32, device=dev)
        length = torch.empty((n,), dtype=torch.int32, device=dev)
        score = torch.empty((n,), dtype=torch.float32, device=dev)
        wquads = torch.zeros((n, MAX_WORDS, 8), dtype=torch.int32, device=dev)
        wspans = torch.zeros((n, MAX_WORDS, 2), dtype=torch.int32, device=dev)
        wscores = torch.zeros((n, MAX_WORDS), dtype=torch.float32, device=dev)
        wcounts = torch.zeros((n,), dtype=torch.int32, device=dev)
        if n:
            quads, widths = quads.contiguous(), widths.contiguous()
            flip = None if flip is None else flip.contiguous()
            self._chk(self.lib.lumina_ocr_ctc_decode_words(self._h, _ptr(idx), _ptr(prob), n, _ptr(quads), _ptr(widths), _ptr(flip), int(space_id),
                                                           _ptr(text), _ptr(length), _ptr(score), _ptr(wquads), _ptr(wspans), _ptr(wscores),
                                                           _ptr(wcounts), self._stream()))
        return text, length, score, wquads, wspans, wscores, wcounts

    # -- kernel-level ---------------------------------------------------------------------
    def conv2d(self, x, w_ohwi_f32: np.ndarray, bias: np.ndarray, ks: int, stride: int, act: int = 0, res=None):
        """x bf16 [N,H,W,Cin] device; weights OHWI float32 (bf16-exact) host -> y bf16 [N,Ho,Wo,Cout]."""
        torch = _torch()
        n, h, w, cin = x.shape
        cout = w_ohwi_f32.shape[0]
        ho = (h - 1) // stride + 1 if ks == 3 else h // stride
        wo = (w - 1) // stride + 1 if ks == 3 else w // stride
        y = torch.empty((n, ho, wo, cout), dtype=torch.bfloat16, device=x.device)
        wb = np.ascontiguousarray(arch.f32_to_bf16_bits(w_ohwi_f32))
        bb = np.ascontiguousarray(bias, np.float32)
        self._chk(self.lib.lumina_ocr_conv2d(self._h, _ptr(x), n, h, w, cin, wb.ctypes.data, bb.ctypes.data, cout, ks, stride, act,
                                             _ptr(res), _ptr(y), self._stream()))
        return y

    def read_tap(self, name: str, dtype: str = "bf16") -> np.ndarray:
        """Intermediate tensor of the last forward as float32 (dtype: the storage type of that tensor — "f16" for an SVTR fp16 model)."""
        dims = (ctypes.c_int * 4)()
        self._chk(self.lib.lumina_ocr_read_tap(self._h, name.encode(), None, 0, dims))
        n = int(np.prod(list(dims)))
        buf = np.empty(n, np.uint16)
        self._chk(self.lib.lumina_ocr_read_tap(self._h, name.encode(), buf.ctypes.data, n, dims))
        vals = buf.view(np.float16).astype(np.float32) if dtype == "f16" else arch.bf16_bits_to_f32(buf)
        return vals.reshape(tuple(dims))

    def conv_timing(self) -> Tuple[float, float, int]:
        ms, fl, n = ctypes.c_double(), ctypes.c_double(), ctypes.c_int()
        self._chk(self.lib.lumina_ocr_conv_timing(self._h, ctypes.byref(ms), ctypes.byref(fl), ctypes.byref(n)))
        return ms.value, fl.value, n.value

    def conv_timing_detail(self):
        buf = ctypes.create_string_buffer(1 << 20)
        self._chk(self.lib.lumina_ocr_conv_timing_detail(self._h, buf, len(buf)))
        rows = []
        for line in buf.value.decode().splitlines():
            name, kern, ms, gf, mb = line.split()
            rows.append((name, kern, float(ms), float(gf), float(mb)))
        return rows

    # -- pre-processing on device (image_preprocessing.py:81-110, :132-158) -----------------
    def resize_lanczos(self, img, out_h: int, out_w: int):
        torch = _torch()
        n, h, w, c = img.shape
        out = torch.empty((n, out_h, out_w, c), dtype=torch.uint8, device=img.device)
        self._chk(self.lib.lumina_ocr_resize_lanczos(self._h, _ptr(img), n, h, w, c, _ptr(out), out_h, out_w, self._stream()))
        return out

    # -- de-skew (image_preprocessing.py:372-460) ---------------------------------------------
    def deskew(self, pages, debug: bool = False, estimate_only: bool = False):
        """uint8 [n,H,W,3] device -> (de-skewed pages (or None), rot float64 [n,3] device = sin, cos, flag).  Asynchronous: the
        rotation of each page is estimated and applied on the device.  debug=True also returns (info int32 [n,2] = segments,
        peaks; Canny edge maps uint8 [n,H,W]; segments int32 [n,512,8,4]; segments per peak slot int32 [n,512])."""
        torch = _torch()
        n, h, w, c = pages.shape
        assert c == 3 and pages.dtype == torch.uint8 and pages.is_contiguous()
        out = None if estimate_only else torch.empty_like(pages)
        rot = torch.empty((n, 3), dtype=torch.float64, device=pages.device)
        info = torch.empty((n, 2), dtype=torch.int32, device=pages.device)
        edges = segs = nsegs = None
        if debug:
            edges = torch.empty((n, h, w), dtype=torch.uint8, device=pages.device)
            segs = torch.zeros((n, 512, 8, 4), dtype=torch.int32, device=pages.device)
            nsegs = torch.zeros((n, 512), dtype=torch.int32, device=pages.device)
        self._chk(self.lib.lumina_ocr_deskew(self._h, _ptr(pages), n, h, w, _ptr(out), _ptr(rot), _ptr(info), _ptr(edges), _ptr(segs), _ptr(nsegs),
                                             self._stream()))
        return (out, rot, info, edges, segs, nsegs) if debug else (out, rot)

    def deskew_warp(self, pages, rot):
        """The cubic warp alone for given (sin, cos, flag) triples (float64 [n,3] device); flag != 3 copies the page."""
        torch = _torch()
        n, h, w, _ = pages.shape
        out = torch.empty_like(pages)
        self._chk(self.lib.lumina_ocr_deskew_warp(self._h, _ptr(pages), n, h, w, _ptr(rot), _ptr(out), self._stream()))
        return out

    # -- ruled tables (the device half of the reference's `table` / `table_cell` entries, ocr_service.py:324-352) ----------------
    def table_rules(self, pages, threshold=None, gap=None, min_len=None, max_thick=None, max_rules=None, debug: bool = False):
        """uint8 [n,H,W,3] device -> (hrules int32 [n,max_rules,5], vrules int32 [n,max_rules,5], counts int32 [n,2]) on the device:
        the long thin ink lines of each page as x0, y0, x1, y1, area, horizontal ones sorted by (y0, x0, y1, x1), vertical ones by
        (x0, y0, x1, y1); counts = the true numbers (a list whose count exceeds max_rules is not written).  Parameters default to
        arch.TABLE_PARAMS.  Asynchronous.  debug=True also returns the ink mask as int64 [n,H,ceil(W/64)] (the uint64 words' bits)."""
        torch = _torch()
        n, h, w, c = pages.shape
        assert c == 3 and pages.dtype == torch.uint8 and pages.is_contiguous()
        tp = arch.TABLE_PARAMS
        threshold, gap, min_len = (tp[k] if v is None else int(v) for k, v in (("threshold", threshold), ("gap", gap), ("min_len", min_len)))
        max_thick, max_rules = (tp[k] if v is None else int(v) for k, v in (("max_thick", max_thick), ("max_rules", max_rules)))
        hrules = torch.zeros((n, max_rules, 5), dtype=torch.int32, device=pages.device)
        vrules = torch.zeros((n, max_rules, 5), dtype=torch.int32, device=pages.device)
        counts = torch.zeros((n, 2), dtype=torch.int32, device=pages.device)
        mask = torch.zeros((n, h, (w + 63) // 64), dtype=torch.int64, device=pages.device) if debug else None
        self._chk(self.lib.lumina_ocr_table_rules(self._h, _ptr(pages), n, h, w, threshold, gap, min_len, max_thick, max_rules, _ptr(hrules),
                                                  _ptr(vrules), _ptr(counts), _ptr(mask), self._stream()))
        return (hrules, vrules, counts, mask) if debug else (hrules, vrules, counts)

    # -- selection marks (the device half of the reference's `selection_mark` entries, ocr_service.py:313-322) -------------------
    @staticmethod
    def _mark_params(min_side, max_side, max_marks):
        mp = arch.MARK_PARAMS
        return tuple(mp[k] if v is None else int(v) for k, v in (("min_side", min_side), ("max_side", max_side), ("max_marks", max_marks)))

    def selection_marks(self, pages, threshold=None, min_side=None, max_side=None, max_marks=None, debug: bool = False):
        """uint8 [n,H,W,3] device -> (marks int32 [n,max_marks,8], counts int32 [n]) on the device: the checkboxes of each page as
        x0, y0, x1, y1, edge, ink_in, area_in, state (1 = selected), sorted by (y0, x0, y1, x1); counts = the true numbers (a list
        whose count exceeds max_marks is not written).  Parameters default to arch.MARK_PARAMS.  Asynchronous.  debug=True also
        returns the ink mask as int64 [n,H,ceil(W/64)] (the uint64 words' bits)."""
        torch = _torch()
        n, h, w, c = pages.shape
        assert c == 3 and pages.dtype == torch.uint8 and pages.is_contiguous()
        threshold = arch.MARK_PARAMS["threshold"] if threshold is None else int(threshold)
        min_side, max_side, max_marks = self._mark_params(min_side, max_side, max_marks)
        marks = torch.zeros((n, max(max_marks, 0), 8), dtype=torch.int32, device=pages.device)
        counts = torch.zeros((n,), dtype=torch.int32, device=pages.device)
        mask = torch.zeros((n, h, (w + 63) // 64), dtype=torch.int64, device=pages.device) if debug else None
        self._chk(self.lib.lumina_ocr_selection_marks(self._h, _ptr(pages), n, h, w, threshold, min_side, max_side, max_marks, _ptr(marks),
                                                      _ptr(counts), _ptr(mask), self._stream()))
        return (marks, counts, mask) if debug else (marks, counts)

    # -- barcodes (Code 128, Code 39, EAN / UPC, ITF; the host half is utils/barcodes.py) ------------------------------------------
    def barcodes(self, pages, threshold=None, quiet=None, max_dist=None, min_rows=None, row_gap=None, max_codes=None, mask_in=None,
                 debug: bool = False, kinds=None):
        """uint8 [n,H,W,3] device -> (codes int32 [n,max_codes,8], syms int32 [n,max_codes,64], counts int32 [n]) on the device: the
        barcodes of each page as x0, y0, x1, y1, kind (0 Code 128, 1 Code 39, 2 EAN-13, 3 EAN-8, 4 UPC-E, 5 ITF), nsym, rows, flags (bit 0
        reversed, bit 1 vertical, bit 2 ITF-14), sorted by (y0, x0, y1, x1), with their symbol values; counts = the true numbers (a list
        whose count exceeds max_codes is not written).  kinds: None reads Code 128 and Code 39 (lumina_ocr_barcodes); otherwise the set
        to read (lumina_ocr_barcodes_kinds) as a bit mask, bit k = kind k, or as names of arch.BARCODE_KINDS.  Parameters default to
        arch.BARCODE_PARAMS.  mask_in: the ink mask of the pages at this threshold, int64
        [n,H,ceil(W/64)], when it is there already.  Asynchronous.  debug=True also returns the ink mask the pass worked on."""
        torch = _torch()
        n, h, w, c = pages.shape
        assert c == 3 and pages.dtype == torch.uint8 and pages.is_contiguous()
        bp = arch.BARCODE_PARAMS
        threshold, quiet, max_dist, min_rows, row_gap, max_codes = (bp[k] if v is None else int(v) for k, v in (
            ("threshold", threshold), ("quiet", quiet), ("max_dist", max_dist), ("min_rows", min_rows), ("row_gap", row_gap), ("max_codes", max_codes)))
        if mask_in is not None:
            assert mask_in.dtype == torch.int64 and mask_in.is_contiguous() and tuple(mask_in.shape) == (n, h, (w + 63) // 64)
        codes = torch.zeros((n, max(max_codes, 0), 8), dtype=torch.int32, device=pages.device)
        syms = torch.zeros((n, max(max_codes, 0), 64), dtype=torch.int32, device=pages.device)
        counts = torch.zeros((n,), dtype=torch.int32, device=pages.device)
        mask = torch.zeros((n, h, (w + 63) // 64), dtype=torch.int64, device=pages.device) if debug else None
        args = (self._h, _ptr(pages), n, h, w, threshold, quiet, max_dist, min_rows, row_gap, max_codes, _ptr(codes), _ptr(syms), _ptr(counts),
                _ptr(mask_in), _ptr(mask), self._stream())
        if kinds is None:
            self._chk(self.lib.lumina_ocr_barcodes(*args))
        else:
            self._chk(self.lib.lumina_ocr_barcodes_kinds(*args, kinds if isinstance(kinds, int) else arch.barcode_kinds_mask(kinds)))
        return (codes, syms, counts, mask) if debug else (codes, syms, counts)

    # -- the matrix codes: what qrcodes, qrcodes_versions, datamatrix, datamatrix_sizes, aztec and aztec_layers share ------------------------------------
    def _matrix_codes(self, name, keys, defaults, data_cols, data_dtype, pages, params, mask_in, debug, extra=()):
        """lumina_ocr_<name> on pages: the scalars are params' values for `keys` (the last one is max_codes), defaulting to `defaults`,
        then `extra`; rows of 12 ints, data rows of data_cols elements of torch.<data_dtype>.
        -> (codes, data, counts), with debug also the ink mask and the finder or candidate counts."""
        torch = _torch()
        n, h, w, c = pages.shape
        assert c == 3 and pages.dtype == torch.uint8 and pages.is_contiguous()
        unknown = set(params) - set(keys)
        if unknown:
            raise TypeError("%s: unknown parameters %s" % (name, sorted(unknown)))
        q = [int(params[k]) if params.get(k) is not None else defaults[k] for k in keys]
        max_codes = q[-1]
        if mask_in is not None:
            assert mask_in.dtype == torch.int64 and mask_in.is_contiguous() and tuple(mask_in.shape) == (n, h, (w + 63) // 64)
        codes = torch.zeros((n, max(max_codes, 0), 12), dtype=torch.int32, device=pages.device)
        data = torch.zeros((n, max(max_codes, 0), data_cols), dtype=getattr(torch, data_dtype), device=pages.device)
        counts = torch.zeros((n,), dtype=torch.int32, device=pages.device)
        mask = torch.zeros((n, h, (w + 63) // 64), dtype=torch.int64, device=pages.device) if debug else None
        slots = torch.zeros((n,), dtype=torch.int32, device=pages.device) if debug else None
        self._chk(getattr(self.lib, "lumina_ocr_" + name)(self._h, _ptr(pages), n, h, w, *q, *(int(v) for v in extra), _ptr(codes), _ptr(data),
                                                          _ptr(counts), _ptr(slots), _ptr(mask_in), _ptr(mask), self._stream()))
        return (codes, data, counts, mask, slots) if debug else (codes, data, counts)

    # -- QR codes (Model 2; qrcodes: versions 1-10, qrcodes_versions: 1-40; the host half is utils/qrcodes.py) --------------------------------------------------------
    _QR_KEYS = ("threshold", "min_module", "max_module", "quiet", "centre_tol", "ring_tol", "timing_max", "max_finders", "max_codes")

    def qrcodes(self, pages, mask_in=None, debug: bool = False, **params):
        """uint8 [n,H,W,3] device -> (codes int32 [n,max_codes,12], data int32 [n,max_codes,288], counts int32 [n]) on the device: the
        QR symbols of each page as x0, y0, x1, y1, version, level (0..3 = L, M, Q, H), mask, ndata, corrected errors, rotation, format
        distance, timing mismatches, sorted by (y0, x0, y1, x1), with their corrected data codewords; counts = the true numbers (a list
        whose count exceeds max_codes is not written).  params: any of arch.QR_PARAMS' keys, defaulting to them.  mask_in: the ink
        mask of the pages at this threshold, int64 [n,H,ceil(W/64)], when it is there already.  Asynchronous.  debug=True also
        returns the ink mask the pass worked on and the finder count of every page."""
        return self._matrix_codes("qrcodes", self._QR_KEYS, arch.QR_PARAMS, 288, "int32", pages, params, mask_in, debug)

    def qrcodes_versions(self, pages, max_version: int, mask_in=None, debug: bool = False, **params):
        """qrcodes for versions 1 .. max_version (10..40): uint8 [n,H,W,3] device -> (codes int32 [n,max_codes,12], data uint8
        [n,max_codes,2956], counts int32 [n]).  Versions 1-10 are read as qrcodes reads them, with the same rows; a corner finder that
        gave no such symbol is tried for versions 11 .. max_version (lumina_ocr_qrcodes_versions).  The data codewords are bytes here.
        params, mask_in and debug as in qrcodes."""
        return self._matrix_codes("qrcodes_versions", self._QR_KEYS, arch.QR_PARAMS, 2956, "uint8", pages, params, mask_in, debug, (max_version,))

    # -- Data Matrix (ECC 200; datamatrix: 10 x 10 .. 52 x 52 and the rectangles, datamatrix_sizes: up to 144 x 144; the host half is utils/datamatrix.py) ------------------------------
    _DM_KEYS = ("threshold", "min_module", "max_module", "quiet", "timing_max", "solid_max", "max_candidates", "max_codes")

    def datamatrix(self, pages, mask_in=None, debug: bool = False, **params):
        """uint8 [n,H,W,3] device -> (codes int32 [n,max_codes,12], data int32 [n,max_codes,208], counts int32 [n]) on the device: the
        Data Matrix symbols of each page as x0, y0, x1, y1, rows, cols, ndata, corrected errors, rotation, timing mismatches, L misses,
        0, sorted by (y0, x0, y1, x1), with their corrected data codewords; counts = the true numbers (a list whose count exceeds
        max_codes is not written).  params: any of arch.DM_PARAMS' keys, defaulting to them.  mask_in: the ink mask of the pages at
        this threshold, int64 [n,H,ceil(W/64)], when it is there already.  Asynchronous.  debug=True also returns the ink mask the
        pass worked on and the candidate count of every page."""
        return self._matrix_codes("datamatrix", self._DM_KEYS, arch.DM_PARAMS, 208, "int32", pages, params, mask_in, debug)

    def datamatrix_sizes(self, pages, max_size: int, mask_in=None, debug: bool = False, **params):
        """datamatrix for every ECC 200 size up to max_size (52..144) modules a side: uint8 [n,H,W,3] device -> (codes int32
        [n,max_codes,12], data uint8 [n,max_codes,1560], counts int32 [n]).  Every symbol datamatrix reads comes with the same row and
        codewords; a component of 64 min_module .. 144 max_module a side that gave no such row goes through the second stage, which
        reads the squares of 64 x 64 .. max_size (lumina_ocr_datamatrix_sizes).  The data codewords are bytes here.  params, mask_in and
        debug as in datamatrix; the candidate count debug returns is the first stage's."""
        return self._matrix_codes("datamatrix_sizes", self._DM_KEYS, arch.DM_PARAMS, 1560, "uint8", pages, params, mask_in, debug, (max_size,))

    # -- Aztec (aztec: compact 1-4 layers, full-range 1-11 layers; aztec_layers: full-range up to 32; the host half is utils/aztec.py) ----------------------------------------------
    _AZTEC_KEYS = ("threshold", "min_module", "max_module", "quiet", "centre_tol", "ring_tol", "mark_max", "max_finders", "max_codes")

    def aztec(self, pages, mask_in=None, debug: bool = False, **params):
        """uint8 [n,H,W,3] device -> (codes int32 [n,max_codes,12], data int32 [n,max_codes,320], counts int32 [n]) on the device: the
        Aztec symbols of each page as x0, y0, x1, y1, layers, compact, codeword width, ndata, corrected errors, rotation, mode-message
        errors, mismatches, sorted by (y0, x0, y1, x1), with their corrected data codewords (still bit-stuffed); counts = the true
        numbers (a list whose count exceeds max_codes is not written).  params: any of arch.AZTEC_PARAMS' keys, defaulting to them.
        mask_in: the ink mask of the pages at this threshold, int64 [n,H,ceil(W/64)], when it is there already.  Asynchronous.
        debug=True also returns the ink mask the pass worked on and the finder count of every page."""
        return self._matrix_codes("aztec", self._AZTEC_KEYS, arch.AZTEC_PARAMS, 320, "int32", pages, params, mask_in, debug)

    def aztec_layers(self, pages, max_layers: int, mask_in=None, debug: bool = False, **params):
        """aztec for full-range symbols of up to max_layers (11..32) layers: uint8 [n,H,W,3] device -> (codes int32 [n,max_codes,12], data
        uint16 [n,max_codes,1664], counts int32 [n]).  Every symbol aztec reads comes with the same row and codewords; a full-range finder
        of 12 .. max_layers layers that gave no such row goes through the second stage (lumina_ocr_aztec_layers).  params, mask_in and
        debug as in aztec."""
        out = self._matrix_codes("aztec_layers", self._AZTEC_KEYS, arch.AZTEC_PARAMS, 1664, "int16", pages, params, mask_in, debug, (max_layers,))
        return out[:1] + (out[1].view(_torch().uint16),) + out[2:]   # (allocated as int16: the words are unsigned)

    def rules_and_marks(self, pages, threshold=None, gap=None, min_len=None, max_thick=None, max_rules=None, min_side=None, max_side=None,
                        max_marks=None):
        """table_rules and selection_marks of the same pages at one threshold, the ink mask computed once.
        -> (hrules, vrules, rule counts, marks, mark counts), each as the two calls return it."""
        torch = _torch()
        n, h, w, c = pages.shape
        assert c == 3 and pages.dtype == torch.uint8 and pages.is_contiguous()
        tp = arch.TABLE_PARAMS
        threshold, gap, min_len = (tp[k] if v is None else int(v) for k, v in (("threshold", threshold), ("gap", gap), ("min_len", min_len)))
        max_thick, max_rules = (tp[k] if v is None else int(v) for k, v in (("max_thick", max_thick), ("max_rules", max_rules)))
        min_side, max_side, max_marks = self._mark_params(min_side, max_side, max_marks)
        hrules = torch.zeros((n, max_rules, 5), dtype=torch.int32, device=pages.device)
        vrules = torch.zeros((n, max_rules, 5), dtype=torch.int32, device=pages.device)
        rcounts = torch.zeros((n, 2), dtype=torch.int32, device=pages.device)
        marks = torch.zeros((n, max_marks, 8), dtype=torch.int32, device=pages.device)
        mcounts = torch.zeros((n,), dtype=torch.int32, device=pages.device)
        self._chk(self.lib.lumina_ocr_rules_and_marks(self._h, _ptr(pages), n, h, w, threshold, gap, min_len, max_thick, max_rules, _ptr(hrules),
                                                      _ptr(vrules), _ptr(rcounts), min_side, max_side, max_marks, _ptr(marks), _ptr(mcounts),
                                                      self._stream()))
        return hrules, vrules, rcounts, marks, mcounts

    @staticmethod
    def _round_params(round_params):
        rp = dict(arch.ROUND_MARK_PARAMS if round_params is None else round_params)
        return tuple(int(rp[k]) for k in ("out_max", "ring_div", "band_div", "band_min"))

    def selection_marks_round(self, pages, threshold=None, min_side=None, max_side=None, max_marks=None, round_params=None, debug: bool = False):
        """selection_marks plus the round marks (radio buttons) of the same pages -> (marks, counts, round marks int32 [n,max_marks,8],
        round counts int32 [n]) on the device: the first two are selection_marks' outputs, the round list has the same row format, order
        and capacity.  round_params defaults to arch.ROUND_MARK_PARAMS.  Asynchronous.  debug=True also returns the ink mask."""
        torch = _torch()
        n, h, w, c = pages.shape
        assert c == 3 and pages.dtype == torch.uint8 and pages.is_contiguous()
        threshold = arch.MARK_PARAMS["threshold"] if threshold is None else int(threshold)
        min_side, max_side, max_marks = self._mark_params(min_side, max_side, max_marks)
        marks, rounds = (torch.zeros((n, max(max_marks, 0), 8), dtype=torch.int32, device=pages.device) for _ in range(2))
        counts, rcounts = (torch.zeros((n,), dtype=torch.int32, device=pages.device) for _ in range(2))
        mask = torch.zeros((n, h, (w + 63) // 64), dtype=torch.int64, device=pages.device) if debug else None
        self._chk(self.lib.lumina_ocr_selection_marks_round(self._h, _ptr(pages), n, h, w, threshold, min_side, max_side, max_marks, _ptr(marks),
                                                            _ptr(counts), _ptr(mask), *self._round_params(round_params), _ptr(rounds),
                                                            _ptr(rcounts), self._stream()))
        return (marks, counts, rounds, rcounts) + ((mask,) if debug else ())

    def rules_and_marks_round(self, pages, threshold=None, gap=None, min_len=None, max_thick=None, max_rules=None, min_side=None, max_side=None,
                              max_marks=None, round_params=None):
        """table_rules and selection_marks_round of the same pages at one threshold, the ink mask computed once.
        -> (hrules, vrules, rule counts, marks, mark counts, round marks, round counts), each as the two calls return it."""
        torch = _torch()
        n, h, w, c = pages.shape
        assert c == 3 and pages.dtype == torch.uint8 and pages.is_contiguous()
        tp = arch.TABLE_PARAMS
        threshold, gap, min_len = (tp[k] if v is None else int(v) for k, v in (("threshold", threshold), ("gap", gap), ("min_len", min_len)))
        max_thick, max_rules = (tp[k] if v is None else int(v) for k, v in (("max_thick", max_thick), ("max_rules", max_rules)))
        min_side, max_side, max_marks = self._mark_params(min_side, max_side, max_marks)
        hrules, vrules = (torch.zeros((n, max_rules, 5), dtype=torch.int32, device=pages.device) for _ in range(2))
        rcounts = torch.zeros((n, 2), dtype=torch.int32, device=pages.device)
        marks, rounds = (torch.zeros((n, max_marks, 8), dtype=torch.int32, device=pages.device) for _ in range(2))
        mcounts, ocounts = (torch.zeros((n,), dtype=torch.int32, device=pages.device) for _ in range(2))
        self._chk(self.lib.lumina_ocr_rules_and_marks_round(self._h, _ptr(pages), n, h, w, threshold, gap, min_len, max_thick, max_rules, _ptr(hrules),
                                                            _ptr(vrules), _ptr(rcounts), min_side, max_side, max_marks, _ptr(marks), _ptr(mcounts),
                                                            *self._round_params(round_params), _ptr(rounds), _ptr(ocounts), self._stream()))
        return hrules, vrules, rcounts, marks, mcounts, rounds, ocounts

    # -- page orientation (utils/page_orient.py, OcrPipeline.run_oriented) ---------------------------------------------------------
    def page_quarter(self, pages, threshold=None, ratio=None):
        """uint8 [n,H,W,3] device -> (energies int64 [n,2] = E_r, E_c: the summed squared differences of neighbouring row / column ink
        counts; sideways int32 [n]: E_c > ratio * E_r) on the device.  Parameters default to arch.PAGE_ORIENT_PARAMS.  Asynchronous."""
        torch = _torch()
        n, h, w, c = pages.shape
        assert c == 3 and pages.dtype == torch.uint8 and pages.is_contiguous()
        pp = arch.PAGE_ORIENT_PARAMS
        threshold, ratio = (pp[k] if v is None else int(v) for k, v in (("threshold", threshold), ("ratio", ratio)))
        energies = torch.zeros((n, 2), dtype=torch.int64, device=pages.device)
        sideways = torch.zeros((n,), dtype=torch.int32, device=pages.device)
        self._chk(self.lib.lumina_ocr_page_quarter(self._h, _ptr(pages), n, h, w, threshold, ratio, _ptr(energies), _ptr(sideways), self._stream()))
        return energies, sideways

    def page_turn(self, pages, index, turn: int):
        """uint8 [n,H,W,3] device, index int32 [m] device (entries 0..n-1, any order, repeats allowed), turn 0..3 -> uint8 [m,H',W',3]:
        page j = np.rot90(pages[index[j]], turn) byte for byte; (H', W') = (W, H) for turn 1 and 3.  Asynchronous."""
        torch = _torch()
        n, h, w, c = pages.shape
        assert c == 3 and pages.dtype == torch.uint8 and pages.is_contiguous()
        if index.dtype != torch.int32 or index.device != pages.device or index.dim() != 1:
            raise ValueError("index must be int32 [m] on %s" % pages.device)
        if turn not in (0, 1, 2, 3):
            raise ValueError("turn must be 0..3")
        index = index.contiguous()
        m = index.shape[0]
        out = torch.empty((m, w, h, 3) if turn & 1 else (m, h, w, 3), dtype=torch.uint8, device=pages.device)
        self._chk(self.lib.lumina_ocr_page_turn(self._h, _ptr(pages), n, h, w, _ptr(index), m, int(turn), _ptr(out), self._stream()))
        return out

    def page_compose(self, canvas_hw, n: int, layers):
        """Pages painted from decoded layers (lumina_ocr_page_compose): canvas_hw = (H, W) of every page, layers = [(page 0..n-1, kind 0..3,
        (x0, y0, x1, y1), flip 0 | 1, fill (r, g, b), src, mask), ...] grouped by page in ascending order, each page's in paint order, at
        most 64 a page; src / mask: uint8 [h,w,3] device tensors as the decoders write them (a mask is read from channel 0), None where the
        kind has none (0 opaque image: src; 1 stencil: mask; 2 image with soft mask, 3 image with explicit mask: both).  A pixel starts
        white and takes, per layer whose rectangle holds it, the sample that holds its centre -> uint8 [n,H,W,3].  The table is checked
        before anything is launched (EngineError with the reason).  Asynchronous; the caller keeps src / mask alive until the stream is
        past the call."""
        torch = _torch()
        h, w = int(canvas_hw[0]), int(canvas_hw[1])
        dev = torch.device("cuda", self.device)
        table = (ComposeLayer * max(1, len(layers)))()
        for rec, (page, kind, rect, flip, fill, src, mask) in zip(table, layers):
            for t in (src, mask):
                if t is not None and not (t.dtype == torch.uint8 and t.dim() == 3 and t.shape[2] == 3 and t.is_contiguous() and t.device == dev):
                    raise ValueError("src and mask must be contiguous uint8 [h,w,3] on %s" % dev)
            rec.page, rec.kind, rec.flip = int(page), int(kind), int(flip)
            rec.x0, rec.y0, rec.x1, rec.y1 = (int(v) for v in rect)
            rec.fill = int(fill[0]) | int(fill[1]) << 8 | int(fill[2]) << 16
            rec.src, rec.h, rec.w = (None, 0, 0) if src is None else (src.data_ptr(), src.shape[0], src.shape[1])
            rec.mask, rec.mh, rec.mw = (None, 0, 0) if mask is None else (mask.data_ptr(), mask.shape[0], mask.shape[1])
        if not (0 < h <= 65535 and 0 < w <= 65535 and n >= 0):
            raise ValueError("canvas sides must be 1..65535")
        out = torch.empty((n, h, w, 3), dtype=torch.uint8, device=dev)
        self._chk(self.lib.lumina_ocr_page_compose(self._h, ctypes.addressof(table), len(layers), int(n), h, w, _ptr(out), self._stream()))
        return out

    def page_vote(self, flip, page_idx, pages: int):
        """cls_forward's flip flags int32 [n] + the lines' page indices int32 [n] (device) -> int32 [pages, 2] device: lines of each
        page, lines among them whose flag is set.  Asynchronous."""
        torch = _torch()
        n = flip.shape[0]
        if flip.dtype != torch.int32 or page_idx.dtype != torch.int32 or tuple(page_idx.shape) != (n,) or flip.dim() != 1:
            raise ValueError("flip and page_idx must be int32 [n]")
        counts = torch.zeros((pages, 2), dtype=torch.int32, device=flip.device)
        self._chk(self.lib.lumina_ocr_page_vote(self._h, _ptr(flip.contiguous()), _ptr(page_idx.contiguous()), n, int(pages), _ptr(counts), self._stream()))
        return counts

    @staticmethod
    def skew_degrees(rot) -> list:
        """rot (device or host [n,3]) -> the angle the reference's deskew() returns next to the image (:441-447, :460):
        the detected angle when the page was rotated or left alone below 0.5 degrees, 0.0 otherwise.  Synchronises."""
        r = rot.cpu().numpy() if hasattr(rot, "cpu") else np.asarray(rot)
        return [float(np.degrees(np.arctan2(s, c))) if int(f) in (1, 3) else 0.0 for s, c, f in r]

    def binarize(self, img, adaptive: bool = True, threshold: int = 128):
        """image_preprocessing.py:462-494 (adaptive=True: Gaussian 11x11 adaptive threshold, C = 2) / :175-185 (adaptive=False: L > threshold,
        the reference's behaviour without OpenCV).  uint8 [n,H,W,3] device -> 0 / 255 on all three channels."""
        torch = _torch()
        n, h, w, c = img.shape
        assert c == 3 and img.dtype == torch.uint8
        out = torch.empty_like(img)
        self._chk(self.lib.lumina_ocr_binarize(self._h, _ptr(img), n, h, w, int(bool(adaptive)), int(threshold), _ptr(out), self._stream()))
        return out

    def exif_transpose(self, img, orientation: int):
        """auto_orient / ImageOps.exif_transpose (image_preprocessing.py:171-173) for EXIF orientation 1..8.  uint8 [n,H,W,3] device -> [n,H,W,3]
        (1..4) or [n,W,H,3] (5..8)."""
        torch = _torch()
        n, h, w, c = img.shape
        assert c == 3 and img.dtype == torch.uint8
        if orientation in (0, 1):
            return img
        out = torch.empty((n, w, h, 3) if orientation >= 5 else (n, h, w, 3), dtype=torch.uint8, device=img.device)
        self._chk(self.lib.lumina_ocr_exif_transpose(self._h, _ptr(img), n, h, w, int(orientation), _ptr(out), self._stream()))
        return out

    def grayscale(self, img):
        """convert_to_grayscale (image_preprocessing.py:167-169): PIL convert('L'), on all three channels.  uint8 [n,H,W,3] device."""
        torch = _torch()
        n, h, w, c = img.shape
        assert c == 3 and img.dtype == torch.uint8
        out = torch.empty_like(img)
        self._chk(self.lib.lumina_ocr_grayscale(self._h, _ptr(img), n, h, w, _ptr(out), self._stream()))
        return out

    def denoise(self, img):
        """denoise (image_preprocessing.py:160-165): PIL MedianFilter(3) per channel.  uint8 [n,H,W,3] device."""
        torch = _torch()
        n, h, w, c = img.shape
        assert c == 3 and img.dtype == torch.uint8
        out = torch.empty_like(img)
        self._chk(self.lib.lumina_ocr_denoise(self._h, _ptr(img), n, h, w, _ptr(out), self._stream()))
        return out

    def enhance(self, img, contrast: float = 1.2, sharpness: float = 1.1):
        torch = _torch()
        n, h, w, c = img.shape
        out = torch.empty_like(img)
        tmp = torch.empty_like(img)
        self._chk(self.lib.lumina_ocr_enhance(self._h, _ptr(img), n, h, w, contrast, sharpness, _ptr(tmp), _ptr(out), self._stream()))
        return out
