"""A PDF container reader for scanned documents: finds, per page, the one image that IS the page, without decoding a pixel.

The reference rasterises every PDF page with pdf2image / poppler (image_preprocessing.py pdf_to_images, ocr_service.py:508-660).  Most
PDFs that need OCR are scans: each page is one image XObject painted over the whole MediaBox, compressed with DCT (JPEG), Flate or CCITT
Group 4.  For those this module hands the compressed stream to the device decoders (lumina_ocr_jpeg_decode, lumina_ocr_flate_image_decode,
lumina_ocr_ccitt_decode), so a page is recognised at the scanner's own sample grid and only compressed bytes cross PCIe.

    read_pages(data) -> [PageImage | PdfRefused, ...]      one entry per page, in page order

Everything outside the scanned-page subset is refused with one exception type, PdfRefused, carrying the reason: raised for the file
(no header, no cross-reference, /Encrypt, a broken page tree), returned in the page's slot for a page (text, several images, a skewed
placement, an image dictionary outside the list below).  The caller sends refused pages to the rasteriser.

Supported container: %PDF- header, startxref, classic xref tables with /Prev, xref streams (with hybrid /XRefStm), object streams.  The
small metadata streams (xref streams, object streams, page contents, /Indexed lookups) are inflated on the host with zlib, PNG predictors
included; they are kilobytes, not pixels, and their inflated size is capped.
Supported page: content streams holding nothing but q, Q, cm and exactly one Do of an image XObject, whose matrix maps the unit square
onto the MediaBox: axis-aligned, positive scales, each edge within 1 % of the box side.
Supported image: /BitsPerComponent 1 or 8 (2 and 4 for grey / indexed Flate images); /ColorSpace DeviceGray, DeviceRGB, ICCBased with
N = 1 or 3 (READ AS ITS DEVICE ALTERNATE: the profile is not applied, as Pillow does not apply it to a JPEG or PNG file either), or
Indexed over those with hival <= 255; one /Filter (a name or a one-element array) of DCTDecode, FlateDecode, CCITTFaxDecode (and, with
strip_filters, LZWDecode and RunLengthDecode under the Flate rules); /Decode the default, or [1 0] on one-component Flate / CCITT
images; no /ImageMask, /SMask or /Mask.  With jpx=True also /JPXDecode (JPEG 2000, for lumina_ocr_jp2_decode): /ColorSpace absent or
DeviceGray / DeviceRGB matching the codestream's 1 or 3 components, /SMaskInData absent or 0, no /Decode, and the size in the codestream
equal to the dictionary's.

Layered pages (read_pages(..., layers=True); the provider asks with LUMINA_OCR_PDF_LAYERS=1): scanner output painted from several
images.  A page with one opaque image and no mask still yields the PageImage above, now also when it carries invisible text; any other
accepted page yields a PageLayers record, whose layers lumina_ocr_page_compose puts together on an integer canvas.
Content accepted: q, Q, cm and up to MAX_LAYERS = 64 Do of image XObjects; the fill colour by g, rg, or cs /DeviceGray | /DeviceRGB
followed by sc / scn with 1 or 3 numbers in [0, 1] (8 bits a channel as floor(v * 255 + 0.5), black by default, saved by q / Q); gs
when the ExtGState holds nothing beyond Type, SA, OP, op, OPM, CA / ca equal to 1, BM /Normal or /Compatible, SMask /None and AIS false;
the marked-content operators BMC BDC EMC MP DP (skipped); text objects whose text rendering mode (Tr: graphics state, saved by q / Q,
0 by default) is 3 at every showing operator (Tj TJ ' "), the other text operators being parsed and ignored.  Everything else is refused
with the reasons of the one-image reader: paths, clipping, inline images, shading, form XObjects, k / K, visible text.
Placement: every Do axis-aligned with positive scales; the hull of all layer rectangles covers the MediaBox within EDGE_TOLERANCE (a
single layer need not).
Layer kinds, kept in paint order: 0 an opaque image under the image rules above; 1 a stencil (/ImageMask true, 1 bit, Flate or CCITT,
LZW / RunLength with strip_filters; /Decode absent, [0 1] or [1 0]) painted in the fill colour current at its Do; 2 an image with an
/SMask (DeviceGray, 1 or 8 bits, Flate, CCITT, grey DCT, grey JPX with jpx; of any size of its own; /Decode default or [1 0]; no
/Matte); 3 an image with a /Mask stream (a 1-bit /ImageMask image; a sample that reads 1 after /Decode is masked out).  Refused, each
with its reason: a colour-key /Mask array, /SMaskInData other than 0, /SMask or /Mask on a stencil or on a mask, /SMask and /Mask on
one image, /Matte.
Canvas: with the MediaBox (X0, Y0, X1, Y1), layer i placed by cm (a, 0, 0, d, e, f) and showing an image of w x h samples (a stencil's
own size counts, the size of an /SMask or /Mask does not): sx = max w / a, sy = max h / d, R(v) = floor(v + 0.5), W = R((X1 - X0) sx),
H = R((Y1 - Y0) sy), and the layer's rectangle is x0 = R((e - X0) sx), x1 = R((e + a - X0) sx), y0 = R((Y1 - f - d) sy),
y1 = R((Y1 - f) sy), all in double precision on the host.  W or H above 65535, or W H above MAX_CANVAS_PIXELS (2^26: A4 at 600 dpi is
34.8 M), is refused; a rectangle may stick out of the canvas; one that is empty or misses the canvas is dropped.
JBIG2 (read_pages(..., jbig2=True); the provider asks with LUMINA_OCR_PDF_JBIG2=1): /JBIG2Decode images of one bit, DeviceGray or an
/ImageMask, /Decode absent, [0 1] or [1 0], with /DecodeParms << /JBIG2Globals stream >> resolved and handed over as bytes: as the one
image of a page and, with layers, as a stencil, a /Mask stream or a 1-bit /SMask.  Whether the stream is inside the decoder's subset
(generic regions; symbol-coded text is not) is the decoder's own parser's business: lumina_ocr_jbig2_probe / _decode answer -2 there.
Not read (the page is refused and goes to the rasteriser): JBIG2 without that option, rotated or flipped placements, clipped strips (re W n), white
re f underlays, form XObjects, CMYK fill, /Matte, colour-key masks, blend modes and constant alpha.  /Interpolate true is sampled as
false: every layer is shown by the sample that holds the pixel centre.

The reader ends on any input: every loop advances through the file or a decoded stream, /Prev chains, page-tree nodes and indirect
references (ExtGState and mask references among them) are followed through visited-sets, every offset and /Length is checked against the
file size, and the number of objects, the nesting depth, the number of pages and the number of layers of a page are capped.
"""
from __future__ import annotations

import math
import zlib
from dataclasses import dataclass, field
from typing import Any, Dict, List, Optional, Tuple, Union

MAX_OBJECTS = 1 << 20        # cross-reference entries / objects loaded
MAX_DEPTH = 48               # nesting of arrays and dictionaries, page-tree depth, graphics-state stack
MAX_PAGES = 20000
MAX_META_BYTES = 32 << 20    # inflated size of one metadata stream
EDGE_TOLERANCE = 0.01        # each image edge within this fraction of the MediaBox side
FILTERS = ("DCTDecode", "FlateDecode", "CCITTFaxDecode")
STRIP_FILTERS = ("LZWDecode", "RunLengthDecode")   # taken only when read_pages is asked to (strip_filters=True)
JPX_FILTER = "JPXDecode"                            # taken only when read_pages is asked to (jpx=True)
JBIG2_FILTER = "JBIG2Decode"                        # taken only when read_pages is asked to (jbig2=True)
MAX_LAYERS = 64                      # images painted on one page (read_pages with layers=True)
MAX_CANVAS_PIXELS = 1 << 26          # canvas of a layered page: A4 at 600 dpi is 4960 x 7016 = 34.8 M samples
MAX_COORD = 1 << 24                  # |coordinate| of a layer rectangle on the canvas grid

_WS = b"\x00\t\n\x0c\r "
_DELIM = b"()<>[]{}/%"
_TEXT_OPS = {"BT", "ET", "Tj", "TJ", "'", '"', "Tf", "Td", "TD", "Tm", "T*", "Tc", "Tw", "Tz", "TL", "Tr", "Ts"}
_CLIP_OPS = {"W", "W*"}


class PdfRefused(Exception):
    """The file, or one page of it, is outside the scanned-page subset; .reason says why."""
    def __init__(self, reason: str):
        super().__init__(reason)
        self.reason = reason


class Name(str):
    pass


@dataclass(frozen=True)
class Ref:
    num: int
    gen: int


class Stream(dict):
    """a stream's dictionary; .raw is the undecoded data as a memoryview into the file"""
    raw: memoryview = memoryview(b"")


@dataclass
class PageImage:
    filter: str                     # "DCTDecode" | "FlateDecode" | "CCITTFaxDecode" | "LZWDecode" | "RunLengthDecode" | "JPXDecode" | "JBIG2Decode"
    stream: memoryview              # the image's raw stream, a view into the file
    params: Dict[str, Any]          # FlateDecode, LZWDecode, RunLengthDecode: predictor, components, bits, indexed, invert, palette
    #                                 (768 bytes RGB or None); predictor is 1 | 2 for LZWDecode and 1 for RunLengthDecode
    #                                 CCITTFaxDecode: K, EncodedByteAlign, BlackIs1, invert;  DCTDecode, JPXDecode: components
    #                                 JBIG2Decode: globals (the /JBIG2Globals stream's bytes or None), invert
    width: int
    height: int
    rotate: int                     # /Rotate, 0 / 90 / 180 / 270 (clockwise, when displayed)
    media_box: Tuple[float, float, float, float] = field(default=(0.0, 0.0, 0.0, 0.0))


# ------------------------------------------------------------------------------------------------------------------ syntax
class _Parser:
    def __init__(self, data, pos: int = 0, end: Optional[int] = None):
        self.d = data
        self.p = pos
        self.end = len(data) if end is None else end

    def skip_ws(self) -> None:
        d, end = self.d, self.end
        while self.p < end:
            c = d[self.p]
            if c in _WS:
                self.p += 1
            elif c == 0x25:   # % comment, to the end of the line
                while self.p < end and d[self.p] not in b"\r\n":
                    self.p += 1
            else:
                return

    def token(self) -> bytes:
        """a run of regular characters (a number, a keyword or an operator); b"" at a delimiter or the end"""
        d, end, s = self.d, self.end, self.p
        p = s
        while p < end and d[p] not in _WS and d[p] not in _DELIM:
            p += 1
        self.p = p
        return bytes(d[s:p])

    def obj(self, depth: int = 0):
        if depth > MAX_DEPTH:
            raise PdfRefused("nesting too deep")
        self.skip_ws()
        d, end = self.d, self.end
        if self.p >= end:
            raise PdfRefused("unexpected end of data")
        c = d[self.p]
        if c == 0x3C:   # <
            if self.p + 1 < end and d[self.p + 1] == 0x3C:
                self.p += 2
                out: Dict[str, Any] = {}
                while True:
                    self.skip_ws()
                    if self.p + 1 < end and d[self.p] == 0x3E and d[self.p + 1] == 0x3E:
                        self.p += 2
                        return out
                    if self.p >= end or d[self.p] != 0x2F:
                        raise PdfRefused("malformed dictionary")
                    key = self.obj(depth + 1)
                    out[str(key)] = self.obj(depth + 1)
            self.p += 1
            s = self.p
            while self.p < end and d[self.p] != 0x3E:
                self.p += 1
            if self.p >= end:
                raise PdfRefused("unterminated hex string")
            hexs = bytes(d[s:self.p]).translate(None, _WS)
            self.p += 1
            try:
                return bytes.fromhex((hexs + (b"0" if len(hexs) & 1 else b"")).decode("ascii"))
            except (ValueError, UnicodeDecodeError):
                raise PdfRefused("malformed hex string")
        if c == 0x5B:   # [
            self.p += 1
            arr: List[Any] = []
            while True:
                self.skip_ws()
                if self.p >= end:
                    raise PdfRefused("unterminated array")
                if d[self.p] == 0x5D:
                    self.p += 1
                    return arr
                arr.append(self.obj(depth + 1))
        if c == 0x28:   # (
            return self._literal_string()
        if c == 0x2F:   # /
            self.p += 1
            raw = self.token()
            if b"#" in raw:
                parts = raw.split(b"#")
                try:
                    raw = parts[0] + b"".join(bytes([int(q[:2], 16)]) + q[2:] for q in parts[1:])
                except ValueError:
                    raise PdfRefused("malformed name")
            return Name(raw.decode("latin-1"))
        t = self.token()
        if not t:
            raise PdfRefused("unexpected delimiter %r" % chr(c))
        if t == b"true":
            return True
        if t == b"false":
            return False
        if t == b"null":
            return None
        num = _number(t)
        if num is None:
            raise PdfRefused("unexpected keyword %r" % t[:16].decode("latin-1"))
        if isinstance(num, int) and num >= 0:   # "N G R"?
            save = self.p
            self.skip_ws()
            g = _number(self.token())
            if isinstance(g, int) and 0 <= g <= 65535:
                self.skip_ws()
                if self.token() == b"R":
                    return Ref(num, g)
            self.p = save
        return num

    def _literal_string(self) -> bytes:
        d, end = self.d, self.end
        self.p += 1
        out = bytearray()
        level = 1
        while self.p < end:
            c = d[self.p]
            self.p += 1
            if c == 0x5C:   # backslash
                if self.p >= end:
                    break
                e = d[self.p]
                self.p += 1
                if e in b"nrtbf":
                    out.append(b"\n\r\t\b\f"[b"nrtbf".index(e)])
                elif 0x30 <= e <= 0x37:
                    v = e - 0x30
                    for _ in range(2):
                        if self.p < end and 0x30 <= d[self.p] <= 0x37:
                            v = v * 8 + d[self.p] - 0x30
                            self.p += 1
                    out.append(v & 255)
                elif e == 0x0D:
                    if self.p < end and d[self.p] == 0x0A:
                        self.p += 1
                elif e != 0x0A:
                    out.append(e)
            elif c == 0x28:
                level += 1
                out.append(c)
            elif c == 0x29:
                level -= 1
                if level == 0:
                    return bytes(out)
                out.append(c)
            else:
                out.append(c)
        raise PdfRefused("unterminated string")


def _number(t: bytes):
    if not t or len(t) > 32:
        return None
    try:
        return int(t)
    except ValueError:
        pass
    try:
        if any(ch not in b"+-.0123456789" for ch in t):
            return None
        return float(t)
    except ValueError:
        return None


# ------------------------------------------------------------------------------------------------------------------ host-side stream decoding
def _inflate(raw) -> bytes:
    try:
        z = zlib.decompressobj()
        out = z.decompress(bytes(raw), MAX_META_BYTES + 1)
    except zlib.error as e:
        raise PdfRefused("metadata stream does not inflate (%s)" % e)
    if len(out) > MAX_META_BYTES:
        raise PdfRefused("metadata stream too large")
    return out


def _png_unpredict(data: bytes, columns: int, colors: int, bits: int) -> bytes:
    """PNG row filters of a metadata stream (/Predictor >= 10), rows of 1 + ceil(columns * colors * bits / 8) bytes"""
    bpp = max(1, colors * bits // 8)
    rb = (columns * colors * bits + 7) // 8
    if rb <= 0 or len(data) % (rb + 1):
        raise PdfRefused("predictor rows do not fit the metadata stream")
    prev = bytearray(rb)
    out = bytearray()
    for r in range(len(data) // (rb + 1)):
        ft = data[r * (rb + 1)]
        row = bytearray(data[r * (rb + 1) + 1:(r + 1) * (rb + 1)])
        if ft == 2:
            row = bytearray((a + b) & 255 for a, b in zip(row, prev))
        elif ft == 1:
            for i in range(bpp, rb):
                row[i] = (row[i] + row[i - bpp]) & 255
        elif ft == 3:
            for i in range(rb):
                row[i] = (row[i] + (((row[i - bpp] if i >= bpp else 0) + prev[i]) >> 1)) & 255
        elif ft == 4:
            for i in range(rb):
                a, b, c = (row[i - bpp] if i >= bpp else 0), prev[i], (prev[i - bpp] if i >= bpp else 0)
                p = a + b - c
                pa, pb, pc = abs(p - a), abs(p - b), abs(p - c)
                row[i] = (row[i] + (a if pa <= pb and pa <= pc else b if pb <= pc else c)) & 255
        elif ft != 0:
            raise PdfRefused("bad row filter in a metadata stream")
        out += row
        prev = row
    return bytes(out)


# ------------------------------------------------------------------------------------------------------------------ the file
class _Document:
    def __init__(self, data):
        self.d = data if isinstance(data, (bytes, bytearray, memoryview)) else bytes(data)
        self.view = memoryview(self.d)
        self.n = len(self.d)
        self.xref: Dict[int, Tuple[int, int, int]] = {}   # object number -> (type 1: offset, generation | type 2: object stream, index)
        self.trailer: Dict[str, Any] = {}
        self.cache: Dict[int, Any] = {}
        self.objstm: Dict[int, Tuple[bytes, List[Tuple[int, int]]]] = {}
        self.loading: set = set()
        self.loaded = 0
        head = bytes(self.view[:1024])
        if b"%PDF-" not in head:
            raise PdfRefused("no %PDF- header")
        self._read_xref()
        if "Encrypt" in self.trailer:
            raise PdfRefused("encrypted (/Encrypt)")

    # ---- cross-reference ----
    def _read_xref(self) -> None:
        tail_at = max(0, self.n - 2048)
        tail = bytes(self.view[tail_at:])
        k = tail.rfind(b"startxref")
        if k < 0:
            raise PdfRefused("no startxref")
        p = _Parser(self.d, tail_at + k + 9)
        p.skip_ws()
        off = _number(p.token())
        if not isinstance(off, int):
            raise PdfRefused("malformed startxref")
        seen: set = set()
        pending = [off]
        while pending:
            off = pending.pop(0)
            if off in seen:
                continue   # a /Prev loop: every section is read once
            seen.add(off)
            if len(seen) > 4096:
                raise PdfRefused("too many cross-reference sections")
            if not 0 <= off < self.n:
                raise PdfRefused("cross-reference offset outside the file")
            trailer = self._xref_section(off)
            if not self.trailer:
                self.trailer = trailer
            nxt = []
            for key in ("XRefStm", "Prev"):
                v = trailer.get(key)
                if isinstance(v, int):
                    nxt.append(v)
            pending = nxt + pending
        if not isinstance(self.trailer.get("Root"), Ref):
            raise PdfRefused("no /Root in the trailer")

    def _set_entry(self, num: int, entry) -> None:
        if num not in self.xref:   # sections are read newest first
            if len(self.xref) >= MAX_OBJECTS:
                raise PdfRefused("too many objects")
            self.xref[num] = entry

    def _xref_section(self, off: int) -> Dict[str, Any]:
        p = _Parser(self.d, off)
        p.skip_ws()
        save = p.p
        if p.token() == b"xref":
            while True:
                p.skip_ws()
                save = p.p
                t = p.token()
                if t == b"trailer":
                    break
                first = _number(t)
                p.skip_ws()
                count = _number(p.token())
                if not isinstance(first, int) or not isinstance(count, int) or first < 0 or count < 0 or count > MAX_OBJECTS:
                    raise PdfRefused("malformed xref subsection")
                for i in range(count):
                    p.skip_ws()
                    o = _number(p.token())
                    p.skip_ws()
                    g = _number(p.token())
                    p.skip_ws()
                    kind = p.token()
                    if not isinstance(o, int) or not isinstance(g, int) or kind not in (b"n", b"f"):
                        raise PdfRefused("malformed xref entry")
                    if kind == b"n":
                        self._set_entry(first + i, (1, o, g))
            trailer = p.obj()
            if not isinstance(trailer, dict):
                raise PdfRefused("malformed trailer")
            return trailer
        # an xref stream
        p.p = save
        obj = self._indirect_at(off, None)
        if not isinstance(obj, Stream) or obj.get("Type") != "XRef":
            raise PdfRefused("no cross-reference at startxref")
        data = self._decode_meta(obj)
        w = obj.get("W")
        size = obj.get("Size")
        if not (isinstance(w, list) and len(w) == 3 and all(isinstance(x, int) and 0 <= x <= 8 for x in w)) or not isinstance(size, int):
            raise PdfRefused("malformed xref stream")
        index = obj.get("Index", [0, size])
        if not isinstance(index, list) or len(index) % 2 or not all(isinstance(x, int) and x >= 0 for x in index):
            raise PdfRefused("malformed xref stream /Index")
        rl = sum(w)
        if rl == 0:
            raise PdfRefused("malformed xref stream /W")
        at = 0
        for first, count in zip(index[0::2], index[1::2]):
            if count > MAX_OBJECTS:
                raise PdfRefused("too many objects")
            for i in range(count):
                if at + rl > len(data):
                    raise PdfRefused("xref stream shorter than its /Index")
                f = [int.from_bytes(data[at + sum(w[:k]):at + sum(w[:k + 1])], "big") for k in range(3)]
                at += rl
                kind = f[0] if w[0] else 1
                if kind == 1:
                    self._set_entry(first + i, (1, f[1], f[2]))
                elif kind == 2:
                    self._set_entry(first + i, (2, f[1], f[2]))
        return dict(obj)

    # ---- objects ----
    def _indirect_at(self, off: int, want: Optional[int]):
        """the object of "N G obj ... endobj" at `off` (its stream data located and bounds-checked, not decoded)"""
        if not 0 <= off < self.n:
            raise PdfRefused("object offset outside the file")
        p = _Parser(self.d, off)
        p.skip_ws()
        num = _number(p.token())
        p.skip_ws()
        gen = _number(p.token())
        p.skip_ws()
        if not isinstance(num, int) or not isinstance(gen, int) or p.token() != b"obj":
            raise PdfRefused("no object at its cross-reference offset")
        if want is not None and num != want:
            raise PdfRefused("object number differs from its cross-reference entry")
        obj = p.obj()
        p.skip_ws()
        save = p.p
        if isinstance(obj, dict) and p.token() == b"stream":
            d = self.d
            if p.p < self.n and d[p.p] == 0x0D:
                p.p += 1
            if p.p < self.n and d[p.p] == 0x0A:
                p.p += 1
            start = p.p
            length = obj.get("Length")
            if isinstance(length, Ref):
                length = self.resolve(length)
            if not isinstance(length, int) or length < 0 or start + length > self.n:
                raise PdfRefused("stream /Length outside the file")
            q = _Parser(self.d, start + length)
            q.skip_ws()
            if q.token() != b"endstream":
                raise PdfRefused("stream /Length does not end at endstream")
            s = Stream(obj)
            s.raw = self.view[start:start + length]
            return s
        p.p = save
        return obj

    def get(self, ref: Ref):
        if ref.num in self.cache:
            return self.cache[ref.num]
        entry = self.xref.get(ref.num)
        if entry is None:
            return None   # a reference to a missing object is null
        if ref.num in self.loading:
            raise PdfRefused("indirect reference loop")
        self.loaded += 1
        if self.loaded > MAX_OBJECTS:
            raise PdfRefused("too many objects")
        self.loading.add(ref.num)
        try:
            if entry[0] == 1:
                obj = self._indirect_at(entry[1], ref.num)
            else:
                obj = self._from_object_stream(entry[1], entry[2], ref.num)
        finally:
            self.loading.discard(ref.num)
        self.cache[ref.num] = obj
        return obj

    def resolve(self, obj):
        seen = set()
        while isinstance(obj, Ref):
            if obj.num in seen:
                raise PdfRefused("indirect reference loop")
            seen.add(obj.num)
            obj = self.get(obj)
        return obj

    def _from_object_stream(self, stm_num: int, index: int, want: int):
        if stm_num not in self.objstm:
            entry = self.xref.get(stm_num)
            if entry is None or entry[0] != 1:
                raise PdfRefused("object stream is not a plain object")
            stm = self.get(Ref(stm_num, 0))
            if not isinstance(stm, Stream) or stm.get("Type") != "ObjStm":
                raise PdfRefused("malformed object stream")
            n, first = stm.get("N"), stm.get("First")
            data = self._decode_meta(stm)
            if not isinstance(n, int) or not isinstance(first, int) or not 0 <= n <= MAX_OBJECTS or not 0 <= first <= len(data):
                raise PdfRefused("malformed object stream")
            p = _Parser(data, 0, first)
            pairs = []
            for _ in range(n):
                p.skip_ws()
                a = _number(p.token())
                p.skip_ws()
                b = _number(p.token())
                if not isinstance(a, int) or not isinstance(b, int) or b < 0 or first + b > len(data):
                    raise PdfRefused("malformed object stream header")
                pairs.append((a, first + b))
            self.objstm[stm_num] = (data, pairs)
        data, pairs = self.objstm[stm_num]
        if not 0 <= index < len(pairs) or pairs[index][0] != want:
            raise PdfRefused("object stream index differs from its cross-reference entry")
        return _Parser(data, pairs[index][1]).obj()

    # ---- metadata streams: decoded on the host ----
    def single_filter(self, stm: Stream) -> Tuple[Optional[str], Dict[str, Any]]:
        """(/Filter as one name or None, its /DecodeParms); a chain is refused"""
        f = self.resolve(stm.get("Filter"))
        parms = self.resolve(stm.get("DecodeParms"))
        if isinstance(f, list):
            if len(f) > 1:
                raise PdfRefused("filter chain")
            f = self.resolve(f[0]) if f else None
            if isinstance(parms, list):
                parms = self.resolve(parms[0]) if parms else None
        if f is not None and not isinstance(f, Name):
            raise PdfRefused("malformed /Filter")
        if parms is not None and not isinstance(parms, dict):
            raise PdfRefused("malformed /DecodeParms")
        return (None if f is None else str(f)), {k: self.resolve(v) for k, v in (parms or {}).items()}

    def _decode_meta(self, stm: Stream) -> bytes:
        f, parms = self.single_filter(stm)
        if f is None:
            if len(stm.raw) > MAX_META_BYTES:
                raise PdfRefused("metadata stream too large")
            return bytes(stm.raw)
        if f != "FlateDecode":
            raise PdfRefused("metadata stream filter %s" % f)
        data = _inflate(stm.raw)
        pred = parms.get("Predictor", 1)
        if pred == 1:
            return data
        if not isinstance(pred, int) or pred < 10:
            raise PdfRefused("metadata stream predictor %r" % (pred,))
        cols, colors, bits = parms.get("Columns", 1), parms.get("Colors", 1), parms.get("BitsPerComponent", 8)
        if not all(isinstance(v, int) and 0 < v <= 65536 for v in (cols, colors, bits)):
            raise PdfRefused("malformed predictor parameters")
        return _png_unpredict(data, cols, colors, bits)

    # ---- pages ----
    def pages(self) -> List[Tuple[Dict[str, Any], Dict[str, Any]]]:
        """[(page dictionary, inherited attributes)] in page order"""
        root = self.resolve(self.trailer["Root"])
        if not isinstance(root, dict) or not isinstance(root.get("Pages"), Ref):
            raise PdfRefused("no page tree")
        out: List[Tuple[Dict[str, Any], Dict[str, Any]]] = []
        seen: set = set()
        stack = [(root["Pages"], {}, 0)]
        while stack:
            ref, inherited, depth = stack.pop()
            if depth > MAX_DEPTH:
                raise PdfRefused("page tree too deep")
            if not isinstance(ref, Ref):
                raise PdfRefused("malformed page tree")
            if ref.num in seen:
                raise PdfRefused("page tree cycle")
            seen.add(ref.num)
            node = self.resolve(ref)
            if not isinstance(node, dict):
                raise PdfRefused("malformed page tree")
            attrs = dict(inherited)
            for key in ("MediaBox", "Rotate", "Resources"):
                if key in node:
                    attrs[key] = node[key]
            kids = self.resolve(node.get("Kids"))
            if node.get("Type") == "Pages" or (node.get("Type") is None and kids is not None):
                if not isinstance(kids, list):
                    raise PdfRefused("malformed page tree")
                for kid in reversed(kids):
                    stack.append((kid, attrs, depth + 1))
            else:
                out.append((node, attrs))
                if len(out) > MAX_PAGES:
                    raise PdfRefused("too many pages")
        if not out:
            raise PdfRefused("no pages")
        return out


# ------------------------------------------------------------------------------------------------------------------ one page
def _mul(m, n):
    """m applied first, then n (row vectors, as PDF writes matrices)"""
    a1, b1, c1, d1, e1, f1 = m
    a2, b2, c2, d2, e2, f2 = n
    return (a1 * a2 + b1 * c2, a1 * b2 + b1 * d2, c1 * a2 + d1 * c2, c1 * b2 + d1 * d2, e1 * a2 + f1 * c2 + e2, e1 * b2 + f1 * d2 + f2)


def _content_image(content: bytes) -> Tuple[str, Tuple[float, ...]]:
    """(XObject name, CTM at its Do) of a content stream that holds q / Q / cm and exactly one Do"""
    p = _Parser(content)
    ctm = (1.0, 0.0, 0.0, 1.0, 0.0, 0.0)
    stack: List[Tuple[float, ...]] = []
    operands: List[Any] = []
    found = None
    while True:
        p.skip_ws()
        if p.p >= p.end:
            break
        c = content[p.p]
        if c in b"/[(<" or c in b"+-.0123456789":
            operands.append(p.obj())
            if len(operands) > 64:
                raise PdfRefused("malformed content stream")
            continue
        op = p.token().decode("latin-1")
        if not op:
            raise PdfRefused("malformed content stream")
        if op == "q":
            stack.append(ctm)
            if len(stack) > MAX_DEPTH:
                raise PdfRefused("graphics state nested too deep")
        elif op == "Q":
            if not stack:
                raise PdfRefused("unbalanced Q")
            ctm = stack.pop()
        elif op == "cm":
            if len(operands) != 6 or not all(isinstance(v, (int, float)) and not isinstance(v, bool) for v in operands):
                raise PdfRefused("malformed cm")
            ctm = _mul(tuple(float(v) for v in operands), ctm)
        elif op == "Do":
            if len(operands) != 1 or not isinstance(operands[0], Name):
                raise PdfRefused("malformed Do")
            if found is not None:
                raise PdfRefused("several images on the page")
            found = (str(operands[0]), ctm)
        elif op in ("BI", "ID", "EI"):
            raise PdfRefused("inline image")
        elif op in _TEXT_OPS:
            raise PdfRefused("text operators on the page (%s)" % op)
        elif op in _CLIP_OPS:
            raise PdfRefused("clipping on the page (%s)" % op)
        else:
            raise PdfRefused("content operator %r" % op[:8])
        operands = []
    if found is None:
        raise PdfRefused("no image on the page")
    return found


def _components(doc: _Document, cs) -> int:
    """components of a device colour space, or of an ICCBased one taken as its device alternate"""
    cs = doc.resolve(cs)
    if isinstance(cs, Name):
        if cs == "DeviceGray":
            return 1
        if cs == "DeviceRGB":
            return 3
        raise PdfRefused("colour space %s" % cs)
    if isinstance(cs, list) and len(cs) == 2 and doc.resolve(cs[0]) == "ICCBased":
        prof = doc.resolve(cs[1])
        n = doc.resolve(prof.get("N")) if isinstance(prof, Stream) else None
        if n in (1, 3):
            return n
        raise PdfRefused("ICCBased colour space with N = %r" % (n,))
    raise PdfRefused("colour space %s" % (doc.resolve(cs[0]) if isinstance(cs, list) and cs else "malformed"))


def _colour_space(doc: _Document, cs):
    """-> (components of a sample, palette or None): palette = 768 bytes of RGB, entries past hival repeat the last one"""
    cs = doc.resolve(cs)
    if isinstance(cs, list) and len(cs) == 4 and doc.resolve(cs[0]) == "Indexed":
        base = _components(doc, cs[1])
        hival = doc.resolve(cs[2])
        if not isinstance(hival, int) or not 0 <= hival <= 255:
            raise PdfRefused("Indexed colour space with hival %r" % (hival,))
        lookup = doc.resolve(cs[3])
        if isinstance(lookup, Stream):
            lookup = doc._decode_meta(lookup)
        if not isinstance(lookup, bytes) or len(lookup) < (hival + 1) * base:
            raise PdfRefused("Indexed lookup shorter than hival")
        pal = bytearray()
        for i in range(256):
            k = min(i, hival) * base
            pal += lookup[k:k + 3] if base == 3 else bytes([lookup[k]]) * 3
        return 1, bytes(pal)
    return _components(doc, cs), None


def _jpx_size(raw) -> Tuple[int, int, int]:
    """(width, height, components) from the SIZ segment of a JPEG 2000 stream (a raw codestream, or the first jp2c box of a JP2 / JPX
    file); raises PdfRefused.  Nothing else is checked here: the decoder's own parser decides whether the stream is read."""
    d = bytes(raw[:1 << 16]) if len(raw) > (1 << 16) else bytes(raw)
    p = 0
    if d[:12] == b"\x00\x00\x00\x0cjP  \r\n\x87\n":
        p = 12
        for _ in range(64):
            if p + 8 > len(d):
                raise PdfRefused("JPX stream without a codestream box in its first 64 KB")
            ln, typ, hl = int.from_bytes(d[p:p + 4], "big"), d[p + 4:p + 8], 8
            if ln == 1:
                ln, hl = int.from_bytes(d[p + 8:p + 16], "big"), 16
            if typ == b"jp2c":
                p += hl
                break
            if ln < hl:
                raise PdfRefused("JPX stream with a malformed box")
            p += ln
        else:
            raise PdfRefused("JPX stream with too many boxes")
    if d[p:p + 4] != b"\xff\x4f\xff\x51" or p + 42 > len(d):
        raise PdfRefused("JPX stream without SOC and SIZ")
    q = p + 4
    x1, y1, x0, y0 = (int.from_bytes(d[q + o:q + o + 4], "big") for o in (4, 8, 12, 16))
    comps = int.from_bytes(d[q + 36:q + 38], "big")
    if x1 <= x0 or y1 <= y0:
        raise PdfRefused("JPX stream with an empty image")
    return x1 - x0, y1 - y0, comps


def _jpx_page_image(doc: _Document, img: Stream, width: int, height: int, rotate: int, media_box) -> PageImage:
    smask_in_data = doc.resolve(img.get("SMaskInData", 0))
    if smask_in_data != 0:
        raise PdfRefused("/SMaskInData %r" % (smask_in_data,))
    if doc.resolve(img.get("Decode")) is not None:
        raise PdfRefused("/Decode on a JPX image")
    cs = doc.resolve(img.get("ColorSpace"))
    if cs is not None and cs not in ("DeviceGray", "DeviceRGB"):
        raise PdfRefused("JPX image with /ColorSpace %r" % (cs if isinstance(cs, str) else type(cs).__name__,))
    w, h, comps = _jpx_size(img.raw)
    if (w, h) != (width, height):
        raise PdfRefused("JPX codestream is %d x %d, the image dictionary says %d x %d" % (w, h, width, height))
    if comps not in (1, 3) or (cs is not None and comps != (1 if cs == "DeviceGray" else 3)):
        raise PdfRefused("JPX codestream with %d components under /ColorSpace %r" % (comps, cs))
    return PageImage(filter=JPX_FILTER, stream=img.raw, params={"components": comps}, width=w, height=h, rotate=rotate, media_box=media_box)


def _jbig2_page_image(doc: _Document, img: Stream, parms: Dict[str, Any], width: int, height: int, rotate: int, media_box) -> PageImage:
    """the record of a /JBIG2Decode image: one bit of DeviceGray, /Decode absent, [0 1] or [1 0]; /JBIG2Globals (resolved by
    single_filter through the visited-set of every reference) is a stream whose bytes go in front of the image's"""
    bits = doc.resolve(img.get("BitsPerComponent", 1))
    cs = doc.resolve(img.get("ColorSpace"))
    if bits != 1 or cs != "DeviceGray":
        raise PdfRefused("JBIG2 image that is not one bit of grey")
    g = parms.get("JBIG2Globals")
    if g is not None and not isinstance(g, Stream):
        raise PdfRefused("/JBIG2Globals is not a stream")
    return PageImage(filter=JBIG2_FILTER, stream=img.raw, params={"globals": None if g is None else doc._decode_meta(g), "invert": bool(_mask_decode(doc, img))},
                     width=width, height=height, rotate=rotate, media_box=media_box)


def _page_frame(doc: _Document, page: Dict[str, Any], attrs: Dict[str, Any]):
    """-> ((x0, y0, x1, y1) of the MediaBox, /Rotate, the page's content bytes)"""
    box = doc.resolve(attrs.get("MediaBox"))
    if not isinstance(box, list) or len(box) != 4:
        raise PdfRefused("no MediaBox")
    box = [doc.resolve(v) for v in box]
    if not all(isinstance(v, (int, float)) and not isinstance(v, bool) for v in box):
        raise PdfRefused("malformed MediaBox")
    x0, x1 = sorted((float(box[0]), float(box[2])))
    y0, y1 = sorted((float(box[1]), float(box[3])))
    bw, bh = x1 - x0, y1 - y0
    if not (bw > 0 and bh > 0):
        raise PdfRefused("empty MediaBox")
    rotate = doc.resolve(attrs.get("Rotate", 0))
    if not isinstance(rotate, int) or rotate % 90:
        raise PdfRefused("malformed /Rotate")
    rotate %= 360
    # content
    contents = doc.resolve(page.get("Contents"))
    parts = contents if isinstance(contents, list) else [contents]
    if len(parts) > 64:
        raise PdfRefused("too many content streams")
    chunks = []
    for part in parts:
        s = doc.resolve(part)
        if not isinstance(s, Stream):
            raise PdfRefused("no page content")
        chunks.append(doc._decode_meta(s))
    return (x0, y0, x1, y1), rotate, b"\n".join(chunks)


def _xobject_image(doc: _Document, attrs: Dict[str, Any], name: str) -> Stream:
    res = doc.resolve(attrs.get("Resources"))
    xobjs = doc.resolve(res.get("XObject")) if isinstance(res, dict) else None
    img = doc.resolve(xobjs.get(name)) if isinstance(xobjs, dict) else None
    if not isinstance(img, Stream):
        raise PdfRefused("XObject %s not found" % name)
    if doc.resolve(img.get("Subtype")) != "Image":
        raise PdfRefused("XObject %s is not an image" % name)
    return img


def _page_image(doc: _Document, page: Dict[str, Any], attrs: Dict[str, Any], strip_filters: bool = False, jpx: bool = False,
                jbig2: bool = False) -> PageImage:
    (x0, y0, x1, y1), rotate, content = _page_frame(doc, page, attrs)
    bw, bh = x1 - x0, y1 - y0
    name, m = _content_image(content)
    a, b, c, d, e, f = m
    if not (a > 0 and d > 0) or abs(b) > 1e-4 * a or abs(c) > 1e-4 * d:
        raise PdfRefused("image placement is not axis-aligned with positive scales")
    if (abs(e - x0) > EDGE_TOLERANCE * bw or abs(e + a - x1) > EDGE_TOLERANCE * bw or abs(f - y0) > EDGE_TOLERANCE * bh
            or abs(f + d - y1) > EDGE_TOLERANCE * bh):
        raise PdfRefused("image does not cover the MediaBox")
    img = _xobject_image(doc, attrs, name)
    if doc.resolve(img.get("ImageMask")) is True:
        # a JBIG2 stencil alone on the page: painted in the fill colour no operator of this subset can change (black) on the white page,
        # which is the picture of the same samples as DeviceGray
        if not (jbig2 and doc.single_filter(img)[0] == JBIG2_FILTER):
            raise PdfRefused("/ImageMask")
        img = _without(img, ("ImageMask", "ColorSpace", "SMaskInData"), ColorSpace=Name("DeviceGray"), BitsPerComponent=doc.resolve(img.get("BitsPerComponent", 1)))
    for key in ("SMask", "Mask"):
        if doc.resolve(img.get(key)) is not None:
            raise PdfRefused("/" + key)
    return _image_record(doc, img, rotate, (x0, y0, x1, y1), strip_filters, jpx, jbig2)


def _image_record(doc: _Document, img: Stream, rotate: int, media_box, strip_filters: bool, jpx: bool, jbig2: bool = False) -> PageImage:
    """the record of one opaque image XObject (its mask keys are the caller's business)"""
    x0, y0, x1, y1 = media_box
    width, height = doc.resolve(img.get("Width")), doc.resolve(img.get("Height"))
    if not all(isinstance(v, int) and 0 < v <= 65535 for v in (width, height)):
        raise PdfRefused("malformed image size")
    filt, parms = doc.single_filter(img)
    if jpx and filt == JPX_FILTER:
        return _jpx_page_image(doc, img, width, height, rotate, (x0, y0, x1, y1))
    if jbig2 and filt == JBIG2_FILTER:
        return _jbig2_page_image(doc, img, parms, width, height, rotate, (x0, y0, x1, y1))
    if filt not in FILTERS and not (strip_filters and filt in STRIP_FILTERS):
        raise PdfRefused("image filter %s" % filt)
    bits = doc.resolve(img.get("BitsPerComponent", 1 if filt == "CCITTFaxDecode" else None))
    comps, palette = _colour_space(doc, img.get("ColorSpace"))
    decode = doc.resolve(img.get("Decode"))
    invert = False
    if decode is not None:
        decode = [doc.resolve(v) for v in decode] if isinstance(decode, list) else None
        top = (1 << bits) - 1 if (palette is not None and isinstance(bits, int) and 0 < bits <= 8) else 1
        if decode == [0, top] * comps:
            pass
        elif decode == [1, 0] and comps == 1 and palette is None and filt != "DCTDecode":
            invert = True
        else:
            raise PdfRefused("/Decode %r" % (decode,))
    if filt == "DCTDecode":
        if bits != 8 or palette is not None:
            raise PdfRefused("DCT image with %r bits per component" % (bits,))
        params: Dict[str, Any] = {"components": comps}
    elif filt == "CCITTFaxDecode":
        if bits != 1 or comps != 1 or palette is not None:
            raise PdfRefused("CCITT image that is not one bit of grey")
        k, cols, rows = parms.get("K", 0), parms.get("Columns", 1728), parms.get("Rows", 0)
        if not all(isinstance(v, int) for v in (k, cols, rows)) or cols != width or rows not in (0, height):
            raise PdfRefused("CCITT /Columns or /Rows differ from the image size")
        params = {"K": k, "EncodedByteAlign": parms.get("EncodedByteAlign", False) is True, "BlackIs1": parms.get("BlackIs1", False) is True,
                  "invert": invert}
    else:   # FlateDecode, LZWDecode, RunLengthDecode: the same rows, the same rules for bits, colour space and /Decode
        kind = {"FlateDecode": "Flate", "LZWDecode": "LZW", "RunLengthDecode": "RunLength"}[filt]
        if bits not in ((1, 2, 4, 8) if comps == 1 else (8,)):
            raise PdfRefused("%s image with %r bits per component" % (kind, bits))
        if filt == "RunLengthDecode":
            parms = {}                                   # (the filter has no parameters)
        if filt == "LZWDecode" and parms.get("EarlyChange", 1) != 1:
            raise PdfRefused("LZW /EarlyChange %r" % (parms.get("EarlyChange"),))
        pred = parms.get("Predictor", 1)
        if pred not in ((1, 2, 10, 11, 12, 13, 14, 15) if filt == "FlateDecode" else (1, 2)):
            raise PdfRefused("%s /Predictor %r" % (kind, pred))
        if pred != 1 and (parms.get("Colors", 1), parms.get("BitsPerComponent", 8), parms.get("Columns", 1)) != (comps, bits, width):
            raise PdfRefused("predictor parameters differ from the image")
        if pred == 2 and bits != 8:
            raise PdfRefused("TIFF predictor with %d-bit samples" % bits)
        params = {"predictor": pred, "components": comps, "bits": bits, "indexed": palette is not None, "invert": invert, "palette": palette}
    return PageImage(filter=filt, stream=img.raw, params=params, width=width, height=height, rotate=rotate, media_box=(x0, y0, x1, y1))


# ------------------------------------------------------------------------------------------------------------------ layered pages
@dataclass
class Layer:
    kind: int                        # 0 opaque image | 1 stencil | 2 image with /SMask | 3 image with a /Mask stream
    rect: Tuple[int, int, int, int]  # x0, y0, x1, y1 on the canvas grid, rows counted from the top; may stick out of the canvas
    fill: Tuple[int, int, int]       # the fill colour at the Do, 8 bits a channel (what a stencil is painted in)
    flip: int                        # the mask's /Decode is [1 0]: its samples are read inverted (masks are decoded with invert = 0)
    image: Optional[PageImage]       # kinds 0, 2, 3
    mask: Optional[PageImage]        # kinds 1, 2, 3: one grey component, read from channel 0 of the decoded image


@dataclass
class PageLayers:
    width: int                       # the canvas: the MediaBox at the finest sample grid among the layers
    height: int
    layers: List[Layer]              # in paint order, at most MAX_LAYERS
    rotate: int
    media_box: Tuple[float, float, float, float] = field(default=(0.0, 0.0, 0.0, 0.0))


_TEXT_SHOW_OPS = {"Tj", "TJ", "'", '"'}
_TEXT_STATE_OPS = {"Tf": 2, "Td": 2, "TD": 2, "Tm": 6, "T*": 0, "Tc": 1, "Tw": 1, "Tz": 1, "TL": 1, "Ts": 1}   # operands; parsed and ignored
_MARKED_OPS = {"BMC", "BDC", "EMC", "MP", "DP"}
_GS_HARMLESS = ("Type", "SA", "OP", "op", "OPM")


def _is_num(v) -> bool:
    return isinstance(v, (int, float)) and not isinstance(v, bool)


def _colour8(vals) -> Tuple[int, int, int]:
    if len(vals) not in (1, 3) or not all(_is_num(v) and 0 <= v <= 1 for v in vals):
        raise PdfRefused("malformed fill colour")
    c = [int(float(v) * 255 + 0.5) for v in vals]
    return (c[0], c[0], c[0]) if len(c) == 1 else (c[0], c[1], c[2])


def _gs_harmless(doc: _Document, attrs: Dict[str, Any], name: str) -> None:
    """refuses a `gs` whose ExtGState could change what an image paints"""
    res = doc.resolve(attrs.get("Resources"))
    table = doc.resolve(res.get("ExtGState")) if isinstance(res, dict) else None
    gs = doc.resolve(table.get(name)) if isinstance(table, dict) else None
    if not isinstance(gs, dict):
        raise PdfRefused("ExtGState %s not found" % name)
    for key, v in gs.items():
        v = doc.resolve(v)
        if key in _GS_HARMLESS:
            continue
        if key in ("CA", "ca"):
            if not _is_num(v) or v != 1:
                raise PdfRefused("ExtGState /%s %r (constant alpha)" % (key, v))
        elif key == "BM":
            if v not in ("Normal", "Compatible"):
                raise PdfRefused("ExtGState /BM %s (blend mode)" % (v if isinstance(v, str) else "malformed"))
        elif key == "SMask":
            if v != "None":
                raise PdfRefused("ExtGState /SMask")
        elif key == "AIS":
            if v is not False:
                raise PdfRefused("ExtGState /AIS true")
        else:
            raise PdfRefused("ExtGState /%s" % key[:16])


def _content_layers(doc: _Document, attrs: Dict[str, Any], content: bytes) -> List[Tuple[str, Tuple[float, ...], Tuple[int, int, int]]]:
    """[(XObject name, CTM at its Do, fill colour at its Do)] in paint order, of a content stream that holds q / Q / cm / Do, fill
    colours, harmless gs, marked content and invisible text (text rendering mode 3 at every showing operator)"""
    p = _Parser(content)
    state = ((1.0, 0.0, 0.0, 1.0, 0.0, 0.0), (0, 0, 0), 1, 0)   # CTM, fill colour, components of the fill colour space, Tr
    stack: List[Any] = []
    operands: List[Any] = []
    found: List[Tuple[str, Tuple[float, ...], Tuple[int, int, int]]] = []
    in_text = False
    while True:
        p.skip_ws()
        if p.p >= p.end:
            break
        c = content[p.p]
        if c in b"/[(<" or c in b"+-.0123456789":
            operands.append(p.obj())
            if len(operands) > 64:
                raise PdfRefused("malformed content stream")
            continue
        op = p.token().decode("latin-1")
        if not op:
            raise PdfRefused("malformed content stream")
        ctm, fill, fill_comps, tr = state
        if op == "q":
            stack.append(state)
            if len(stack) > MAX_DEPTH:
                raise PdfRefused("graphics state nested too deep")
        elif op == "Q":
            if not stack:
                raise PdfRefused("unbalanced Q")
            state = stack.pop()
        elif op == "cm":
            if len(operands) != 6 or not all(_is_num(v) for v in operands):
                raise PdfRefused("malformed cm")
            state = (_mul(tuple(float(v) for v in operands), ctm), fill, fill_comps, tr)
        elif op == "Do":
            if len(operands) != 1 or not isinstance(operands[0], Name):
                raise PdfRefused("malformed Do")
            if len(found) >= MAX_LAYERS:
                raise PdfRefused("more than %d images on the page" % MAX_LAYERS)
            found.append((str(operands[0]), ctm, fill))
        elif op in ("g", "rg"):
            if len(operands) != (1 if op == "g" else 3):
                raise PdfRefused("malformed fill colour")
            state = (ctm, _colour8(operands), len(operands), tr)
        elif op == "cs":
            if len(operands) != 1 or operands[0] not in ("DeviceGray", "DeviceRGB"):
                raise PdfRefused("fill colour space %s" % (operands[0] if operands and isinstance(operands[0], Name) else "malformed"))
            state = (ctm, (0, 0, 0), 1 if operands[0] == "DeviceGray" else 3, tr)
        elif op in ("sc", "scn"):
            if len(operands) != fill_comps:
                raise PdfRefused("malformed fill colour")
            state = (ctm, _colour8(operands), fill_comps, tr)
        elif op == "gs":
            if len(operands) != 1 or not isinstance(operands[0], Name):
                raise PdfRefused("malformed gs")
            _gs_harmless(doc, attrs, str(operands[0]))
        elif op in _MARKED_OPS:
            pass
        elif op == "BT":
            if in_text:
                raise PdfRefused("malformed content stream")
            in_text = True
        elif op == "ET":
            if not in_text:
                raise PdfRefused("malformed content stream")
            in_text = False
        elif op == "Tr":
            if len(operands) != 1 or not isinstance(operands[0], int) or isinstance(operands[0], bool):
                raise PdfRefused("malformed Tr")
            state = (ctm, fill, fill_comps, operands[0])
        elif op in _TEXT_STATE_OPS:
            if len(operands) != _TEXT_STATE_OPS[op]:
                raise PdfRefused("malformed %s" % op)
        elif op in _TEXT_SHOW_OPS:
            if not in_text or tr != 3:
                raise PdfRefused("text operators on the page (%s)" % op)
        elif op in ("BI", "ID", "EI"):
            raise PdfRefused("inline image")
        elif op in _CLIP_OPS:
            raise PdfRefused("clipping on the page (%s)" % op)
        else:
            raise PdfRefused("content operator %r" % op[:8])
        operands = []
    if not found:
        raise PdfRefused("no image on the page")
    return found


def _mask_decode(doc: _Document, stm: Stream) -> int:
    """-> 1 when the mask's /Decode is [1 0], 0 when it is absent or [0 1]"""
    decode = doc.resolve(stm.get("Decode"))
    if decode is None:
        return 0
    decode = [doc.resolve(v) for v in decode] if isinstance(decode, list) else None
    if decode == [0, 1]:
        return 0
    if decode == [1, 0]:
        return 1
    raise PdfRefused("/Decode %r on a mask" % (decode,))


def _without(stm: Stream, drop, **add) -> Stream:
    s = Stream({k: v for k, v in stm.items() if k not in drop})
    s.update(add)
    s.raw = stm.raw
    return s


def _stencil_record(doc: _Document, stm: Stream, rotate: int, media_box, strip_filters: bool, jbig2: bool = False) -> Tuple[PageImage, int]:
    """(record, flip) of an /ImageMask image: one bit a sample, Flate or CCITT (LZW / RunLength under strip_filters, JBIG2 under jbig2)"""
    for key in ("SMask", "Mask"):
        if doc.resolve(stm.get(key)) is not None:
            raise PdfRefused("/%s on a stencil" % key)
    bits = doc.resolve(stm.get("BitsPerComponent", 1))
    if bits != 1:
        raise PdfRefused("stencil with %r bits per component" % (bits,))
    filt, _ = doc.single_filter(stm)
    if filt not in ("FlateDecode", "CCITTFaxDecode") and not (strip_filters and filt in STRIP_FILTERS) and not (jbig2 and filt == JBIG2_FILTER):
        raise PdfRefused("stencil filter %s" % filt)
    flip = _mask_decode(doc, stm)
    rec = _image_record(doc, _without(stm, ("Decode", "ImageMask", "ColorSpace", "SMaskInData"), ColorSpace=Name("DeviceGray"), BitsPerComponent=1),
                        rotate, media_box, strip_filters, False, jbig2)
    return rec, flip


def _soft_mask_record(doc: _Document, stm, rotate: int, media_box, jpx: bool, jbig2: bool = False) -> Tuple[PageImage, int]:
    """(record, flip) of an /SMask image: DeviceGray, 1 or 8 bits, Flate, CCITT, grey DCT (grey JPX with jpx, JBIG2 with jbig2), no /Matte"""
    if not isinstance(stm, Stream) or doc.resolve(stm.get("Subtype")) != "Image":
        raise PdfRefused("/SMask is not an image")
    if doc.resolve(stm.get("Matte")) is not None:
        raise PdfRefused("/Matte")
    for key in ("SMask", "Mask"):
        if doc.resolve(stm.get(key)) is not None:
            raise PdfRefused("/%s on a mask" % key)
    filt, _ = doc.single_filter(stm)
    if filt not in ("FlateDecode", "CCITTFaxDecode", "DCTDecode") and not (jpx and filt == JPX_FILTER) and not (jbig2 and filt == JBIG2_FILTER):
        raise PdfRefused("/SMask filter %s" % filt)
    cs = doc.resolve(stm.get("ColorSpace"))
    if cs != "DeviceGray" and not (filt == JPX_FILTER and cs is None):
        raise PdfRefused("/SMask colour space %s" % (cs if isinstance(cs, Name) else "is not a name"))
    flip = _mask_decode(doc, stm)
    rec = _image_record(doc, _without(stm, ("Decode",)), rotate, media_box, False, jpx, jbig2)
    bits = rec.params.get("bits", 1 if filt in ("CCITTFaxDecode", JBIG2_FILTER) else 8)
    if rec.params.get("components", 1) != 1 or bits not in (1, 8):
        raise PdfRefused("/SMask with %r components of %r bits" % (rec.params.get("components", 1), bits))
    return rec, flip


def _layer(doc: _Document, img: Stream, rect, fill, rotate: int, media_box, strip_filters: bool, jpx: bool, jbig2: bool = False) -> Layer:
    if doc.resolve(img.get("ImageMask")) is True:
        rec, flip = _stencil_record(doc, img, rotate, media_box, strip_filters, jbig2)
        return Layer(kind=1, rect=rect, fill=fill, flip=flip, image=None, mask=rec)
    smask, mask = doc.resolve(img.get("SMask")), doc.resolve(img.get("Mask"))
    sid = doc.resolve(img.get("SMaskInData", 0))
    if sid != 0:
        raise PdfRefused("/SMaskInData %r" % (sid,))
    base = _image_record(doc, img, rotate, media_box, strip_filters, jpx, jbig2)
    if smask is not None and mask is not None:
        raise PdfRefused("/SMask and /Mask on one image")
    if smask is not None:
        rec, flip = _soft_mask_record(doc, smask, rotate, media_box, jpx, jbig2)
        return Layer(kind=2, rect=rect, fill=fill, flip=flip, image=base, mask=rec)
    if mask is not None:
        if isinstance(mask, list):
            raise PdfRefused("colour-key /Mask")
        if not isinstance(mask, Stream) or doc.resolve(mask.get("Subtype")) != "Image" or doc.resolve(mask.get("ImageMask")) is not True:
            raise PdfRefused("/Mask is not an /ImageMask image")
        rec, flip = _stencil_record(doc, mask, rotate, media_box, strip_filters, jbig2)
        return Layer(kind=3, rect=rect, fill=fill, flip=flip, image=base, mask=rec)
    return Layer(kind=0, rect=rect, fill=fill, flip=0, image=base, mask=None)


def _round(v: float) -> int:
    return int(math.floor(v + 0.5))


def _page_layers(doc: _Document, page: Dict[str, Any], attrs: Dict[str, Any], strip_filters: bool, jpx: bool,
                 jbig2: bool = False) -> Union[PageImage, PageLayers]:
    (X0, Y0, X1, Y1), rotate, content = _page_frame(doc, page, attrs)
    bw, bh = X1 - X0, Y1 - Y0
    placed = []
    for name, m, fill in _content_layers(doc, attrs, content):
        a, b, c, d, e, f = m
        if not (a > 0 and d > 0) or abs(b) > 1e-4 * a or abs(c) > 1e-4 * d:
            raise PdfRefused("image placement is not axis-aligned with positive scales")
        placed.append((name, a, d, e, f, fill))
    hx0, hx1 = min(q[3] for q in placed), max(q[3] + q[1] for q in placed)
    hy0, hy1 = min(q[4] for q in placed), max(q[4] + q[2] for q in placed)
    if abs(hx0 - X0) > EDGE_TOLERANCE * bw or abs(hx1 - X1) > EDGE_TOLERANCE * bw or abs(hy0 - Y0) > EDGE_TOLERANCE * bh or abs(hy1 - Y1) > EDGE_TOLERANCE * bh:
        raise PdfRefused("image does not cover the MediaBox" if len(placed) == 1 else "the images do not cover the MediaBox")
    box = (X0, Y0, X1, Y1)
    layers = [_layer(doc, _xobject_image(doc, attrs, name), None, fill, rotate, box, strip_filters, jpx, jbig2) for name, _, _, _, _, fill in placed]
    if len(layers) == 1 and layers[0].kind == 0:
        return layers[0].image   # one opaque image over the whole box: today's record
    # the canvas: the MediaBox at the finest sample grid among the layers (a stencil's own size counts, a mask's does not)
    sizes = [(l.image or l.mask).width for l in layers], [(l.image or l.mask).height for l in layers]
    sx = max(w / q[1] for w, q in zip(sizes[0], placed))
    sy = max(h / q[2] for h, q in zip(sizes[1], placed))
    W, H = _round(bw * sx), _round(bh * sy)
    if not (0 < W <= 65535 and 0 < H <= 65535):
        raise PdfRefused("canvas of %d x %d samples" % (W, H))
    if W * H > MAX_CANVAS_PIXELS:
        raise PdfRefused("canvas of %d x %d samples is above the cap of %d" % (W, H, MAX_CANVAS_PIXELS))
    kept = []
    for l, (_, a, d, e, f, _) in zip(layers, placed):
        x0, x1 = _round((e - X0) * sx), _round((e + a - X0) * sx)
        y0, y1 = _round((Y1 - f - d) * sy), _round((Y1 - f) * sy)
        if x0 >= x1 or y0 >= y1 or x0 >= W or x1 <= 0 or y0 >= H or y1 <= 0:
            continue   # empty, or wholly outside the canvas: it paints nothing
        if max(abs(x0), abs(x1), abs(y0), abs(y1)) > MAX_COORD:
            raise PdfRefused("image placed far outside the page")
        l.rect = (x0, y0, x1, y1)
        kept.append(l)
    if not kept:
        raise PdfRefused("no image on the page")
    return PageLayers(width=W, height=H, layers=kept, rotate=rotate, media_box=box)


def read_pages(data, strip_filters: bool = False, jpx: bool = False, layers: bool = False,
               jbig2: bool = False) -> List[Union[PageImage, PageLayers, PdfRefused]]:
    """One entry per page of the PDF in `data` (bytes, or anything with the buffer protocol: the records' streams are views into it):
    the page's image record, or the PdfRefused that says why the page is not a scanned page.  Raises PdfRefused for the whole file.
    strip_filters: also take /LZWDecode (/EarlyChange 1 or absent, /Predictor 1 or 2) and /RunLengthDecode images, which
    lumina_ocr_strip_image_decode decodes as one-strip pages (the provider asks for them with LUMINA_OCR_DEVICE_TIFF=1); without it
    they are refused as any other filter is.
    jpx: also take /JPXDecode images (JPEG 2000), which lumina_ocr_jp2_decode decodes (the provider asks for them with
    LUMINA_OCR_DEVICE_JP2=1); without it they are refused as any other filter is.
    layers: also take pages painted from up to MAX_LAYERS images (strips, stencils, images with /SMask or a /Mask stream) and pages
    with invisible text, as the module docstring lists them: such a page yields a PageLayers record for lumina_ocr_page_compose (the
    provider asks for them with LUMINA_OCR_PDF_LAYERS=1); without it every answer is the one given before the option existed.
    jbig2: also take /JBIG2Decode images (one bit of DeviceGray or an /ImageMask, /Decode [0 1] or [1 0], /JBIG2Globals resolved), which
    lumina_ocr_jbig2_decode decodes where they are made of generic regions: as the one image of a page and, with layers, as a stencil,
    a /Mask stream or a 1-bit /SMask (the provider asks for them with LUMINA_OCR_PDF_JBIG2=1); without it every answer and reason is the
    one given before the option existed."""
    try:
        doc = _Document(data)
        out: List[Union[PageImage, PdfRefused]] = []
        for page, attrs in doc.pages():
            try:
                out.append(_page_layers(doc, page, attrs, strip_filters, jpx, jbig2) if layers else _page_image(doc, page, attrs, strip_filters, jpx, jbig2))
            except PdfRefused as e:
                out.append(e)
        return out
    except RecursionError:
        raise PdfRefused("nesting too deep")
    except (OverflowError, MemoryError, ValueError, TypeError, AttributeError, IndexError, KeyError) as e:   # hostile values in odd places
        raise PdfRefused("malformed file (%s)" % type(e).__name__)
