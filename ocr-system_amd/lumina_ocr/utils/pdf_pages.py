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

The reader ends on any input: every loop advances through the file or a decoded stream, /Prev chains, page-tree nodes and indirect
references are followed through visited-sets, every offset and /Length is checked against the file size, and the number of objects, the
nesting depth and the number of pages are capped.
"""
from __future__ import annotations

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
    filter: str                     # "DCTDecode" | "FlateDecode" | "CCITTFaxDecode" | "LZWDecode" | "RunLengthDecode" | "JPXDecode"
    stream: memoryview              # the image's raw stream, a view into the file
    params: Dict[str, Any]          # FlateDecode, LZWDecode, RunLengthDecode: predictor, components, bits, indexed, invert, palette
    #                                 (768 bytes RGB or None); predictor is 1 | 2 for LZWDecode and 1 for RunLengthDecode
    #                                 CCITTFaxDecode: K, EncodedByteAlign, BlackIs1, invert;  DCTDecode, JPXDecode: components
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


def _page_image(doc: _Document, page: Dict[str, Any], attrs: Dict[str, Any], strip_filters: bool = False, jpx: bool = False) -> PageImage:
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
    name, m = _content_image(b"\n".join(chunks))
    a, b, c, d, e, f = m
    if not (a > 0 and d > 0) or abs(b) > 1e-4 * a or abs(c) > 1e-4 * d:
        raise PdfRefused("image placement is not axis-aligned with positive scales")
    if (abs(e - x0) > EDGE_TOLERANCE * bw or abs(e + a - x1) > EDGE_TOLERANCE * bw or abs(f - y0) > EDGE_TOLERANCE * bh
            or abs(f + d - y1) > EDGE_TOLERANCE * bh):
        raise PdfRefused("image does not cover the MediaBox")
    # the image
    res = doc.resolve(attrs.get("Resources"))
    xobjs = doc.resolve(res.get("XObject")) if isinstance(res, dict) else None
    img = doc.resolve(xobjs.get(name)) if isinstance(xobjs, dict) else None
    if not isinstance(img, Stream):
        raise PdfRefused("XObject %s not found" % name)
    if doc.resolve(img.get("Subtype")) != "Image":
        raise PdfRefused("XObject %s is not an image" % name)
    if doc.resolve(img.get("ImageMask")) is True:
        raise PdfRefused("/ImageMask")
    for key in ("SMask", "Mask"):
        if doc.resolve(img.get(key)) is not None:
            raise PdfRefused("/" + key)
    width, height = doc.resolve(img.get("Width")), doc.resolve(img.get("Height"))
    if not all(isinstance(v, int) and 0 < v <= 65535 for v in (width, height)):
        raise PdfRefused("malformed image size")
    filt, parms = doc.single_filter(img)
    if jpx and filt == JPX_FILTER:
        return _jpx_page_image(doc, img, width, height, rotate, (x0, y0, x1, y1))
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


def read_pages(data, strip_filters: bool = False, jpx: bool = False) -> List[Union[PageImage, PdfRefused]]:
    """One entry per page of the PDF in `data` (bytes, or anything with the buffer protocol: the records' streams are views into it):
    the page's image record, or the PdfRefused that says why the page is not a scanned page.  Raises PdfRefused for the whole file.
    strip_filters: also take /LZWDecode (/EarlyChange 1 or absent, /Predictor 1 or 2) and /RunLengthDecode images, which
    lumina_ocr_strip_image_decode decodes as one-strip pages (the provider asks for them with LUMINA_OCR_DEVICE_TIFF=1); without it
    they are refused as any other filter is.
    jpx: also take /JPXDecode images (JPEG 2000), which lumina_ocr_jp2_decode decodes (the provider asks for them with
    LUMINA_OCR_DEVICE_JP2=1); without it they are refused as any other filter is."""
    try:
        doc = _Document(data)
        out: List[Union[PageImage, PdfRefused]] = []
        for page, attrs in doc.pages():
            try:
                out.append(_page_image(doc, page, attrs, strip_filters, jpx))
            except PdfRefused as e:
                out.append(e)
        return out
    except RecursionError:
        raise PdfRefused("nesting too deep")
    except (OverflowError, MemoryError, ValueError, TypeError, AttributeError, IndexError, KeyError) as e:   # hostile values in odd places
        raise PdfRefused("malformed file (%s)" % type(e).__name__)
