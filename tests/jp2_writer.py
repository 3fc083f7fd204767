"""A test-side JPEG 2000 writer in plain Python / numpy, the mirror image of tests/jp2_reference.py: it builds valid files that
OpenJPEG's encoder (and so Pillow) never writes, for the decoder's acceptance tests.  Nothing here is hostile; every file is valid.

rewrite(file, ...)     marker- and box-level edits of a Pillow-written file with no re-encoding: guard bits, header order, COM / TLM /
                       COC / QCC / PLT segments, tile-parts at packet boundaries (found by running the restatement's tier 2 and recording
                       where each packet's bit reader starts), trailing empty layers, box lengths 0 and 64-bit, extra boxes, jpx brand.
MQEncoder, t1_encode   jp2_reference.MQ and tier1_block_walk with every decode(cx) turned into encode(cx, bit of the known coefficient).
TagTreeEncoder, BitWriter, packet headers: the mirror of TagTree.decode, Bits and _npasses.
synth(...)             a complete codestream (or JP2) from coefficient planes in the restatement's Mallat layout, with a per-block plan:
                       zero bit-planes, pass count, a cut of the codeword, the split of passes and bytes over layers, extra Lblock.
deep_planes(...)       coefficient planes whose detail bands are large and random and whose LL band is solved for, so that the output
                       samples at the positions LL alone moves are a chosen 8-bit target while LL itself needs 15 bit-planes."""
import numpy as np

import jp2_irreversible_reference as ir
import jp2_reference as jr
from jp2_reference import _QE, _NMPS, _NLPS, _SWITCH, _SC, CTX_RUN, CTX_UNI, zc_context

SIGNATURE = b"\x00\x00\x00\x0cjP  \r\n\x87\n"


def _u16(v):
    return int(v).to_bytes(2, "big")


def _u32(v):
    return int(v).to_bytes(4, "big")


def box(typ, body, xl=False, zero=False):
    if zero:
        return _u32(0) + typ + body
    if xl:
        return _u32(1) + typ + int(len(body) + 16).to_bytes(8, "big") + body
    return _u32(len(body) + 8) + typ + body


def segment(marker, body):
    return _u16(marker) + _u16(len(body) + 2) + body


def com(text):
    return segment(0xFF64, _u16(1) + text.encode("latin-1"))


# ---------------------------------------------------------------------------------------------------------------- reading a file apart
def split_boxes(data):
    """-> [(type, body)] of the top-level boxes after the signature, or None for a raw codestream"""
    if data[:4] == b"\xff\x4f\xff\x51":
        return None
    assert data[:12] == SIGNATURE
    out, p = [], 12
    while p < len(data):
        ln, typ = jr._be(data, p, 4), data[p + 4:p + 8]
        assert ln >= 8, "the base file uses plain box lengths"
        out.append((typ, data[p + 8:p + ln]))
        p += ln
    assert p == len(data)
    return out


def split_codestream(cs):
    """-> (SIZ body, [(marker, body)] of the rest of the main header, first byte of the packet data); the base has one tile-part"""
    assert cs[:4] == b"\xff\x4f\xff\x51" and cs[-2:] == b"\xff\xd9"
    p, segs = 2, []
    while jr._be(cs, p, 2) != 0xFF90:
        m, L = jr._be(cs, p, 2), jr._be(cs, p + 2, 2)
        segs.append((m, cs[p + 4:p + 2 + L]))
        p += 2 + L
    assert jr._be(cs, p + 6, 4) == len(cs) - 2 - p and cs[p + 10] == 0, "the base file has one tile-part"
    q = p + 12
    while jr._be(cs, q, 2) != 0xFF93:
        q += 2 + jr._be(cs, q + 2, 2)
    assert segs[0][0] == 0xFF51
    return segs[0][1], segs[1:], q + 2


def packets_of(cs):
    """-> (Params, [((layer, resolution, component), bytes)]) of a one-tile-part codestream, in file order"""
    info = [0] * 8
    P = ir.parse_headers(cs, 0, len(cs), None, info)
    assert len(P.parts) == 1
    comps = jr.geometry(P)
    starts = []

    saved = jr.Bits

    class Recording(saved):
        def __init__(self, d, p, end):
            starts.append(p)
            saved.__init__(self, d, p, end)

    jr.Bits = Recording
    try:
        jr.tier2(cs, P, comps)
    finally:
        jr.Bits = saved
    order = jr.packet_order(P)
    assert len(starts) == len(order)
    ends = starts[1:] + [P.parts[0][1]]
    return P, [(key, cs[a:b]) for key, a, b in zip(order, starts, ends)]


def _varint(n):
    out = [n & 0x7F]
    n >>= 7
    while n:
        out.append(0x80 | (n & 0x7F))
        n >>= 7
    return bytes(reversed(out))


def tile_parts(packets, k, psot0_last=False, tnsot=None, part_com=False, plt=False):
    """the packets (bytes) cut into k tile-parts of near-equal packet counts -> (bytes of all tile-parts, [Psot as the lengths are])"""
    n = len(packets)
    assert 1 <= k <= n
    cuts = [(i * n) // k for i in range(k + 1)]
    out, lengths = b"", []
    for i in range(k):
        mine = packets[cuts[i]:cuts[i + 1]]
        hdr = b""
        if part_com:
            hdr += com("tile-part %d" % i)
        if plt:
            hdr += segment(0xFF58, bytes([0]) + b"".join(_varint(len(pk)) for pk in mine))
            if part_com:
                hdr += com("after PLT")
        body = hdr + b"\xff\x93" + b"".join(mine)
        psot = 12 + len(body)
        lengths.append(psot)
        last = i == k - 1
        out += b"\xff\x90" + _u16(10) + _u16(0) + _u32(0 if last and psot0_last else psot) + bytes([i, k if tnsot is None else tnsot]) + body
    return out, lengths


# ---------------------------------------------------------------------------------------------------------------- rewrite
def rewrite(data, guard=None, qcd_first=False, coms=False, tlm=False, coc_qcc=False, parts=1, psot0_last=False, tnsot=None, part_com=False,
            plt=False, extra_layers=0, xlbox=False, len0=False, extra_boxes=False, res=False, jpx=False):
    """`data` (a Pillow-written JP2 or raw codestream) with the asked edits; its packets are kept byte for byte.
    guard: the number of guard bits, the exponents shifted so that every Mb stays.   qcd_first: QCD before COD.   coms: COM segments
    after SIZ, between the others and before the first SOT.   tlm: a TLM (Stlm 0x40: no tile index, 32-bit lengths).   coc_qcc: a COC
    and a QCC per component, equal to COD and QCD.   parts / psot0_last / tnsot / part_com / plt: see tile_parts.   extra_layers:
    that many empty layers on top, each packet the byte 0x00 at its place in the progression.   xlbox / len0: the jp2c box with the
    64-bit length / with length 0.   extra_boxes: rreq, xml and uuid boxes before and after jp2h.   res: a res box inside jp2h.
    jpx: the jpx brand with jp2 in the compatibility list."""
    boxes = split_boxes(data)
    cs = data if boxes is None else dict(boxes)[b"jp2c"]
    siz, segs, _ = split_codestream(cs)
    P, packets = packets_of(cs)
    segs = [(m, b) for m, b in segs if m in (0xFF52, 0xFF5C)]      # COD and QCD; whatever else the base had is written afresh
    cod, qcd = dict(segs)[0xFF52], dict(segs)[0xFF5C]
    if guard is not None:
        old = qcd[0] >> 5
        style = qcd[0] & 31
        new = bytes([(guard << 5) | style])
        if style == 0:
            for b in qcd[1:]:
                e = (b >> 3) + old - guard
                assert 0 <= e <= 31
                new += bytes([e << 3])
        else:
            assert style == 2
            for i in range(1, len(qcd), 2):
                v = jr._be(qcd, i, 2)
                e = (v >> 11) + old - guard
                assert 0 <= e <= 31
                new += _u16((e << 11) | (v & 0x7FF))
        qcd = new
    if extra_layers:
        layers = P.layers + extra_layers
        cod = cod[:2] + _u16(layers) + cod[4:]
        have = dict(packets)
        Q = jr.Params()
        Q.layers, Q.levels, Q.C, Q.order = layers, P.levels, P.C, P.order
        packets = [(key, have.get(key, b"\x00")) for key in jr.packet_order(Q)]
    body, lengths = tile_parts([pk for _, pk in packets], parts, psot0_last, tnsot, part_com, plt)
    main = [segment(0xFF5C, qcd), segment(0xFF52, cod)] if qcd_first else [segment(0xFF52, cod), segment(0xFF5C, qcd)]
    if coc_qcc:
        for c in range(P.C):
            main.append(segment(0xFF53, bytes([c, cod[0] & 1]) + cod[5:]))
            main.append(segment(0xFF5D, bytes([c]) + qcd))
    if tlm:
        main.append(segment(0xFF55, bytes([0, 0x40]) + b"".join(_u32(n) for n in lengths)))
    if coms:
        with_coms = [com("after SIZ")]
        for i, s in enumerate(main):
            with_coms += [s, com("after segment %d, a longer comment to move every later offset" % i)]
        main = with_coms
    cs = b"\xff\x4f" + segment(0xFF51, siz) + b"".join(main) + body + b"\xff\xd9"
    if boxes is None:
        assert not (xlbox or len0 or extra_boxes or res or jpx)
        return cs
    out = SIGNATURE
    extras = [box(b"xml ", b"<?xml version=\"1.0\"?><note>scanned</note>"), box(b"uuid", bytes(range(16)) + b"vendor data"),
              box(b"xml ", b"<a/>")]
    for typ, b in boxes:
        if typ == b"ftyp":
            if jpx:
                b = b"jpx " + _u32(0) + b"jpx " + b"jp2 "
            out += box(typ, b)
            if extra_boxes:   # the reader requirements box directly after ftyp, as JPX asks
                out += box(b"rreq", bytes([1, 0x80, 0x80]) + _u16(1) + _u16(5) + bytes([0x80]) + _u16(0)) + extras[0] + extras[1]
        elif typ == b"jp2h":
            if res:   # capture resolution 300 / 1 * 10^0 both ways, after ihdr and colr
                b += box(b"res ", box(b"resc", _u16(300) + _u16(1) + _u16(300) + _u16(1) + bytes([0, 0])))
            out += box(typ, b)
            if extra_boxes:
                out += extras[2] + extras[1]
        elif typ == b"jp2c":
            out += box(typ, cs, xl=xlbox, zero=len0)
        else:
            out += box(typ, b)
    return out


# ---------------------------------------------------------------------------------------------------------------- MQ encoder, tier 1
class MQEncoder:
    """the arithmetic encoder jp2_reference.MQ decodes; finish() ends the codeword (and drops a trailing 0xFF)"""

    def __init__(self):
        self.I = [0] * 19
        self.mps = [0] * 19
        self.I[0], self.I[CTX_RUN], self.I[CTX_UNI] = 4, 3, 46
        self.a, self.c, self.ct = 0x8000, 0, 12
        self.out = bytearray([0])     # out[0] stands for the byte before the codeword; out[-1] is the byte being formed

    def _byteout(self):
        if self.out[-1] == 0xFF:
            self.out.append((self.c >> 20) & 0xFF)
            self.c &= 0xFFFFF
            self.ct = 7
        elif self.c & 0x8000000 == 0:
            self.out.append((self.c >> 19) & 0xFF)
            self.c &= 0x7FFFF
            self.ct = 8
        else:
            assert len(self.out) > 1
            self.out[-1] += 1
            if self.out[-1] == 0xFF:
                self.c &= 0x7FFFFFF
                self.out.append((self.c >> 20) & 0xFF)
                self.c &= 0xFFFFF
                self.ct = 7
            else:
                self.out.append((self.c >> 19) & 0xFF)
                self.c &= 0x7FFFF
                self.ct = 8

    def _renorm(self):
        while True:
            self.a <<= 1
            self.c <<= 1
            self.ct -= 1
            if self.ct == 0:
                self._byteout()
            if self.a & 0x8000:
                break

    def encode(self, cx, bit):
        i = self.I[cx]
        qe = _QE[i]
        self.a -= qe
        if bit == self.mps[cx]:
            if self.a & 0x8000:
                self.c += qe
                return
            if self.a < qe:
                self.a = qe
            else:
                self.c += qe
            self.I[cx] = _NMPS[i]
        else:
            if self.a < qe:
                self.c += qe
            else:
                self.a = qe
            if _SWITCH[i]:
                self.mps[cx] = 1 - self.mps[cx]
            self.I[cx] = _NLPS[i]
        self._renorm()

    def finish(self):
        t = self.c + self.a
        self.c |= 0xFFFF
        if self.c >= t:
            self.c -= 0x8000
        self.c <<= self.ct
        self._byteout()
        self.c <<= self.ct
        self._byteout()
        data = bytes(self.out[1:])
        return data[:-1] if data.endswith(b"\xff") else data


def t1_encode(coef, orient, nbps, npasses):
    """the codeword of one code-block: int [h, w] coefficients below 2^nbps in magnitude, `npasses` passes from bit-plane nbps - 1
    down (the first a clean-up pass) -- jp2_reference.tier1_block_walk with the decisions taken from the coefficients"""
    h, w = coef.shape
    S = w + 2
    sig = [0] * ((h + 2) * S)
    vis = [0] * ((h + 2) * S)
    ref = [0] * ((h + 2) * S)
    mag = [0] * ((h + 2) * S)
    neg = [0] * ((h + 2) * S)
    for y in range(h):
        for x in range(w):
            v = int(coef[y, x])
            assert abs(v) < (1 << nbps)
            mag[(y + 1) * S + x + 1], neg[(y + 1) * S + x + 1] = abs(v), int(v < 0)
    mq = MQEncoder()
    put = mq.encode

    def nbr(i):
        hh = (sig[i - 1] != 0) + (sig[i + 1] != 0)
        vv = (sig[i - S] != 0) + (sig[i + S] != 0)
        dd = (sig[i - S - 1] != 0) + (sig[i - S + 1] != 0) + (sig[i + S - 1] != 0) + (sig[i + S + 1] != 0)
        return hh, vv, dd

    def sign(i):
        hc = max(-1, min(1, sig[i - 1] + sig[i + 1]))
        vc = max(-1, min(1, sig[i - S] + sig[i + S]))
        cx, x = _SC[(hc, vc)]
        put(cx, neg[i] ^ x)
        sig[i] = -1 if neg[i] else 1

    bp = nbps - 1
    kind = 2
    for _ in range(npasses):
        for y0 in range(0, h, 4):
            rows = min(4, h - y0)
            for x in range(w):
                base = (y0 + 1) * S + x + 1
                if kind == 0:
                    for k in range(rows):
                        i = base + k * S
                        if sig[i] == 0:
                            hh, vv, dd = nbr(i)
                            if hh or vv or dd:
                                bit = (mag[i] >> bp) & 1
                                put(zc_context(orient, hh, vv, dd), bit)
                                if bit:
                                    sign(i)
                                vis[i] = 1
                elif kind == 1:
                    for k in range(rows):
                        i = base + k * S
                        if sig[i] != 0 and not vis[i]:
                            if ref[i]:
                                cx = 16
                            else:
                                hh, vv, dd = nbr(i)
                                cx = 15 if hh or vv or dd else 14
                            put(cx, (mag[i] >> bp) & 1)
                            ref[i] = 1
                else:
                    k = 0
                    if rows == 4 and all(sig[base + j * S] == 0 and not vis[base + j * S] and nbr(base + j * S) == (0, 0, 0) for j in range(4)):
                        first = [j for j in range(4) if (mag[base + j * S] >> bp) & 1]
                        if not first:
                            put(CTX_RUN, 0)
                            continue
                        k = first[0]
                        put(CTX_RUN, 1)
                        put(CTX_UNI, k >> 1)
                        put(CTX_UNI, k & 1)
                        sign(base + k * S)
                        k += 1
                    for k in range(k, rows):
                        i = base + k * S
                        if sig[i] == 0 and not vis[i]:
                            bit = (mag[i] >> bp) & 1
                            put(zc_context(orient, *nbr(i)), bit)
                            if bit:
                                sign(i)
        if kind == 2:
            vis = [0] * len(vis)
            bp -= 1
        kind = (kind + 1) % 3
    return mq.finish()


# ---------------------------------------------------------------------------------------------------------------- tier 2
class BitWriter:
    """the packet-header bit writer jp2_reference.Bits reads: after a 0xFF byte the next byte carries 7 bits"""

    def __init__(self):
        self.out, self.buf, self.ct = bytearray(), 0, 8

    def bit(self, b):
        if self.ct == 0:
            self.out.append(self.buf)
            self.ct = 7 if self.buf == 0xFF else 8
            self.buf = 0
        self.ct -= 1
        self.buf |= (b & 1) << self.ct

    def bits(self, v, n):
        assert 0 <= v < (1 << n) or n == 0 and v == 0
        for k in range(n - 1, -1, -1):
            self.bit((v >> k) & 1)

    def align(self):
        self.out.append(self.buf)
        if self.buf == 0xFF:
            self.out.append(0)
        return bytes(self.out)


class TagTreeEncoder:
    """values: {(x, y): value} of the leaves; encode() mirrors TagTree.decode call for call"""

    def __init__(self, nx, ny, values):
        self.levels = []
        off = 0
        dims = []
        while True:
            self.levels.append((off, nx, ny))
            dims.append((nx, ny))
            off += nx * ny
            if nx * ny <= 1:
                break
            nx, ny = (nx + 1) // 2, (ny + 1) // 2
        self.value = [1 << 30] * off
        self.low = [0] * off
        self.known = [False] * off
        o0, nx0, ny0 = self.levels[0]
        for (x, y), v in values.items():
            self.value[o0 + y * nx0 + x] = v
        for lv in range(1, len(self.levels)):
            (op, px, py), (o, nx, ny) = self.levels[lv - 1], self.levels[lv]
            for y in range(py):
                for x in range(px):
                    n = o + (y >> 1) * nx + (x >> 1)
                    self.value[n] = min(self.value[n], self.value[op + y * px + x])

    def encode(self, bw, x, y, threshold):
        path = []
        for off, nx, ny in self.levels:
            path.append(off + y * nx + x)
            x, y = x >> 1, y >> 1
        low = 0
        for node in reversed(path):
            if low > self.low[node]:
                self.low[node] = low
            else:
                low = self.low[node]
            while low < threshold and not self.known[node]:
                if low >= self.value[node]:
                    bw.bit(1)
                    self.known[node] = True
                else:
                    bw.bit(0)
                    low += 1
            self.low[node] = low
        return self.known[path[0]] and self.value[path[0]] < threshold


def put_npasses(bw, n):
    assert 1 <= n <= 164
    if n == 1:
        bw.bits(0, 1)
    elif n == 2:
        bw.bits(2, 2)
    elif n <= 5:
        bw.bits(3, 2)
        bw.bits(n - 3, 2)
    elif n <= 36:
        bw.bits(15, 4)
        bw.bits(n - 6, 5)
    else:
        bw.bits(511, 9)
        bw.bits(n - 37, 7)


def write_packet(bands, layer, explicit_empty=False):
    """one packet of the bands of a resolution of a component; every block carries .contrib = {layer: (passes, bytes)}, .zbp, and the
    writer's state (.w_included, .w_lblock); the band carries .w_incl / .w_zbp tag-tree encoders"""
    blocks = [(B, K) for B in bands for K in B.blocks]
    if not any(layer in K.contrib for _, K in blocks) and not explicit_empty:
        return b"\x00"
    bw = BitWriter()
    bw.bit(1)
    body = b""
    for B, K in blocks:
        here = K.contrib.get(layer)
        if not K.w_included:
            inc = B.w_incl.encode(bw, K.bx, K.by, layer + 1)
            assert inc == (here is not None)
        else:
            bw.bit(int(here is not None))
        if here is None:
            continue
        if not K.w_included:
            i = 1
            while not B.w_zbp.encode(bw, K.bx, K.by, i):
                i += 1
            assert i - 1 == K.zbp
            K.w_included = True
        n, chunk = here
        put_npasses(bw, n)
        width = K.w_lblock + n.bit_length() - 1
        need = max(0, len(chunk).bit_length() - width)
        inc = need + K.extra.get(layer, 0)
        K.lblock_needed += need
        for _ in range(inc):
            bw.bit(1)
        bw.bit(0)
        K.w_lblock += inc
        bw.bits(len(chunk), K.w_lblock + n.bit_length() - 1)
        body += chunk
    return bw.align() + body


# ---------------------------------------------------------------------------------------------------------------- synth
def synth(planes, levels, mb, cb=(64, 64), order=0, layers=1, mct=0, irreversible=False, guard=2, plan=None, explicit_empty=False, jp2=True):
    """-> (file, report).  planes: int [C, H, W] coefficients in the restatement's Mallat layout (for 9/7: the quantiser indices);
    mb: Mb of every sub-band in QCD order, the same for all components; cb: (code-block width, height).
    plan(K, need) -> dict or None for the block K (a jp2_reference Block) whose coefficients need `need` bit-planes:
      never: True leaves the block out of every layer;  zbp: the zero bit-plane count (default Mb - need);  npasses: the passes coded
      (default all, 3 * planes - 2);  cut: the codeword cut to that many bytes;  split: [(layer, passes, weight)], the passes of each
      contribution and the share of the bytes it gets (weight 0: no byte);  extra: {layer: Lblock increments beyond what is needed}.
    report: one dict per block (c, r, orient, bx, by, mb, zbp, nbps, passes, first, lblock, lblock_needed, sizes)."""
    planes = np.asarray(planes)
    C, H, W = planes.shape
    P = jr.Params()
    P.W, P.H, P.C, P.levels, P.layers, P.order, P.mct = W, H, C, levels, layers, order, mct
    P.cbw, P.cbh = cb
    P.mb = list(mb)
    assert len(P.mb) == 3 * levels + 1
    comps = jr.geometry(P)
    report = []
    for c in range(C):
        for bands in comps[c]:
            for B in bands:
                first, zbps = {}, {}
                for K in B.blocks:
                    blk = planes[c, K.y:K.y + K.h, K.x:K.x + K.w]
                    need = int(np.abs(blk).max()).bit_length()
                    spec = (plan(K, need) if plan else None) or {}
                    K.contrib, K.extra, K.w_included, K.w_lblock, K.lblock_needed = {}, spec.get("extra", {}), False, 3, 0
                    if spec.get("never") or (need == 0 and "zbp" not in spec):
                        K.zbp = 0
                        continue
                    K.zbp = spec.get("zbp", K.mb - need)
                    nbps = K.mb - K.zbp
                    assert nbps >= max(need, 1), (K.mb, K.zbp, need)
                    n = spec.get("npasses", 3 * nbps - 2)
                    assert 1 <= n <= 3 * nbps - 2
                    data = t1_encode(blk, K.orient, nbps, n)
                    if "cut" in spec:
                        data = data[:spec["cut"]]
                    split = spec.get("split", [(0, n, 1)])
                    assert sum(s[1] for s in split) == n and all(s[1] >= 1 for s in split)
                    total, acc, pos = sum(s[2] for s in split), 0, 0
                    for layer, passes, weight in split:
                        acc += weight
                        end = len(data) * acc // total if total else 0
                        K.contrib[layer] = (passes, data[pos:end])
                        pos = end
                    assert pos == len(data) or not total
                    first[(K.bx, K.by)] = min(K.contrib)
                    zbps[(K.bx, K.by)] = K.zbp
                    report.append(dict(c=c, r=K.r, orient=K.orient, bx=K.bx, by=K.by, mb=K.mb, zbp=K.zbp, nbps=nbps, passes=n,
                                       first=min(K.contrib), block=K, sizes=[(l, p, len(b)) for l, (p, b) in sorted(K.contrib.items())]))
                for K in B.blocks:
                    if not K.contrib:
                        report.append(dict(c=c, r=K.r, orient=K.orient, bx=K.bx, by=K.by, mb=K.mb, zbp=0, nbps=0, passes=0, first=None,
                                           block=K, sizes=[]))
                B.w_incl, B.w_zbp = TagTreeEncoder(B.nx, B.ny, first), TagTreeEncoder(B.nx, B.ny, zbps)
    data = b"".join(write_packet(comps[c][r], layer, explicit_empty) for layer, r, c in jr.packet_order(P))
    for row in report:
        K = row.pop("block")
        row["lblock"], row["lblock_needed"] = K.w_lblock, 3 + K.lblock_needed
    siz = _u16(0) + _u32(W) + _u32(H) + _u32(0) * 2 + _u32(W) + _u32(H) + _u32(0) * 2 + _u16(C) + bytes([7, 1, 1]) * C
    cod = bytes([0, order]) + _u16(layers) + bytes([mct, levels, cb[0].bit_length() - 3, cb[1].bit_length() - 3, 0, 0 if irreversible else 1])
    if irreversible:   # expounded, mantissa 0
        qcd = bytes([(guard << 5) | 2]) + b"".join(_u16((m - guard + 1) << 11) for m in P.mb)
    else:
        qcd = bytes([guard << 5]) + bytes((m - guard + 1) << 3 for m in P.mb)
    assert all(0 <= m - guard + 1 <= 31 for m in P.mb)
    body = b"\xff\x93" + data
    cs = (b"\xff\x4f" + segment(0xFF51, siz) + segment(0xFF52, cod) + segment(0xFF5C, qcd) + b"\xff\x90" + _u16(10) + _u16(0) + _u32(12 + len(body)) +
          bytes([0, 1]) + body + b"\xff\xd9")
    if not jp2:
        return cs, report
    ihdr = _u32(H) + _u32(W) + _u16(C) + bytes([7, 7, 0, 0])
    colr = bytes([1, 0, 0]) + _u32(16 if C == 3 else 17)
    return SIGNATURE + box(b"ftyp", b"jp2 " + _u32(0) + b"jp2 ") + box(b"jp2h", box(b"ihdr", ihdr) + box(b"colr", colr)) + box(b"jp2c", cs), report


# ---------------------------------------------------------------------------------------------------------------- deep blocks
def band_slices(W, H, levels):
    """-> [(r, orient, row slice, column slice)] of the sub-bands of a [H, W] Mallat plane, in QCD order"""
    out = []
    for r in range(levels + 1):
        rw, rh = jr._cdiv(W, 1 << (levels - r)), jr._cdiv(H, 1 << (levels - r))
        if r == 0:
            out.append((0, 0, slice(0, rh), slice(0, rw)))
        else:
            lw, lh = (rw + 1) // 2, (rh + 1) // 2
            out += [(r, 1, slice(0, lh), slice(lw, rw)), (r, 2, slice(lh, rh), slice(0, lw)), (r, 3, slice(lh, rh), slice(lw, rw))]
    return out


def solve_ll(plane, levels, target):
    """plane: int [H, W] Mallat plane whose LL band is ignored; target: uint8 [h_ll, w_ll].  Sets LL so that the decoded sample at
    (y << levels, x << levels) is target[y, x]: the inverse 5/3 transform is exactly additive in LL at those positions (an even
    sample is its low-pass input minus a rounded sum of high-pass values only, at every level and in both directions)."""
    H, W = plane.shape
    _, _, ys, xs = band_slices(W, H, levels)[0]
    plane[ys, xs] = 0
    rest = jr.inverse_dwt(plane.astype(np.int32).copy(), W, H, levels)
    plane[ys, xs] = target.astype(np.int64) - 128 - rest[::1 << levels, ::1 << levels]
    return plane
