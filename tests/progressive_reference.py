"""Progressive JPEG (SOF2) restated in pure Python / numpy: the definition the device decoder (csrc/jpegdec.hip, jp_* kernels) restates.

Three parts:
  * parse / decode: a progressive file -> its quantised coefficients (all scans applied), with the device's acceptance rules
    (Refused.code is the status the device gives: -1 corrupt / illegal progression, -2 outside the subset);
  * write_baseline: coefficients -> a sequential file with one interleaved scan (a lossless transcode);
  * write_progressive: coefficients -> a progressive file under a given scan script, with Huffman tables built here (no code is all
    ones: libjpeg's table check), for the scan scripts Pillow cannot write.
There is no IDCT here: the module is validated against Pillow alone — Pillow's decode of the baseline transcode of a file must equal
Pillow's decode of the file (tests/test_progressive_reference.py)."""
import numpy as np

ZZ = [0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28, 35, 42, 49, 56,
      57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63]
MAX_SCANS = 32


class Refused(Exception):
    def __init__(self, code, why):
        super().__init__("%d: %s" % (code, why))
        self.code = code


def _need(cond, code, why):
    if not cond:
        raise Refused(code, why)


# ------------------------------------------------------------------------------------------------ Huffman tables
def _counts_ok(bits, vals, dc):
    code = 0
    for l in range(1, 17):
        code += bits[l]
        if code >= (1 << l):
            return False
        code <<= 1
    return not (dc and any(v > 15 for v in vals))


def _lut(bits, vals):
    """16-bit look-up: entry = (length << 8) | symbol, 0 where no code matches."""
    lut = np.zeros(65536, np.int32)
    code, k = 0, 0
    for l in range(1, 17):
        for _ in range(bits[l]):
            lo = code << (16 - l)
            lut[lo:lo + (1 << (16 - l))] = (l << 8) | vals[k]
            code += 1
            k += 1
        code <<= 1
    return lut.tolist()


# ------------------------------------------------------------------------------------------------ parser
class Frame:
    pass


def parse(data: bytes) -> Frame:
    """Markers of a progressive file -> Frame (geometry, quantisation tables, APPn segments, scans with their table snapshots and
    entropy-coded bytes).  Raises Refused with the device's status."""
    f, n = data, len(data)
    _need(n >= 4 and f[0] == 0xFF and f[1] == 0xD8, -1, "no SOI")
    fr = Frame()
    fr.scans, fr.app, fr.qt, fr.progressive = [], [], {}, False
    huff = {}
    p, sof, adobe, restart = 2, False, -1, 0
    cbits = None
    while True:
        _need(p + 2 <= n and f[p] == 0xFF, -1, "marker expected")
        while p < n and f[p] == 0xFF:
            p += 1
        _need(p < n, -1, "truncated")
        m = f[p]
        p += 1
        if m == 0xD9:
            break
        if m == 0xD8 or 0xD0 <= m <= 0xD7 or m == 0x01:
            continue
        _need(p + 2 <= n, -1, "truncated")
        ln = (f[p] << 8) | f[p + 1]
        _need(ln >= 2 and p + ln <= n, -1, "segment length")
        s = f[p + 2:p + ln]
        sl = ln - 2
        if m == 0xDB:
            _need(not fr.scans, -2, "DQT after the first scan")
            i = 0
            while i < sl:
                pq, t = s[i] >> 4, s[i] & 15
                i += 1
                _need(t <= 3 and pq <= 1 and i + (128 if pq else 64) <= sl, -1, "DQT")
                fr.qt[t] = [(s[i + 2 * k] << 8) | s[i + 2 * k + 1] for k in range(64)] if pq else list(s[i:i + 64])
                i += 128 if pq else 64
        elif m == 0xC4:
            i = 0
            while i < sl:
                tc, t = s[i] >> 4, s[i] & 15
                i += 1
                _need(tc <= 1 and t <= 3 and i + 16 <= sl, -1, "DHT")
                bits = [0] + list(s[i:i + 16])
                i += 16
                cnt = sum(bits)
                _need(cnt <= 256 and i + cnt <= sl, -1, "DHT")
                vals = list(s[i:i + cnt])
                i += cnt
                _need(_counts_ok(bits, vals, tc == 0), -1, "DHT code space")
                huff[(tc, t)] = (bits, vals)
        elif m in (0xC0, 0xC1):
            _need(not sof, -1, "second SOF")
            raise Refused(1, "sequential")
        elif m == 0xC2:
            _need(sl >= 6 and not sof, -1, "SOF")
            _need(s[0] == 8, -2, "precision")
            fr.height, fr.width, fr.ncomp = (s[1] << 8) | s[2], (s[3] << 8) | s[4], s[5]
            _need(fr.height and fr.width and fr.ncomp in (1, 3), -2, "frame")
            _need(sl == 6 + 3 * fr.ncomp, -1, "SOF length")
            samp, fr.tq = [], []
            for c in range(fr.ncomp):
                _need(s[6 + 3 * c] == c + 1, -2, "component id")
                samp.append((s[7 + 3 * c] >> 4, s[7 + 3 * c] & 15))
                fr.tq.append(s[8 + 3 * c])
                _need(fr.tq[c] <= 3, -1, "Tq")
            if fr.ncomp == 1:
                samp = [(1, 1)]
            else:
                _need(samp[1] == (1, 1) and samp[2] == (1, 1) and samp[0] in ((1, 1), (2, 1), (2, 2)), -2, "sampling")
            fr.hs, fr.vs = samp[0]
            fr.mcux, fr.mcuy = -(-fr.width // (8 * fr.hs)), -(-fr.height // (8 * fr.vs))
            cbits = [[-1] * 64 for _ in range(fr.ncomp)]
            sof = fr.progressive = True
        elif 0xC3 <= m <= 0xCF and m != 0xC8:
            raise Refused(-2, "SOF%d" % (m - 0xC0))
        elif m == 0xDD:
            _need(sl == 2, -1, "DRI")
            restart = (s[0] << 8) | s[1]
        elif m == 0xDC:
            raise Refused(-2, "DNL")
        elif m == 0xDA:
            _need(sof and sl >= 1, -1, "SOS before SOF")
            ncs = s[0]
            _need(1 <= ncs <= fr.ncomp and sl == 1 + 2 * ncs + 3, -1, "SOS")
            _need(len(fr.scans) < MAX_SCANS, -2, "more than %d scans" % MAX_SCANS)
            if not fr.scans:
                _need(all(fr.tq[c] in fr.qt for c in range(fr.ncomp)), -2, "quantisation table after the first scan")
            ss, se, ah, al = s[1 + 2 * ncs], s[2 + 2 * ncs], s[3 + 2 * ncs] >> 4, s[3 + 2 * ncs] & 15
            _need(ss <= se <= 63 and ah <= 13 and al <= 13, -1, "spectral selection")
            _need(se == 0 if ss == 0 else ncs == 1, -1, "DC with AC, or AC of several components")
            _need(ah == 0 or al == ah - 1, -1, "Al != Ah - 1")
            sc = dict(comps=[], ss=ss, se=se, ah=ah, al=al, restart=restart, dc=[], ac=None)
            for i in range(ncs):
                c, td, ta = s[1 + 2 * i] - 1, s[2 + 2 * i] >> 4, s[2 + 2 * i] & 15
                _need(0 <= c < fr.ncomp and td <= 3 and ta <= 3, -1, "scan component")
                if i:
                    _need(c != sc["comps"][-1], -1, "component twice")
                    _need(c > sc["comps"][-1], -2, "component order")
                sc["comps"].append(c)
                _need(ss == 0 or cbits[c][0] >= 0, -1, "AC before DC")
                for k in range(ss, se + 1):
                    _need(not (ah == 0 and cbits[c][k] == 0), -2, "a complete coefficient sent again as a first scan")
                    _need(ah == (0 if cbits[c][k] < 0 else cbits[c][k]), -1, "Ah chain")
                    cbits[c][k] = al
                if ss == 0 and ah == 0:
                    _need((0, td) in huff, -1, "DC table")
                    sc["dc"].append(huff[(0, td)])
                if ss:
                    _need((1, ta) in huff, -1, "AC table")
                    sc["ac"] = huff[(1, ta)]
            q = p + ln
            sc["off"] = q
            while True:
                q = f.find(b"\xff", q)
                _need(q >= 0 and q + 1 < n and f[q + 1] != 0xFF, -1, "entropy data runs to the end of the file")
                if f[q + 1] != 0 and (f[q + 1] & 0xF8) != 0xD0:
                    break
                q += 2
            sc["data"] = f[sc["off"]:q]
            fr.scans.append(sc)
            p = q
            continue
        else:
            if m == 0xEE and sl >= 12 and s[:5] == b"Adobe":
                adobe = s[11]
            if 0xE0 <= m <= 0xEF:
                fr.app.append(bytes(f[p - 2:p + ln]))
        p += ln
    _need(sof and fr.scans, -1, "no scan")
    _need(not (fr.ncomp == 3 and adobe >= 0 and adobe != 1), -2, "Adobe transform")
    _need(all(v == 0 for c in cbits for v in c), -2, "scans stop short of full precision")
    return fr


def comp_geometry(fr, c):
    """-> (hs, vs, blocks per row / rows of the component's own raster, of the MCU-padded grid)"""
    hsc, vsc = (fr.hs, fr.vs) if c == 0 else (1, 1)
    wc = fr.width if c == 0 else -(-fr.width // fr.hs)
    hc = fr.height if c == 0 else -(-fr.height // fr.vs)
    return hsc, vsc, -(-wc // 8), -(-hc // 8), fr.mcux * hsc, fr.mcuy * vsc


def scan_blocks(fr, comps):
    """Block addresses (component, block row, block column) in the scan's order, and the blocks per MCU: an interleaved scan walks the
    MCU-padded grid, a single-component scan that component's own raster."""
    if len(comps) == 1:
        c = comps[0]
        _, _, bw, bh, _, _ = comp_geometry(fr, c)
        return [(c, by, bx) for by in range(bh) for bx in range(bw)], 1
    out = []
    for my in range(fr.mcuy):
        for mx in range(fr.mcux):
            for c in comps:
                hsc, vsc = comp_geometry(fr, c)[:2]
                for j in range(hsc * vsc):
                    out.append((c, my * vsc + j // hsc, mx * hsc + j % hsc))
    return out, sum(comp_geometry(fr, c)[0] * comp_geometry(fr, c)[1] for c in comps)


def _segments(data, nseg):
    """Un-stuff one scan: -> the clean bytes of its restart segments (RSTn in sequence, exactly one between two segments)."""
    segs, cur, i, n, r = [], bytearray(), 0, len(data), 0
    while True:
        j = data.find(b"\xff", i)
        if j < 0:
            cur += data[i:]
            break
        cur += data[i:j]
        _need(j + 1 < n, -1, "0xFF at the end of a scan")
        if data[j + 1] == 0:
            cur.append(0xFF)
        else:
            _need(data[j + 1] == 0xD0 + (r & 7), -1, "RSTn out of sequence")
            r += 1
            segs.append(bytes(cur))
            cur = bytearray()
        i = j + 2
    segs.append(bytes(cur))
    _need(len(segs) == nseg, -1, "%d restart segments, %d expected" % (len(segs), nseg))
    return segs


def decode(data: bytes, stats=None):
    """A progressive file -> (Frame, [per component int32 [block rows, block columns, 64] in zig-zag order, MCU-padded grid])."""
    fr = parse(data)
    coefs = [np.zeros((comp_geometry(fr, c)[5], comp_geometry(fr, c)[4], 64), np.int32) for c in range(fr.ncomp)]
    if stats is not None:
        stats["max_eob_category"] = -1
        stats["scan_bytes"] = []
    for sc in fr.scans:
        blocks, bps = scan_blocks(fr, sc["comps"])
        nmcu = len(blocks) // bps
        per = sc["restart"] if sc["restart"] else nmcu
        segs = _segments(sc["data"], -(-nmcu // per))
        if stats is not None:
            stats["scan_bytes"].append(sum(len(s) for s in segs))
        ss, se, ah, al = sc["ss"], sc["se"], sc["ah"], sc["al"]
        luts = [_lut(*t) for t in sc["dc"]] if ss == 0 and ah == 0 else ([_lut(*sc["ac"])] if ss else [])
        ci_of = []
        if ss == 0:
            for k, c in enumerate(sc["comps"]):
                ci_of += [k] * (comp_geometry(fr, c)[0] * comp_geometry(fr, c)[1] if len(sc["comps"]) > 1 else 1)
        for si, seg in enumerate(segs):
            buf, end, pos = seg + bytes(8), len(seg) * 8, 0
            _need(end > 0, -1, "empty segment")
            blks = blocks[si * per * bps:(si + 1) * per * bps]

            def bits(nb):
                nonlocal pos
                if nb == 0:
                    return 0
                v = (int.from_bytes(buf[pos >> 3:(pos >> 3) + 4], "big") >> (32 - (pos & 7) - nb)) & ((1 << nb) - 1)
                pos += nb
                return v

            def sym(lut):
                nonlocal pos
                e = lut[(int.from_bytes(buf[pos >> 3:(pos >> 3) + 3], "big") >> (8 - (pos & 7))) & 0xFFFF]
                _need(e != 0, -1, "no Huffman code matches")
                pos += e >> 8
                return e & 255

            eobrun = 0
            if ss == 0 and ah == 0:
                pred = [0] * len(sc["comps"])
                for j, (c, by, bx) in enumerate(blks):
                    k = ci_of[j % bps]
                    cat = sym(luts[k])
                    _need(cat <= 11, -1, "DC category")
                    if cat:
                        v = bits(cat)
                        pred[k] += v if v >= (1 << (cat - 1)) else v - (1 << cat) + 1
                    _need(pos <= end and -32768 <= pred[k] <= 32767 and -32768 <= pred[k] * (1 << al) <= 32767, -1, "DC range or data end")
                    coefs[c][by, bx, 0] = pred[k] * (1 << al)
            elif ss == 0:
                for j, (c, by, bx) in enumerate(blks):
                    _need(pos < end, -1, "DC refinement bits run out")
                    if bits(1):
                        coefs[c][by, bx, 0] |= 1 << al
            elif ah == 0:
                lut = luts[0]
                for (c, by, bx) in blks:
                    if eobrun:
                        eobrun -= 1
                        continue
                    blk = coefs[c][by, bx]
                    k = ss
                    while k <= se:
                        rs = sym(lut)
                        run, sz = rs >> 4, rs & 15
                        if sz:
                            k += run
                            v = bits(sz)
                            v = (v if v >= (1 << (sz - 1)) else v - (1 << sz) + 1) * (1 << al)
                            _need(k <= se and pos <= end and -32768 <= v <= 32767, -1, "AC index, range or data end")
                            blk[k] = v
                        elif run == 15:
                            k += 15
                            _need(k <= se and pos <= end, -1, "zero run past the band")
                        else:
                            eobrun = (1 << run) + bits(run) - 1
                            if stats is not None:
                                stats["max_eob_category"] = max(stats["max_eob_category"], run)
                            _need(pos <= end, -1, "data end")
                            break
                        k += 1
            else:
                lut, p1 = luts[0], 1 << al

                def correct(blk, k):
                    if bits(1) and not (int(blk[k]) & p1):
                        blk[k] += p1 if blk[k] >= 0 else -p1

                for (c, by, bx) in blks:
                    blk = coefs[c][by, bx]
                    k = ss
                    if eobrun == 0:
                        while k <= se:
                            rs = sym(lut)
                            run, sz, val = rs >> 4, rs & 15, 0
                            if sz:
                                _need(sz == 1, -1, "refinement size")
                                val = p1 if bits(1) else -p1
                            elif run != 15:
                                eobrun = (1 << run) + bits(run)
                                if stats is not None:
                                    stats["max_eob_category"] = max(stats["max_eob_category"], run)
                                break
                            while k <= se:
                                if blk[k] != 0:
                                    correct(blk, k)
                                else:
                                    run -= 1
                                    if run < 0:
                                        break
                                k += 1
                            _need(pos <= end, -1, "data end")
                            if val:
                                _need(k <= se, -1, "new coefficient past the band")
                                blk[k] = val
                            k += 1
                    if eobrun > 0:
                        while k <= se:
                            if blk[k] != 0:
                                correct(blk, k)
                            k += 1
                        eobrun -= 1
                    _need(pos <= end, -1, "data end")
            rem = end - pos
            _need(eobrun == 0 and 0 <= rem < 8 and (rem == 0 or bits(rem) == (1 << rem) - 1), -1, "data does not end with its segment")
    return fr, coefs


def status(data: bytes) -> int:
    """The entropy-level status the device gives (0 / -1 / -2), short of the IDCT's range check."""
    try:
        decode(data)
        return 0
    except Refused as e:
        return e.code


# ------------------------------------------------------------------------------------------------ writers
def gen_table(freq):
    """Optimal Huffman table for symbol counts, code lengths <= 16, no all-ones code (libjpeg's jpeg_gen_optimal_table) -> (bits, vals)"""
    f = [0] * 257
    for s, c in freq.items():
        f[s] = c
    if not any(f):
        f[0] = 1
    f[256] = 1
    size, others = [0] * 257, [-1] * 257
    while True:
        c1, v = -1, 1 << 60
        for i in range(257):
            if f[i] and f[i] <= v:
                v, c1 = f[i], i
        c2, v = -1, 1 << 60
        for i in range(257):
            if f[i] and f[i] <= v and i != c1:
                v, c2 = f[i], i
        if c2 < 0:
            break
        f[c1] += f[c2]
        f[c2] = 0
        size[c1] += 1
        while others[c1] >= 0:
            c1 = others[c1]
            size[c1] += 1
        others[c1] = c2
        size[c2] += 1
        while others[c2] >= 0:
            c2 = others[c2]
            size[c2] += 1
    bits = [0] * 34
    for i in range(257):
        if size[i]:
            bits[size[i]] += 1
    for i in range(32, 16, -1):
        while bits[i] > 0:
            j = i - 2
            while bits[j] == 0:
                j -= 1
            bits[i] -= 2
            bits[i - 1] += 1
            bits[j + 1] += 2
            bits[j] -= 1
    i = 16
    while bits[i] == 0:
        i -= 1
    bits[i] -= 1
    vals = [s for l in range(1, 33) for s in range(256) if size[s] == l]
    return bits[:17], vals


def _codes(bits, vals):
    out, code, k = {}, 0, 0
    for l in range(1, 17):
        for _ in range(bits[l]):
            out[vals[k]] = (code, l)
            code += 1
            k += 1
        code <<= 1
    return out


def _emit(tokens, codes):
    """tokens: (table key or None, symbol / value, number of raw bits) -> stuffed bytes, padded with ones"""
    acc, nb, out = 0, 0, bytearray()
    for key, a, b in tokens:
        if key is None:
            acc, nb = (acc << b) | a, nb + b
        else:
            code, l = codes[key][a]
            acc, nb = (acc << l) | code, nb + l
        while nb >= 8:
            byte = (acc >> (nb - 8)) & 255
            out.append(byte)
            if byte == 255:
                out.append(0)
            nb -= 8
        acc &= (1 << nb) - 1
    if nb:
        byte = ((acc << (8 - nb)) | ((1 << (8 - nb)) - 1)) & 255
        out.append(byte)
        if byte == 255:
            out.append(0)
    return bytes(out)


def _mag(v):
    """-> (category, the category's extra bits) of a non-zero value or a DC difference"""
    n = abs(v).bit_length()
    return n, (v if v >= 0 else v - 1) & ((1 << n) - 1)


def _slot(c):
    return 0 if c == 0 else 1


def _scan_tokens(fr, coefs, comps, ss, se, ah, al, restart):
    """-> token lists, one per restart segment, of one scan (jcphuff.c's four encoders, or the sequential one for ss == 0, se == 63)"""
    blocks, bps = scan_blocks(fr, comps)
    per = (restart if restart else len(blocks) // bps) * bps
    segs = []
    for s0 in range(0, len(blocks), per):
        t = []
        pred = {}
        st = dict(eobrun=0, be=[])

        def flush_eob(key):
            if st["eobrun"]:
                n = st["eobrun"].bit_length() - 1
                t.append((key, n << 4, 0))
                if n:
                    t.append((None, st["eobrun"] & ((1 << n) - 1), n))
                st["eobrun"] = 0
                t.extend((None, b, 1) for b in st["be"])
                st["be"] = []

        for (c, by, bx) in blocks[s0:s0 + per]:
            blk = coefs[c][by, bx]
            akey = (1, _slot(c))
            if ss == 0 and ah == 0:
                v = int(blk[0]) >> al
                n, extra = _mag(v - pred.get(c, 0))
                pred[c] = v
                t.append(((0, _slot(c)), n, 0))
                if n:
                    t.append((None, extra, n))
                if se == 0:
                    continue
                r = 0   # sequential: the AC coefficients follow in the same scan
                for k in range(1, 64):
                    v = int(blk[k])
                    if v == 0:
                        r += 1
                        continue
                    while r > 15:
                        t.append((akey, 0xF0, 0))
                        r -= 16
                    n, extra = _mag(v)
                    t.append((akey, (r << 4) | n, 0))
                    t.append((None, extra, n))
                    r = 0
                if r:
                    t.append((akey, 0, 0))
            elif ss == 0:
                t.append((None, (int(blk[0]) >> al) & 1, 1))
            elif ah == 0:
                r = 0
                for k in range(ss, se + 1):
                    v = int(blk[k])
                    a = abs(v) >> al
                    if a == 0:
                        r += 1
                        continue
                    flush_eob(akey)
                    while r > 15:
                        t.append((akey, 0xF0, 0))
                        r -= 16
                    n = a.bit_length()
                    t.append((akey, (r << 4) | n, 0))
                    t.append((None, (a if v > 0 else ~a) & ((1 << n) - 1), n))
                    r = 0
                if r:
                    st["eobrun"] += 1
                    if st["eobrun"] == 0x7FFF:
                        flush_eob(akey)
            else:
                absv = [abs(int(blk[k])) >> al for k in range(64)]
                eob = max([k for k in range(ss, se + 1) if absv[k] == 1], default=0)
                r, br = 0, []
                for k in range(ss, se + 1):
                    a = absv[k]
                    if a == 0:
                        r += 1
                        continue
                    while r > 15 and k <= eob:
                        flush_eob(akey)
                        t.append((akey, 0xF0, 0))
                        r -= 16
                        t.extend((None, b, 1) for b in br)
                        br = []
                    if a > 1:
                        br.append(a & 1)
                        continue
                    flush_eob(akey)
                    t.append((akey, (r << 4) | 1, 0))
                    t.append((None, 0 if blk[k] < 0 else 1, 1))
                    t.extend((None, b, 1) for b in br)
                    br = []
                    r = 0
                if r or br:
                    st["eobrun"] += 1
                    st["be"] += br
                    if st["eobrun"] == 0x7FFF or len(st["be"]) > 937:
                        flush_eob(akey)
        if ss:
            flush_eob((1, _slot(comps[0])))
        segs.append(t)
    return segs


def _dht(tables):
    out = bytearray()
    for (tc, t), (bits, vals) in sorted(tables.items()):
        body = bytes([(tc << 4) | t]) + bytes(bits[1:17]) + bytes(vals)
        out += b"\xff\xc4" + (len(body) + 2).to_bytes(2, "big") + body
    return bytes(out)


def _write(fr, coefs, sof, script, restarts, tables_first):
    toks = [_scan_tokens(fr, coefs, comps, ss, se, ah, al, rst) for (comps, ss, se, ah, al), rst in zip(script, restarts)]

    def tables_of(scans):
        freq = {}
        for segs in scans:
            for t in segs:
                for key, a, _ in t:
                    if key is not None:
                        freq.setdefault(key, {})
                        freq[key][a] = freq[key].get(a, 0) + 1
        return {k: gen_table(v) for k, v in freq.items()}

    out = bytearray(b"\xff\xd8")
    for a in fr.app:
        out += a
    wide = any(v > 255 for c in range(fr.ncomp) for v in fr.qt[fr.tq[c]])
    for t in sorted(set(fr.tq)):
        body = bytes([((1 if wide else 0) << 4) | t]) + b"".join(v.to_bytes(2 if wide else 1, "big") for v in fr.qt[t])
        out += b"\xff\xdb" + (len(body) + 2).to_bytes(2, "big") + body
    if sof == 0xC0 and wide:
        sof = 0xC1
    body = bytes([8]) + fr.height.to_bytes(2, "big") + fr.width.to_bytes(2, "big") + bytes([fr.ncomp])
    for c in range(fr.ncomp):
        hsc, vsc = comp_geometry(fr, c)[:2]
        body += bytes([c + 1, (hsc << 4) | vsc, fr.tq[c]])
    out += bytes([0xFF, sof]) + (len(body) + 2).to_bytes(2, "big") + body
    every = tables_of(toks) if tables_first else None
    if tables_first:
        out += _dht(every)
    last_rst = 0
    for (comps, ss, se, ah, al), rst, segs in zip(script, restarts, toks):
        tables = every if tables_first else tables_of([segs])
        if not tables_first:
            out += _dht(tables)
        if rst != last_rst:
            out += b"\xff\xdd\x00\x04" + rst.to_bytes(2, "big")
            last_rst = rst
        body = bytes([len(comps)]) + b"".join(bytes([c + 1, (_slot(c) << 4) | _slot(c)]) for c in comps) + bytes([ss, se, (ah << 4) | al])
        out += b"\xff\xda" + (len(body) + 2).to_bytes(2, "big") + body
        codes = {k: _codes(*v) for k, v in tables.items()}
        for i, t in enumerate(segs):
            if i:
                out += bytes([0xFF, 0xD0 + ((i - 1) & 7)])
            out += _emit(t, codes)
    return bytes(out + b"\xff\xd9")


def write_baseline(fr, coefs) -> bytes:
    """The coefficients as a sequential file with one interleaved scan: a lossless transcode (the blocks a single-component scan never
    sends, outside the picture, keep their zeros)."""
    return _write(fr, coefs, 0xC0, [(list(range(fr.ncomp)), 0, 63, 0, 0)], [0], False)


def write_progressive(fr, coefs, script, restarts=None, tables_first=False) -> bytes:
    """The coefficients under a scan script: [(components, Ss, Se, Ah, Al)], one restart interval per scan (0: none), every scan's tables
    before its SOS or all tables before the first scan."""
    return _write(fr, coefs, 0xC2, [(list(c), ss, se, ah, al) for c, ss, se, ah, al in script], list(restarts) if restarts else [0] * len(script), tables_first)
