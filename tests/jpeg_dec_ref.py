"""NumPy restatement of the project's baseline JPEG decoder (csrc/jpeg_parse.cpp, csrc/jpeg_dec_dev.hpp,
csrc/jpeg_dec.hip; the codec is stated in include/mq_hip.h under mq_jpeg_decode).

Integer arithmetic only, no data-dependent order: the GPU and this file agree byte for byte, and on the streams
Pillow (libjpeg-turbo) accepts this file equals ``Image.open(...).convert('RGB')`` on every pixel.

  parse      SOI, then segments up to SOS: SOF0 8 bit, 1 component or YCbCr with luma 1x1 / 2x1 / 2x2 and chroma
             1x1, DQT Pq = 0, DHT ids 0-1 (the Annex K tables when the stream has none), DRI, APPn / COM skipped;
             one scan over all components, Ss 0, Se 63, Ah = Al = 0; the first FF D9 after SOS ends it.  Everything
             else is refused with a negative code (E_*).
  intervals  FF D0..D7 / FF D9 pairs after SOS split the scan; interval i ends in D0 + (i mod 8), the last in D9;
             there must be ceil(n_mcu / RI) of them (1 when RI is 0), else status 1 and nothing is decoded.
  entropy    bits MSB first, FF 00 -> FF, DC predictors 0 at the start of an interval (kept as int16, wrapping),
             EXTEND of Annex F, ZRL 0xF0, any other AC symbol with size 0 is EOB.  An interval stops at its first
             fault: 2 no code matches (4 if fewer than 16 bits are left), 3 a run past coefficient 63, 4 bits
             exhausted.  A frame's status is the largest code of its intervals.
  IDCT       libjpeg's jpeg_idct_islow (CONST_BITS 13, PASS1_BITS 2) in 32-bit arithmetic that wraps (a malformed
             stream can overflow it; a valid one never does: ``stats['wrapped']``), + 128, clamp.
  upsample   libjpeg's fancy h2v1 / h2v2 on the true chroma extent, replication when the chroma plane is at most 2
             samples wide; edges repeat the last true row / column.
  colour     libjpeg's 16-bit fixed point YCbCr -> RGB, stored B, G, R.
"""
import numpy as np

import jpeg_ref

ZIGZAG = jpeg_ref.ZIGZAG
LOOK_BITS = 9          # csrc/jpeg_dec_dev.hpp JPEG_DEC_LOOK_BITS: longer codes take the maxcode walk

E_NOT_JPEG, E_TRUNCATED, E_SOF, E_PRECISION, E_DQT, E_COMPONENTS = -20, -21, -22, -23, -24, -25
E_SAMPLING, E_SCANS, E_TABLE, E_HUFFMAN, E_NO_EOI, E_SIZE = -26, -27, -28, -29, -30, -31
ST_OK, ST_MARKERS, ST_NO_CODE, ST_RUN, ST_EXHAUSTED = 0, 1, 2, 3, 4


class ParseError(ValueError):
    def __init__(self, code, what=""):
        super().__init__(f"jpeg parse error {code} {what}")
        self.code = code


class Info:
    """What mq_jpeg_info holds."""
    FIELDS = ("height", "width", "n_comp", "h_luma", "v_luma", "restart_interval", "scan_offset")

    def __init__(self):
        self.height = self.width = self.n_comp = self.h_luma = self.v_luma = self.restart_interval = 0
        self.scan_offset = 0
        self.quant = np.zeros((3, 64), dtype=np.uint8)          # per component, natural order
        self.dc_sel, self.ac_sel = [0, 0, 0], [0, 0, 0]
        self.dc = [([0] * 16, [0] * 256), ([0] * 16, [0] * 256)]   # (bits, vals)
        self.ac = [([0] * 16, [0] * 256), ([0] * 16, [0] * 256)]

    @property
    def blocks(self):
        return 1 if self.n_comp == 1 else self.h_luma * self.v_luma + 2

    @property
    def mcus(self):
        mw, mh = (8 * self.h_luma, 8 * self.v_luma) if self.n_comp == 3 else (8, 8)
        return -(-self.height // mh), -(-self.width // mw)


def _check_huffman(bits, n_vals, dc, vals):
    if sum(bits) > 256 or sum(bits) != n_vals:
        return False
    code = 0
    for length in range(1, 17):
        code += bits[length - 1]
        if code > (1 << length):
            return False
        code <<= 1
    return not (dc and any(v > 15 for v in vals))


def parse(data):
    """``Info`` of a stream, or ``ParseError`` with the code mq_jpeg_parse returns."""
    data = bytes(data)
    n = len(data)
    if n < 2 or data[:2] != b"\xff\xd8":
        raise ParseError(E_NOT_JPEG)
    info = Info()
    qt, dht = {}, {}
    comps, adobe = None, None
    pos = 2
    while True:
        if pos + 4 > n:
            raise ParseError(E_TRUNCATED)
        if data[pos] != 0xFF:
            raise ParseError(E_NOT_JPEG)
        m = data[pos + 1]
        if m == 0xFF:                      # fill byte
            pos += 1
            continue
        seglen = int.from_bytes(data[pos + 2:pos + 4], "big")
        if seglen < 2 or pos + 2 + seglen > n:
            raise ParseError(E_TRUNCATED)
        p = data[pos + 4:pos + 2 + seglen]
        pos += 2 + seglen
        if m == 0xC0:
            if comps is not None:
                raise ParseError(E_SOF)
            if len(p) < 6:
                raise ParseError(E_TRUNCATED)
            if p[0] != 8:
                raise ParseError(E_PRECISION)
            info.height, info.width = int.from_bytes(p[1:3], "big"), int.from_bytes(p[3:5], "big")
            nc = p[5]
            if nc not in (1, 3):
                raise ParseError(E_COMPONENTS)
            if len(p) != 6 + 3 * nc:
                raise ParseError(E_TRUNCATED)
            if info.height == 0 or info.width == 0:
                raise ParseError(E_SIZE)
            comps = [(p[6 + 3 * c], p[7 + 3 * c] >> 4, p[7 + 3 * c] & 15, p[8 + 3 * c]) for c in range(nc)]
            info.n_comp = nc
        elif m in (0xC1, 0xC2, 0xC3, 0xC5, 0xC6, 0xC7, 0xC9, 0xCA, 0xCB, 0xCD, 0xCE, 0xCF, 0xCC):
            raise ParseError(E_SOF)
        elif m == 0xDB:
            k = 0
            while k < len(p):
                if p[k] >> 4 or (p[k] & 15) > 3:
                    raise ParseError(E_DQT)
                if k + 65 > len(p):
                    raise ParseError(E_TRUNCATED)
                t = np.zeros(64, dtype=np.uint8)
                t[ZIGZAG] = np.frombuffer(p[k + 1:k + 65], dtype=np.uint8)
                qt[p[k] & 15] = t
                k += 65
        elif m == 0xC4:
            k = 0
            while k < len(p):
                if k + 17 > len(p):
                    raise ParseError(E_TRUNCATED)
                tc, th = p[k] >> 4, p[k] & 15
                bits = list(p[k + 1:k + 17])
                if tc > 1 or th > 1 or sum(bits) > 256:
                    raise ParseError(E_HUFFMAN)
                if k + 17 + sum(bits) > len(p):
                    raise ParseError(E_TRUNCATED)
                vals = list(p[k + 17:k + 17 + sum(bits)])
                if not _check_huffman(bits, len(vals), tc == 0, vals):
                    raise ParseError(E_HUFFMAN)
                dht[(tc, th)] = (bits, vals + [0] * (256 - len(vals)))
                k += 17 + sum(bits)
        elif m == 0xDD:
            if len(p) != 2:
                raise ParseError(E_TRUNCATED)
            info.restart_interval = int.from_bytes(p, "big")
        elif m == 0xEE and p[:5] == b"Adobe" and len(p) >= 12:
            adobe = p[11]
        elif m == 0xDA:
            if comps is None:
                raise ParseError(E_SOF)
            if len(p) < 1 or len(p) != 4 + 2 * p[0]:
                raise ParseError(E_TRUNCATED)
            if p[0] != info.n_comp:
                raise ParseError(E_SCANS)
            for c in range(info.n_comp):
                if p[1 + 2 * c] != comps[c][0]:
                    raise ParseError(E_SCANS)
                info.dc_sel[c], info.ac_sel[c] = p[2 + 2 * c] >> 4, p[2 + 2 * c] & 15
            if tuple(p[1 + 2 * info.n_comp:]) != (0, 63, 0):
                raise ParseError(E_SCANS)
            break
        elif m in (0xD8, 0xD9) or 0xD0 <= m <= 0xD7 or m == 0x01 or m == 0x00:
            raise ParseError(E_NOT_JPEG)
        # APPn, COM, anything else with a length: skipped
    if info.n_comp == 3:
        if adobe is not None and adobe != 1:
            raise ParseError(E_COMPONENTS)
        (_, h0, v0, _), (_, h1, v1, _), (_, h2, v2, _) = comps
        if (h1, v1, h2, v2) != (1, 1, 1, 1) or (h0, v0) not in ((1, 1), (2, 1), (2, 2)):
            raise ParseError(E_SAMPLING)
        info.h_luma, info.v_luma = h0, v0
    else:
        info.h_luma = info.v_luma = 1      # a single component is never interleaved: its factors do not matter
    if not dht:
        dht = {(tid >> 4, tid & 15): (list(b), list(v) + [0] * (256 - len(v))) for tid, (b, v) in
               jpeg_ref.HUFFMAN.items()}
    for c in range(info.n_comp):
        if comps[c][3] not in qt or info.dc_sel[c] > 1 or info.ac_sel[c] > 1 or (0, info.dc_sel[c]) not in dht \
                or (1, info.ac_sel[c]) not in dht:
            raise ParseError(E_TABLE)
        info.quant[c] = qt[comps[c][3]]
    for t in range(2):
        if (0, t) in dht:
            info.dc[t] = dht[(0, t)]
        if (1, t) in dht:
            info.ac[t] = dht[(1, t)]
    info.scan_offset = pos
    while True:                          # the scan: only stuffing, fill bytes and RSTn up to the first EOI
        pos = data.find(b"\xff", pos)
        if pos < 0 or pos + 1 >= n:
            raise ParseError(E_NO_EOI)
        m = data[pos + 1]
        if m == 0xD9:
            return info
        if m == 0xFF:
            pos += 1
        elif m == 0 or 0xD0 <= m <= 0xD7:
            pos += 2
        else:
            raise ParseError(E_SCANS)


# ------------------------------------------------------------------------------------------------ entropy
class Tables:
    """csrc/jpeg_dec_dev.hpp JpegDecTables: per table (DC 0, DC 1, AC 0, AC 1) a first-level lookup of LOOK_BITS
    bits and the canonical maxcode / valoff of every length."""

    def __init__(self, info):
        self.look, self.maxcode, self.valoff, self.vals = [], [], [], []
        for bits, vals in (info.dc[0], info.dc[1], info.ac[0], info.ac[1]):
            look, maxcode, valoff = [0] * (1 << LOOK_BITS), [-1] * 18, [0] * 18
            code = k = 0
            for length in range(1, 17):
                valoff[length] = k - code
                for _ in range(bits[length - 1]):
                    if length <= LOOK_BITS and k < 256:
                        lo = code << (LOOK_BITS - length)
                        for e in range(lo, min(lo + (1 << (LOOK_BITS - length)), 1 << LOOK_BITS)):
                            look[e] = (length << 8) | vals[k]
                    code += 1
                    k += 1
                maxcode[length] = code - 1 if bits[length - 1] else -1
                code <<= 1
            self.look.append(look), self.maxcode.append(maxcode), self.valoff.append(valoff), self.vals.append(vals)


def intervals(data, info):
    """[(begin, end)] of the restart intervals, or None (status 1)."""
    n_mcu = info.mcus[0] * info.mcus[1]
    want = -(-n_mcu // info.restart_interval) if info.restart_interval else 1
    out, begin, pos, n = [], info.scan_offset, info.scan_offset, len(data)
    while True:
        pos = data.find(b"\xff", pos)
        if pos < 0 or pos + 1 >= n:
            return None
        m = data[pos + 1]
        if m == 0xD9 or 0xD0 <= m <= 0xD7:
            k = len(out)
            if k >= want or m != (0xD9 if k == want - 1 else 0xD0 + (k & 7)):
                return None
            out.append((begin, pos))
            if m == 0xD9:
                return out
            pos += 2
            begin = pos
        else:
            pos += 1


def _unstuff(seg):
    """FF 00 -> FF, left to right; every other byte stays."""
    return seg.replace(b"\xff\x00", b"\xff")


def decode_interval(seg, T, info, n_mcus, stats=None):
    """(coef int (n_mcus, blocks, 64) natural order, status) of one interval's bytes."""
    nb = info.blocks
    nl = nb - 2 if info.n_comp == 3 else 1
    coef = np.zeros((n_mcus, nb, 64), dtype=np.int64)
    raw = _unstuff(seg)
    total = 8 * len(raw)
    big = int.from_bytes(raw + b"\x00\x00\x00", "big") if raw else 0
    width = total + 24
    pos = 0
    pred = [0, 0, 0]

    def peek16():
        return (big >> (width - pos - 16)) & 0xFFFF

    for m in range(n_mcus):
        for b in range(nb):
            comp = 0 if b < nl else b - nl + 1
            k = 0
            while k < 64:
                t = info.dc_sel[comp] if k == 0 else 2 + info.ac_sel[comp]
                if pos >= total:
                    return coef, ST_EXHAUSTED
                v = peek16()
                e = T.look[t][v >> (16 - LOOK_BITS)]
                if e:
                    length, sym = e >> 8, e & 255
                else:
                    length = 0
                    for ln in range(LOOK_BITS + 1, 17):
                        c = v >> (16 - ln)
                        if c <= T.maxcode[t][ln]:
                            length, sym = ln, T.vals[t][(T.valoff[t][ln] + c) & 255]
                            break
                    if not length:
                        return coef, (ST_EXHAUSTED if total - pos < 16 else ST_NO_CODE)
                    if stats is not None:
                        stats["long_codes"] = stats.get("long_codes", 0) + 1
                if length > total - pos:
                    return coef, ST_EXHAUSTED
                pos += length
                s = sym & 15
                if s > total - pos:
                    return coef, ST_EXHAUSTED
                bits = (peek16() >> (16 - s)) if s else 0
                pos += s
                val = bits - (1 << s) + 1 if s and bits < (1 << (s - 1)) else bits
                if k == 0:
                    pred[comp] = ((pred[comp] + val + 32768) & 0xFFFF) - 32768
                    coef[m, b, 0] = pred[comp]
                    k = 1
                    continue
                r = sym >> 4
                if s == 0:
                    if r != 15:
                        break                     # EOB
                    k += 16
                    if k > 64:
                        return coef, ST_RUN
                    continue
                k += r
                if k > 63:
                    return coef, ST_RUN
                coef[m, b, ZIGZAG[k]] = val
                k += 1
    return coef, ST_OK


# ------------------------------------------------------------------------------------------------ pixels
def _w32(x, stats):
    w = ((x + (1 << 31)) & 0xFFFFFFFF) - (1 << 31)
    if stats is not None and not np.array_equal(w, x):
        stats["wrapped"] = True
    return w


def _idct_pass(x, shift, stats):
    """jpeg_idct_islow's butterfly along axis -2 of (..., 8, n): out = (sum + (1 << (shift - 1))) >> shift."""
    i0, i1, i2, i3, i4, i5, i6, i7 = (x[..., k, :] for k in range(8))
    z1 = (i2 + i6) * 4433
    tmp2 = z1 - i6 * 15137
    tmp3 = z1 + i2 * 6270
    tmp0 = (i0 + i4) << 13
    tmp1 = (i0 - i4) << 13
    t10, t13, t11, t12 = tmp0 + tmp3, tmp0 - tmp3, tmp1 + tmp2, tmp1 - tmp2
    t0, t1, t2, t3 = i7, i5, i3, i1
    z1, z2, z3, z4 = t0 + t3, t1 + t2, t0 + t2, t1 + t3
    z5 = (z3 + z4) * 9633
    t0, t1, t2, t3 = t0 * 2446, t1 * 16819, t2 * 25172, t3 * 12299
    z1, z2, z3, z4 = -z1 * 7373, -z2 * 20995, -z3 * 16069 + z5, -z4 * 3196 + z5
    t0, t1, t2, t3 = t0 + z1 + z3, t1 + z2 + z4, t2 + z2 + z3, t3 + z1 + z4
    out = np.stack([t10 + t3, t11 + t2, t12 + t1, t13 + t0, t13 - t0, t12 - t1, t11 - t2, t10 - t3], axis=-2)
    return _w32(out + (1 << (shift - 1)), stats) >> shift


def idct(coef, q, stats=None):
    """(..., 64) quantised coefficients in natural order, q (64,) -> uint8-valued (..., 8, 8) samples."""
    x = (coef.astype(np.int64) * q.astype(np.int64)).reshape(coef.shape[:-1] + (8, 8))
    a = _idct_pass(x, 11, stats)                                   # columns: along the rows' index
    b = _idct_pass(np.swapaxes(a, -1, -2), 18, stats)              # rows
    return np.clip(np.swapaxes(b, -1, -2) + 128, 0, 255)


def _plane(blocks, my, mx, v, h):
    """(my * mx, v * h, 8, 8) -> (my * v * 8, mx * h * 8)."""
    return blocks.reshape(my, mx, v, h, 8, 8).transpose(0, 2, 4, 1, 3, 5).reshape(my * v * 8, mx * h * 8)


def upsample(c, H, W, h, v):
    """Chroma plane (padded) -> (H, W) by libjpeg's rules on the true extent ceil(H / v) x ceil(W / h)."""
    ch, cw = -(-H // v), -(-W // h)
    c = c[:ch, :cw].astype(np.int64)
    if h == 1:
        return c[:H, :W]
    if cw <= 2:
        return np.repeat(np.repeat(c, v, axis=0), h, axis=1)[:H, :W]
    left, right = np.maximum(np.arange(cw) - 1, 0), np.minimum(np.arange(cw) + 1, cw - 1)
    out = np.empty((ch * v, cw * 2), dtype=np.int64)
    if v == 1:
        out[:, 0::2] = (3 * c + c[:, left] + 1) >> 2
        out[:, 1::2] = (3 * c + c[:, right] + 2) >> 2
    else:
        up, down = c[np.maximum(np.arange(ch) - 1, 0)], c[np.minimum(np.arange(ch) + 1, ch - 1)]
        for par, other in ((0, up), (1, down)):
            s = 3 * c + other
            out[par::2, 0::2] = (3 * s + s[:, left] + 8) >> 4
            out[par::2, 1::2] = (3 * s + s[:, right] + 7) >> 4
    return out[:H, :W]


def colour(y, cb, cr):
    cb, cr = cb - 128, cr - 128
    r = y + ((91881 * cr + 32768) >> 16)
    g = y + ((-22554 * cb - 46802 * cr + 32768) >> 16)
    b = y + ((116130 * cb + 32768) >> 16)
    return np.clip(np.stack([b, g, r], axis=-1), 0, 255).astype(np.uint8)


def pixels(coef, info, stats=None):
    """(n_mcu, blocks, 64) -> uint8 (H, W, 3) BGR."""
    my, mx = info.mcus
    H, W = info.height, info.width
    if info.n_comp == 1:
        y = _plane(idct(coef[:, 0], info.quant[0], stats), my, mx, 1, 1)[:H, :W]
        return np.repeat(y[..., None], 3, axis=-1).astype(np.uint8)
    h, v = info.h_luma, info.v_luma
    nl = h * v
    y = _plane(idct(coef[:, :nl], info.quant[0], stats), my, mx, v, h)[:H, :W]
    cb = _plane(idct(coef[:, nl], info.quant[1], stats), my, mx, 1, 1)
    cr = _plane(idct(coef[:, nl + 1], info.quant[2], stats), my, mx, 1, 1)
    return colour(y, upsample(cb, H, W, h, v), upsample(cr, H, W, h, v))


def decode_status(data, info=None, stats=None, coef_out=None):
    """The status of a stream whose header parses, without the pixels (what the host check program prints)."""
    data = bytes(data)
    info = info or parse(data)
    iv = intervals(data, info)
    if iv is None:
        return ST_MARKERS
    T = Tables(info)
    n_mcu = info.mcus[0] * info.mcus[1]
    ri = info.restart_interval or n_mcu
    status = 0
    for i, (a, b) in enumerate(iv):
        n = min(ri, n_mcu - i * ri)
        c, st = decode_interval(data[a:b], T, info, n, stats)
        if coef_out is not None:
            coef_out[i * ri:i * ri + n] = c
        status = max(status, st)
    return status


def decode(data, info=None, stats=None):
    """(uint8 (H, W, 3) BGR, status).  ``info`` is the header the frame is decoded under (its own by default)."""
    data = bytes(data)
    info = info or parse(data)
    n_mcu = info.mcus[0] * info.mcus[1]
    coef = np.zeros((n_mcu, info.blocks, 64), dtype=np.int64)
    status = decode_status(data, info, stats, coef)
    return pixels(coef, info, stats), status


class JpegError(ValueError):
    def __init__(self, frame, code):
        super().__init__(f"frame {frame}: jpeg error {code}")
        self.frame, self.code = frame, code


class Decoder:
    """``mqhip.mjpeg.JpegDecoder``'s interface on this file: what CPU tests inject as ``decoder``."""

    def __init__(self, device=0):
        self.device = device

    def decode(self, streams):
        out = []
        for i, s in enumerate(streams):
            try:
                img, st = decode(s)
            except ParseError as e:
                raise JpegError(i, e.code) from None
            if st:
                raise JpegError(i, st)
            if out and img.shape != out[0].shape:
                raise ValueError("frames differ in height x width")
            out.append(img)
        return np.stack(out) if out else np.zeros((0, 0, 0, 3), dtype=np.uint8)

    decode_device = decode


# ------------------------------------------------------------------------------------------------ streams
def strip_dht(data):
    """The stream without its DHT segments (what Motion-JPEG AVI frames habitually look like)."""
    data = bytes(data)
    out, pos = bytearray(data[:2]), 2
    while True:
        m, n = data[pos + 1], int.from_bytes(data[pos + 2:pos + 4], "big")
        if m != 0xC4:
            out += data[pos:pos + 2 + n]
        pos += 2 + n
        if m == 0xDA:
            return bytes(out) + data[pos:]


def pillow_stream(img_bgr, mode="RGB", **kw):
    import io

    from PIL import Image
    b = io.BytesIO()
    im = Image.fromarray(np.ascontiguousarray(img_bgr[..., ::-1]))
    if mode != "RGB":
        im = im.convert(mode)
    im.save(b, "JPEG", **kw)
    return b.getvalue()


def mixed_image(h, w, seed):
    """Smooth content with a band of noise: both short and long codes."""
    img = jpeg_ref.smooth_image(h, w, seed)
    k = max(h // 3, 1)
    img[:k] = np.random.default_rng(seed).integers(0, 256, (k, w, 3), dtype=np.uint8)
    return img


def streams():
    """[(name, bytes)]: the seven streams of jpeg_ref.streams() (this project's encoder)."""
    return [(name, jpeg_ref.encode(img, q, ri)[0]) for name, img, q, ri in jpeg_ref.streams()]


PILLOW_SIZES = ((40, 56), (17, 33), (8, 8), (1, 1), (31, 2), (50, 47))
PILLOW_MODES = (("444", dict(subsampling=0, quality=85)), ("422", dict(subsampling=1, quality=85)),
                ("420", dict(subsampling=2, quality=85)), ("420rb1", dict(subsampling=2, restart_marker_blocks=1)),
                ("420rb2", dict(subsampling=2, restart_marker_blocks=2)),
                ("422rb3", dict(subsampling=1, restart_marker_blocks=3)),
                ("444rb5", dict(subsampling=0, restart_marker_blocks=5)),
                ("420rr1", dict(subsampling=2, restart_marker_rows=1)),
                ("420opt", dict(subsampling=2, optimize=True, quality=85)),
                ("420q30", dict(subsampling=2, quality=30)), ("444q100", dict(subsampling=0, quality=100)),
                ("L", dict(quality=85)))


def case_streams():
    """{name: bytes}: the small cases the GPU tests and the host check program share."""
    out = dict(streams())
    p = dict(pillow_streams())
    for k in ("31x2-420", "1x1-420", "31x2-422", "40x56-422", "40x56-444", "40x56-L", "40x56-420opt", "50x47-420",
              "17x33-422rb3", "50x47-444rb5"):
        out[k] = p[k]
    return out


def pillow_streams():
    """[(name, bytes)] written by Pillow: every size x mode of the lists above."""
    out = []
    for h, w in PILLOW_SIZES:
        img = mixed_image(h, w, h * 100 + w)
        for name, kw in PILLOW_MODES:
            out.append((f"{h}x{w}-{name}", pillow_stream(img, "L" if name == "L" else "RGB", **kw)))
    return out
