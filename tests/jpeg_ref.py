"""NumPy restatement of the project's baseline JPEG encoder (csrc/jpeg.hip, include/mq_hip.h mq_jpeg_encode).

Integer arithmetic only, so the GPU and this file agree byte for byte.  A frame is uint8 (H, W, 3) BGR; the stream
is baseline sequential JPEG, 8 bit, YCbCr 4:2:0, one interleaved scan with a restart marker every ``ri`` MCUs:

  padding   H and W up to multiples of 16 by replicating the last row / column (SOF0 carries the true size)
  colour    Y  = (19595 R + 38470 G + 7471 B + 32768) >> 16
            Cb = clamp(((-11059 R - 21709 G + 32768 B + 32768) >> 16) + 128, 0, 255)
            Cr = clamp(((32768 R - 27439 G - 5329 B + 32768) >> 16) + 128, 0, 255)
  chroma    each 2 x 2 quad -> (a + b + c + d + bias) >> 2, bias = 1 in even chroma columns and 2 in odd ones
            (libjpeg's h2v2 rule: a constant 2 rounds every tie up and costs 0.25 dB on smooth images);  then
            every sample - 128
  DCT       A = (T X + 1024) >> 11, B = A T^T (scale 2^15; u, the first index, is the vertical frequency)
  quantise  q = sign(B) ((|B| + (Q << 14)) // (Q << 15)), Q the Annex K table scaled by libjpeg's quality rule
  entropy   the four Annex K "typical" Huffman tables, DC differences per component with the predictor reset at
            each restart interval, ZRL / EOB as usual, 0xFF bytes stuffed, 1-bit padding before every marker
"""
import numpy as np

# T[u][x] = rint(8192 c_u / 2 cos((2x + 1) u pi / 16)), c_0 = sqrt(1/2)
T = np.array([
    [2896, 2896, 2896, 2896, 2896, 2896, 2896, 2896],
    [4017, 3406, 2276, 799, -799, -2276, -3406, -4017],
    [3784, 1567, -1567, -3784, -3784, -1567, 1567, 3784],
    [3406, -799, -4017, -2276, 2276, 4017, 799, -3406],
    [2896, -2896, -2896, 2896, 2896, -2896, -2896, 2896],
    [2276, -4017, 799, 3406, -3406, -799, 4017, -2276],
    [1567, -3784, 3784, -1567, -1567, 3784, -3784, 1567],
    [799, -2276, 3406, -4017, 4017, -3406, 2276, -799]], dtype=np.int64)

# ZIGZAG[k] = natural (row-major, u * 8 + v) index of the k-th coefficient of the scan
ZIGZAG = np.array([
    0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21,
    28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61,
    54, 47, 55, 62, 63])

# Annex K.1 / K.2, natural order
Q_LUMA = np.array([
    16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29,
    51, 87, 80, 62, 18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120,
    101, 72, 92, 95, 98, 112, 100, 103, 99])
Q_CHROMA = np.array([
    17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99,
    99, 99, 99, 99] + [99] * 32)

# Annex K.3 - K.6: (code lengths 1..16, symbols)
DC_LUMA = ([0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0], list(range(12)))
DC_CHROMA = ([0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0], list(range(12)))
AC_LUMA = ([0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 125], [
    0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71, 0x14,
    0x32, 0x81, 0x91, 0xa1, 0x08, 0x23, 0x42, 0xb1, 0xc1, 0x15, 0x52, 0xd1, 0xf0, 0x24, 0x33, 0x62, 0x72, 0x82, 0x09,
    0x0a, 0x16, 0x17, 0x18, 0x19, 0x1a, 0x25, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x34, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a,
    0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65,
    0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88,
    0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9,
    0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca,
    0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe1, 0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea,
    0xf1, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa])
AC_CHROMA = ([0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 119], [
    0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22, 0x32,
    0x81, 0x08, 0x14, 0x42, 0x91, 0xa1, 0xb1, 0xc1, 0x09, 0x23, 0x33, 0x52, 0xf0, 0x15, 0x62, 0x72, 0xd1, 0x0a, 0x16,
    0x24, 0x34, 0xe1, 0x25, 0xf1, 0x17, 0x18, 0x19, 0x1a, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x35, 0x36, 0x37, 0x38, 0x39,
    0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64,
    0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x82, 0x83, 0x84, 0x85, 0x86,
    0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7,
    0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8,
    0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9,
    0xea, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa])
HUFFMAN = {0x00: DC_LUMA, 0x10: AC_LUMA, 0x01: DC_CHROMA, 0x11: AC_CHROMA}

HEADER_BYTES = 629
BLOCK_MAX_BITS = 20 + 63 * 26     # DC: 9-bit code + 11 bits; 63 AC: 16-bit code + 10 bits (a ZRL only shortens it)


def quant_tables(quality):
    """(luma, chroma) int64 (64,) natural order: libjpeg's jpeg_quality_scaling on the Annex K tables."""
    if not 1 <= int(quality) <= 100:
        raise ValueError("quality must be in [1, 100]")
    q = int(quality)
    s = 5000 // q if q < 50 else 200 - 2 * q
    return tuple(np.clip((base * s + 50) // 100, 1, 255) for base in (Q_LUMA, Q_CHROMA))


def huffman_codes(table):
    """{symbol: (code, length)} of a (lengths, symbols) table: canonical codes, Annex C."""
    bits, vals = table
    out, code, k = {}, 0, 0
    for length in range(1, 17):
        for _ in range(bits[length - 1]):
            out[vals[k]] = (code, length)
            code += 1
            k += 1
        code <<= 1
    return out


def max_bytes(height, width, ri):
    """The bound mq_jpeg_max_bytes states: header, and per restart interval its worst-case bits with every byte
    stuffed and one two-byte marker (RSTn, or EOI after the last)."""
    n_mcu = ((height + 15) // 16) * ((width + 15) // 16)
    n_int = (n_mcu + ri - 1) // ri
    return HEADER_BYTES + n_int * (2 * ((ri * 6 * BLOCK_MAX_BITS + 7) // 8) + 2)


def _seg(marker, payload):
    return bytes([0xFF, marker]) + (len(payload) + 2).to_bytes(2, "big") + bytes(payload)


def header(height, width, quality, ri):
    ql, qc = quant_tables(quality)
    h = b"\xff\xd8"
    h += _seg(0xE0, b"JFIF\x00\x01\x01\x00\x00\x01\x00\x01\x00\x00")
    h += _seg(0xDB, bytes([0]) + bytes(int(v) for v in ql[ZIGZAG]))
    h += _seg(0xDB, bytes([1]) + bytes(int(v) for v in qc[ZIGZAG]))
    h += _seg(0xC0, bytes([8]) + height.to_bytes(2, "big") + width.to_bytes(2, "big") +
              bytes([3, 1, 0x22, 0, 2, 0x11, 1, 3, 0x11, 1]))
    for tid in (0x00, 0x10, 0x01, 0x11):
        bits, vals = HUFFMAN[tid]
        h += _seg(0xC4, bytes([tid]) + bytes(bits) + bytes(vals))
    h += _seg(0xDD, ri.to_bytes(2, "big"))
    h += _seg(0xDA, bytes([3, 1, 0x00, 2, 0x11, 3, 0x11, 0, 63, 0]))
    assert len(h) == HEADER_BYTES
    return h


def coefficients(img, quality):
    """Quantised coefficients int64 (n_mcu, 6, 64) in zigzag order, MCUs in raster order, blocks Y00 Y01 Y10 Y11
    Cb Cr."""
    img = np.asarray(img)
    if img.dtype != np.uint8 or img.ndim != 3 or img.shape[2] != 3:
        raise ValueError("img must be uint8 (H, W, 3)")
    H, W = img.shape[:2]
    if not (1 <= H <= 65535 and 1 <= W <= 65535):
        raise ValueError("H and W must be in [1, 65535]")
    Hp, Wp = (H + 15) // 16 * 16, (W + 15) // 16 * 16
    p = np.pad(img, ((0, Hp - H), (0, Wp - W), (0, 0)), mode="edge").astype(np.int64)
    B, G, R = p[..., 0], p[..., 1], p[..., 2]
    Y = (19595 * R + 38470 * G + 7471 * B + 32768) >> 16
    Cb = np.clip(((-11059 * R - 21709 * G + 32768 * B + 32768) >> 16) + 128, 0, 255)
    Cr = np.clip(((32768 * R - 27439 * G - 5329 * B + 32768) >> 16) + 128, 0, 255)
    sub = lambda c: (c[0::2, 0::2] + c[0::2, 1::2] + c[1::2, 0::2] + c[1::2, 1::2] +
                     (1 + (np.arange(Wp // 2) & 1))[None, :]) >> 2
    ql, qc = quant_tables(quality)

    def blocks(plane, Q):                      # (h, w) -> (h/8, w/8, 64) quantised, zigzag
        h, w = plane.shape
        X = (plane - 128).reshape(h // 8, 8, w // 8, 8).transpose(0, 2, 1, 3)          # (by, bx, y, x)
        A = (np.einsum("uy,abyx->abux", T, X) + 1024) >> 11
        Bc = np.einsum("abux,vx->abuv", A, T).reshape(h // 8, w // 8, 64)
        q = np.sign(Bc) * ((np.abs(Bc) + (Q << 14)) // (Q << 15))
        return q[..., ZIGZAG]

    y, cb, cr = blocks(Y, ql), blocks(sub(Cb), qc), blocks(sub(Cr), qc)
    my, mx = Hp // 16, Wp // 16
    out = np.empty((my, mx, 6, 64), dtype=np.int64)
    out[:, :, 0], out[:, :, 1] = y[0::2, 0::2], y[0::2, 1::2]
    out[:, :, 2], out[:, :, 3] = y[1::2, 0::2], y[1::2, 1::2]
    out[:, :, 4], out[:, :, 5] = cb, cr
    return out.reshape(my * mx, 6, 64)


class _Bits:
    def __init__(self):
        self.acc, self.n, self.out, self.stuffed = 0, 0, bytearray(), 0

    def put(self, code, length):
        self.acc = (self.acc << length) | code
        self.n += length
        while self.n >= 8:
            b = (self.acc >> (self.n - 8)) & 0xFF
            self.n -= 8
            self.out.append(b)
            if b == 0xFF:
                self.out.append(0)
                self.stuffed += 1
        self.acc &= (1 << self.n) - 1

    def flush(self):
        if self.n:
            self.put((1 << (8 - self.n)) - 1, 8 - self.n)


def encode(img, quality=90, ri=16):
    """(bytes, stats): the complete JPEG of ``img`` and the symbol classes its scan used."""
    if not 1 <= int(ri) <= 32:
        raise ValueError("restart_interval must be in [1, 32]")
    H, W = np.asarray(img).shape[:2]
    coef = coefficients(img, quality)
    dc = (huffman_codes(DC_LUMA), huffman_codes(DC_CHROMA))
    ac = (huffman_codes(AC_LUMA), huffman_codes(AC_CHROMA))
    stats = dict(zrl=0, eob=0, no_eob=0, dc_cat=set(), ac_cat=set(), stuffed=0, rst=0, blocks=0)
    w = _Bits()
    n_mcu = len(coef)
    for m in range(n_mcu):
        if m % ri == 0:
            if m:
                w.flush()
                w.out += bytes([0xFF, 0xD0 + ((m // ri - 1) % 8)])
                stats["rst"] += 1
            pred = [0, 0, 0]
        for b in range(6):
            c = coef[m, b]
            comp = 0 if b < 4 else b - 3
            t = 0 if b < 4 else 1
            v = int(c[0]) - pred[comp]
            pred[comp] = int(c[0])
            s = abs(v).bit_length()
            stats["dc_cat"].add(s)
            w.put(*dc[t][s])
            if s:
                w.put(v if v >= 0 else v + (1 << s) - 1, s)
            run = 0
            for k in range(1, 64):
                v = int(c[k])
                if v == 0:
                    run += 1
                    continue
                while run >= 16:
                    w.put(*ac[t][0xF0])
                    stats["zrl"] += 1
                    run -= 16
                s = abs(v).bit_length()
                stats["ac_cat"].add(s)
                w.put(*ac[t][(run << 4) | s])
                w.put(v if v >= 0 else v + (1 << s) - 1, s)
                run = 0
            if run:
                w.put(*ac[t][0x00])
                stats["eob"] += 1
            else:
                stats["no_eob"] += 1
            stats["blocks"] += 1
    w.flush()
    w.out += b"\xff\xd9"
    stats["stuffed"] = w.stuffed
    return header(H, W, int(quality), int(ri)) + bytes(w.out), stats


class Encoder:
    """``mqhip.mjpeg.JpegEncoder``'s interface on this file: what CPU tests inject as ``encoder``."""

    def __init__(self, height, width, quality=90, restart_interval=16, device=0):
        self.H, self.W, self.quality, self.ri = height, width, quality, restart_interval

    def encode(self, frames):
        frames = frames.cpu().numpy() if hasattr(frames, "cpu") else np.asarray(frames)
        return [encode(f, self.quality, self.ri)[0] for f in frames]


def stress_image():
    """48 x 64 BGR, 12 MCUs.  Row 1: an all-0 MCU next to an all-255 MCU (the largest DC difference), 4-pixel
    black / white stripes, a pure (7, 7)-frequency cosine (a run of zeros up to the last coefficient: ZRLs and
    no EOB).  Row 2: seeded noise (every coefficient non-zero at quality 100).  Row 3: a ramp."""
    img = np.zeros((48, 64, 3), dtype=np.uint8)
    img[0:16, 16:32] = 255
    img[0:16, 32:48] = np.where((np.arange(16) // 4) % 2 == 0, 0, 255).astype(np.uint8)[None, :, None]
    k = np.arange(16) % 8
    c = np.cos((2 * k + 1) * 7 * np.pi / 16)
    img[0:16, 48:64] = np.clip(np.rint(128 + 100 * np.outer(c, c)), 0, 255).astype(np.uint8)[:, :, None]
    img[16:32] = np.random.default_rng(7).integers(0, 256, (16, 64, 3), dtype=np.uint8)
    img[32:48] = (np.arange(64) * 4)[None, :, None].astype(np.uint8)
    img[32:48, :, 1] = (np.arange(16) * 16)[:, None].astype(np.uint8)
    return img


def smooth_image(h, w, seed):
    """A seeded sum of low-frequency waves per channel: the content a camera frame has between its edges."""
    r = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    ch = [127 + 60 * np.sin(xx / r.uniform(5, 9) + r.uniform(0, 3)) * np.cos(yy / r.uniform(4, 8)) +
          40 * np.sin((xx + yy) / r.uniform(9, 15)) for _ in range(3)]
    return np.clip(np.rint(np.stack(ch, axis=-1)), 0, 255).astype(np.uint8)


def streams():
    """The small streams the CPU and GPU tests share: (name, image, quality, ri)."""
    rng = np.random.default_rng(0)
    return [("flat16", np.full((16, 16, 3), (10, 200, 90), dtype=np.uint8), 90, 16),
            ("stress", stress_image(), 100, 1),
            ("17x33", rng.integers(0, 256, (17, 33, 3), dtype=np.uint8), 50, 16),
            ("40x24", smooth_image(40, 24, 1), 90, 16),
            ("48x80ri4", rng.integers(0, 256, (48, 80, 3), dtype=np.uint8), 75, 4),
            ("q1", rng.integers(0, 256, (24, 40, 3), dtype=np.uint8), 1, 16),
            ("q100", smooth_image(24, 40, 2), 100, 8)]
