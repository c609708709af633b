"""The MJPEG export's bitstream contract (include/vbt_hip.h, "MJPEG export") in numpy and plain Python: test infrastructure only,
written from the contract's text.  encode() gives the bytes of one frame - a complete baseline JFIF file, 4:2:0, one restart
interval per MCU row - and, on request, the list of Huffman symbols it coded.  Also a minimal RIFF walker for the AVI tests."""
import struct

import numpy as np

ZIGZAG = np.array([0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28,
                   35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63])

# Annex K.1 / K.2, natural order
BASE_LUMA = np.array([16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87, 80, 62,
                      18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99])
BASE_CHROMA = np.array([17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99, 99]
                       + [99] * 32)

# Annex K.3: (BITS, HUFFVAL)
DC_LUMA = ([0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0], list(range(12)))
DC_CHROMA = ([0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0], list(range(12)))
AC_LUMA = ([0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7d],
           [0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71, 0x14, 0x32, 0x81, 0x91, 0xa1, 0x08,
            0x23, 0x42, 0xb1, 0xc1, 0x15, 0x52, 0xd1, 0xf0, 0x24, 0x33, 0x62, 0x72, 0x82, 0x09, 0x0a, 0x16, 0x17, 0x18, 0x19, 0x1a, 0x25, 0x26, 0x27, 0x28,
            0x29, 0x2a, 0x34, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59,
            0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89,
            0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6,
            0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe1, 0xe2,
            0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf1, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa])
AC_CHROMA = ([0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77],
             [0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22, 0x32, 0x81, 0x08, 0x14, 0x42, 0x91,
              0xa1, 0xb1, 0xc1, 0x09, 0x23, 0x33, 0x52, 0xf0, 0x15, 0x62, 0x72, 0xd1, 0x0a, 0x16, 0x24, 0x34, 0xe1, 0x25, 0xf1, 0x17, 0x18, 0x19, 0x1a, 0x26,
              0x27, 0x28, 0x29, 0x2a, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58,
              0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x82, 0x83, 0x84, 0x85, 0x86, 0x87,
              0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4,
              0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda,
              0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa])

ZRL, EOB = 0xF0, 0x00


def huff_codes(spec):
    """symbol -> (code, length), the canonical assignment of Annex C"""
    bits, vals = spec
    out, code, k = {}, 0, 0
    for length in range(1, 17):
        for _ in range(bits[length - 1]):
            out[vals[k]] = (code, length)
            code += 1
            k += 1
        code <<= 1
    return out


def quant_tables(q):
    """(luma, chroma) in natural order by the IJG rule"""
    s = 5000 // q if q < 50 else 200 - 2 * q
    return tuple(np.clip((b * s + 50) // 100, 1, 255).astype(np.int64) for b in (BASE_LUMA, BASE_CHROMA))


def dct_matrix():
    k, n = np.meshgrid(np.arange(8), np.arange(8), indexing="ij")
    s = np.where(k == 0, np.sqrt(1.0 / 8.0), 0.5)
    return np.rint(8192.0 * s * np.cos((2 * n + 1) * k * np.pi / 16.0)).astype(np.int64)


T = dct_matrix()


def fdct(x):
    """x: int [..., 8, 8] level-shifted samples -> F[..., v, u]"""
    x = np.asarray(x, np.int64)
    A = (x @ T.T + (1 << 10)) >> 11
    return (T @ A + (1 << 14)) >> 15


def quantise(F, Q):
    """F [..., 8, 8], Q natural order [64] -> levels [..., 8, 8]; the DC clamp is -1024..1023, the AC clamp +-1023"""
    Q = np.asarray(Q, np.int64).reshape(8, 8)
    lv = np.sign(F) * ((np.abs(F) + (Q >> 1)) // Q)
    out = np.clip(lv, -1023, 1023)
    out[..., 0, 0] = np.clip(lv[..., 0, 0], -1024, 1023)
    return out


def _pad_edge(p, mh, mw):
    return np.pad(p, ((0, mh - p.shape[0]), (0, mw - p.shape[1])) + ((0, 0),) * (p.ndim - 2), mode="edge")


def rgb_to_ycc(r, g, b):
    """one pixel standing for its whole 2 x 2 cell: (Y, Cb, Cr)"""
    r, g, b = int(r), int(g), int(b)
    y = (19595 * r + 38470 * g + 7471 * b + 32768) >> 16
    cb = ((-11059 * 4 * r - 21709 * 4 * g + 32768 * 4 * b + (1 << 17)) >> 18) + 128
    cr = ((32768 * 4 * r - 27439 * 4 * g - 5329 * 4 * b + (1 << 17)) >> 18) + 128
    return y, min(max(cb, 0), 255), min(max(cr, 0), 255)


def planes_rgb(img):
    """uint8 [H, W, 3] -> (Y [16 MH, 16 MW], Cb, Cr [8 MH, 8 MW]) int64; the edge pixel is replicated before the 2 x 2 sum"""
    H, W = img.shape[:2]
    mh, mw = -(-H // 16) * 16, -(-W // 16) * 16
    p = _pad_edge(np.asarray(img, np.int64), mh, mw)
    R, G, B = p[..., 0], p[..., 1], p[..., 2]
    Y = (19595 * R + 38470 * G + 7471 * B + 32768) >> 16
    S = p.reshape(mh // 2, 2, mw // 2, 2, 3).sum(axis=(1, 3))
    Cb = ((-11059 * S[..., 0] - 21709 * S[..., 1] + 32768 * S[..., 2] + (1 << 17)) >> 18) + 128
    Cr = ((32768 * S[..., 0] - 27439 * S[..., 1] - 5329 * S[..., 2] + (1 << 17)) >> 18) + 128
    return Y, np.clip(Cb, 0, 255), np.clip(Cr, 0, 255)


def _round_div(n, d):
    """n / d to nearest, ties away from zero"""
    n = np.asarray(n, np.int64)
    return np.sign(n) * ((2 * np.abs(n) + d) // (2 * d))


def expand_luma(y):
    return np.clip(_round_div((np.asarray(y, np.int64) - 16) * 255, 219), 0, 255)


def expand_chroma(c):
    return np.clip(_round_div((np.asarray(c, np.int64) - 128) * 255, 224) + 128, 0, 255)


def planes_yuv(frame, pix_fmt):
    """uint8 [H * 3 // 2, W] NV12 / I420, BT.601 limited range -> full-range planes, padded by replicating each plane's last column and row"""
    W = frame.shape[1]
    H = frame.shape[0] * 2 // 3
    flat = np.asarray(frame).reshape(-1)
    Y = flat[:H * W].reshape(H, W)
    c = flat[H * W:]
    if pix_fmt == "nv12":
        uv = c.reshape(H // 2, W // 2, 2)
        U, V = uv[..., 0], uv[..., 1]
    else:
        U, V = c[:H * W // 4].reshape(H // 2, W // 2), c[H * W // 4:].reshape(H // 2, W // 2)
    mh, mw = -(-H // 16) * 16, -(-W // 16) * 16
    return (_pad_edge(expand_luma(Y), mh, mw), _pad_edge(expand_chroma(U), mh // 2, mw // 2), _pad_edge(expand_chroma(V), mh // 2, mw // 2))


def header(H, W, quality):
    """SOI .. SOS: everything before the scan"""
    ql, qc = quant_tables(quality)
    out = b"\xff\xd8" + b"\xff\xe0" + struct.pack(">H5sBBBHHBB", 16, b"JFIF\0", 1, 1, 0, 1, 1, 0, 0)
    for i, q in enumerate((ql, qc)):
        out += b"\xff\xdb" + struct.pack(">HB", 67, i) + bytes(int(v) for v in q[ZIGZAG])
    out += b"\xff\xc0" + struct.pack(">HBHHB", 17, 8, H, W, 3) + bytes([1, 0x22, 0, 2, 0x11, 1, 3, 0x11, 1])
    for tc_th, (bits, vals) in ((0x00, DC_LUMA), (0x10, AC_LUMA), (0x01, DC_CHROMA), (0x11, AC_CHROMA)):
        out += b"\xff\xc4" + struct.pack(">HB", 19 + len(vals), tc_th) + bytes(bits) + bytes(vals)
    out += b"\xff\xdd" + struct.pack(">HH", 4, -(-W // 16))
    out += b"\xff\xda" + struct.pack(">HB", 12, 3) + bytes([1, 0x00, 2, 0x11, 3, 0x11, 0, 63, 0])
    return out


def _category(v):
    return int(abs(int(v))).bit_length()


class BitWriter:
    def __init__(self):
        self.acc, self.n = 0, 0

    def put(self, code, length):
        self.acc = (self.acc << length) | (code & ((1 << length) - 1))
        self.n += length

    def flush(self):
        """(bytes padded with 1-bits to a byte boundary, number of bits before the padding)"""
        n = self.n
        pad = -n % 8
        acc = (self.acc << pad) | ((1 << pad) - 1)
        return acc.to_bytes((n + pad) // 8, "big"), n


def code_block(bw, zz, pred, dc_codes, ac_codes, symbols=None):
    """one block of 64 levels in zigzag order; returns its DC level (the next predictor)"""
    diff = int(zz[0]) - pred
    s = _category(diff)
    bw.put(*dc_codes[s])
    if s:
        bw.put(diff if diff > 0 else diff + (1 << s) - 1, s)
    if symbols is not None:
        symbols.append(("DC", s, diff))
    run = 0
    for k in range(1, 64):
        v = int(zz[k])
        if v == 0:
            run += 1
            continue
        while run >= 16:
            bw.put(*ac_codes[ZRL])
            if symbols is not None:
                symbols.append(("ZRL",))
            run -= 16
        s = _category(v)
        bw.put(*ac_codes[(run << 4) | s])
        bw.put(v if v > 0 else v + (1 << s) - 1, s)
        if symbols is not None:
            symbols.append(("AC", run, s, v))
        run = 0
    if run:
        bw.put(*ac_codes[EOB])
        if symbols is not None:
            symbols.append(("EOB",))
    return int(zz[0])


def levels(planes, quality):
    """(Y, Cb, Cr) planes -> zigzag levels: luma [2 MH, 2 MW, 64], chroma [MH, MW, 64] each"""
    ql, qc = quant_tables(quality)
    out = []
    for p, q in zip(planes, (ql, qc, qc)):
        h, w = p.shape
        blocks = (p - 128).reshape(h // 8, 8, w // 8, 8).transpose(0, 2, 1, 3)
        lv = quantise(fdct(blocks), q)
        out.append(lv.reshape(h // 8, w // 8, 64)[..., ZIGZAG])
    return out


def scan(lv, info=None):
    """the entropy-coded segment: one restart interval per MCU row.  info (a dict) receives `symbols`, the unstuffed bit length of
    every interval (`bits`) and the unstuffed bytes (`raw`)"""
    Yl, Cbl, Crl = lv
    MH, MW = Cbl.shape[:2]
    dcl, acl, dcc, acc = (huff_codes(t) for t in (DC_LUMA, AC_LUMA, DC_CHROMA, AC_CHROMA))
    symbols = [] if info is not None else None
    out, bits, raw = b"", [], []
    for i in range(MH):
        bw = BitWriter()
        py = pcb = pcr = 0
        for m in range(MW):
            for dy in (0, 1):
                for dx in (0, 1):
                    py = code_block(bw, Yl[2 * i + dy, 2 * m + dx], py, dcl, acl, symbols)
            pcb = code_block(bw, Cbl[i, m], pcb, dcc, acc, symbols)
            pcr = code_block(bw, Crl[i, m], pcr, dcc, acc, symbols)
        data, n = bw.flush()
        bits.append(n)
        raw.append(data)
        out += data.replace(b"\xff", b"\xff\x00")
        if i + 1 < MH:
            out += bytes([0xFF, 0xD0 + i % 8])
    if info is not None:
        info.update(symbols=symbols, bits=bits, raw=raw)
    return out


def encode(frame, quality=85, pix_fmt="rgb24", info=None):
    """one frame (uint8 [H, W, 3], or [H * 3 // 2, W] for nv12 / i420) -> the bytes of its JFIF file"""
    if pix_fmt == "rgb24":
        H, W = frame.shape[:2]
        planes = planes_rgb(frame)
    else:
        H, W = frame.shape[0] * 2 // 3, frame.shape[1]
        planes = planes_yuv(frame, pix_fmt)
    return header(H, W, quality) + scan(levels(planes, quality), info) + b"\xff\xd9"


def segments(jpeg):
    """[(marker, payload)] of the segments before the scan (SOI has no payload)"""
    assert jpeg[:2] == b"\xff\xd8"
    out, p = [(0xD8, b"")], 2
    while True:
        assert jpeg[p] == 0xFF, p
        m = jpeg[p + 1]
        n = struct.unpack(">H", jpeg[p + 2:p + 4])[0]
        out.append((m, jpeg[p + 4:p + 2 + n]))
        p += 2 + n
        if m == 0xDA:
            return out


def dqt_tables(jpeg):
    """{table id: natural-order list} from the DQT segments"""
    out = {}
    for m, payload in segments(jpeg):
        if m == 0xDB:
            nat = [0] * 64
            for k, v in enumerate(payload[1:65]):
                nat[ZIGZAG[k]] = v
            out[payload[0] & 15] = nat
    return out


def psnr(a, b):
    d = np.asarray(a, np.float64) - np.asarray(b, np.float64)
    return 10.0 * np.log10(255.0 ** 2 / max(float(np.mean(d * d)), 1e-12))


# ---- RIFF ----
def riff_walk(data, start=0, end=None):
    """[(fourcc, offset of the chunk header, payload size, children or None)]; LIST / RIFF chunks carry (list type, children)"""
    end = len(data) if end is None else end
    out, p = [], start
    while p + 8 <= end:
        cc, n = data[p:p + 4], struct.unpack("<I", data[p + 4:p + 8])[0]
        assert p + 8 + n <= end, (cc, p, n, end)
        kids = None
        if cc in (b"RIFF", b"LIST"):
            kids = (data[p + 8:p + 12], riff_walk(data, p + 12, p + 8 + n))
        out.append((cc, p, n, kids))
        p += 8 + n + (n & 1)
    assert p == end, (p, end)
    return out


def avi_parse(data):
    """dict: avih and strh fields of interest, frames = the 00dc payloads in movi order, idx = [(ckid, flags, offset, size)], movi = offset
    of the 'movi' fourcc"""
    top = riff_walk(data)
    assert len(top) == 1 and top[0][0] == b"RIFF" and top[0][3][0] == b"AVI " and top[0][2] + 8 == len(data)
    res = {"frames": [], "frame_offsets": []}
    for cc, p, n, kids in top[0][3][1]:
        if cc == b"LIST" and kids[0] == b"hdrl":
            for c2, p2, n2, k2 in kids[1]:
                if c2 == b"avih":
                    v = struct.unpack("<14I", data[p2 + 8:p2 + 64])
                    res["avih"] = {"us_per_frame": v[0], "flags": v[3], "total_frames": v[4], "streams": v[6], "width": v[8], "height": v[9]}
                if c2 == b"LIST" and k2[0] == b"strl":
                    for c3, p3, n3, _ in k2[1]:
                        if c3 == b"strh":
                            res["strh"] = {"type": data[p3 + 8:p3 + 12], "handler": data[p3 + 12:p3 + 16]}
                            res["strh"]["scale"], res["strh"]["rate"], _, res["strh"]["length"] = struct.unpack("<4I", data[p3 + 28:p3 + 44])
                        if c3 == b"strf":
                            v = struct.unpack("<IiiHH4sI", data[p3 + 8:p3 + 32])
                            res["strf"] = {"width": v[1], "height": v[2], "compression": v[5]}
        if cc == b"LIST" and kids[0] == b"movi":
            res["movi"] = p + 8
            for c2, p2, n2, _ in kids[1]:
                assert c2 == b"00dc", c2
                res["frames"].append(data[p2 + 8:p2 + 8 + n2])
                res["frame_offsets"].append(p2)
        if cc == b"idx1":
            res["idx"] = [struct.unpack("<4sIII", data[p + 8 + 16 * k:p + 24 + 16 * k]) for k in range(n // 16)]
    return res
