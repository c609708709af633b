"""The MJPEG import's reconstruction contract (include/vbt_hip.h, "MJPEG import") in numpy and plain Python: test infrastructure only,
written from the contract's text and the published algorithms (ITU-T T.81; the IJG "islow" IDCT, "fancy" upsampling and YCbCr tables).
decode() gives the RGB24 frame of one baseline JPEG file; parse() the header descriptor, or raises Refused with the reason.  Does
not import the package under test."""
import functools
import io
import struct

import numpy as np

from mjpeg_ref import AC_CHROMA, AC_LUMA, DC_CHROMA, DC_LUMA, ZIGZAG

STD_TABLES = {(0, 0): DC_LUMA, (0, 1): DC_CHROMA, (1, 0): AC_LUMA, (1, 1): AC_CHROMA}       # (class, id): the tables of a frame without DHT
MAX_SIDE = 16384

# scan status codes (vbt_mjpeg_decode_status)
ST_OVERRUN, ST_BAD_CODE, ST_BAD_INDEX, ST_RST_COUNT, ST_RST_ORDER = 1, 2, 3, 4, 5


class Refused(ValueError):
    pass


def _u16(b, p):
    return (b[p] << 8) | b[p + 1]


def parse(jpeg, size=None):
    """bytes -> descriptor dict: H, W, comps [(h, v, tq, td, ta)], q {id: natural-order int64[64]}, huff {(class, id): (bits, vals)},
    ri, scan (offset, length).  size = (H, W): the size the frame must have."""
    b = bytes(jpeg)
    n = len(b)
    if n < 4 or b[0] != 0xFF or b[1] != 0xD8:
        raise Refused("no SOI marker")
    p, q, huff, sof, ri, any_dht = 2, {}, {}, None, 0, False
    while True:
        if p + 2 > n:
            raise Refused("missing SOS: the data ends in the headers")
        if b[p] != 0xFF:
            raise Refused(f"byte {p}: 0x{b[p]:02x} where a marker should start")
        while p + 1 < n and b[p + 1] == 0xFF:
            p += 1                                                          # fill bytes
        if p + 2 > n:
            raise Refused("missing SOS: the data ends in the headers")
        m = b[p + 1]
        p += 2
        if m == 0xD8 or m == 0x01 or 0xD0 <= m <= 0xD7:
            continue
        if m == 0xD9:
            raise Refused("missing SOS: EOI before any scan")
        if p + 2 > n:
            raise Refused(f"segment length past the end: marker 0x{m:02x} at byte {p - 2}")
        L = _u16(b, p)
        if L < 2 or p + L > n:
            raise Refused(f"segment length past the end: marker 0x{m:02x} at byte {p - 2} says {L} bytes, {n - p} are left")
        s, e = p + 2, p + L
        if m == 0xDB:
            while s < e:
                pq, tq = b[s] >> 4, b[s] & 15
                if pq != 0:
                    raise Refused("16-bit DQT (8-bit tables only)")
                if tq > 3 or s + 65 > e:
                    raise Refused("malformed DQT")
                t = np.zeros(64, np.int64)
                t[ZIGZAG] = np.frombuffer(b[s + 1:s + 65], np.uint8)
                q[tq] = t
                s += 65
        elif m == 0xC4:
            while s < e:
                if s + 17 > e:
                    raise Refused("malformed DHT")
                tc, th = b[s] >> 4, b[s] & 15
                bits = list(b[s + 1:s + 17])
                cnt = sum(bits)
                if tc > 1 or th > 1 or cnt > 256 or s + 17 + cnt > e:
                    raise Refused("malformed DHT (class 0-1, id 0-1, at most 256 symbols)")
                code = 0
                for length in range(1, 17):
                    code += bits[length - 1]
                    if code > (1 << length):
                        raise Refused("malformed DHT (more codes than a length holds)")
                    code <<= 1
                huff[(tc, th)] = (bits, list(b[s + 17:s + 17 + cnt]))
                any_dht = True
                s += 17 + cnt
        elif m == 0xC0:
            if sof is not None:
                raise Refused("two SOF segments")
            if L < 8:
                raise Refused("malformed SOF0")
            prec, H, W, nc = b[s], _u16(b, s + 1), _u16(b, s + 3), b[s + 5]
            if prec != 8:
                raise Refused(f"{prec}-bit precision (8-bit only)")
            if nc not in (1, 3) or L != 8 + 3 * nc:
                raise Refused(f"{nc} components (1 or 3)")
            if not (1 <= H <= MAX_SIDE and 1 <= W <= MAX_SIDE):
                raise Refused(f"size {W}x{H} outside 1..{MAX_SIDE}")
            sof = (H, W, [(b[s + 6 + 3 * i], b[s + 7 + 3 * i] >> 4, b[s + 7 + 3 * i] & 15, b[s + 8 + 3 * i]) for i in range(nc)])
        elif 0xC1 <= m <= 0xCF and m not in (0xC4, 0xC8, 0xCC):
            kind = {0xC1: "extended sequential", 0xC2: "progressive"}.get(m, "arithmetic" if m >= 0xC9 else "lossless" if m in (0xC3, 0xC7, 0xCB) else "hierarchical")
            raise Refused(f"SOF{m - 0xC0} ({kind}): baseline SOF0 only")
        elif m == 0xDD:
            if L != 4:
                raise Refused("malformed DRI")
            ri = _u16(b, s)
        elif m == 0xEE:
            if L >= 14 and b[s:s + 5] == b"Adobe" and b[s + 11] != 1:
                raise Refused(f"Adobe APP14 transform {b[s + 11]} (YCbCr only)")
        elif m == 0xDA:
            if sof is None:
                raise Refused("missing SOF before SOS")
            H, W, comps = sof
            nc = len(comps)
            if L != 6 + 2 * nc or b[s] != nc:
                raise Refused("more than one scan (the scan does not hold all components)")
            out = []
            for i, (cid, h, v, tq) in enumerate(comps):
                if b[s + 1 + 2 * i] != cid:
                    raise Refused("the scan's components are not the frame's")
                td, ta = b[s + 2 + 2 * i] >> 4, b[s + 2 + 2 * i] & 15
                if td > 1 or ta > 1:
                    raise Refused("Huffman table id above 1")
                if tq not in q:
                    raise Refused(f"missing DQT: table {tq}")
                out.append((h, v, tq, td, ta))
            if (b[s + 1 + 2 * nc], b[s + 2 + 2 * nc], b[s + 3 + 2 * nc]) != (0, 63, 0):
                raise Refused("the scan is not Ss 0, Se 63, Ah/Al 0 (progressive?)")
            if nc == 1:
                out[0] = (1, 1) + out[0][2:]
            elif (out[0][:2] not in ((1, 1), (2, 1), (2, 2))) or out[1][:2] != (1, 1) or out[2][:2] != (1, 1):
                raise Refused("sampling " + ",".join(f"{h}x{v}" for h, v, *_ in out) + " (4:4:4, 4:2:2, 4:2:0 only)")
            if not any_dht:
                huff = dict(STD_TABLES)
            for _, _, _, td, ta in out:
                if (0, td) not in huff or (1, ta) not in huff:
                    raise Refused("missing DHT: a table the scan names")
            if size is not None and (H, W) != tuple(size):
                raise Refused(f"size {W}x{H}, the handle is for {size[1]}x{size[0]}")
            start = e
            k = start
            while k < n:
                if b[k] == 0xFF and k + 1 < n and b[k + 1] != 0 and b[k + 1] != 0xFF and not 0xD0 <= b[k + 1] <= 0xD7:
                    break
                if b[k] == 0xFF and k + 1 >= n:
                    break
                k += 1
            end = k
            while k + 1 < n:                                                 # behind the scan: nothing but EOI is expected
                if b[k] != 0xFF:
                    break
                if b[k + 1] == 0xFF:
                    k += 1
                    continue
                if b[k + 1] == 0xD9:
                    break
                if b[k + 1] == 0xDA or 0xC0 <= b[k + 1] <= 0xCF or b[k + 1] in (0xDB, 0xDD):
                    raise Refused("more than one scan")
                if k + 4 > n:
                    break
                k += 2 + _u16(b, k + 2)
            return {"H": H, "W": W, "comps": out, "q": q, "huff": huff, "ri": ri, "scan": (start, end - start)}
        p = e


# ---- entropy decoding ----
class _Bits:
    def __init__(self, data):
        self.d, self.p, self.acc, self.n, self.over = data, 0, 0, 0, False

    def get(self, k):
        while self.n < k:
            if self.p < len(self.d):
                v = self.d[self.p]
                self.p += 1
                if v == 0xFF:
                    if self.p < len(self.d) and self.d[self.p] == 0:
                        self.p += 1
                    else:
                        self.p = len(self.d)
                        self.over = True
                        return None
            else:
                self.over = True
                return None
            self.acc = ((self.acc << 8) | v) & 0xFFFFFFFFFF
            self.n += 8
        self.n -= k
        return (self.acc >> self.n) & ((1 << k) - 1)


def _decoder(spec):
    bits, vals = spec
    out, code, k = {}, 0, 0
    for length in range(1, 17):
        for _ in range(bits[length - 1]):
            out[(length, code)] = vals[k]
            code += 1
            k += 1
        code <<= 1
    return out


def _symbol(br, tab):
    code = 0
    for length in range(1, 17):
        bit = br.get(1)
        if bit is None:
            return None, ST_OVERRUN
        code = (code << 1) | bit
        if (length, code) in tab:
            return tab[(length, code)], 0
    return None, ST_BAD_CODE


def _extend(r, s):
    return r - (1 << s) + 1 if r < (1 << (s - 1)) else r


def _block(br, dc, ac, pred, out):
    """one block into out[64] (natural order); returns (new predictor, status)"""
    s, st = _symbol(br, dc)
    if st:
        return pred, st
    if s > 16:
        return pred, ST_BAD_CODE
    if s:
        r = br.get(s)
        if r is None:
            return pred, ST_OVERRUN
        pred += _extend(r, s)
    out[0] = pred
    k = 1
    while k < 64:
        rs, st = _symbol(br, ac)
        if st:
            return pred, st
        r, s = rs >> 4, rs & 15
        if s:
            k += r
            if k > 63:
                return pred, ST_BAD_INDEX
            v = br.get(s)
            if v is None:
                return pred, ST_OVERRUN
            out[ZIGZAG[k]] = _extend(v, s)
            k += 1
        elif r == 15:
            k += 16
        else:
            break
    return pred, 0


def intervals(scan):
    """[(start, end, m)] of the scan's restart intervals: m = the RSTm that ends the interval, None for the last"""
    out, start = [], 0
    for i in range(len(scan) - 1):
        if scan[i] == 0xFF and 0xD0 <= scan[i + 1] <= 0xD7:
            out.append((start, i, scan[i + 1] & 7))
            start = i + 2
    out.append((start, len(scan), None))
    return out


def levels(d, scan):
    """-> ([per component: int64 [block rows, block columns, 64] natural order], status)"""
    comps = d["comps"]
    hmax, vmax = comps[0][0], comps[0][1]
    MW, MH = -(-d["W"] // (8 * hmax)), -(-d["H"] // (8 * vmax))
    lv = [np.zeros((MH * v, MW * h, 64), np.int64) for h, v, *_ in comps]
    mcus = MW * MH
    ri = d["ri"] or mcus
    n_int = -(-mcus // ri)
    iv = intervals(scan)
    if len(iv) != n_int:
        return lv, ST_RST_COUNT
    if any(m != k % 8 for k, (_, _, m) in enumerate(iv[:-1])):
        return lv, ST_RST_ORDER
    tabs = {k: _decoder(v) for k, v in d["huff"].items()}
    status = 0
    for k, (s, e, _) in enumerate(iv):
        br = _Bits(scan[s:e])
        pred = [0] * len(comps)
        st = 0
        for m in range(k * ri, min((k + 1) * ri, mcus)):
            my, mx = divmod(m, MW)
            for c, (h, v, _, td, ta) in enumerate(comps):
                for by in range(v):
                    for bx in range(h):
                        pred[c], st = _block(br, tabs[(0, td)], tabs[(1, ta)], pred[c], lv[c][my * v + by, mx * h + bx])
                        if st:
                            break
                    if st:
                        break
                if st:
                    break
            if st:
                break
        status = max(status, st)
    return lv, status


# ---- reconstruction ----
_F = dict(f0_298=2446, f0_390=3196, f0_541=4433, f0_765=6270, f0_899=7373, f1_175=9633, f1_501=12299, f1_847=15137, f1_961=16069, f2_053=16819,
          f2_562=20995, f3_072=25172)


def _pass(x, shift):
    """the islow butterfly along the first axis of x [8, ...]; the results descaled by `shift` bits"""
    z1 = (x[2] + x[6]) * _F["f0_541"]
    t2 = z1 - x[6] * _F["f1_847"]
    t3 = z1 + x[2] * _F["f0_765"]
    t0 = (x[0] + x[4]) << 13
    t1 = (x[0] - x[4]) << 13
    t10, t13, t11, t12 = t0 + t3, t0 - t3, t1 + t2, t1 - t2
    a0, a1, a2, a3 = x[7], x[5], x[3], x[1]
    z1, z2, z3, z4 = a0 + a3, a1 + a2, a0 + a2, a1 + a3
    z5 = (z3 + z4) * _F["f1_175"]
    a0, a1, a2, a3 = a0 * _F["f0_298"], a1 * _F["f2_053"], a2 * _F["f3_072"], a3 * _F["f1_501"]
    z1, z2, z3, z4 = -z1 * _F["f0_899"], -z2 * _F["f2_562"], -z3 * _F["f1_961"] + z5, -z4 * _F["f0_390"] + z5
    a0, a1, a2, a3 = a0 + z1 + z3, a1 + z2 + z4, a2 + z2 + z3, a3 + z1 + z4
    r = 1 << (shift - 1)
    return np.stack([t10 + a3, t11 + a2, t12 + a1, t13 + a0, t13 - a0, t12 - a1, t11 - a2, t10 - a3]) + r >> shift


def idct(lv, q):
    """levels [..., 64] natural order, q [64] -> samples uint8 [..., 8, 8]"""
    x = (np.asarray(lv, np.int64) * np.asarray(q, np.int64)).reshape(lv.shape[:-1] + (8, 8))
    ws = _pass(np.moveaxis(x, -2, 0), 11)                         # pass 1 over columns: [v, ..., u] -> [y, ..., u]
    out = _pass(np.moveaxis(ws, -1, 0), 18)                       # pass 2 over rows: [u, y, ...] -> [x, y, ...]
    out = np.moveaxis(out, (0, 1), (-1, -2))
    return np.clip(out + 128, 0, 255).astype(np.uint8)


def plane(lv, q):
    """block levels [bh, bw, 64] -> the component's samples [8 bh, 8 bw]"""
    s = idct(lv, q)
    bh, bw = s.shape[:2]
    return s.transpose(0, 2, 1, 3).reshape(bh * 8, bw * 8)


def upsample_h2v1(c, dw, W):
    """c [rows, >= dw] -> [rows, W]: the triangle filter; a component of one or two columns is replicated"""
    c = c[:, :dw].astype(np.int64)
    if dw <= 2:
        return np.repeat(c, 2, axis=1)[:, :W]
    left = np.concatenate([c[:, :1], c[:, :-1]], axis=1)
    right = np.concatenate([c[:, 1:], c[:, -1:]], axis=1)
    out = np.empty((c.shape[0], 2 * dw), np.int64)
    out[:, 0::2] = (3 * c + left + 1) >> 2
    out[:, 1::2] = (3 * c + right + 2) >> 2
    out[:, 0], out[:, -1] = c[:, 0], c[:, -1]
    return out[:, :W]


def upsample_h2v2(c, dh, dw, H, W):
    c = c[:dh, :dw].astype(np.int64)
    if dw <= 2:
        return np.repeat(np.repeat(c, 2, axis=0), 2, axis=1)[:H, :W]
    up = np.concatenate([c[:1], c[:-1]], axis=0)
    down = np.concatenate([c[1:], c[-1:]], axis=0)
    out = np.empty((2 * dh, 2 * dw), np.int64)
    for par, other in ((0, up), (1, down)):
        s = 3 * c + other                                         # the column sums of this output row
        left = np.concatenate([s[:, :1], s[:, :-1]], axis=1)
        right = np.concatenate([s[:, 1:], s[:, -1:]], axis=1)
        row = np.empty((dh, 2 * dw), np.int64)
        row[:, 0::2] = (3 * s + left + 8) >> 4
        row[:, 1::2] = (3 * s + right + 7) >> 4
        row[:, 0], row[:, -1] = (4 * s[:, 0] + 8) >> 4, (4 * s[:, -1] + 7) >> 4
        out[par::2] = row
    return out[:H, :W]


def ycc_to_rgb(y, cb, cr):
    y, cb, cr = (np.asarray(v, np.int64) for v in (y, cb - 128, cr - 128))
    r = y + ((91881 * cr + 32768) >> 16)
    g = y + ((-22554 * cb - 46802 * cr + 32768) >> 16)
    b = y + ((116130 * cb + 32768) >> 16)
    return np.clip(np.stack([r, g, b], axis=-1), 0, 255).astype(np.uint8)


def reconstruct(d, lv):
    H, W, comps = d["H"], d["W"], d["comps"]
    planes = [plane(lv[c], d["q"][comps[c][2]]) for c in range(len(comps))]
    y = planes[0][:H, :W]
    if len(comps) == 1:
        return np.repeat(y[..., None], 3, axis=-1)
    h, v = comps[0][:2]
    dw, dh = -(-W // h), -(-H // v)
    if (h, v) == (1, 1):
        cb, cr = (p[:H, :W].astype(np.int64) for p in planes[1:])
    elif (h, v) == (2, 1):
        cb, cr = (upsample_h2v1(p[:H], dw, W) for p in planes[1:])
    else:
        cb, cr = (upsample_h2v2(p, dh, dw, H, W) for p in planes[1:])
    return ycc_to_rgb(y, cb, cr)


def decode(jpeg, size=None, with_status=False):
    d = parse(jpeg, size)
    s, n = d["scan"]
    lv, status = levels(d, bytes(jpeg)[s:s + n])
    img = reconstruct(d, lv)
    return (img, status) if with_status else img


def strip_dht(jpeg):
    """the same file without its DHT segments"""
    b, p, out = bytes(jpeg), 2, bytes(jpeg)[:2]
    while True:
        m, L = b[p + 1], _u16(b, p + 2)
        if m != 0xC4:
            out += b[p:p + 2 + L]
        p += 2 + L
        if m == 0xDA:
            return out + b[p:]


def damaged_frame(jpeg):
    """the same file cut inside its last restart interval and padded to its old length with zeros"""
    d = parse(jpeg)
    s, n = d["scan"]
    last = intervals(jpeg[s:s + n])[-1]
    cut = s + last[0] + (last[1] - last[0]) // 3
    return jpeg[:cut] + bytes(len(jpeg) - cut)


# ---- RIFF ----
def build_avi(chunks, W, H, rate=30, scale=1, idx1=False):
    """a minimal AVI: chunks = [(fourcc, payload)] inside movi"""
    strh = struct.pack("<4s4sIHHIIIIIIiI4h", b"vids", b"MJPG", 0, 0, 0, 0, scale, rate, 0, len(chunks), 0, -1, 0, 0, 0, W, H)
    strf = struct.pack("<IiiHH4sIiiII", 40, W, H, 1, 24, b"MJPG", W * H * 3, 0, 0, 0, 0)
    avih = struct.pack("<14I", 1000000 * scale // rate, 0, 0, 0x10 if idx1 else 0, len(chunks), 0, 1, 0, W, H, 0, 0, 0, 0)
    strl = b"strl" + b"strh" + struct.pack("<I", len(strh)) + strh + b"strf" + struct.pack("<I", len(strf)) + strf
    hdrl = b"hdrl" + b"avih" + struct.pack("<I", len(avih)) + avih + b"LIST" + struct.pack("<I", len(strl)) + strl
    movi, index = b"movi", b""
    for cc, data in chunks:
        index += struct.pack("<4sIII", cc, 0x10, len(movi), len(data))
        movi += cc + struct.pack("<I", len(data)) + data + (b"\0" if len(data) & 1 else b"")
    body = b"AVI " + b"LIST" + struct.pack("<I", len(hdrl)) + hdrl + b"LIST" + struct.pack("<I", len(movi)) + movi
    if idx1:
        body += b"idx1" + struct.pack("<I", len(index)) + index
    return b"RIFF" + struct.pack("<I", len(body)) + body


# ---- the test vectors: this project's encoder (mjpeg_ref.encode) and Pillow at test time; nothing is stored ----
def noise(shape, seed):
    return np.random.default_rng(seed).integers(0, 256, shape, dtype=np.uint8)


def smooth(H, W, seed):
    """gradients and products under half-amplitude noise: long and short blocks side by side"""
    y, x = np.mgrid[:H, :W]
    base = np.stack([(x * 5 + y * 3) % 256, (x * y) % 256, (255 - x * 2 - y) % 256], -1).astype(np.uint8)
    return base // 2 + noise((H, W, 3), seed) // 2


def pil_jpeg(img, **kw):
    from PIL import Image
    b = io.BytesIO()
    Image.fromarray(img).save(b, "JPEG", **kw)
    return b.getvalue()


def pil_decode(jpeg):
    from PIL import Image
    return np.asarray(Image.open(io.BytesIO(jpeg)).convert("RGB"))


def fnv1a(a):
    h = 2166136261
    for v in np.asarray(a, np.uint8).reshape(-1).tolist():
        h = ((h ^ v) * 16777619) & 0xFFFFFFFF
    return h


def extremes_frame():
    """32 x 48 noise with a 0 / 255 checkerboard block: the largest coefficients"""
    f = noise((32, 48, 3), 14)
    f[:8, :8] = (np.indices((8, 8)).sum(0) & 1)[..., None] * 255
    return f


def long_frame():
    f = noise((16, 2064, 3), 12)
    f[:, 700:1500] = (np.arange(800)[None, :, None] // 4).astype(np.uint8)
    return f


@functools.lru_cache(maxsize=None)
def vectors():
    """name -> the bytes of one JPEG file"""
    from mjpeg_ref import encode
    v = {f"own-{h}x{w}": encode(noise((h, w, 3), s), 85) for h, w, s in ((16, 16, 1), (1, 1, 3), (17, 33, 2))}
    v["pil-24x40-444"] = pil_jpeg(smooth(24, 40, 1), quality=85, subsampling=0)
    v["pil-17x33-422"] = pil_jpeg(smooth(17, 33, 2), quality=85, subsampling=1)
    v["pil-9x23-grey"] = pil_jpeg(smooth(9, 23, 3)[..., 0], quality=85)
    v["pil-40x56-420-optimize"] = pil_jpeg(smooth(40, 56, 4), quality=85, subsampling=2, optimize=True)
    v["pil-40x56-no-restarts"] = pil_jpeg(smooth(40, 56, 4), quality=85, subsampling=2)
    v["pil-40x56-restart-rows-1"] = pil_jpeg(smooth(40, 56, 4), quality=85, subsampling=2, restart_marker_rows=1)
    v["pil-40x56-restart-blocks-1"] = pil_jpeg(smooth(40, 56, 4), quality=85, subsampling=2, restart_marker_blocks=1)
    v["own-160x32-noise-q95"] = encode(noise((160, 32, 3), 11), 95)
    v["own-16x2064-one-interval"] = encode(long_frame(), 85)
    v["own-32x48-q1"] = encode(extremes_frame(), 1)
    v["own-32x48-q100"] = encode(extremes_frame(), 100)
    v["own-17x33-no-dht"] = strip_dht(v["own-17x33"])
    return v


@functools.lru_cache(maxsize=None)
def expected(name):
    """the numpy statement's frame of vectors()[name]; computed once, shared by the tests, read-only"""
    img = decode(vectors()[name])
    img.setflags(write=False)
    return img
