"""Test infrastructure: crafted int8 tensors for running single plan steps (tests/test_gpu_steps_alone.py), and what they are meant to
reach (asserted on the numpy reference alone by tests/test_graph_ref_host.py).

A pattern is a deterministic function of (tensor id, shape, pattern, image, seed); the images of a batch always differ.  The graph input
takes the same patterns as uint8 (value + 128: what QUANTIZE makes of a frame).

  U  uniform random bytes over the whole int8 range, whatever range the producer could reach, with +127 and -128 each placed once per
     image at a seeded position (a 972-byte tensor would otherwise miss a rail in one case out of forty).
  S  rails: image 0 all +127, image 1 all -128, image 2 a one-element checkerboard of the two over (y + x + c).
  X  extremes aligned with the tensor's consumer.  A tensor read by several ops takes the pattern of its FIRST consumer in op order;
     the later consumers of such a tensor (the second lateral conv on a backbone level, the residual ADD behind an expand conv) see
     that pattern, not one of their own - `first_consumer` says which op a tensor serves.
       pointwise conv   pixel p of image b carries target g = p + b * H * W: channel g mod N with x = +127 where that channel's weight
                        is positive and -128 elsewhere (the accumulator's attainable maximum) for g mod 2N < N, the inverse (its
                        minimum) otherwise.  (An image that would start on the target an earlier one started on starts 5 further on.)
       depthwise, stem  the map is tiled with period P = stride * ceil(k / stride) from the first window that lies wholly inside it, so
                        that every P / stride-th output reads exactly one tile.  Depthwise: every channel of a tile carries the signs of
                        its own k x k weights, inverted on every other tile and image (image 2, which shares image 0's polarity, is
                        moved sideways by one stride).  Stem: tile t of image b targets output channel (t + b * tiles) mod N, then
                        the inverted set, as above.
       ADD, resamples   (also tensors only the post-process reads).  Channels c = 0 (mod 32) hold +127 and c = 1 (mod 32) hold -128 at
                        every pixel - a constant channel survives the max pools and resizes of a BiFPN node, so all sources of a sum
                        meet on one rail there and a 3-input sum saturates its partial sum at each rail wherever its parameters let any
                        pair do so.  The other elements, in (image, y, x, c) order, take one byte of a sequence of (a, b) pairs seeded
                        by the ADD they serve: input 0 the a byte, input 1 the b byte.  With 65 536 or more such elements in the
                        batch the sequence opens with a permutation of the whole 256 x 256 grid; otherwise with the 16 pairs of
                        {-128, -127, 126, 127}^2; then random pairs.  Two inputs of one ADD that both serve it therefore meet in
                        every pair of the grid.
"""
import numpy as np

from graph_ref import CONVS, OP_ADD, OP_DW, OP_MAXPOOL, OP_PW, OP_RESIZE_NN, OP_STEM

PATTERNS = ("U", "S", "X")
NEAR_RAILS = (-128, -127, 126, 127)
GRID = 65536


def write_clamped(src, dst):
    """The explicit-clamp container the kernel-family tests share as their `clamped` fixture: two thirds of the convs of `src` get an
    activation range narrower than int8."""
    from vbt_amd.container import Container
    raw = bytearray(open(src, "rb").read())
    c = Container(src)
    ops = np.frombuffer(raw, dtype=c.ops.dtype, count=len(c.ops), offset=128 + 32 * len(c.tensors))
    n = 0
    for i, r in enumerate(ops):
        if int(r["type"]) in (1, 2, 3) and i % 3 != 0:
            r["act_min"], r["act_max"] = max(int(r["act_min"]), -101 + i % 7), min(int(r["act_max"]), 96 - i % 5)
            n += 1
    assert n > 100
    open(dst, "wb").write(bytes(raw))
    return dst


KB_LIMIT = 2 ** 22 - 1          # the library's proof: 255 * sum |w| + |b| < KB_LIMIT on every channel (planner.hip: conv_kb)
KB_CHANNELS = (2, 3)            # the channels write_kb_edge rewrites: + 2^22 and - 2^22


def mbconv_blocks(g):
    """(expand, depthwise, project) op triples: a pointwise conv whose output only a depthwise conv reads, whose output only a pointwise
    conv reads"""
    out = []
    for e in range(g.n_ops - 2):
        d, p = e + 1, e + 2
        if (g.type(e), g.type(d), g.type(p)) == (OP_PW, OP_DW, OP_PW) and g.readers.get(g.output(e)) == [d] and g.readers.get(g.output(d)) == [p]:
            out.append((e, d, p))
    return out


def write_kb_edge(src, dst):
    """A container whose accumulators run at the edge of the range the library's RQ_KBIAS proof covers.  In every MBConv block whose
    inner tensors have zero point -128 (x - z spans 0..255), channels KB_CHANNELS of (the depthwise and the project conv only where
    the conv passes the proof as it is - a conv that fails it takes the converting flavour anyway)
      the depthwise conv  get weights +127 / -127 on the whole window and a bias that brings 255 * sum |w| + |b| to 2^22 - 2,
      the project conv    get +127 / -127 on as many inputs as 255 * sum |w| stays below the limit, the rest of it as bias,
      the expand conv     get weights +64, bias 0 and multiplier 1.0, so that all-high inputs (S, image 0) saturate them to +127 and
                          the depthwise channels behind them run at both edges INSIDE the fused kernels too.
    The edge channels' multipliers are 60 / 2^22, so that an accumulator at the edge requantises to about +-60 and a wrong one shows.
    -> (dst, {blocks: the (expand, depthwise, project) triples touched, dw / pw: the depthwise / project convs rewritten})"""
    import graph_ref
    from vbt_amd.container import Container
    g = graph_ref.GraphRef(src)
    raw = bytearray(open(src, "rb").read())
    c = Container(src)
    bo = int(c.header["blob_offset"])
    view = lambda dt, off, n: np.frombuffer(raw, dtype=dt, count=n, offset=bo + int(off))
    c0, c1 = KB_CHANNELS
    edge_mult = np.float32(60.0 / 2 ** 22)
    edge = {"blocks": [], "dw": [], "pw": []}
    for e, d, p in mbconv_blocks(g):
        proven = [bool(np.all(kb_bound(g, o) < KB_LIMIT)) for o in (e, d, p)]
        if g.zero_point(g.output(e)) != -128 or g.zero_point(g.output(d)) != -128:
            continue
        re_, rd, rp = c.ops[e], c.ops[d], c.ops[p]
        K, C, N = g.shape(g.inputs(e)[0])[2], g.shape(g.output(d))[2], g.shape(g.output(p))[2]
        k = int(rd["k"])
        if 255 * 64 * K >= KB_LIMIT or min(C, N) <= c1:
            continue
        if proven[1]:
            edge["dw"].append(d)
        if proven[2]:
            edge["pw"].append(p)
        we, be, me = view(np.int8, re_["w_off"], C * K).reshape(C, K), view("<i4", re_["b_off"], C), view("<f4", re_["m_off"], C)
        we[[c0, c1]], be[[c0, c1]], me[[c0, c1]] = 64, 0, 1.0
        wd, bd, md = view(np.int8, rd["w_off"], k * k * C).reshape(k, k, C), view("<i4", rd["b_off"], C), view("<f4", rd["m_off"], C)
        fill = KB_LIMIT - 1 - 255 * 127 * k * k
        if proven[1]:
            wd[:, :, c0], wd[:, :, c1], bd[c0], bd[c1], md[[c0, c1]] = 127, -127, fill, -fill, edge_mult
        wp, bp, mp = view(np.int8, rp["w_off"], N * C).reshape(N, C), view("<i4", rp["b_off"], N), view("<f4", rp["m_off"], N)
        total = min((KB_LIMIT - 1) // 255, 127 * C)
        row = np.zeros(C, np.int64)
        row[:total // 127] = 127
        if total // 127 < C:
            row[total // 127] = total % 127
        fill = KB_LIMIT - 1 - 255 * int(row.sum())
        if proven[2]:
            wp[c0], wp[c1], bp[c0], bp[c1], mp[[c0, c1]] = row, -row, fill, -fill, edge_mult
        edge["blocks"].append((e, d, p))
    assert len(edge["dw"]) >= 8 and len(edge["pw"]) >= 5, edge
    open(dst, "wb").write(bytes(raw))
    return dst, edge


def tiling(h, w, k, s, pad_t, pad_l):
    """The X tiling of an [h, w] map under a k x k / s window: per input row (column) the window row it plays (k and above: between
    tiles) and the tile it belongs to (-1: in front of the first), the period, and the number of whole tiles per axis."""
    P = s * -(-k // s)

    def axis(n, pad):
        base = -(-pad // s) * s - pad                  # input row of the first window that needs no leading padding
        i = np.arange(n)
        rel = (i - base) % P
        tile = (i - base) // P
        n_tiles = 0 if n - base < k else (n - base - k) // P + 1
        tile = np.where((tile >= 0) & (tile < n_tiles), tile, -1)
        return rel, tile, n_tiles
    ry, ty, ny = axis(h, pad_t)
    rx, tx, nx = axis(w, pad_l)
    return ry, ty, ny, rx, tx, nx


def _image_offsets(B, per_image, period):
    """First target of every image: b * per_image, moved on by 5 until no earlier image starts on the same target modulo the period (the
    images in between have then been round the whole period, so nothing is lost) - the images of a batch always differ."""
    offs = []
    for b in range(B):
        o = b * per_image
        while any((o - p) % period == 0 for p in offs):
            o += 5
        offs.append(o)
    return np.asarray(offs)


class Cases:
    def __init__(self, g, B, seed=0):
        self.g, self.B, self.seed = g, int(B), int(seed)
        self._memo = {}

    def first_consumer(self, tid):
        r = self.g.readers.get(tid)
        return r[0] if r else None

    def serves_add(self, tid):
        """(ADD op, input slot) the tensor's X pattern is built for: its first consumer if that is an ADD, the first ADD behind a chain
        of first-consumer resamples otherwise; (None, 0) if neither."""
        g = self.g
        t = tid
        while True:
            oi = self.first_consumer(t)
            if oi is None:
                return None, 0
            ty = g.type(oi)
            if ty == OP_ADD:
                return oi, g.inputs(oi).index(t)
            if ty not in (OP_MAXPOOL, OP_RESIZE_NN):
                return None, 0
            t = g.output(oi)

    def usable(self, oi):
        """extreme accumulators the X pattern of conv `oi`'s input can hold: one per pixel (pointwise), one per whole tile (stem), both
        extremes of every channel per tile polarity present (depthwise)"""
        g = self.g
        h, w, _ = g.shape(g.inputs(oi)[0])
        r = g.ops[oi]
        if g.type(oi) == OP_PW:
            return self.B * h * w
        _, _, ny, _, _, nx = tiling(h, w, int(r["k"]), int(r["stride"]), int(r["pad_t"]), int(r["pad_l"]))
        if g.type(oi) == OP_STEM:
            return self.B * ny * nx
        N = g.shape(g.output(oi))[2]
        pol = {(b + jy + jx) & 1 for b in range(self.B) for jy in range(ny) for jx in range(nx)}
        return N * len(pol)

    def tensor(self, tid, pattern):
        """int8 [B,h,w,c] (the graph input: uint8); the same array on every call - do not write into it"""
        key = (tid, pattern)
        if key not in self._memo:
            a = {"U": self._uniform, "S": self._rails, "X": self._extremes}[pattern](tid)
            assert a.dtype == np.int8 and a.shape == (self.B,) + self.g.shape(tid)
            if tid == self.g.input_tensor:
                a = (a.astype(np.int16) + 128).astype(np.uint8)
            a.setflags(write=False)
            self._memo[key] = a
        return self._memo[key]

    def _rng(self, *key):
        return np.random.default_rng([self.seed, *[int(k) for k in key]])

    def _uniform(self, tid):
        shp = self.g.shape(tid)
        out = np.empty((self.B,) + shp, np.int8)
        for b in range(self.B):
            rng = self._rng(1, tid, b)
            img = rng.integers(-128, 128, shp, dtype=np.int8).reshape(-1)
            hi, lo = rng.choice(img.size, 2, replace=False)
            img[hi], img[lo] = 127, -128
            out[b] = img.reshape(shp)
        return out

    def _rails(self, tid):
        h, w, c = self.g.shape(tid)
        chk = (np.add.outer(np.add.outer(np.arange(h), np.arange(w)), np.arange(c)) & 1).astype(bool)
        imgs = [np.full((h, w, c), 127, np.int8), np.full((h, w, c), -128, np.int8), np.where(chk, np.int8(-128), np.int8(127))]
        return np.stack([imgs[b % 3] if b < 3 else np.where(chk, np.int8(127), np.int8(-128)) for b in range(self.B)])

    def _extremes(self, tid):
        g = self.g
        oi = self.first_consumer(tid)
        ty = g.type(oi) if oi is not None else None
        h, w, c = g.shape(tid)
        B = self.B
        if ty == OP_PW:
            wt = g.conv_params(oi)[0]                         # [N, K]
            N = wt.shape[0]
            tgt = ((np.arange(h * w)[None, :] + _image_offsets(B, h * w, 2 * N)[:, None]) % (2 * N)).reshape(-1)
            pos = (wt > 0)[tgt % N] ^ (tgt >= N)[:, None]
            return np.where(pos, np.int8(127), np.int8(-128)).reshape(B, h, w, c)
        if ty in (OP_DW, OP_STEM):
            r = g.ops[oi]
            k = int(r["k"])
            ry, tyy, ny, rx, txx, nx = tiling(h, w, k, int(r["stride"]), int(r["pad_t"]), int(r["pad_l"]))
            wt = g.conv_params(oi)[0]
            ky, kx = np.minimum(ry, k - 1)[:, None], np.minimum(rx, k - 1)[None, :]     # (rows between tiles repeat the last window row)
            jy, jx = np.maximum(tyy, 0)[:, None], np.maximum(txx, 0)[None, :]
            out = np.empty((B, h, w, c), np.int8)
            for b in range(B):
                if ty == OP_DW:
                    pos = (wt > 0)[ky, kx] ^ (((b + jy + jx) & 1) == 1)[:, :, None]
                else:
                    N = wt.shape[0]
                    tgt = (jy * nx + jx + _image_offsets(B, ny * nx, 2 * N)[b]) % (2 * N)
                    pos = (wt > 0)[tgt % N, ky, kx] ^ (tgt >= N)[:, :, None]
                out[b] = np.where(pos, np.int8(127), np.int8(-128))
                if ty == OP_DW and b >= 2:                   # images 0 and 2 share a polarity: the later one is moved by whole strides
                    out[b] = np.roll(out[b], int(r["stride"]) * (b // 2), axis=1)
            return out
        # ADD, resamples, post-process inputs
        add, slot = self.serves_add(tid)
        out = np.empty((B, h, w, c), np.int8)
        ch = np.arange(c) % 32
        free = np.broadcast_to(ch >= 2, out.shape)
        n_free = int(free.sum())
        rng = self._rng(2, add if add is not None else g.n_ops + tid)
        head = rng.permutation(GRID) if n_free >= GRID else np.asarray([(a + 128) * 256 + (b + 128) for a in NEAR_RAILS for b in NEAR_RAILS])
        pairs = np.concatenate([head, rng.integers(0, GRID, max(n_free - head.size, 0))])[:n_free]
        out[free] = ((pairs % 256 if slot else pairs // 256) - 128).astype(np.int8)
        out[..., ch == 0] = 127
        out[..., ch == 1] = -128
        return out


def conv_extremes(g, oi):
    """The attainable extremes of conv `oi`'s accumulator per output channel, in closed form: b + sum max(w (127 - z), w (-128 - z)) and
    the matching minimum, over a whole window."""
    w, bias, _ = g.conv_params(oi)
    z = g.zero_point(g.inputs(oi)[0])
    ty = g.type(oi)
    hi, lo = np.maximum(w * (127 - z), w * (-128 - z)), np.minimum(w * (127 - z), w * (-128 - z))
    axes = (1, 2, 3) if ty == OP_STEM else (1,) if ty == OP_PW else (0, 1)
    return bias + hi.sum(axis=axes), bias + lo.sum(axis=axes)


def kb_bound(g, oi):
    """255 * sum |w| + |b| per output channel: what bounds |accumulator| for EVERY input.  The library starts a conv's accumulators at
    bias + 0x4B400000 and reads them back as floats when this stays below 2^22 - 1 on every channel (planner.hip: conv_kb)."""
    w, bias, _ = g.conv_params(oi)
    ty = g.type(oi)
    axes = (1, 2, 3) if ty == OP_STEM else (1,) if ty == OP_PW else (0, 1)
    return 255 * np.abs(w).sum(axis=axes) + np.abs(bias)


def conv_ops(g):
    return [oi for oi in range(g.n_ops) if g.type(oi) in CONVS]
