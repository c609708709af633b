"""Test infrastructure: an exact numpy evaluator of the six op types a `.vbtm` container holds besides the post-process.

Written from the arithmetic contract of DESIGN.md section 2, in array code, on whole batches ([B,H,W,C]); everything it uses - weights,
biases, float32 multipliers, zero points, activation ranges, the ADD's integer parameters, the pads - is read from the file through
vbt_amd.container.Container.  It is a second statement of what oracle/detector.c states in loops (tests/test_graph_ref_host.py compares
the two on every tensor of four models) and the reference of tests/test_gpu_steps_alone.py, which runs single plan steps on crafted
tensors.

  conv         acc = sum (x - z_x) * w + b as an integer.  Pointwise: one float64 matrix product - exact, since |x - z_x| <= 255,
               |w| <= 128 and K <= 2112 keep every partial sum below 2^28 < 2^53.  Depthwise, stem: shifted slices of the input padded
               with zeros (x - z_x = 0) by the op's SAME pads, int64.
  requantise   float32(acc) * float32(mult) as ONE float32 product (the conversion rounds to nearest even beyond 2^24), rounded to
               nearest even, + z_y, clamped to the op's range.
  ADD          XNNPACK qs8-vadd in integers: the form of tests/test_quant_kat.ref_add, vectorised.
  max pool     shifted slices of the input padded with -128.
  resize       src = min(floor(dst * (float32) in / out), in - 1), evaluated in float32.
"""
import numpy as np

from vbt_amd.container import Container

OP_STEM, OP_PW, OP_DW, OP_ADD, OP_MAXPOOL, OP_RESIZE_NN, OP_POSTPROCESS = 1, 2, 3, 4, 5, 6, 7
CONVS = (OP_STEM, OP_PW, OP_DW)


def requantize(acc, mult, zp, lo, hi):
    """int accumulators, float32 multipliers (broadcast over the last axis) -> int8"""
    t = np.asarray(acc, np.int64).astype(np.float32) * np.asarray(mult, np.float32)      # int64 -> float32: one rounding, to nearest even
    assert t.dtype == np.float32
    return np.clip(np.rint(t).astype(np.int64) + int(zp), int(lo), int(hi)).astype(np.int8)


def add_q(a, b, params, zo, lo, hi):
    """tests/test_quant_kat.ref_add on arrays"""
    bias, am, bm, shift = (int(v) for v in params)
    acc = bias + np.asarray(a, np.int64) * am + np.asarray(b, np.int64) * bm
    t = np.clip(acc >> shift, -32768, 32767)          # arithmetic shift of an int64 = floor division
    t = np.clip(t + int(zo), -32768, 32767)
    t = np.clip(t, -128, 127)
    return np.clip(t, int(lo), int(hi)).astype(np.int8)


def _windows(xp, k, s, oh, ow):
    """the k x k shifted, strided slices of a padded [B,H,W,C] array, as (ky, kx, view [B,oh,ow,C])"""
    for ky in range(k):
        for kx in range(k):
            yield ky, kx, xp[:, ky:ky + s * (oh - 1) + 1:s, kx:kx + s * (ow - 1) + 1:s]


class GraphRef:
    def __init__(self, path):
        c = self.c = Container(path)
        self.input_tensor = int(c.header["input_tensor"])
        self.ops = c.ops
        self.tensors = c.tensors
        self.n_ops = len(c.ops)
        self.producer = {int(r["output"]): i for i, r in enumerate(c.ops)}
        self.readers = {}
        for i, r in enumerate(c.ops):
            for t in self.inputs(i):
                self.readers.setdefault(t, []).append(i)

    # ---- the file ----
    def type(self, oi):
        return int(self.ops[oi]["type"])

    def inputs(self, oi):
        r = self.ops[oi]
        return [int(t) for t in r["inputs"][:int(r["n_inputs"])]]

    def output(self, oi):
        return int(self.ops[oi]["output"])

    def shape(self, tid):
        t = self.tensors[tid]
        return int(t["h"]), int(t["w"]), int(t["c"])

    def zero_point(self, tid):
        return int(self.tensors[tid]["zero_point"])

    def conv_params(self, oi):
        """-> w, bias [N] int64, mult [N] float32.  w: stem [N,k,k,Cin], pointwise [N,K], depthwise [k,k,C] (the container's layouts)"""
        r, c = self.ops[oi], self.c
        ci = self.shape(self.inputs(oi)[0])[2]
        N = self.shape(self.output(oi))[2]
        k = int(r["k"])
        ty = self.type(oi)
        if ty == OP_STEM:
            w = c.i8(int(r["w_off"]), N * k * k * ci).reshape(N, k, k, ci)
        elif ty == OP_PW:
            w = c.i8(int(r["w_off"]), N * ci).reshape(N, ci)
        else:
            w = c.i8(int(r["w_off"]), k * k * N).reshape(k, k, N)
        return w.astype(np.int64), c.i32(int(r["b_off"]), N).astype(np.int64), c.f32(int(r["m_off"]), N).copy()

    def _pads(self, oi):
        """(top, bottom), (left, right) of the op's SAME padding: the recorded leading pads, and what the last window still needs"""
        r = self.ops[oi]
        k, s, pt, pl = int(r["k"]), int(r["stride"]), int(r["pad_t"]), int(r["pad_l"])
        h, w, _ = self.shape(self.inputs(oi)[0])
        oh, ow, _ = self.shape(self.output(oi))
        return k, s, oh, ow, (pt, max((oh - 1) * s + k - h - pt, 0)), (pl, max((ow - 1) * s + k - w - pl, 0))

    # ---- the arithmetic ----
    def accumulator(self, oi, x):
        """the integer accumulator of conv op `oi` on x ([B,H,W,Cin]: int8, or the uint8 frames for the stem) -> int64 [B,oh,ow,N]"""
        ty = self.type(oi)
        w, bias, _ = self.conv_params(oi)
        x = np.asarray(x)
        if ty == OP_STEM:
            assert x.dtype == np.uint8
            x = x.astype(np.int64) - 128                      # QUANTIZE uint8 -> int8 at one scale
        else:
            assert x.dtype == np.int8
            x = x.astype(np.int64)
        x = x - self.zero_point(self.inputs(oi)[0])
        if ty == OP_PW:
            B, H, W, K = x.shape
            acc = np.rint(x.reshape(-1, K).astype(np.float64) @ w.T.astype(np.float64)).astype(np.int64)
            return acc.reshape(B, H, W, -1) + bias
        k, s, oh, ow, py, px = self._pads(oi)
        xp = np.pad(x, ((0, 0), py, px, (0, 0)))
        B = x.shape[0]
        acc = np.zeros((B, oh, ow, w.shape[0] if ty == OP_STEM else w.shape[2]), np.int64)
        for ky, kx, v in _windows(xp, k, s, oh, ow):
            if ty == OP_STEM:
                acc += v @ w[:, ky, kx, :].T
            else:
                acc += v * w[ky, kx]
        return acc + bias

    def eval_op(self, oi, ins):
        """op `oi` on its input arrays (batches) -> int8 [B,oh,ow,C]"""
        r = self.ops[oi]
        ty = self.type(oi)
        out = self.output(oi)
        lo, hi = int(r["act_min"]), int(r["act_max"])
        if ty in CONVS:
            return requantize(self.accumulator(oi, ins[0]), self.conv_params(oi)[2], self.zero_point(out), lo, hi)
        if ty == OP_ADD:
            return add_q(ins[0], ins[1], r["add_q"], self.zero_point(out), lo, hi)
        if ty == OP_MAXPOOL:
            k, s, oh, ow, py, px = self._pads(oi)
            xp = np.pad(ins[0], ((0, 0), py, px, (0, 0)), constant_values=-128)
            res = None
            for _, _, v in _windows(xp, k, s, oh, ow):
                res = v.copy() if res is None else np.maximum(res, v)
            return res
        if ty == OP_RESIZE_NN:
            x = ins[0]
            oh, ow, _ = self.shape(out)

            def src(n_out, n_in):
                scale = np.float32(n_in) / np.float32(n_out)
                return np.minimum(np.floor(np.arange(n_out, dtype=np.float32) * scale).astype(np.int64), n_in - 1)
            return x[:, src(oh, x.shape[1])][:, :, src(ow, x.shape[2])]
        raise ValueError(f"op {oi}: type {ty} is not evaluated here")

    def reference(self, tid, state, frames=None, memo=None):
        """What graph tensor `tid` must hold: its producer evaluated on inputs taken from `state` (tensor id -> host copy of a
        materialised tensor) where the tensor is there, and from the input's own producer, recursively, where it is not (a tensor that
        lives only inside a fused kernel).  frames: the uint8 batch, for the stem."""
        memo = {} if memo is None else memo
        if tid in memo:
            return memo[tid]
        oi = self.producer[tid]
        ins = []
        for t in self.inputs(oi):
            if t == self.input_tensor:
                assert frames is not None, "the reference reaches the stem: frames needed"
                ins.append(frames)
            elif t in state:
                ins.append(state[t])
            else:
                ins.append(self.reference(t, state, frames, memo))
        memo[tid] = self.eval_op(oi, ins)
        return memo[tid]

    def run_graph(self, frames):
        """every tensor of the graph on a uint8 batch [B,S,S,3] -> {tensor id: int8 [B,h,w,c]} (the post-process is not evaluated)"""
        val = {}
        for oi in range(self.n_ops):
            if self.type(oi) == OP_POSTPROCESS:
                continue
            val[self.output(oi)] = self.eval_op(oi, [frames if t == self.input_tensor else val[t] for t in self.inputs(oi)])
        return val
