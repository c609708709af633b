"""`Interpreter`: the detector object of the reference hot loop, backed by libvbt_hip.so.

Mirrors the slice of tflite_runtime.interpreter.Interpreter the reference uses:
  Interpreter(model_path=..., num_threads=...)  reference track.py:93, eval.py:167
  .allocate_tensors()                           reference track.py:94
  .get_input_details()[0]['shape']              reference odt.py:86-87
  .get_signature_runner()(images=uint8[1,H,W,3]) -> {'output_0'..'output_3'}   reference odt.py:58-66
"""
import ctypes
import os

import numpy as np

from . import _lib

MAXDET = 25


class Interpreter:
    def __init__(self, model_path, num_threads=4, device=0, max_batch=1, fuse=True, flags=None):
        # num_threads is accepted for signature compatibility (reference track.py:72); the GPU path ignores it.
        self.model_path = str(model_path)
        self.num_threads = num_threads
        self.device = device
        self.max_batch = int(max_batch)
        self._h = ctypes.c_void_p()
        if flags is None:
            flags = int(os.environ.get('VBT_FUSION_FLAGS', '0')) if fuse else 1
        # --model may name a TFLite flatbuffer like the reference's (track.py:67): it is converted to the container
        # format on the fly (vbt_amd/tflite_import.py); the library itself only parses containers.
        from .tflite_import import as_container_path
        path, temporary = as_container_path(self.model_path)
        try:
            _lib.check(_lib.lib().vbt_model_create_ex(path.encode(), device, self.max_batch, flags, ctypes.byref(self._h)))
        finally:
            if temporary:
                os.unlink(path)
        shp = (ctypes.c_int * 4)()
        _lib.check(_lib.lib().vbt_model_input_shape(self._h, shp))
        self._shape = np.array([1, shp[1], shp[2], shp[3]], dtype=np.int32)

    @classmethod
    def _borrowed(cls, handle, model_path, device, max_batch, owner):
        """A view of a detector instance owned by a vbt_pipeline (never destroyed from here; `owner` is kept alive)."""
        self = cls.__new__(cls)
        self.model_path, self.num_threads, self.device, self.max_batch = str(model_path), 4, device, int(max_batch)
        self._h, self._owner = ctypes.c_void_p(handle), owner
        shp = (ctypes.c_int * 4)()
        _lib.check(_lib.lib().vbt_model_input_shape(self._h, shp))
        self._shape = np.array([1, shp[1], shp[2], shp[3]], dtype=np.int32)
        return self

    def __del__(self):
        h = getattr(self, "_h", None)
        if h and getattr(self, "_owner", None) is None and _lib is not None and _lib._lib is not None:
            _lib._lib.vbt_model_destroy(h)
            self._h = None

    @property
    def handle(self):
        return self._h

    def allocate_tensors(self):
        return None     # buffers are allocated at construction; kept for call-shape parity

    def get_input_details(self):
        return [{"name": "images", "index": 0, "shape": self._shape.copy(), "dtype": np.uint8}]

    def get_signature_runner(self, signature_key=None):
        def run(images):
            images = np.asarray(images)
            if images.dtype != np.uint8 or images.ndim != 4 or tuple(images.shape[1:]) != tuple(self._shape[1:]):
                raise ValueError(f"images must be uint8 [B,{self._shape[1]},{self._shape[2]},3], got {images.dtype} {images.shape}")
            boxes, scores, classes, counts = self.detect(images)
            if images.shape[0] == 1:
                return {"output_0": counts.astype(np.float32), "output_1": scores, "output_2": classes, "output_3": boxes}
            return {"output_0": counts.astype(np.float32), "output_1": scores, "output_2": classes, "output_3": boxes}
        return run

    def detect(self, frames):
        """frames uint8 [B,H,W,3] (host) -> boxes [B,25,4], scores [B,25], classes [B,25], counts [B]."""
        frames = np.ascontiguousarray(frames, dtype=np.uint8)
        B = frames.shape[0]
        boxes = np.empty((B, MAXDET, 4), np.float32)
        scores = np.empty((B, MAXDET), np.float32)
        classes = np.empty((B, MAXDET), np.float32)
        counts = np.empty((B,), np.int32)
        _lib.check(_lib.lib().vbt_detect(self._h, frames.ctypes.data, B, 0, None, boxes.ctypes.data, scores.ctypes.data,
                                         classes.ctypes.data, counts.ctypes.data, 0))
        return boxes, scores, classes, counts

    # --- parity/debug helpers -------------------------------------------------
    def num_tensors(self):
        return _lib.lib().vbt_model_num_tensors(self._h)

    def materialized(self, tid):
        return bool(_lib.lib().vbt_model_tensor_materialized(self._h, tid))

    def num_launches(self):
        return _lib.lib().vbt_model_num_launches(self._h)

    def plan_space(self):
        """Every step of every alternative of every plan group, in that order, as a dict: group, alt, step, chosen (the group's
        current alternative), variant (the step's current one), first_op / last_op (the graph ops it evaluates), family, and
        variants (what a plan file may name for the step: vbt_model_plan_space)."""
        n = ctypes.c_int()
        rc = _lib.lib().vbt_model_plan_space(self._h, None, 0, ctypes.byref(n))
        if rc not in (0, -4):       # VBT_ERR_CAPACITY: the count of entries is in n
            _lib.check(rc)
        buf = (_lib.PlanStepSpace * max(n.value, 1))()
        _lib.check(_lib.lib().vbt_model_plan_space(self._h, buf, n.value, ctypes.byref(n)))
        return [{"group": e.group, "alt": e.alt, "step": e.step, "chosen": bool(e.chosen), "variant": e.variant, "first_op": e.first_op,
                 "last_op": e.last_op, "family": e.family.decode(), "variants": list(e.variants[:e.n_variants])} for e in buf[:n.value]]

    def plan_steps(self):
        """The execution list, one dict per plan step (the indices run_steps counts): family, variant, reads_frames, image0_only,
        group / step (its place in the plan space; -1 for the merged side-conv launch), first_op / last_op, n_members
        (vbt_model_plan_steps)."""
        n = ctypes.c_int()
        rc = _lib.lib().vbt_model_plan_steps(self._h, None, 0, ctypes.byref(n))
        if rc not in (0, -4):       # VBT_ERR_CAPACITY: the count of steps is in n
            _lib.check(rc)
        buf = (_lib.PlanStepInfo * max(n.value, 1))()
        _lib.check(_lib.lib().vbt_model_plan_steps(self._h, buf, n.value, ctypes.byref(n)))
        return [{"family": e.family.decode(), "variant": e.variant, "reads_frames": bool(e.reads_frames), "image0_only": bool(e.image0_only),
                 "group": e.group, "step": e.step, "first_op": e.first_op, "last_op": e.last_op, "n_members": e.n_members}
                for e in buf[:n.value]]

    def run_steps(self, step0, step1, img0, n_img, frames=None):
        """Plan steps [step0, step1) alone on images img0 .. img0 + n_img - 1 of the tensors as they stand (test equipment, see
        write_tensor), then a synchronisation.  frames: uint8 [n_img,S,S,3] (host), the frames OF THAT RANGE, for a range that holds a
        step reading them.  Decode + NMS has run_postprocess."""
        buf, ptr = None, None
        if frames is not None:
            from .mem import DeviceBuffer
            f = np.ascontiguousarray(frames, dtype=np.uint8)
            if f.ndim != 4 or f.shape[0] != n_img or tuple(f.shape[1:]) != tuple(self._shape[1:]):
                raise ValueError(f"frames must be uint8 [{n_img},{self._shape[1]},{self._shape[2]},3], got {f.shape}")
            buf = DeviceBuffer.from_host(f, self.device)
            ptr = ctypes.c_void_p(buf.ptr)
        try:
            _lib.check(_lib.lib().vbt_detect_range_async(self._h, ptr, img0, n_img, step0, step1, None, None, None, None, None))
        finally:
            _lib.check(_lib.lib().vbt_device_synchronize(self.device))   # (before `buf` is freed, whatever the call answered)

    def proj_tail(self, group, alt, step):
        """Live tiles of the part-filled last output block that plan-space step runs tile-major under its current variant; 0: block-major
        (vbt_model_step_proj_tail)."""
        n = _lib.lib().vbt_model_step_proj_tail(self._h, group, alt, step)
        if n < 0:
            _lib.check(n)
        return n

    def fused_params(self, group, alt, step):
        """True where that plan-space step is a fused_mbconv launch that fetches its chunk parameters once per workgroup, through LDS
        (vbt_model_step_fused_params)."""
        n = _lib.lib().vbt_model_step_fused_params(self._h, group, alt, step)
        if n < 0:
            _lib.check(n)
        return bool(n)

    def read_tensor(self, tid, B):
        shp = (ctypes.c_int * 3)()
        _lib.check(_lib.lib().vbt_model_tensor_shape(self._h, tid, shp))
        out = np.empty((B, shp[0], shp[1], shp[2]), np.int8)
        _lib.check(_lib.lib().vbt_model_read_tensor(self._h, tid, B, out.ctypes.data))
        return out

    def write_tensor(self, tid, array):
        """int8 [B,h,w,c] (host) into the device buffer of graph tensor `tid` (test equipment: vbt_model_write_tensor)."""
        shp = (ctypes.c_int * 3)()
        _lib.check(_lib.lib().vbt_model_tensor_shape(self._h, tid, shp))
        a = np.ascontiguousarray(array, dtype=np.int8)
        if a.ndim != 4 or tuple(a.shape[1:]) != (shp[0], shp[1], shp[2]):
            raise ValueError(f"tensor {tid} is int8 [B,{shp[0]},{shp[1]},{shp[2]}], got {a.shape}")
        _lib.check(_lib.lib().vbt_model_write_tensor(self._h, tid, a.shape[0], a.ctypes.data))

    def run_postprocess(self, B, fill=0xA5):
        """The plan's last step (decode + NMS) alone on the head tensors as they stand, frames 0..B-1 (test equipment, see
        write_tensor).  The four outputs are device buffers filled with the byte `fill` before the launch, so that rows the kernel
        leaves unwritten show.  -> boxes [B,25,4], scores [B,25], classes [B,25], counts [B]."""
        from .mem import DeviceBuffer
        shapes = ((B, MAXDET, 4), (B, MAXDET), (B, MAXDET), (B,))
        dtypes = (np.float32, np.float32, np.float32, np.int32)
        bufs = [DeviceBuffer.from_host(np.full(int(np.prod(s)) * 4, fill, np.uint8), self.device) for s in shapes]
        last = self.num_launches() - 1
        _lib.check(_lib.lib().vbt_detect_range_async(self._h, None, 0, B, last, -1, None, *[ctypes.c_void_p(b.ptr) for b in bufs]))
        return tuple(b.to_host(s, d) for b, s, d in zip(bufs, shapes, dtypes))
