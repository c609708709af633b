"""Detector evaluation - the reference's eval.py: VOC annotations, detections of every test image at threshold 0, Hungarian matching
against the ground truth, precision-recall / ROC curves, AP and AUC per model, and the figures of both curve kinds
(`plot_precision_recall`, `plot_roc`: rendered and encoded on the GPU, vbt_amd/curve_figure.py).

Matching and curves run on the GPU (`vbt_eval_*`, include/vbt_hip.h; vbt_amd/csrc/evaluate.hip); the detections never leave the
device between the detector and the matcher.  No torch, no scipy, no scikit-learn.

The second set of numbers the reference reports its detectors by - the twelve COCO detection metrics and the per-class AP that
model.evaluate prints at the end of the training logs (train.py:64,70) - comes from the same image path and a second matcher on the
device (`vbt_coco_*`; vbt_amd/csrc/evaluate_coco.hip): CocoEvaluator, coco_metrics, coco_dump.  No pycocotools.

Images.  eval.py reads every image with cv2.imread and hands that **BGR** array to the network unswapped (eval.py:173-180;
track.py:171 swaps, eval.py does not).  The default here reproduces that: `.npy` files hold a decoded image uint8 [H,W,3] in cv2's BGR
order; `.png` files are decoded with PIL and reordered to BGR; `rgb=True` (CLI `--rgb`) feeds RGB instead.

`.jpg` files are decoded on the GPU (`vbt_jpeg_stills`, vbt_amd/stills.py): baseline files of any mix of sizes go, in the given
order, in batches of compressed bytes to the device, where they are decoded and resized to the network input in one pass - no Pillow,
no decoded frame on the host or on the bus.  The reconstruction is libjpeg-turbo's default, bit for bit (what Pillow and cv2 give for
such files), so the result equals the `.npy` route on the same pixels.  A `.jpg` the decoder refuses (progressive, CMYK, ...) is
decoded with PIL as before; `jpeg_decode` (CLI `--jpeg_decode auto|gpu|host`) makes that an error ("gpu") or the route of every
`.jpg` ("host").
"""
import ctypes
import os
import xml.etree.ElementTree as ET

import numpy as np

from . import _lib
from .mem import DeviceBuffer

LABEL = "barbell"                  # eval.py:23
MAX_DETECTIONS = 25
MAX_GT = 64                        # VBT_EVAL_MAX_GT
NO_POSITIVES, NO_NEGATIVES = 1, 2  # VBT_EVAL_NO_*
BATCH = 64
COCO_KEYS = ("AP", "AP50", "AP75", "APs", "APm", "APl", "ARmax1", "ARmax10", "ARmax100", "ARs", "ARm", "ARl", "AP_/" + LABEL)   # the log's dict


class Annotations(dict):
    """{filename: int array [n,4] = ymin,xmin,ymax,xmax} as eval.py:487-504 builds it, in sorted file order, plus
    `.sizes` = {filename: (height, width)} from the XML's <size> element (None when the file has none)."""

    def __init__(self):
        super().__init__()
        self.sizes = {}


def read_annotations(annotations_dir, label=LABEL):
    """eval.py:487-504: every *.xml of the directory (VOC), objects whose <name> is not `label` skipped."""
    out = Annotations()
    for f in sorted(os.listdir(annotations_dir)):
        if not f.endswith(".xml"):
            continue
        root = ET.parse(os.path.join(annotations_dir, f)).getroot()
        key = root.find("filename").text
        boxes = []
        for o in root.findall("object"):
            if o.find("name").text != label:
                continue
            bb = o.find("bndbox")
            boxes.append([bb.find(k).text for k in ("ymin", "xmin", "ymax", "xmax")])
        out[key] = np.array(boxes, dtype=int).reshape(-1, 4)
        size = root.find("size")
        out.sizes[key] = (int(size.find("height").text), int(size.find("width").text)) if size is not None else None
    return out


def find_image(img_dir, filename):
    """the annotation's <filename> inside img_dir, or the same stem as .npy / .png / .jpg"""
    stem = os.path.splitext(filename)[0]
    for cand in (filename, stem + ".npy", stem + ".png", stem + ".jpg"):
        p = os.path.join(img_dir, cand)
        if os.path.isfile(p):
            return p
    raise FileNotFoundError(f"{os.path.join(img_dir, filename)}: no such image (also tried .npy / .png / .jpg)")


def load_image(path):
    """uint8 [H,W,3] in BGR order (see the module docstring)."""
    if path.endswith(".npy"):
        a = np.load(path)
        if a.ndim != 3 or a.shape[2] != 3 or a.dtype != np.uint8:
            raise ValueError(f"{path}: expected uint8 [H,W,3], got {a.dtype} {a.shape}")
        return np.ascontiguousarray(a)
    try:
        from PIL import Image
    except ImportError:
        raise RuntimeError(f"{path}: reading .jpg / .png images needs PIL (pillow); store the decoded image as .npy uint8 [H,W,3] instead") from None
    with Image.open(path) as im:
        return np.ascontiguousarray(np.asarray(im.convert("RGB"))[:, :, ::-1])


class CurveResult:
    """precision, recall, pr_thresholds (precision_recall_curve); fpr, tpr, roc_thresholds (roc_curve); ap, auc; n_rows, n_pos,
    n_neg; flags (NO_POSITIVES / NO_NEGATIVES: the rates and scalars that have no denominator are NaN)."""

    def __init__(self, s, arrays):
        self.n_rows, self.n_pos, self.n_neg, self.flags, self.ap, self.auc = s.n_rows, s.n_pos, s.n_neg, s.flags, s.ap, s.auc
        self.precision, self.recall, self.pr_thresholds, self.fpr, self.tpr, self.roc_thresholds = arrays


def _curve_call(fn, n_rows):
    """run fn(summary, six arrays, capacities): n_rows + 1 points are always enough"""
    cap = int(n_rows) + 1
    p, r, f, t = (np.empty(cap, np.float64) for _ in range(4))
    pt, rt = np.empty(cap, np.float32), np.empty(cap, np.float32)
    s = _lib.EvalSummary()
    _lib.check(fn(ctypes.byref(s), p.ctypes.data, r.ctypes.data, pt.ctypes.data, cap, f.ctypes.data, t.ctypes.data, rt.ctypes.data, cap))
    return CurveResult(s, (p[:s.n_pr].copy(), r[:s.n_pr].copy(), pt[:s.n_pr - 1].copy(), f[:s.n_roc].copy(), t[:s.n_roc].copy(), rt[:s.n_roc].copy()))


def curves_from_table(scores, ious, iou_threshold=0.5, device=0):
    """vbt_eval_curves_from_table: curves of one model's table (Score float32, IoU float64) held by the caller."""
    sc = np.ascontiguousarray(scores, dtype=np.float32)
    io = np.ascontiguousarray(ious, dtype=np.float64)
    if sc.shape != io.shape or sc.ndim != 1:
        raise ValueError("scores and ious must be one-dimensional and of one length")
    L = _lib.lib()
    return _curve_call(lambda s, *a: L.vbt_eval_curves_from_table(sc.ctypes.data, io.ctypes.data, len(sc), float(iou_threshold), int(device), s, *a),
                       len(sc))


def _csr(hw, gt_list):
    """(hw int32 [B,2], B, offsets int32 [B+1], boxes int32 [*,4]) of per-image sizes and ground-truth arrays"""
    hw = np.ascontiguousarray(hw, dtype=np.int32).reshape(-1, 2)
    B = len(hw)
    if len(gt_list) != B:
        raise ValueError("one ground-truth array per image")
    off = np.zeros(B + 1, np.int32)
    off[1:] = np.cumsum([len(g) for g in gt_list])
    gt = np.ascontiguousarray(np.concatenate([np.asarray(g, np.int64).reshape(-1, 4) for g in gt_list]) if B else np.zeros((0, 4)), dtype=np.int32)
    return hw, B, off, gt


class Evaluator:
    """One model's detection table on the device (`vbt_eval`, include/vbt_hip.h)."""

    def __init__(self, rows_cap, max_batch=BATCH, device=0):
        self._h = ctypes.c_void_p()
        self.rows_cap, self.max_batch, self.device = int(rows_cap), int(max_batch), int(device)
        _lib.check(_lib.lib().vbt_eval_create(self.device, self.max_batch, self.rows_cap, ctypes.byref(self._h)))

    def __del__(self):
        if getattr(self, "_h", None):
            _lib.lib().vbt_eval_destroy(self._h)
            self._h = None

    def reset(self):
        _lib.check(_lib.lib().vbt_eval_reset(self._h))

    def add(self, boxes_ptr, scores_ptr, counts_ptr, hw, gt_list, stream=None):
        """B images' detections (raw device pointers, the detector's layout) + per image (height, width) and ground-truth boxes
        int [n,4] = ymin,xmin,ymax,xmax.  Enqueue only."""
        hw, B, off, gt = _csr(hw, gt_list)
        _lib.check(_lib.lib().vbt_eval_add_detections(self._h, boxes_ptr, scores_ptr, counts_ptr, B, hw.ctypes.data, off.ctypes.data,
                                                      gt.ctypes.data if len(gt) else None, stream))

    def table(self):
        """{"score" f32, "iou" f64, "image" i32, "det_idx" i32, "gt_idx" i32}, rows in emission order (synchronises)."""
        L = _lib.lib()
        n = ctypes.c_int(0)
        _lib.check(L.vbt_eval_table(self._h, ctypes.byref(n), None, None, None, None, None, 0))
        out = {"score": np.empty(n.value, np.float32), "iou": np.empty(n.value, np.float64), "image": np.empty(n.value, np.int32),
               "det_idx": np.empty(n.value, np.int32), "gt_idx": np.empty(n.value, np.int32)}
        if n.value:
            _lib.check(L.vbt_eval_table(self._h, ctypes.byref(n), *(out[k].ctypes.data for k in ("score", "iou", "image", "det_idx", "gt_idx")), n.value))
        return out

    def curves(self, iou_threshold=0.5):
        """vbt_eval_curves over the device table."""
        L = _lib.lib()
        return _curve_call(lambda s, *a: L.vbt_eval_curves(self._h, float(iou_threshold), s, *a), self.rows_cap)


class CocoResult:
    """vbt_coco_accumulate's outputs: stats {name: value} in the log's order (COCO_KEYS without the per-class entry), precision
    [10,101,4,3], recall [10,4,3], scores [10,101,4,3] (COCOeval's arrays without the category axis), n_gt [4], n_images, n_rows."""

    def __init__(self, s, precision, recall, scores):
        self.stats = dict(zip(COCO_KEYS[:12], (float(v) for v in s.stats)))
        self.n_images, self.n_rows, self.n_gt = int(s.n_images), int(s.n_rows), np.array(list(s.n_gt), np.int64)
        self.precision, self.recall, self.scores = precision, recall, scores

    def metrics(self):
        """the dict model.evaluate prints (train.py:64): the twelve stats and the per-class AP, which with one class is AP"""
        return dict(self.stats, **{COCO_KEYS[12]: self.stats["AP"]})


class CocoEvaluator:
    """One model's COCO rows on the device (`vbt_coco`, include/vbt_hip.h): the shape of Evaluator."""

    def __init__(self, rows_cap, max_batch=BATCH, device=0):
        self._h = ctypes.c_void_p()
        self.rows_cap, self.max_batch, self.device = int(rows_cap), int(max_batch), int(device)
        _lib.check(_lib.lib().vbt_coco_create(self.device, self.max_batch, self.rows_cap, ctypes.byref(self._h)))

    def __del__(self):
        if getattr(self, "_h", None):
            _lib.lib().vbt_coco_destroy(self._h)
            self._h = None

    def reset(self):
        _lib.check(_lib.lib().vbt_coco_reset(self._h))

    def add(self, boxes_ptr, scores_ptr, counts_ptr, hw, gt_list, stream=None):
        """Evaluator.add's arguments.  Enqueue only."""
        hw, B, off, gt = _csr(hw, gt_list)
        _lib.check(_lib.lib().vbt_coco_add_detections(self._h, boxes_ptr, scores_ptr, counts_ptr, B, hw.ctypes.data, off.ctypes.data,
                                                      gt.ctypes.data if len(gt) else None, stream))

    def table(self):
        """{"score" f32, "image" i32, "rank" i32, "matched" u64, "ignored" u64}: images in the order added, inside an image by descending
        score; bit a * 10 + t of the masks belongs to area range a and IoU threshold t (synchronises)."""
        L = _lib.lib()
        n = ctypes.c_int(0)
        _lib.check(L.vbt_coco_table(self._h, ctypes.byref(n), None, None, None, None, None, 0))
        out = {"score": np.empty(n.value, np.float32), "image": np.empty(n.value, np.int32), "rank": np.empty(n.value, np.int32),
               "matched": np.empty(n.value, np.uint64), "ignored": np.empty(n.value, np.uint64)}
        if n.value:
            _lib.check(L.vbt_coco_table(self._h, ctypes.byref(n), *(out[k].ctypes.data for k in ("score", "image", "rank", "matched", "ignored")), n.value))
        return out

    def accumulate(self):
        """vbt_coco_accumulate over the device table: CocoResult."""
        p, r, sc = np.empty((10, 101, 4, 3)), np.empty((10, 4, 3)), np.empty((10, 101, 4, 3))
        s = _lib.CocoSummary()
        _lib.check(_lib.lib().vbt_coco_accumulate(self._h, ctypes.byref(s), p.ctypes.data, r.ctypes.data, sc.ctypes.data))
        return CocoResult(s, p, r, sc)


def match_bboxes(gt_bboxes, det_bboxes, device=0):
    """match_bboxes of eval.py:96-153, same call shape and return value (idx_gt_actual, idx_pred_actual, ious_actual), on the device
    kernel: integer boxes [n,4] = ymin,xmin,ymax,xmax.  At most 25 predictions and 64 ground-truth boxes (the kernel's sides);
    coordinates below 2^24 in magnitude (they travel as float32)."""
    gt = np.asarray(gt_bboxes).reshape(-1, 4).astype(np.int64)
    det = np.asarray(det_bboxes).reshape(-1, 4).astype(np.int64)
    if len(det) > MAX_DETECTIONS:
        raise ValueError(f"match_bboxes: {len(det)} predictions, the device matcher takes {MAX_DETECTIONS}")
    if len(det) and np.abs(det).max() >= 1 << 24:
        raise ValueError("match_bboxes: box coordinates must be below 2^24 in magnitude")
    boxes = np.zeros((1, MAX_DETECTIONS, 4), np.float32)
    boxes[0, :len(det)] = det                                  # times (height, width) = (1, 1): the integers come back exactly
    scores = np.zeros((1, MAX_DETECTIONS), np.float32)
    bufs = [DeviceBuffer.from_host(a, device) for a in (boxes, scores, np.array([len(det)], np.int32))]
    ev = Evaluator(MAX_DETECTIONS, 1, device)
    ev.add(bufs[0].ptr, bufs[1].ptr, bufs[2].ptr, [(1, 1)], [gt])
    t = ev.table()
    return t["gt_idx"].astype(np.int64), t["det_idx"].astype(np.int64), t["iou"]


def model_name(path):
    return os.path.basename(path).split(".")[0]               # eval.py:188


JPEG_DECODE_MODES = ("auto", "gpu", "host")
STILLS_MAX_BLOCK_BUDGET = 1 << 22  # most 8 x 8 blocks per batch of the GPU JPEG decoder (196 B of scratch each): eighty-five 1920 x 1080 files at 4:2:0


class JpegRefused(ValueError):
    """jpeg_decode="gpu" and a .jpg file the GPU decoder does not take; the text names the file and the reason"""


class JpegDamaged(ValueError):
    """a .jpg file whose scan the GPU decoder could not decode to its end; the text names the file and the scan status"""


def is_jpeg(path):
    return path.lower().endswith((".jpg", ".jpeg"))


def jpeg_header(jpeg):
    """(height, width, blocks) of one .jpg the GPU decoder accepts - `jpeg`: the file's bytes, or its path - from vbt_jpeg_probe and
    vbt_jpeg_blocks (host only, no Pillow), or the reason the decoder refuses it, as a str"""
    if isinstance(jpeg, str):
        with open(jpeg, "rb") as f:
            jpeg = f.read()
    L = _lib.lib()
    buf = np.frombuffer(jpeg or b"\0", np.uint8)
    H, W, n = ctypes.c_int(), ctypes.c_int(), ctypes.c_uint32()
    if L.vbt_jpeg_probe(buf.ctypes.data, len(jpeg), ctypes.byref(H), ctypes.byref(W), None, None) or L.vbt_jpeg_blocks(buf.ctypes.data, len(jpeg), ctypes.byref(n)):
        text = L.vbt_last_error().decode()
        for prefix in ("vbt_jpeg_probe: ", "vbt_jpeg_blocks: "):
            if text.startswith(prefix):
                text = text[len(prefix):]
        return text
    return H.value, W.value, int(n.value)


def image_size(path):
    """(height, width) of an image file from its header, without decoding it.  .jpg: Pillow reads only the header when it is there;
    without Pillow vbt_jpeg_probe says it for the files the GPU decoder accepts."""
    if path.endswith(".npy"):
        shp = np.load(path, mmap_mode="r").shape
        if len(shp) != 3 or shp[2] != 3:
            raise ValueError(f"{path}: expected uint8 [H,W,3], got shape {shp}")
        return int(shp[0]), int(shp[1])
    try:
        from PIL import Image
    except ImportError:
        head = jpeg_header(path) if is_jpeg(path) else None
        if head is not None and not isinstance(head, str):
            return head[0], head[1]
        raise RuntimeError(f"{path}: reading .png images and .jpg images the GPU decoder refuses needs PIL (pillow); store the decoded image as "
                           ".npy uint8 [H,W,3] instead") from None
    with Image.open(path) as im:
        return int(im.size[1]), int(im.size[0])


class SortedImages:
    """`images` = [(filename, path)] split by route.  stills: the names of the .jpg files the GPU decoder takes, in the given order, with
    heads[name] = (height, width, blocks) and data[name] = the file's bytes - each file is read once, here, and the compressed bytes stay
    in memory for as long as this object lives; host: every other name."""

    def __init__(self, images, jpeg_decode="auto"):
        if jpeg_decode not in JPEG_DECODE_MODES:
            raise ValueError(f"jpeg_decode {jpeg_decode!r}: one of {', '.join(JPEG_DECODE_MODES)}")
        self.stills, self.heads, self.data, self.host = [], {}, {}, []
        for name, path in images:
            if jpeg_decode != "host" and is_jpeg(path):
                with open(path, "rb") as f:
                    data = f.read()
                head = jpeg_header(data)
                if not isinstance(head, str) and head[2] > STILLS_MAX_BLOCK_BUDGET:
                    head = f"{head[2]} blocks of 8 x 8, a batch holds {STILLS_MAX_BLOCK_BUDGET}"
                if not isinstance(head, str):
                    self.stills.append(name)
                    self.heads[name], self.data[name] = head, data
                    continue
                if jpeg_decode == "gpu":
                    raise JpegRefused(f"{path}: the GPU JPEG decoder refuses the file: {head} (--jpeg_decode auto decodes such files on the host)")
            self.host.append(name)


def _stills_table(pipe, evs, stream, srt, paths, annotations, rgb, device, batch):
    """The .jpg files the GPU decoder accepts, in the given order and whatever their sizes: cut into batches by count and block budget,
    only the compressed bytes uploaded, decoded and resized to the model's input size into one of two device buffers that detect_into
    takes by pointer - the order of decode and forwards is track_frames' for .avi sources.  The handle's budget is the largest batch's
    need, so a directory of small images takes little device memory.  A file whose scan status is not 0 raises JpegDamaged.  Every
    evaluator of `evs` gets every batch.  Returns the device outputs to keep alive."""
    from .stills import STATUS_TEXT, JpegStills, plan
    names, heads = srt.stills, srt.heads
    n, size = len(names), pipe._size
    out = [DeviceBuffer(n * MAX_DETECTIONS * 4 * 4, device), DeviceBuffer(n * MAX_DETECTIONS * 4, device), DeviceBuffer(n * MAX_DETECTIONS * 4, device),
           DeviceBuffer(n * 4, device)]
    batches = plan([heads[k][2] for k in names], batch, STILLS_MAX_BLOCK_BUDGET)
    dec = JpegStills(batch, max(sum(heads[k][2] for k in names[i0:i1]) for i0, i1 in batches), device)
    bufs = [DeviceBuffer(batch * size * size * 3, device) for _ in range(2)]
    pending = None                                           # the batch whose scan status has not been read yet

    def check_status():
        for k, st in zip(pending, dec.status()):             # one synchronisation of `stream`
            if st:
                raise JpegDamaged(f"{paths[k]}: damaged JPEG scan (status {int(st)}: {STATUS_TEXT.get(int(st), '?')})")

    for j, (i0, i1) in enumerate(batches):
        part = names[i0:i1]
        buf = bufs[j % 2]                                    # written again two batches later: the forwards that read it come first
        pipe.join_detectors(stream.value)
        try:
            dec.decode_resized([srt.data[k] for k in part], buf.ptr, size, size, swap_rb=not rgb, stream=stream)   # the decoder yields RGB, eval.py feeds BGR
        except _lib.VbtError as e:
            raise _lib.VbtError(f"{paths[part[0]]} .. {paths[part[-1]]}: {e}") from None
        ptrs = (out[0].ptr + i0 * MAX_DETECTIONS * 16, out[1].ptr + i0 * MAX_DETECTIONS * 4, out[2].ptr + i0 * MAX_DETECTIONS * 4, out[3].ptr + i0 * 4)
        pipe.detect_into(buf.ptr, *ptrs, stream=stream.value, n_frames=len(part))
        pipe.join_detectors(stream.value)
        for e in evs:
            e.add(ptrs[0], ptrs[1], ptrs[3], [heads[k][:2] for k in part], [annotations[k] for k in part], stream)
        pending = part
        check_status()                                       # (the decoder keeps the status of its last batch only)
    _lib.check(_lib.lib().vbt_stream_synchronize(stream))    # the decoder and the buffers go away with this frame
    return out


def _run_model(model, images, annotations, make_evaluators, finish, rgb=False, device=0, batch=BATCH, jpeg_decode="auto", sorted_images=None):
    """The image path of detections_table for any evaluators: make_evaluators(rows_cap) -> the objects whose add() gets every batch,
    finish(evaluators, groups) -> the result, called while the stream and the device outputs are alive; groups = [(names, [boxes, scores,
    classes, counts] DeviceBuffers)] in processing order.  Returns (finish's result, image names in processing order)."""
    from .track import Pipeline
    L = _lib.lib()
    paths = dict(images)
    srt = sorted_images if sorted_images is not None else SortedImages(images, jpeg_decode)
    groups = {}
    for name in srt.host:
        groups.setdefault(image_size(paths[name]), []).append(name)
    pipe = Pipeline(model, batch, max_frames=1, detection_treshold=0.0, device=device)
    stream = ctypes.c_void_p()
    _lib.check(L.vbt_stream_create(int(device), ctypes.byref(stream)))
    evs = make_evaluators(max(1, len(images)) * MAX_DETECTIONS)
    order, outs, alive = [], [], []                          # outs: (names, device outputs), alive: host frames of steps in flight
    try:
        if srt.stills:
            outs.append((list(srt.stills), _stills_table(pipe, evs, stream, srt, paths, annotations, rgb, device, batch)))
            order += srt.stills
        for (H, W), names in groups.items():
            n = len(names)
            out = [DeviceBuffer(n * MAX_DETECTIONS * 4 * 4, device), DeviceBuffer(n * MAX_DETECTIONS * 4, device),
                   DeviceBuffer(n * MAX_DETECTIONS * 4, device), DeviceBuffer(n * 4, device)]
            outs.append((list(names), out))
            for i0 in range(0, n, batch):
                part = names[i0:i0 + batch]                     # the last batch of a size group may be partial
                B = len(part)
                frames = np.empty((B, H, W, 3), np.uint8)
                for i, k in enumerate(part):
                    a = load_image(paths[k])
                    if a.shape != (H, W, 3):
                        raise ValueError(f"{paths[k]}: decoded to {a.shape}, its header says {(H, W, 3)}")
                    frames[i] = a
                alive.append(frames)                            # host frames stay untouched until their step has run
                ptrs = (out[0].ptr + i0 * MAX_DETECTIONS * 16, out[1].ptr + i0 * MAX_DETECTIONS * 4, out[2].ptr + i0 * MAX_DETECTIONS * 4,
                        out[3].ptr + i0 * 4)
                pipe.detect_into(frames, *ptrs, src_hw=(H, W), swap_rb=rgb)
                pipe.join_detectors(stream.value)
                for e in evs:
                    e.add(ptrs[0], ptrs[1], ptrs[3], [(H, W)] * B, [annotations[k] for k in part], stream)
                order += part
                if len(alive) >= 8:                             # bound the host memory held for steps in flight
                    _lib.check(L.vbt_stream_synchronize(stream))
                    alive.clear()
        result = finish(evs, outs)                              # synchronises `stream`
    finally:
        L.vbt_stream_synchronize(stream)
        L.vbt_stream_destroy(stream)
    return result, order


def detections_table(model, images, annotations, rgb=False, device=0, batch=BATCH, jpeg_decode="auto", sorted_images=None):
    """One model over `images` = [(filename, path)]: every image through the pipeline's detector-only step, the detections handed to
    the matcher on the device.  `.jpg` files the GPU decoder accepts (jpeg_decode "auto" or "gpu") are decoded on the device straight to
    the network input, in the given order whatever their sizes (_stills_table).  Everything else - .npy, .png, a .jpg the decoder
    refuses, or every .jpg with jpeg_decode="host" - is grouped by size (read from the file headers), decoded on the host one batch at a
    time and resized on the device; at most 8 batches of host frames are alive at once.  jpeg_decode="gpu": a refused .jpg raises
    JpegRefused, naming the file and the reason.  sorted_images: SortedImages(images, jpeg_decode) made by the caller, so that several
    models share one reading of the files.
    Returns (table, image_names): table as Evaluator.table(), its `image` column indexing image_names (the order the images were
    processed in, not the order given)."""
    return _run_model(model, images, annotations, lambda rows: [Evaluator(rows, batch, device)], lambda evs, _: evs[0].table(), rgb=rgb,
                      device=device, batch=batch, jpeg_decode=jpeg_decode, sorted_images=sorted_images)


def coco_evaluate(model, images, annotations, rgb=False, device=0, batch=BATCH, jpeg_decode="auto", sorted_images=None):
    """One model over `images` = [(filename, path)] through the image path of detections_table (`.jpg` files are decoded on the GPU), the
    detections handed to the COCO matcher on the device.  Returns (CocoResult, image names in processing order, detections), detections
    = {name: (boxes f32 [n,4] normalised ymin,xmin,ymax,xmax, scores f32 [n])} read back for a dump."""
    def finish(evs, outs):
        res, det = evs[0].accumulate(), {}                      # synchronises the stream
        for names, (boxes, scores, _, counts) in outs:
            n = len(names)
            bx, sc, ct = boxes.to_host((n, MAX_DETECTIONS, 4), np.float32), scores.to_host((n, MAX_DETECTIONS), np.float32), counts.to_host((n,), np.int32)
            for i, k in enumerate(names):
                c = int(min(max(ct[i], 0), MAX_DETECTIONS))
                det[k] = (bx[i, :c].copy(), sc[i, :c].copy())
        return res, det
    (res, det), order = _run_model(model, images, annotations, lambda rows: [CocoEvaluator(rows, batch, device)], finish, rgb=rgb, device=device,
                                   batch=batch, jpeg_decode=jpeg_decode, sorted_images=sorted_images)
    return res, order, det


def coco_metrics(model, images, annotations, rgb=False, device=0, batch=BATCH, jpeg_decode="auto"):
    """The dict model.evaluate prints at the end of the reference's training logs (train.py:64,70): the twelve COCO detection metrics
    (COCOeval: IoU 0.50:0.05:0.95, four area ranges in source-image pixels, maxDets 1 / 10 / 100, 101-point interpolated precision) and
    'AP_/barbell', which with one class equals 'AP'.  Computed on the GPU (vbt_coco_*, include/vbt_hip.h)."""
    return coco_evaluate(model, images, annotations, rgb=rgb, device=device, batch=batch, jpeg_decode=jpeg_decode)[0].metrics()


def coco_dump(dump_dir, annotations, sizes, per_model):
    """What pycocotools needs to cross-check the numbers on a machine that has it: DIR/instances.json (images, annotations with bbox
    xywh, area, iscrowd 0 and ids from 1, one category) and DIR/{model}_detections.json per model (COCO results format) - the boxes of
    the contract in include/vbt_hip.h, doubles written with repr.  sizes = {name: (height, width)}, per_model = {model name: detections
    of coco_evaluate}."""
    import json
    os.makedirs(dump_dir, exist_ok=True)
    ids = {name: i + 1 for i, name in enumerate(annotations)}
    anns = []
    for name, gt in annotations.items():
        for ymin, xmin, ymax, xmax in np.asarray(gt, np.int64).reshape(-1, 4).tolist():
            w, h = float(xmax) - float(xmin), float(ymax) - float(ymin)
            anns.append({"id": len(anns) + 1, "image_id": ids[name], "category_id": 1, "bbox": [float(xmin), float(ymin), w, h], "area": w * h, "iscrowd": 0})
    with open(os.path.join(dump_dir, "instances.json"), "w") as f:
        json.dump({"images": [{"id": ids[k], "file_name": k, "height": int(sizes[k][0]), "width": int(sizes[k][1])} for k in annotations],
                   "annotations": anns, "categories": [{"id": 1, "name": LABEL}]}, f)
    written = [os.path.join(dump_dir, "instances.json")]
    for mname, det in per_model.items():
        rows = []
        for name in annotations:
            boxes, scores = det[name]
            H, W = float(sizes[name][0]), float(sizes[name][1])
            for b, sc in zip(boxes.astype(np.float64).tolist(), scores.astype(np.float64).tolist()):
                x, y = b[1] * W, b[0] * H
                rows.append({"image_id": ids[name], "category_id": 1, "bbox": [x, y, b[3] * W - x, b[2] * H - y], "score": sc})
        path = os.path.join(dump_dir, f"{mname}_detections.json")
        with open(path, "w") as f:
            json.dump(rows, f)                                   # (json writes a float with repr)
        written.append(path)
    return written


def create_detections_df(models, img_dir, annotations, export_path=None, rgb=False, device=0, jpeg_decode="auto"):
    """create_detections_df of eval.py:156-215: the DataFrame with columns Score (float32), Model, IoU (float64), one row per matched
    detection, files outer / models inner in the order of `annotations` (eval.py:194-205); written to export_path as a pickle.
    jpeg_decode: where .jpg files are decoded (detections_table)."""
    import pandas as pd
    images = [(name, find_image(img_dir, name)) for name in annotations]
    srt = SortedImages(images, jpeg_decode)                    # the files are sorted by route, and the .jpg read, once for all models
    per_model = {}
    for m in models:
        table, order = detections_table(m, images, annotations, rgb=rgb, device=device, jpeg_decode=jpeg_decode, sorted_images=srt)
        first = np.searchsorted(table["image"], np.arange(len(order) + 1))       # rows of image k: first[k] .. first[k+1]
        per_model[model_name(m)] = (table, {name: (first[k], first[k + 1]) for k, name in enumerate(order)})
    scores, names, ious = [], [], []
    for name in annotations:
        for mname, (table, span) in per_model.items():
            a, b = span[name]
            scores.append(table["score"][a:b])
            ious.append(table["iou"][a:b])
            names += [mname] * int(b - a)
    df = pd.DataFrame({"Score": np.concatenate(scores).astype(np.float32) if scores else np.zeros(0, np.float32), "Model": names,
                       "IoU": np.concatenate(ious) if ious else np.zeros(0)})
    if export_path is not None:
        d = os.path.dirname(export_path)
        if d:
            os.makedirs(d, exist_ok=True)
        df.to_pickle(export_path)
    return df


def curves(df_or_table, iou_threshold=0.5, device=0):
    """{model: CurveResult} of a detections DataFrame (columns Score, Model, IoU; models in order of first appearance, eval.py:227)
    or of a mapping {model: (scores, ious)}; Label = IoU > iou_threshold (eval.py:515)."""
    if hasattr(df_or_table, "columns"):
        import pandas as pd
        tables = {m: (df_or_table["Score"][df_or_table["Model"] == m].to_numpy(), df_or_table["IoU"][df_or_table["Model"] == m].to_numpy())
                  for m in pd.unique(df_or_table["Model"])}
    else:
        tables = dict(df_or_table)
    return {m: curves_from_table(s, i, iou_threshold, device) for m, (s, i) in tables.items()}


def closest_point(thresholds, value):
    """index of the curve point whose threshold is closest to `value` (the first among equals: idxmin, eval.py:313-315,443-445)"""
    return int(np.argmin(np.abs(np.asarray(thresholds, np.float64) - value)))


def _write_figures(handle_params, figures, paths, fig_format, quality, device):
    """one handle, one set / render / encode and ONE read-back for `figures`; the files go to `paths`"""
    from .curve_figure import CurveFigure
    from .figure import write_frames
    fig = CurveFigure(device, **handle_params)
    fig.set(figures)
    return write_frames(fig, paths, fig_format, quality)


def curve_figures(kind, curves, iou_threshold, score_thresholds=None):
    """(combined figure, [per-model figure, ...]) of `kind` "pr" / "roc" as curve_figure.figure dicts: what plot_precision_recall /
    plot_roc hand to the GPU.  The per-model list is empty without score thresholds (eval.py:278-279,405-406)."""
    from . import curve_figure as CF
    pr = kind == "pr"
    thresholds = list(score_thresholds) if score_thresholds is not None else []
    titles = dict(x_title="Recall", y_title="Precision") if pr else dict(x_title="FP Rate", y_title="TP Rate")
    corner = CF.LOWER_LEFT if pr else CF.LOWER_RIGHT                                # eval.py:264,391
    series, singles = [], []
    for k, (m, c) in enumerate(curves.items()):
        xy = np.stack([c.recall, c.precision], axis=1) if pr else np.stack([c.fpr, c.tpr], axis=1)
        colour = k % CF.PALETTE_SIZE
        text = f"{m}, AP{iou_threshold * 100:.0f}={c.ap:.4f}" if pr else f"{m}, AUC={c.auc:.4f}"      # eval.py:261 (without the TeX), 388
        series.append((xy, text[:63], colour))
        if not thresholds:
            continue
        if pr:
            thr = np.r_[c.pr_thresholds, c.pr_thresholds[-1:]]                      # eval.py:235
            order = thresholds[::-1]                                                # eval.py:313
        else:
            thr, order = c.roc_thresholds, thresholds                               # eval.py:443
        marks = []
        if len(thr):
            for v in order:
                i = closest_point(thr, v)
                marks.append((0, i, f"{thr[i]:.4f}"[:15]))
        text = f"{m}, AP={c.ap:.4f}" if pr else f"{m}, AUC={c.auc:.4f}"             # eval.py:302,429
        singles.append(CF.figure([(xy, text[:63], colour)], marks, corner=corner, minor_x=50, minor_y=50, **titles))    # eval.py:305-306,435-436
    combined = CF.figure(series, corner=corner, minor_x=0 if pr else 100, minor_y=100, **titles)      # eval.py:266,393-394
    return combined, singles


def _plot(kind, stem, curves, fig_dir, iou_threshold, score_thresholds, fig_format, quality, params):
    from . import curve_figure as CF
    if fig_format not in ("jpg", "ppm"):
        raise ValueError(f"fig_format {fig_format!r}: jpg or ppm")
    os.makedirs(fig_dir, exist_ok=True)
    device = int(params.pop("device", 0))
    base = dict(CF.default_params(), **params)
    combined, singles = curve_figures(kind, curves, iou_threshold, score_thresholds)
    points = max(sum(len(xy) for xy, _, _ in combined["series"]), 1)
    base.update(max_figures=1, max_series=max(len(combined["series"]), 1), max_points=points, max_marks=0)
    written = _write_figures(base, [combined], [os.path.join(fig_dir, f"{stem}_iou_{iou_threshold}.{fig_format}")], fig_format, quality, device)
    if singles:
        one = dict(base, height=3 * base["height"] // 4, max_figures=len(singles), max_series=1, max_marks=max(len(f["marks"]) for f in singles))
        paths = [os.path.join(fig_dir, f"{stem}_{m}_iou_{iou_threshold}.{fig_format}") for m in curves]
        written += _write_figures(one, singles, paths, fig_format, quality, device)
    return written


def plot_precision_recall(curves, fig_dir, iou_threshold, score_thresholds=None, fig_format="jpg", quality=90, **params):
    """The reference's plot_precision_recall (eval.py:218) on `curves()`'s result: FIG_DIR/precision_recall_iou_{t}.jpg|ppm with every
    model, W x H, and with score thresholds one precision_recall_{m}_iou_{t} per model, W x 3H/4, in the model's colour, annotated at
    the closest curve point of each threshold.  params: width, height, scale, thickness (curve_figure.default_params), device.
    Returns the paths written."""
    return _plot("pr", "precision_recall", curves, fig_dir, iou_threshold, score_thresholds, fig_format, quality, dict(params))


def plot_roc(curves, fig_dir, iou_threshold, score_thresholds=None, fig_format="jpg", quality=90, **params):
    """The reference's plot_roc (eval.py:341): FIG_DIR/roc_iou_{t}.jpg|ppm and, with score thresholds, roc_{m}_iou_{t} per model."""
    return _plot("roc", "roc", curves, fig_dir, iou_threshold, score_thresholds, fig_format, quality, dict(params))
