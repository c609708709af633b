"""`track()` + export: the reference's per-clip hot loop (reference track.py:129-260, 103-126),
and `Pipeline`, its batched MI355X form (n clips frame-wise through detect -> NMS -> tracker on
one stream, rep analysis at the end).

No GUI: imshow / waitKey (reference track.py:237-247) are out of scope; the
annotated frames of `--video_dir` (track.py:28-62,201-224,241-242) are drawn on the GPU by
vbt_amd/overlay.py.  Frame sources are arrays / iterables of RGB uint8 frames instead of
cv2.VideoCapture (cv2 is not a dependency here).
"""
import collections
import ctypes
import os
import sys

import numpy as np

from . import _lib
from .interpreter import Interpreter
from .ocsort import LIVE_PATH_CAP, LIVE_PHASE_CAP, ROW_DTYPE, MultiClipTracker, OCSort, _live_records
from .rawvideo import colour_codes, frame_dtype, frame_shape, is_new_format, is_yuv, pix_fmt_code, source_hw
from .odt import (calc_bounding_box_center, calc_plate_height, calc_plate_width, results_to_sorttracker_inputs,
                  run_odt)

MAX_AGE = 30                                   # reference track.py:22
COLUMNS = ("id", "time", "x", "y", "dx", "dy", "norm_plate_height", "norm_plate_width")
TRACKERS = ("ocsort", "sort")                  # reference track.py:157 (the default everywhere) and its commented-out alternative, track.py:156


def _tracker_name(tracker):
    if tracker not in TRACKERS:
        raise ValueError(f"tracker must be one of {TRACKERS} (got {tracker!r})")
    return tracker


def track(src, interpreter, detection_treshold=0.5, display_image_height=720, video_path=None, fps=30.0, frame_stride=1, tracker="ocsort"):
    """Per-frame loop of reference track.py:159-234 with the reference's object call shapes.
    src: iterable of RGB uint8 frames.  frame_stride=16 reproduces `frame_count % 16` of the
    snapshot (track.py:166); the committed DataFrames were made with stride 1.
    tracker: "ocsort" = OCSort(max_age=MAX_AGE, asso_func="diou", iou_threshold=0.1) of track.py:157, "sort" = SortTracker(max_age=MAX_AGE)
    of track.py:156."""
    data = {k: [] for k in COLUMNS}
    if _tracker_name(tracker) == "sort":
        from .sort import SortTracker
        tracker = SortTracker(max_age=MAX_AGE)
    else:
        tracker = OCSort(max_age=MAX_AGE, asso_func="diou", iou_threshold=0.1)
    frame_count = 0
    for frame in src:
        frame_count += 1
        if frame_stride > 1 and frame_count % frame_stride:
            continue
        time = frame_count / fps
        results = run_odt(frame=frame, interpreter=interpreter, threshold=detection_treshold)
        if results == []:
            continue
        tracker_out = tracker.update(results_to_sorttracker_inputs(results), [], time=time)
        trackers = tracker.trackers
        for res in tracker_out:
            xmin, ymin, xmax, ymax, tracking_id, _, score = res
            bounding_box = [ymin, xmin, ymax, xmax]
            tracking_id = int(tracking_id)
            kf = None
            for trk in trackers:
                if trk.id == tracking_id - 1:
                    kf = trk.kf
                    break
            dx, dy = kf.x.flatten()[4:6]
            x_center, y_center = calc_bounding_box_center(bounding_box)
            data["id"].append(tracking_id)
            data["time"].append(time)
            data["x"].append(x_center)
            data["y"].append(y_center)
            data["dx"].append(dx)
            data["dy"].append(dy)
            data["norm_plate_height"].append(calc_plate_height(bounding_box))
            data["norm_plate_width"].append(calc_plate_width(bounding_box))
    return data


def track_frames(frames, model_path, fps=30.0, detection_treshold=0.5, frame_stride=1, time_batch=64, device=0, live=None, pix_fmt="rgb24",
                 src_hw=None, video_out=None, video_sink=None, video_quality=85, one_pass=False, hud_live=None, tracker="ocsort", display_hw=None,
                 color_matrix="bt601", color_range="limited"):
    """The whole clip loop of reference track.py:129-260 on the time-batched device path: `time_batch` consecutive (kept)
    frames of the clip per detector batch, OC-SORT walking each batch in frame order on the device, nothing but the finished
    rows coming back.  frames: uint8 [T,H,W,3] RGB (numpy array or memmap; any resolution - resized on the GPU like
    odt.py:10-19).  frame_stride = the `frame_count % 16` of track.py:166: frames whose 1-based number is not a multiple are
    read and dropped, they only advance the clip time.  Returns the reference's dict of lists (track.py:144-145).
    live: optional callable(ocsort.LiveClip, final) - live rep analysis on (a callable with a true attribute `rep_metrics` gets
    ocsort.LiveClipMetrics records, whose .metrics holds the rep metrics of the phases): called after every batch with the clip's record, and
    once more after the last one with the flush view (final=True: the phases the clip close gives).
    pix_fmt "nv12" / "i420": frames is uint8 [T, H*3//2, W], YUV 4:2:0 as a decoder emits it (rawvideo.py); converted and resized
    on the GPU.  src_hw=(H, W) is then optional (the shape gives it).  "yuyv422" / "uyvy422": uint8 [T, H, 2W], packed 4:2:2;
    "p010le": little-endian uint16 [T, H*3//2, W].  color_matrix "bt601" / "bt709" and color_range "limited" / "full": the colour
    description of a YUV source (rawvideo.py); a non-default one with rgb24 frames is a ValueError.  The exports below (video_out,
    video_sink) do not take the three newer formats or a non-default colour description: ValueError.
    video_out: optional uint8 array [T // frame_stride, ...] with the frames' layout (e.g. a numpy.lib.format.open_memmap) that receives
    every kept frame with the tracked boxes, ids and bar paths drawn (overlay.render; the reference's `--video_dir`, track.py:241-242).
    video_sink: optional mjpeg.AviWriter that receives the same frames encoded as JPEG on the device at video_quality.
    one_pass (with video_out or video_sink): the export in the same pass as the tracking instead of a second pass over the clip after
    it - each batch of kept frames is uploaded (or decoded) once into a device buffer, detected and tracked from there, drawn in place
    from the tracker's row log on the device (Overlay.follow; the rows never visit the host) and encoded or copied back.  The same
    bytes and the same rows as without it.  (The rep panel of overlay.render shows the finished analysis, which needs the whole clip: that panel has no one-pass form;
    hud_live below is the one that has.)
    hud_live (with one_pass and an export): a dict - the live rep panel on every exported frame (include/vbt_hip.h, "Rep panel from the
    live analysis"): live rep analysis is switched on (with or without `live`), the panel follows the clip on the device and shows,
    on every frame of a batch, the leader's reps as they stand after that batch.  Keys: plate_diameter (default 0.45, the live
    analysis runs with it) and the panel's x, y, scale, full_scale_cm, bg.  The rows are those of a run without it.
    tracker: "ocsort" (default) or "sort" = SortTracker(max_age=30) of track.py:156; everything above reads the row log and works with either.
    display_hw (with video_out or video_sink): (h, w) - the exported frames are drawn at full size and then resized to h x w on the
    device (include/vbt_hip.h, "Scaled export"; the reference's --display_image_height, track.py:237-239): video_out has the layout
    of (h, w), video_sink gets h x w JPEGs.  The rows are those of a run without it."""
    if hud_live is not None and not (one_pass and (video_out is not None or video_sink is not None)):
        raise ValueError("track_frames: hud_live draws on a one-pass export (one_pass=True with video_out or video_sink)")
    colour = _check_colour("track_frames", pix_fmt, color_matrix, color_range, export=video_out is not None or video_sink is not None)
    if one_pass and (video_out is not None or video_sink is not None):
        return _track_frames(frames, model_path, fps, detection_treshold, frame_stride, time_batch, device, live, pix_fmt, src_hw,
                             export=(video_out, video_sink, video_quality, display_hw), hud_live=hud_live, tracker=tracker)
    data = _track_frames(frames, model_path, fps, detection_treshold, frame_stride, time_batch, device, live, pix_fmt, src_hw, tracker=tracker,
                         color_matrix=colour[0], color_range=colour[1])
    if video_out is not None:
        from .overlay import render
        render(frames, data, fps, frame_stride=frame_stride, pix_fmt=pix_fmt, batch=time_batch, out=video_out, device=device, display_hw=display_hw)
    if video_sink is not None:
        from .overlay import render
        render(frames, data, fps, frame_stride=frame_stride, pix_fmt=pix_fmt, batch=time_batch, device=device, sink=video_sink, quality=video_quality,
               display_hw=display_hw)
    return data


def _check_colour(who, pix_fmt, color_matrix, color_range, export=False):
    """The colour description by name, lower case.  ValueError: an unknown name, a non-default description of rgb24 frames, or an
    export (drawing, scaling, JPEG encoding) of a format or colour description that only the ingest knows."""
    colour_codes(color_matrix, color_range)
    colour = (str(color_matrix).lower(), str(color_range).lower())
    default = colour == ("bt601", "limited")
    if not default and not is_yuv(pix_fmt):
        raise ValueError(f"{who}: color_matrix / color_range describe YUV frames, {pix_fmt} frames carry none")
    if export and (is_new_format(pix_fmt) or not default):
        raise ValueError(f"{who}: exported frames are drawn, scaled and encoded as rgb24, nv12 or i420 under (bt601, limited) only, "
                         f"not {pix_fmt} under ({colour[0]}, {colour[1]})")
    return colour


def _track_frames(frames, model_path, fps, detection_treshold, frame_stride, time_batch, device, live, pix_fmt, src_hw, export=None, hud_live=None,
                  tracker="ocsort", color_matrix="bt601", color_range="limited"):
    """export: None, or (video_out, video_sink, video_quality, display_hw) of a one-pass export; hud_live: None, or the live rep panel's dict"""
    _check_colour("track_frames", pix_fmt, color_matrix, color_range, export=export is not None)
    dtype = frame_dtype(pix_fmt)
    T = int(frames.shape[0])
    H, W = source_hw(frames, pix_fmt)
    if src_hw is not None and (int(src_hw[0]), int(src_hw[1])) != (H, W):
        raise ValueError(f"track_frames: src_hw {tuple(src_hw)} does not match the frames' {(H, W)}")
    stride = max(int(frame_stride), 1)
    kept = T // stride                                               # frames that are processed
    F = max(1, min(int(time_batch), max(kept, 1)))
    hud_live = None if hud_live is None else dict(hud_live)
    plate = {} if hud_live is None else dict(plate_diameter=float(hud_live.pop("plate_diameter", 0.45)))   # the live analysis uses the pipeline's
    pipe = Pipeline(model_path, F, max_frames=max(kept, 1), fps=fps, detection_treshold=detection_treshold, device=device,
                    rows_per_frame=25, tracker_clips=1, tracker=tracker, rep_metrics=bool(getattr(live, "rep_metrics", False)), **plate)
    size = pipe._size
    pipe.set_pixel_format(pix_fmt)
    pipe.set_colour(color_matrix, color_range)
    src_hw = None if (H, W) == (size, size) and not is_yuv(pix_fmt) else (H, W)
    if live is not None or hud_live is not None:
        pipe.enable_live()
    elif export is None and isinstance(frames, np.ndarray) and frames.dtype == dtype and frames.flags.c_contiguous:
        return pipe.track_clip(frames, frame_stride=stride, src_hw=src_hw)      # vbt_track_clip: the whole loop inside the library
    # any other sequence (or live analysis, or a one-pass export): chunk by chunk through contiguous host copies
    idx_all = np.arange(stride - 1, T, stride)
    dev = None
    decoded = hasattr(frames, "decode_into")
    if decoded or export is not None:
        # a compressed source (mjpeg.AviClip): only the kept frames are decoded, on the device, straight into one of two device buffers
        # that step_runs takes by pointer; nothing but compressed bytes crosses the bus.  A one-pass export puts every source's batch
        # there (one copy of the host chunk): the frames the detector reads are the frames that are drawn and written.
        if decoded and is_yuv(pix_fmt):
            raise ValueError("track_frames: a decoded source gives rgb24 frames")
        from .mem import DeviceBuffer
        shape = frame_shape(pix_fmt, H, W)
        fb = int(np.prod(shape))
        dev = [DeviceBuffer(F * fb, device) for _ in range(2)]
    ov = enc = host = scaler = None
    if export is not None:
        from .overlay import HUD_FOLLOW_FLAGGED, Overlay, follow_flag_names, hud_follow_flag_names
        video_out, video_sink, video_quality, display_hw = export
        if display_hw is not None:
            display_hw = (int(display_hw[0]), int(display_hw[1]))
        out_shape = shape if display_hw is None else frame_shape(pix_fmt, *display_hw)
        if video_out is not None and (tuple(video_out.shape) != (kept,) + out_shape or video_out.dtype != np.uint8):
            raise ValueError(f"track_frames: video_out must be uint8 {(kept,) + out_shape}, got {video_out.dtype} {tuple(video_out.shape)}")
        ov = Overlay(H, W, pix_fmt, device=device)
        ov.follow(*pipe.tracker.rows_dev(0), max_frame=max(kept * stride, 1), max_rows_per_frame=25, fps=fps)   # (a frame has at most 25 detections)
        if hud_live is not None:
            ov.hud_follow(pipe.tracker, 0, fps, **hud_live)
        if video_sink is not None and kept:
            from .mjpeg import Encoder
            enc = Encoder(H, W, pix_fmt, quality=video_quality, max_batch=F, device=device, out_hw=display_hw)
        if video_out is not None:
            host = np.empty((F,) + out_shape, np.uint8)
            if display_hw is not None and kept:                          # scaled into a third buffer behind the draw; that one is copied back
                from .scale import Scaler
                scaler = Scaler(H, W, display_hw[0], display_hw[1], pix_fmt, device=device)
                small = DeviceBuffer(F * int(np.prod(out_shape)), device)
    L = _lib.lib()
    for i0 in range(0, len(idx_all), F):
        idx = idx_all[i0:i0 + F]
        if dev is not None:
            # a buffer is written again two batches later: its forwards are waited for here, and a one-pass export has read its drawn
            # frames back by then (Encoder.read and the copy into video_out both synchronise)
            buf = dev[(i0 // F) % 2]
            pipe.join_detectors(0)                                       # the forwards that still read the buffers come first
            if decoded:
                frames.decode_into(idx, buf.ptr, 0)
            else:
                chunk = np.ascontiguousarray(frames[idx[0]:idx[-1] + 1:stride] if stride > 1 else frames[idx[0]:idx[-1] + 1], dtype=np.uint8)
                _lib.check(L.vbt_memcpy(buf.ptr, chunk.ctypes.data, chunk.nbytes, 0))
            pipe.step_runs(buf.ptr, [(0, 0, len(idx), int(idx[0]) + 1, stride)], stream=0, src_hw=src_hw)
            if ov is not None:
                if hud_live is not None and i0 + F >= len(idx_all):      # the clip's last batch: its panel is the flush view, the close's phases
                    ov.hud_follow_flush(True)
                pipe.overlay_draw(ov, buf.ptr, len(idx), int(idx[0]) + 1, stride, stream=0)
                if enc is not None:
                    enc.encode(buf.ptr, len(idx))
                    for jpeg in enc.read():
                        video_sink.write(jpeg)
                if host is not None:
                    if scaler is not None:
                        scaler.run(buf.ptr, small.ptr, len(idx), 0)
                    _lib.check(L.vbt_stream_synchronize(None))
                    _lib.check(L.vbt_memcpy(host.ctypes.data, buf.ptr if scaler is None else small.ptr, len(idx) * int(np.prod(out_shape)), 1))
                    video_out[i0:i0 + len(idx)] = host[:len(idx)]
        else:
            chunk = np.ascontiguousarray(frames[idx[0]:idx[-1] + 1:stride] if stride > 1 else frames[idx[0]:idx[-1] + 1], dtype=dtype)
            pipe.step_runs(chunk, [(0, 0, len(idx), int(idx[0]) + 1, stride)], src_hw=src_hw)
        if live is not None:
            live(pipe.live()[0], False)
    if live is not None:
        live(pipe.live(flush_view=True)[0], True)
    if ov is not None:
        _, flags = ov.follow_status(0)
        if flags:
            raise RuntimeError("track_frames: the one-pass export skipped rows of the tracker's log (VBT_OVERLAY_FOLLOW_" +
                               ", ".join(follow_flag_names(flags)) + "): the exported frames are not those of the two-pass export")
        if hud_live is not None:
            _, _, flags = ov.hud_follow_status(0)
            if flags & ~HUD_FOLLOW_FLAGGED:
                raise RuntimeError("track_frames: the live rep panel met phases it cannot show (VBT_OVERLAY_HUD_FOLLOW_" +
                                   ", ".join(hud_follow_flag_names(flags & ~HUD_FOLLOW_FLAGGED)) + "): the panel was blank on those batches")
            if flags:
                import warnings
                warnings.warn("track_frames: the live rep analysis overflowed (VBT_OVERLAY_HUD_FOLLOW_FLAGGED): the live rep panel is blank "
                              "from that batch on", RuntimeWarning)
    pipe.finish()
    return pipe.rows(0)


def track_many(sources, model_path, concurrent, fps=30.0, detection_treshold=0.5, frame_stride=1, time_batch=64, device=0, pix_fmt="rgb24",
               tracker="ocsort", color_matrix="bt601", color_range="limited"):
    """track_frames() for many clips through ONE pipeline: `concurrent` tracker slots, `time_batch` detector slots per step.  Each
    step hands runs of consecutive frames to the open clips (shard.stream_schedule); a clip whose frames are used up is closed in its
    slot (Pipeline.close_clips) and the next source opens there.  Only clips of one source resolution are open together (the
    resize is set per step).  sources: uint8 [T,H,W,3] arrays (numpy / memmap), or [T,H*3//2,W] with pix_fmt "nv12" / "i420"; fps:
    one value or one per source; tracker: "ocsort" or "sort", as in track_frames (every clip's ids start at 1).  The other pixel
    formats and color_matrix / color_range: as in track_frames, one description for all sources.
    Yields (index, rows) as clips finish - rows = the dict track_frames returns for that source."""
    from .shard import stream_schedule
    _check_colour("track_many", pix_fmt, color_matrix, color_range)
    dtype = frame_dtype(pix_fmt)
    sources = list(sources)
    fps_of = np.broadcast_to(np.asarray(fps, np.float64), (len(sources),))
    stride = max(int(frame_stride), 1)
    kept = [int(s.shape[0]) // stride for s in sources]
    hw = [source_hw(s, pix_fmt) for s in sources]
    for i in range(len(sources)):
        if kept[i] == 0:
            yield i, {k: [] for k in COLUMNS}
    if not any(kept):
        return
    pipe = Pipeline(model_path, max(1, int(time_batch)), max_frames=max(kept), fps=fps_of[0], detection_treshold=detection_treshold,
                    device=device, rows_per_frame=25, tracker_clips=int(concurrent), slot_close=True, tracker=tracker)
    size = pipe._size
    pipe.set_pixel_format(pix_fmt)
    pipe.set_colour(color_matrix, color_range)
    clip_of = {}                                     # tracker slot -> source index of the clip open in it
    unread = {}                                      # tracker slot -> source index of its close not read yet
    for opens, runs, closes in stream_schedule(kept, int(concurrent), pipe.n, groups=hw):
        for slot, i in opens:
            clip_of[slot] = i
            pipe.fps[slot] = fps_of[i]
        i0 = clip_of[runs[0][0]]
        src_hw = None if hw[i0] == (size, size) and not is_yuv(pix_fmt) else hw[i0]
        chunks = []
        for slot, _, n, f0 in runs:
            a = sources[clip_of[slot]]
            first = f0 * stride - 1                  # 0-based index of the run's first kept frame
            chunks.append(np.ascontiguousarray(a[first:first + (n - 1) * stride + 1:stride], dtype=dtype))
        pipe.step_runs(chunks, [(slot, slot0, n, f0 * stride, stride) for slot, slot0, n, f0 in runs], src_hw=src_hw)
        for slot in list(unread):                    # results the device has finished (never waits)
            got = pipe.closed(slot, wait=False)
            if got is not None:
                yield unread.pop(slot), got[1]
        if closes:
            for slot in closes:                      # a slot's previous result is read before the slot closes again: waits only if
                if slot in unread:                   # that close, a whole clip ago, is still not done
                    yield unread.pop(slot), pipe.closed(slot, wait=True)[1]
            pipe.close_clips(closes)
            for slot in closes:
                unread[slot] = clip_of.pop(slot)
    for slot in sorted(unread):
        yield unread[slot], pipe.closed(slot, wait=True)[1]


def export_dataframe(data, src_name, model_path, df_dir=None, write=True):
    """reference track.py:103-126: sort by (id,time) keeping the original row labels, pick the id with
    the largest cumulative path length, name the file f'{video}_id{id}_{model}.pkl.gz'."""
    import pandas as pd
    df = pd.DataFrame.from_dict(data)
    df = df.sort_values(by=["id", "time"])
    df2 = df.copy()
    df2["distance"] = np.where(df2["id"] == df2["id"].shift(),
                               ((df2["x"] - df2["x"].shift()) ** 2 + (df2["y"] - df2["y"].shift()) ** 2) ** 0.5, np.nan)
    df2["cumulative_distance"] = df2.groupby("id")["distance"].cumsum()
    max_distance_id = df2.loc[df2["cumulative_distance"].idxmax(), "id"]
    model_name = os.path.basename(model_path).split(".")[0]
    df_filename = f'{os.path.basename(src_name).split(".")[0]}_id{max_distance_id}_{model_name}.pkl.gz'
    df_path = df_filename if df_dir is None else os.path.join(df_dir, df_filename)
    if write:
        if df_dir is not None:
            os.makedirs(df_dir, exist_ok=True)
        df.to_pickle(df_path)
    return df, int(max_distance_id), df_path


class StreamPlacementError(RuntimeError):
    pass


def _torch():
    """torch, if the caller's process already uses it (never imported from here: the pipeline itself needs no framework)."""
    return sys.modules.get("torch")


def _host_or_device_ptr(x, pix_fmt="rgb24"):
    """(pointer, on_device, keepalive) of a frame source: a torch tensor (device or host / pinned), a numpy array, an object with
    __cuda_array_interface__, or a raw DEVICE pointer (int) the caller keeps alive.  Elements are bytes - 16-bit words for p010le
    (numpy uint16; torch uint16 or int16, the same bits)."""
    if isinstance(x, int):
        return x, True, None
    dtype = frame_dtype(pix_fmt)
    if hasattr(x, "data_ptr"):                                      # torch tensor
        ok = x.dtype == _torch().uint8 if dtype.itemsize == 1 else (x.element_size() == 2 and not x.is_floating_point())
        if not ok or not x.is_contiguous():
            raise ValueError(f"frames must be a contiguous {dtype.name} tensor")
        return x.data_ptr(), x.device.type != "cpu", x
    if hasattr(x, "__cuda_array_interface__"):
        return int(x.__cuda_array_interface__["data"][0]), True, x
    a = np.asarray(x)
    if a.dtype != dtype or not a.flags.c_contiguous:
        raise ValueError(f"frames must be a C-contiguous {dtype.name} array")
    return a.ctypes.data, False, a


class Pipeline:
    """n clips processed frame-wise - the batched form of the clip loop of reference track.py:129-260 - as a thin ctypes wrapper of
    `vbt_pipeline` (include/vbt_hip.h): streams and their placement on hardware queues, the ring of detector outputs, the staging
    ring of the host-fed mode, the deferred tracker groups and the clip close all live in libvbt_hip.so (vbt_amd/csrc/pipeline.hip).
    step(frames) enqueues detect + NMS + one OC-SORT step per clip (with `group` > 1 the network entry at once, the rest of the forward and
    the OC-SORT walk once per `group` calls - same results, wider grids); close() drains, selects each clip's export id and runs the rep
    analysis on the device.  Nothing leaves the GPU until rows() / phases() / close() are read.

    Frame sources: numpy arrays (host memory; `vbt_amd.mem.pinned_empty` gives DMA-able ones), raw device pointers, and - a
    convenience for callers who hold them - torch tensors (device or pinned host).  torch is never imported here."""

    def __init__(self, model_path, n_clips, max_frames, fps=60.0, detection_treshold=0.5, device=0, rows_per_frame=4,
                 plate_diameter=0.45, depth=None, tracker_clips=None, slot_close=False, group=None, tracker="ocsort", id_base=0,
                 rep_metrics=False):
        """tracker: "ocsort" = OCSort(max_age=30, asso_func="diou", iou_threshold=0.1) (track.py:157), "sort" = SortTracker(max_age=30)
        (track.py:156; vbt_pipeline_use_sort) whose ids start at id_base + 1 in every clip.  rep_metrics: the eight per-phase metrics
        (velocity.RM_*) next to every phase list - close_ex(), closed_ex(), and the .metrics of live()'s records."""
        L = _lib.lib()
        self.tracker_name = _tracker_name(tracker)
        self.n = int(n_clips)                       # slots of the detector batch
        # tracker_clips > n_clips: more clips than batch slots; step(clip_map=...) says which clip sits in which slot
        self.n_trk = int(tracker_clips) if tracker_clips is not None else self.n
        self.fps = np.broadcast_to(np.asarray(fps, np.float64), (self.n_trk,)).copy()
        self.thr = float(detection_treshold)
        self.plate_diameter = plate_diameter
        self._dev = int(device)
        prm = _lib.PipelineParams()
        L.vbt_pipeline_default_params(ctypes.byref(prm))
        prm.n_slots, prm.n_clips, prm.device = self.n, self.n_trk, self._dev
        prm.rows_cap = int(max_frames) * rows_per_frame + 3 * 25          # frames 1-3 may emit 25 rows each
        prm.depth = int(depth) if depth is not None else 0                 # 0: VBT_PIPELINE_DEPTH, else 4 for <= 8 slots, else 3
        prm.group = int(group) if group is not None else 0                 # 0: VBT_PIPELINE_GROUP, else 4 for 32..64 slots with a plan at hand, else 1
        prm.detection_threshold = self.thr
        prm.plate_diameter = float(plate_diameter)
        prm.model_flags = int(os.environ.get("VBT_FUSION_FLAGS", "0"))
        # --model may name a TFLite flatbuffer like the reference's (track.py:67): converted to the container format on the fly
        from .tflite_import import as_container_path
        path, temporary = as_container_path(str(model_path))
        h = ctypes.c_void_p()
        try:
            rc = L.vbt_pipeline_create(path.encode(), ctypes.byref(prm), self.fps.ctypes.data, ctypes.byref(h))
        finally:
            if temporary:
                os.unlink(path)
        if rc == -5 and "hardware queue" in L.vbt_last_error().decode():
            raise StreamPlacementError(L.vbt_last_error().decode())
        _lib.check(rc)
        self._owner = _PipelineHandle(h)            # shared with the borrowed Interpreter / tracker views: the library object lives as long as any of them
        self._h = h
        if self.tracker_name == "sort":
            from .sort import sort_params
            _lib.check(L.vbt_pipeline_use_sort(self._h, ctypes.byref(sort_params(max_age=MAX_AGE, id_base=id_base))))
        if slot_close:                              # close_clips() / closed(): their buffers now, so that no close allocates
            _lib.check(L.vbt_pipeline_close_clips_enable(self._h))
        self.rep_metrics = bool(rep_metrics)
        if self.rep_metrics:
            _lib.check(L.vbt_pipeline_rep_metrics_enable(self._h))
        info = self.info()
        self.depth, self._ring, self._defer, self._trk_inline = info.depth, info.ring, info.defer, bool(info.tracker_inline)
        self._size = info.image_size
        self.group = int(info.group)                # step() calls that share one forward (vbt_pipeline_params.group)
        self._det_streams = [_StreamHandle(info.det_streams[k]) for k in range(self.depth)]
        self._copy_stream = _StreamHandle(info.copy_stream)
        self._trk_stream = _StreamHandle(info.tracker_stream)
        self.interpreters = [Interpreter._borrowed(L.vbt_pipeline_model(self._h, k), model_path, device, self.n, self._owner) for k in range(self.depth)]
        self.interpreter = self.interpreters[0]
        self.tracker = MultiClipTracker._borrowed(L.vbt_pipeline_tracker(self._h), self.n_trk, prm.rows_cap, self._owner)
        self.tracker._rep_metrics = self.rep_metrics
        self._step_idx = 0                          # steps enqueued so far (mirror of the library's counter: which stream a step runs on)
        self._keep = collections.deque(maxlen=2 * self._ring + 4)   # host sources / foreign device arrays of the steps in flight
        self._ext = {}                              # torch.cuda.ExternalStream views of the detector streams (record_stream)
        self.pix_fmt = "rgb24"                      # set_pixel_format()

    def info(self):
        out = _lib.PipelineInfo()
        _lib.check(_lib.lib().vbt_pipeline_get_info(self._h, ctypes.byref(out)))
        return out

    @property
    def frame_count(self):
        """time counter of the clips: time = frame_count / fps (track.py:161,169)"""
        return int(self.info().frame_count)

    @frame_count.setter
    def frame_count(self, v):
        _lib.check(_lib.lib().vbt_pipeline_set_frame_count(self._h, int(v)))

    # ---- frame sources ----
    def set_pixel_format(self, pix_fmt):
        """"rgb24" (default), "nv12" or "i420" (vbt_pipeline_set_pixel_format): the format of the frames of every later step(),
        step_runs() and track_clip().  YUV 4:2:0 frames are uint8 [*, H*3//2, W] - the 2-D view of a raw frame, planes as
        include/vbt_hip.h lays them out - need src_hw=(H, W), both even, and take no swap_rb; the BT.601 conversion runs fused with the
        resize on the device.  Also "yuyv422" / "uyvy422" (uint8 [*, H, 2W], W even) and "p010le" (uint16 [*, H*3//2, W], H and W
        even); set_colour() gives the colour description of every YUV format."""
        _lib.check(_lib.lib().vbt_pipeline_set_pixel_format(self._h, pix_fmt_code(pix_fmt)))
        self.pix_fmt = str(pix_fmt).lower()

    def set_colour(self, matrix="bt601", range="limited"):
        """Colour description of the YUV frames of every later step(), step_runs() and track_clip() (vbt_pipeline_set_colour): matrix
        "bt601" / "bt709", range "limited" / "full".  Kept, but not read, while the format is "rgb24".  ValueError, nothing changed: a
        name that is neither."""
        _lib.check(_lib.lib().vbt_pipeline_set_colour(self._h, *colour_codes(matrix, range)))

    def _yuv_hw(self, src_hw, swap_rb):
        """the checks of a YUV step that the library would refuse (check_source_format, pipeline.hip), before a shape is compared"""
        if is_yuv(self.pix_fmt):
            if src_hw is None:
                raise ValueError(f"{self.pix_fmt} frames need src_hw=(H, W)")
            if swap_rb:
                raise ValueError(f"swap_rb does not apply to {self.pix_fmt} frames")

    def _caller_stream(self, stream):
        if stream is not None:
            return int(stream)
        t = _torch()
        if t is not None and t.cuda.is_available() and t.cuda.is_initialized():
            return t.cuda.current_stream().cuda_stream
        return 0

    def _source(self, x, k, n_frames=None, hw=None):
        """pointer / residency of one source; a torch device tensor is told to the caching allocator (its storage is used on the slot's
        stream up to `depth` steps after the call returns), anything else that owns memory is kept referenced while steps are in flight"""
        ptr, on_dev, keep = _host_or_device_ptr(x, self.pix_fmt)
        if keep is not None:
            shp = tuple(keep.shape)
            if is_yuv(self.pix_fmt):
                want = frame_shape(self.pix_fmt, *hw)
                if len(shp) != 3 or shp[1:] != want or (n_frames is not None and shp[0] < n_frames):
                    raise ValueError(f"{self.pix_fmt} frames must be {frame_dtype(self.pix_fmt).name} [{n_frames if n_frames is not None else 'B'}, {want[0]}, {want[1]}], got {shp}")
            elif len(shp) != 4 or shp[3] != 3 or (hw is not None and shp[1:3] != tuple(hw)) or (n_frames is not None and shp[0] < n_frames):
                raise ValueError(f"frames must be uint8 [{n_frames if n_frames is not None else 'B'}, {hw[0] if hw else 'H'}, {hw[1] if hw else 'W'}, 3], got {shp}")
            if on_dev and hasattr(keep, "record_stream"):
                t = _torch()
                if k not in self._ext:
                    self._ext[k] = t.cuda.ExternalStream(self._det_streams[k].cuda_stream, device=keep.device)
                keep.record_stream(self._ext[k])
            else:
                self._keep.append(keep)
        return ptr, on_dev

    def _enqueued(self, rc):
        """after a step call: the mirror of the library's step counter (it selects the stream a torch tensor is recorded on)"""
        if rc == 0:
            self._step_idx += 1
            return
        self._step_idx = int(self.info().steps_enqueued)
        _lib.check(rc)

    def _next_slot(self):
        """detector instance / stream the next step call enqueues on (a torch tensor is recorded on that stream)"""
        if self.group > 1:
            return int(self.info().next_slot)
        return (self._step_idx % self._ring) % self.depth

    def _hw(self, src_hw):
        return (int(src_hw[0]), int(src_hw[1])) if src_hw is not None else (self._size, self._size)

    def step(self, frames_dev_ptr, stream=None, src_hw=None, swap_rb=False, active=None, clip_map=None, frame_idx=None, track=True):
        """frames: uint8 [n,H,W,3], frame `frame_count+1` of every clip - a device tensor / raw device pointer valid on the caller's
        stream (`stream`, default: torch's current stream if torch is in use, else the null stream) and left unmodified until the step
        has run (up to `depth` steps later), or host memory (numpy array, pinned tensor), which must be final when the call is made
        and stay untouched until the step has run (vbt_pipeline_step, include/vbt_hip.h).  src_hw=(H, W) of source-resolution frames:
        the bilinear resize + truncating cast of reference odt.py:10-19 (and, with swap_rb, the BGR->RGB of track.py:171) then run on
        the device ahead of the detector.
        active: optional bool [n] - clips that still have a frame in this step (clips of different lengths batched together; the
        reference processes them one after the other, track.py:85-126).
        clip_map / frame_idx: int [n] - slot i carries frame number frame_idx[i] (1-based) of tracker clip clip_map[i] (-1: empty)."""
        k = self._next_slot()
        self._yuv_hw(src_hw, swap_rb)
        H, W = self._hw(src_hw)
        ptr, on_dev = self._source(frames_dev_ptr, k, self.n, (H, W))
        act = cm = fi = None
        if active is not None:
            act = np.ascontiguousarray(np.asarray(active, bool).astype(np.uint8))
            if act.shape != (self.n,):
                raise ValueError("active must have one entry per slot")
        if clip_map is not None:
            cm = np.ascontiguousarray(clip_map, dtype=np.int32)
            fi = np.ascontiguousarray(frame_idx, dtype=np.int32)
            if cm.shape != (self.n,) or fi.shape != (self.n,):
                raise ValueError("clip_map / frame_idx must have one entry per slot")
        self._enqueued(_lib.lib().vbt_pipeline_step(self._h, ptr, int(on_dev), H if src_hw is not None else 0, W if src_hw is not None else 0, int(bool(swap_rb)),
                                                    act.ctypes.data if act is not None else None, cm.ctypes.data if cm is not None else None,
                                                    fi.ctypes.data if fi is not None else None, int(bool(track)), self._caller_stream(stream) if on_dev else None))

    def step_runs(self, frames, runs, stream=None, src_hw=None, swap_rb=False, track=True, outputs=None):
        """Time-batched step (the reference's unit of work is ONE video, track.py:85-126,159-247): the detector batch holds RUNS of
        consecutive frames of a clip; the OC-SORT steps of a run are walked in frame order by one wavefront inside ONE tracker launch.
        runs: sequence of (clip, slot0, n_frames, frame0[, frame_step]) - frame f of the run sits in batch slot slot0 + f and is frame
        number frame0 + f * frame_step (1-based) of tracker clip `clip`; its time stamp is frame number / fps[clip].
        frames: the assembled batch [B,H,W,3] (device or host), or a list with one source [n_frames,H,W,3] per run (all device or all
        host, contiguous): the batch is then assembled in the library (one gather launch / one H2D copy per run on the copy stream).
        outputs (with track=False): (boxes [B,25,4] f32, scores [B,25] f32, classes [B,25] f32, counts [B] i32) device arrays that
        receive this step's detections instead of the pipeline's ring - the frame-major multi-GPU mode."""
        L = _lib.lib()
        if outputs is not None and track:
            raise ValueError("step_runs: outputs= is for detector-only steps (track=False)")
        k = self._next_slot()
        self._yuv_hw(src_hw, swap_rb)
        H, W = self._hw(src_hw)
        ra = (_lib.Run * len(runs))()
        B = 0
        for i, r in enumerate(runs):
            clip, slot0, nf, frame0 = (int(v) for v in r[:4])
            fstep = int(r[4]) if len(r) > 4 else 1
            if not (0 <= clip < self.n_trk) or nf < 1 or slot0 < 0 or slot0 + nf > self.n:
                raise ValueError(f"run {i}: clip {clip}, slots {slot0}..{slot0 + nf - 1} outside {self.n_trk} clips / {self.n} slots")
            ra[i] = _lib.Run(clip, slot0, 1, nf, frame0, fstep, float(self.fps[clip]))
            B = max(B, slot0 + nf)
        fptr = srcs = None
        if isinstance(frames, (list, tuple)):
            if len(frames) != len(runs):
                raise ValueError("one source tensor per run")
            used = np.zeros(B, bool)
            for r in ra:
                used[r.slot0:r.slot0 + r.n_frames] = True
            if not used.all():
                raise ValueError("step_runs: the runs leave a hole in the detector batch")
            srcs = (ctypes.c_void_p * len(runs))()
            on = set()
            for i, (src, r) in enumerate(zip(frames, ra)):
                # raw pointers base + f * frame_bytes go to the gather kernel / the copies: a short, strided or differently shaped
                # source would make them read past its allocation
                try:
                    srcs[i], d = self._source(src, k, r.n_frames, (H, W))
                except ValueError as e:
                    raise ValueError(f"step_runs: source {i}: {e}") from None
                on.add((d, str(getattr(src, "device", "host"))))
            if len(on) != 1:
                raise ValueError(f"step_runs: the sources live in different memories: {sorted(on)}")
            on_dev = on.pop()[0]
        else:
            fptr, on_dev = self._source(frames, k, B, (H, W))
        outs = [None] * 4
        if outputs is not None:
            for j, (t_, shp_, sz) in enumerate(zip(outputs, ((B, 25, 4), (B, 25), (B, 25), (B,)), (4, 4, 4, 4))):
                if tuple(t_.shape) != shp_ or t_.element_size() != sz or not t_.is_contiguous() or t_.device.type != "cuda":
                    raise ValueError(f"step_runs: outputs must be contiguous 4-byte device tensors {shp_}")
                if k not in self._ext:
                    self._ext[k] = _torch().cuda.ExternalStream(self._det_streams[k].cuda_stream, device=t_.device)
                t_.record_stream(self._ext[k])
                outs[j] = t_.data_ptr()
        self._enqueued(L.vbt_pipeline_step_runs(self._h, fptr, srcs, int(on_dev), ra, len(runs), H if src_hw is not None else 0, W if src_hw is not None else 0,
                                                int(bool(swap_rb)), int(bool(track)), outs[0], outs[1], outs[2], outs[3], self._caller_stream(stream) if on_dev else None))

    def detect_into(self, frames, boxes_ptr, scores_ptr, classes_ptr, counts_ptr, stream=None, src_hw=None, swap_rb=False, n_frames=None):
        """Detector-only step over the B <= n_slots frames of `frames` ([B,H,W,3], host or device, as step() takes them) whose
        detections go to the caller's DEVICE buffers given as raw pointers (boxes float32 [B,25,4], scores / classes float32 [B,25],
        counts int32 [B]) instead of the pipeline's ring; the tracker is not stepped.  The caller keeps the buffers alive and
        untouched until the step has run (join_detectors); no torch on this path (the detector evaluation uses it).
        n_frames: B when `frames` is a raw device pointer, which has no shape (default: all n slots); for an array it must not exceed
        the array's frames."""
        B = int(frames.shape[0]) if hasattr(frames, "shape") else self.n
        if n_frames is not None:
            if hasattr(frames, "shape") and int(n_frames) > B:
                raise ValueError(f"detect_into: n_frames {n_frames}, the array holds {B}")
            B = int(n_frames)
        if not 1 <= B <= self.n:
            raise ValueError(f"detect_into: {B} frames, the pipeline has {self.n} slots")
        k = self._next_slot()
        self._yuv_hw(src_hw, swap_rb)
        H, W = self._hw(src_hw)
        ptr, on_dev = self._source(frames, k, B, (H, W))
        run = (_lib.Run * 1)(_lib.Run(0, 0, 1, B, 1, 1, float(self.fps[0])))
        self._enqueued(_lib.lib().vbt_pipeline_step_runs(self._h, ptr, None, int(on_dev), run, 1, H if src_hw is not None else 0,
                                                         W if src_hw is not None else 0, int(bool(swap_rb)), 0, int(boxes_ptr), int(scores_ptr),
                                                         int(classes_ptr), int(counts_ptr), self._caller_stream(stream) if on_dev else None))

    def join_detectors(self, stream=None):
        """The caller's stream waits for every forward enqueued so far (after detector-only steps their outputs are then safe to read on it)."""
        _lib.check(_lib.lib().vbt_pipeline_join_detectors(self._h, self._caller_stream(stream)))

    def step_seq(self, frames, frame0=None, stream=None, **kw):
        """F consecutive frames of EVERY clip in one step: frames [n_clips, F, H, W, 3] (clip-major, device or host); the clips' frame
        counters advance by F."""
        ncl, F = int(frames.shape[0]), int(frames.shape[1])
        if ncl != self.n_trk or ncl * F > self.n:
            raise ValueError(f"step_seq: {ncl} clips x {F} frames do not fit {self.n_trk} clips / {self.n} slots")
        f0 = self.frame_count + 1 if frame0 is None else int(frame0)
        self.step_runs(frames.reshape((ncl * F,) + tuple(frames.shape[2:])), [(c, c * F, F, f0) for c in range(ncl)], stream, **kw)
        self.frame_count = f0 + F - 1

    def track_clip(self, frames, frame_stride=1, src_hw=None, swap_rb=False):
        """vbt_track_clip: the whole loop of reference track.py:129-260 for ONE clip held in memory (frames uint8 [T,H,W,3] - or
        [T,H*3//2,W] after set_pixel_format("nv12" / "i420") - host or device), `n` consecutive kept frames per detector batch.  Returns the reference's dict of lists (track.py:144-145)."""
        ptr, on_dev, keep = _host_or_device_ptr(frames, self.pix_fmt)
        T = int(frames.shape[0]) if keep is not None else None
        if T is None:
            raise ValueError("track_clip needs an array (its length is the clip's frame count)")
        self._yuv_hw(src_hw, swap_rb)
        H, W = self._hw(src_hw)
        if tuple(frames.shape[1:]) != frame_shape(self.pix_fmt, H, W):
            raise ValueError(f"track_clip: {self.pix_fmt} frames must be [T, {', '.join(str(v) for v in frame_shape(self.pix_fmt, H, W))}], got {tuple(frames.shape)}")
        cap = self.tracker.rows_cap
        ids = np.empty(cap, np.int64)
        cols = np.empty((cap, 7), np.float64)
        n = ctypes.c_int()
        _lib.check(_lib.lib().vbt_track_clip(self._h, ptr, int(on_dev), T, H if src_hw is not None else 0, W if src_hw is not None else 0, int(bool(swap_rb)),
                                             int(frame_stride), ids.ctypes.data, cols.ctypes.data, cap, ctypes.byref(n)))
        self._step_idx = int(self.info().steps_enqueued)
        d = {"id": ids[:n.value].tolist()}
        for j, nm in enumerate(COLUMNS[1:]):
            d[nm] = cols[:n.value, j].tolist()
        return d

    def reset(self):
        """Back to frame 0 of fresh clips (tracker state cleared); models, streams and buffers are kept."""
        _lib.check(_lib.lib().vbt_pipeline_reset(self._h))
        self._step_idx = 0
        self._keep.clear()

    def tracker_only_steps(self, count, slot=0):
        """Measurement split: `count` tracker steps of all clips on the detections sitting in ring slot `slot`."""
        _lib.check(_lib.lib().vbt_pipeline_tracker_only_steps(self._h, int(count), int(slot)))

    def enable_live(self, path_cap=LIVE_PATH_CAP, phase_cap=LIVE_PHASE_CAP):
        """Live rep analysis (before the first step / after reset()): after every tracker launch the rows it emitted feed a
        VelocityTracker per id that can still win the export, on the tracker's stream.  live() reads the result."""
        _lib.check(_lib.lib().vbt_pipeline_live_enable(self._h, int(path_cap), int(phase_cap)))
        self.tracker._live_phase_cap = int(phase_cap)

    def live(self, flush_view=False):
        """One ocsort.LiveClip per clip - leader (the id close() would export now), its list[velocity.Phase], seq, overflow - after
        every step enqueued so far (held-back tracker steps are drained; waits for the last tracker launch only).  flush_view: the
        phases as if the clip ended now."""
        n, cap = self.n_trk, getattr(self.tracker, "_live_phase_cap", LIVE_PHASE_CAP)
        recs = (_lib.LiveClip * n)()
        ph = np.zeros((n, cap, 6), np.float64)
        if self.rep_metrics:                        # records with .metrics: float64 [n_phases, 8] of the leader's phases
            from .ocsort import _live_records_ex
            m = np.zeros((n, cap, 8), np.float64)
            _lib.check(_lib.lib().vbt_pipeline_live_poll_ex(self._h, int(bool(flush_view)), recs, ph.ctypes.data, m.ctypes.data, cap))
            return _live_records_ex(recs, ph, m)
        _lib.check(_lib.lib().vbt_pipeline_live_poll(self._h, int(bool(flush_view)), recs, ph.ctypes.data, cap))
        return _live_records(recs, ph)

    def overlay_draw(self, ov, frames_ptr, B, frame0, frame_step=1, stream=None):
        """vbt_pipeline_overlay_draw: an overlay.Overlay that follows one of this pipeline's clips (Overlay.follow on tracker.rows_dev)
        consumes the rows of every step enqueued so far and draws B frames at device pointer `frames_ptr` - they may be the frames the
        steps were given - in place, frame i = frame number frame0 + i * frame_step.  Enqueue only, on `stream`."""
        _lib.check(_lib.lib().vbt_pipeline_overlay_draw(self._h, ov._h, int(frames_ptr), int(B), int(frame0), int(frame_step), self._caller_stream(stream)))

    def skip_frames(self, n=1):
        """Frames read from the source but not processed (`frame_count % 16` of reference track.py:161-167): they advance the clip
        time and nothing else - no ring slot is used."""
        _lib.check(_lib.lib().vbt_pipeline_skip_frames(self._h, int(n)))

    def _drain(self):
        _lib.check(_lib.lib().vbt_pipeline_drain(self._h))

    def finish(self, stream=None):
        _lib.check(_lib.lib().vbt_pipeline_finish(self._h))

    def close(self, cap=32):
        """Clip close in one go: drain the pipeline, export-id selection + rep analysis on the device, then ONE packed device-to-host
        copy and ONE stream synchronisation.  Returns (best_ids[n], n_rows[n], n_phases[n], overflow[n], phases[n, cap, 6]) - per clip
        the id of reference track.py:107-115 and the Phase list of plot.py:33-47."""
        n = self.n_trk
        best, rows, nph, ovf = (np.zeros(n, np.int32) for _ in range(4))
        ph = np.zeros((n, cap, 6), np.float64)
        _lib.check(_lib.lib().vbt_pipeline_close(self._h, best.ctypes.data, rows.ctypes.data, nph.ctypes.data, ovf.ctypes.data, ph.ctypes.data, int(cap)))
        return best, rows, nph, ovf, ph

    def close_ex(self, cap=32):
        """close() + metrics[n, cap, 8] (a pipeline created with rep_metrics=True), all in the one packed copy"""
        n = self.n_trk
        best, rows, nph, ovf = (np.zeros(n, np.int32) for _ in range(4))
        ph, m = np.zeros((n, cap, 6), np.float64), np.zeros((n, cap, 8), np.float64)
        _lib.check(_lib.lib().vbt_pipeline_close_ex(self._h, best.ctypes.data, rows.ctypes.data, nph.ctypes.data, ovf.ctypes.data, ph.ctypes.data,
                                                    m.ctypes.data, int(cap)))
        return best, rows, nph, ovf, ph, m

    def close_clips(self, clips, next_fps=None):
        """Slot close (a pipeline created with slot_close=True): the listed tracker slots' clips end while the others keep running, and
        each slot starts a fresh clip (fps next_fps - one value or one per slot - or the slot's current one).  Only enqueues
        (vbt_pipeline_close_clips); closed() reads a slot's result, and must have done so before the slot is closed again."""
        cl = np.ascontiguousarray(np.atleast_1d(np.asarray(clips, np.int32)))
        nf = None
        if next_fps is not None:
            nf = np.ascontiguousarray(np.broadcast_to(np.asarray(next_fps, np.float64), cl.shape))
        _lib.check(_lib.lib().vbt_pipeline_close_clips(self._h, cl.ctypes.data, len(cl), nf.ctypes.data if nf is not None else None))
        if nf is not None:
            self.fps[cl] = nf

    def closed(self, clip, wait=True):
        """The result of slot `clip`'s last close_clips(): None while the device has not done it (wait=False), else
        (best_id, rows, phases, overflow) - the export id of reference track.py:107-115, the clip's rows as rows() gives them, its
        list[velocity.Phase] (plot.py:33-47) and the tracker's overflow flags; export_dataframe() takes the rows as they are."""
        return self._closed(clip, wait, False)

    def closed_ex(self, clip, wait=True):
        """closed() + the phases' metrics, float64 [P, 8] (a pipeline created with rep_metrics=True): (best_id, rows, phases, overflow,
        metrics)"""
        return self._closed(clip, wait, True)

    def _closed(self, clip, wait, metrics):
        from .ocsort import _phase_list
        rec = _lib.ClosedClip()
        ready = ctypes.c_int()
        ph = np.zeros((512, 6), np.float64)
        rows = np.empty(self.tracker.rows_cap, ROW_DTYPE)
        if metrics:
            m = np.zeros((512, 8), np.float64)
            _lib.check(_lib.lib().vbt_pipeline_closed_clip_ex(self._h, int(clip), int(bool(wait)), ctypes.byref(ready), ctypes.byref(rec),
                                                              ph.ctypes.data, m.ctypes.data, len(ph), rows.ctypes.data, len(rows)))
        else:
            _lib.check(_lib.lib().vbt_pipeline_closed_clip(self._h, int(clip), int(bool(wait)), ctypes.byref(ready), ctypes.byref(rec), ph.ctypes.data,
                                                           len(ph), rows.ctypes.data, len(rows)))
        if not ready.value:
            return None
        r = rows[:rec.n_rows]
        d = {"id": r["id"].tolist()}
        for nm in COLUMNS[1:]:
            d[nm] = r[nm].tolist()
        out = (int(rec.best_id), d, _phase_list(ph[:rec.n_phases]), int(rec.overflow))
        return out + (m[:rec.n_phases].copy(),) if metrics else out

    def rows_all(self, cap=None, out=None):
        """DataFrame rows of every clip, one strided copy (after close() / finish()): (counts[n], rows[n, cap] of ROW_DTYPE).  `out`:
        optional preallocated (pinned) buffer of at least n * cap * 64 bytes (torch tensor or numpy array)."""
        n = self.n_trk
        cap = int(cap or self.tracker.rows_cap)
        counts = np.zeros(n, np.int32)
        if out is None:
            rows = np.zeros((n, cap), ROW_DTYPE)
            ptr = rows.ctypes.data
        elif hasattr(out, "data_ptr"):
            rows = out.numpy().view(np.uint8).reshape(-1)[:n * cap * 64].view(ROW_DTYPE).reshape(n, cap)
            ptr = out.data_ptr()
        else:
            rows = np.frombuffer(out, np.uint8)[:n * cap * 64].view(ROW_DTYPE).reshape(n, cap)
            ptr = rows.ctypes.data
        _lib.check(_lib.lib().vbt_pipeline_rows_all(self._h, counts.ctypes.data, ptr, cap))
        return counts, rows

    def rows(self, clip):
        cap = self.tracker.rows_cap
        ids = np.empty(cap, np.int64)
        cols = np.empty((cap, 7), np.float64)
        n = ctypes.c_int()
        _lib.check(_lib.lib().vbt_pipeline_rows(self._h, int(clip), ids.ctypes.data, cols.ctypes.data, cap, ctypes.byref(n)))
        d = {"id": ids[:n.value].tolist()}
        for j, nm in enumerate(COLUMNS[1:]):
            d[nm] = cols[:n.value, j].tolist()
        return d

    def phases(self, clip):
        return self.tracker.phases(clip)

    def detections(self):
        """Most recent step's detector outputs (host copies) - for tests."""
        b = np.empty((self.n, 25, 4), np.float32)
        s = np.empty((self.n, 25), np.float32)
        c = np.empty((self.n, 25), np.float32)
        cnt = np.empty((self.n,), np.int32)
        B = ctypes.c_int()
        _lib.check(_lib.lib().vbt_pipeline_detections(self._h, b.ctypes.data, s.ctypes.data, c.ctypes.data, cnt.ctypes.data, self.n, ctypes.byref(B)))
        return b[:B.value], s[:B.value], c[:B.value], cnt[:B.value]


class _PipelineHandle:
    """Owner of a vbt_pipeline handle (destroyed with the last reference: the Pipeline and every view borrowed from it)."""

    def __init__(self, h):
        self.h = h

    def __del__(self):
        h, self.h = self.h, None
        if h and _lib is not None and getattr(_lib, "_lib", None) is not None:
            _lib._lib.vbt_pipeline_destroy(h)


class _StreamHandle:
    """A HIP stream owned by the library, as the raw handle (`.cuda_stream`, the attribute name torch uses)."""

    def __init__(self, handle):
        self.cuda_stream = int(handle or 0)

    def synchronize(self):
        _lib.check(_lib.lib().vbt_stream_synchronize(self.cuda_stream))
