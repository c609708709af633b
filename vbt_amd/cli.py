"""Command line mirror of the reference's entry points, minus GUI/plotting:

  python -m vbt_amd.cli track SRC... [--model M] [--detection_treshold 0.5] [--df_dir DIR] [--video_dir DIR] [--fps 30] [--frame_stride 1]
                            [--live [--report] [--stop_loss PCT]] [--tracker ocsort|sort] [--concurrent N] [--pix_fmt nv12|i420|yuyv422|uyvy422|p010le|rgb24 --size WxH] [--color_matrix bt601|bt709]
                            [--color_range limited|full] [--video_format raw|mjpeg] [--video_quality 85] [--mjpeg_entropy auto|interval|sync] [--hud [--plate_diameter 0.45] [--hud_scale 3] [--hud_pos 16,16]] [--one_pass [--live_hud]]
                            [--display_image_height N]
      reference track.py:65-126.  SRC = .npy stack of RGB uint8 frames [T,H,W,3], or a Motion-JPEG .avi (the reference's
      cv2.VideoCapture, track.py:129-160; cv2 is not a dependency here: the frames are decoded on the GPU - include/vbt_hip.h, "MJPEG
      import" - and --fps, when not given, is the file's rate / scale; --size and a YUV --pix_fmt do not apply to it;
      --mjpeg_entropy picks how its scans are entropy-decoded - one lane per restart interval, subsequences that synchronise (for files
      without restart markers: ffmpeg, cameras, Pillow), or auto by interval length - with the same frames either way); any source
      resolution (resized on the GPU like odt.py:10-19).  Writes
      {video}_id{N}_{model}.pkl.gz with the reference's columns, sort order and retained row labels.
      --live: prints each concentric rep of the clip's leading id as soon as it is complete, in the format of `analyze`; a rep
      list that changes afterwards (the leading id changes, or a larger rep makes the filter drop small ones) is announced with a
      "revised" line and reprinted from the first rep that differs.  The reps standing at the end are those `analyze` prints.
      --live --report: the rep lines of `analyze --report` instead (peak velocity, time to peak, vertical ROM, sideways excursion,
      velocity loss), from the rep metrics formed on the device inside the live analysis.  --live --stop_loss PCT: one "STOP" line
      at the first rep whose loss against the best rep so far reaches PCT percent (finite, > 0) - the set should end there.
      --tracker sort: SortTracker(max_age=30), the commented-out alternative of reference track.py:16,156 (it made the reference's
      dfs/ frames), instead of OCSort (track.py:157, the default); the file name rule and every other option are the same.
      --concurrent N > 1: all files through one pipeline, N clips side by side (a finished clip's tracker slot takes the next
      file); the same files and lines as N = 1, in input order.  Not with --live.
      --pix_fmt nv12|i420 --size 1920x1080: SRC is a headerless raw video file, YUV 4:2:0 as a decoder emits it (what
      `ffmpeg -i clip.mp4 -pix_fmt nv12 -f rawvideo clip.yuv` writes; nothing here runs ffmpeg), mapped read-only; colour conversion and
      resize run fused on the GPU.  --pix_fmt rgb24 --size WxH reads packed raw RGB the same way; without --size SRC is a .npy stack.
      --pix_fmt yuyv422|uyvy422|p010le --size WxH: packed 4:2:2 as webcams and capture cards deliver it, 10-bit 4:2:0 as hardware
      decoders do.  --color_matrix bt601|bt709 and --color_range limited|full describe any YUV source (HD material is bt709, ffmpeg's
      yuvj420p is i420 with full range); not for rgb24 or .avi sources.  These three formats and non-default colour descriptions are
      tracked, not drawn: --video_dir, --one_pass, --hud, --live_hud and --display_image_height are usage errors with them.
      --video_dir DIR (reference track.py:71,96-98,241-242): every processed frame with the tracked boxes, ids and bar paths drawn on
      the GPU (include/vbt_hip.h, "tracking overlay"), as DIR/{video}.npy for .npy sources and as DIR/{video}.rgb / .yuv - headerless,
      in the source's pixel format, what `ffmpeg -f rawvideo -pix_fmt nv12 -s WxH -i` reads - for --size sources.  Unlike the reference,
      frames on which nothing was detected are written too (undrawn): the video does not jump in time.
      --video_format mjpeg: DIR/{video}.avi instead, for every source kind and pixel format - the drawn frames encoded as baseline JPEG
      on the GPU (include/vbt_hip.h, "MJPEG export") at --video_quality, in an AVI that players open; only the compressed bytes are
      copied back.  Its frame rate is fps / frame_stride, so the export plays in real time - a second deliberate difference: the
      reference writes every 16th frame at the source's full fps (track.py:153-154,166), which plays 16 times too fast.
      --hud (with --video_dir): the rep panel on every exported frame, drawn on the GPU with the rest (include/vbt_hip.h, "Rep
      panel") - what the reference's figure shows (plot.py:112-232): the rep count, ROM and ACV of the last completed rep, a bar per
      recent rep and the phase timeline of the export id, exactly the phases `analyze` prints for the exported DataFrame.  The phases
      exist once the clip is analysed, so with --hud the frames are rendered after tracking, for every --concurrent.
      --one_pass (with --video_dir): the export in the same pass as the tracking - each batch of frames is uploaded or decoded once,
      detected, tracked, drawn from the tracker's row log on the device (include/vbt_hip.h, "Following a device row log") and written,
      instead of a second pass over the clip after it.  The same files, byte for byte.  Not with --hud (the panel shows the analysed
      clip) and not with --concurrent above 1.
      --live_hud (with --one_pass --video_dir): the rep panel of --hud fed by the live rep analysis on the device (include/vbt_hip.h,
      "Rep panel from the live analysis"): rep count, ROM and ACV appear on the exported video as each rep completes, with nothing
      copied to the host.  Every frame of a batch (--time_batch) shows the leading id's reps as they stand after that batch; the
      last batch shows what `analyze` prints.  Unlike --hud the count can go down again (the leading id changes, or a larger rep
      makes the filter drop small ones).  Takes --plate_diameter, --hud_scale and --hud_pos; not with --hud, not with --concurrent
      above 1.
      --display_image_height N (with --video_dir; reference track.py:69,139-140,237-239): every exported frame is drawn at full
      size and then resized on the GPU to N lines, the width following the source's aspect ratio - int(N * (W / H)), rounded down to
      even for nv12 / i420 - with cv2.resize's default filter (include/vbt_hip.h, "Scaled export").  The reference resizes what it
      shows in a window and defaults to 720; there is no window here, the export is resized instead and the default is the full size.
      Works with every --video_format, --hud, --one_pass, --live_hud, --concurrent and source kind; the panels are placed and checked
      against the source size and shrink with the frame.
  python -m vbt_amd.cli overlay SRC DATAFRAME [--fps 30] [--frame_stride 1] [--pix_fmt ... --size WxH] [--video_dir DIR]
                              [--video_format raw|mjpeg] [--video_quality 85] [--mjpeg_entropy auto|interval|sync]
                              [--hud [--plate_diameter 0.45] [--hud_scale 3] [--hud_pos 16,16]] [--display_image_height N]
      the same frames drawn later, from the clip and a stored {video}_id{N}_{model}.pkl.gz (all its ids are drawn; --hud takes the
      panel's id from the file name).
  python -m vbt_amd.cli analyze DF.pkl.gz... [--plate_diameter 0.45] [--report [--report_csv FILE]]
      reference plot.py:50-70,73-95,163-173 without the figure: parses {video}_id{N}_{model}.pkl.gz, applies the
      rolling(5)/expanding preprocessing and the VelocityTracker on the GPU, prints ROM and ACV per concentric rep.
      --report: each rep line goes on with PV (peak velocity), TTP (time from the rep's start to the peak), vROM (vertical travel),
      xdev (largest sideways excursion from the start) and loss (velocity loss in percent against the best rep so far); then a "set:"
      line (reps, best / mean ACV, mean / max PV, loss of the last rep, summed concentric / eccentric time, mean xdev).
      --report_csv FILE: one row per concentric rep of every DataFrame, all eight rep metrics, floats written exactly.
  python -m vbt_amd.cli plot DF.pkl.gz... --fig_dir DIR [--plate_diameter 0.45] [--fig_size 1280x800] [--fig_scale 2] [--fig_format jpg|ppm]
                           [--fig_quality 90]
      reference plot.py:50-232 with the figure, and without matplotlib: per DataFrame the smoothed position and velocity curves, a
      tinted span per phase and ROM / ACV over every concentric phase, rendered on the GPU (include/vbt_hip.h, "Rep figure") and written
      as DIR/{name}.jpg (baseline JPEG encoded on the GPU) or DIR/{name}.ppm (the raw frame behind a P6 header) - plot.py:220's name
      with the new extension.  Up to 64 files go through one upload, one render and one encode.  Prints what `analyze` prints.
      There is no display, so --show_fig is not offered.
  python -m vbt_amd.cli validate [--kinovea_dir D | --qualysis_dir D] [--df_dir dfs] [--plate_diameter 0.45]
      [--fig_dir D [--fig_format jpg|ppm] [--fig_quality 90]]
      reference kinovea.py:29-38,57-172,203-215 / qualysis.py:29-38,57-187: per export with a
      matching {video}_id{N}_{model}.pkl.gz, MSE and Pearson r of x(t) and y(t) in metres, then the totals line.  With --fig_dir the
      numbers and the reference's figure of every pair (kinovea.py:124-154,195-197; written there as .pdf) come from one batch on the
      GPU (vbt_validation) as DIR/{video}_id{N}_{model}.jpg|ppm; the lines keep their formats, the last bits of the totals differ from
      the default path's (another summation order).  No --show_fig (no display), no LaTeX table, no p-values.
  python -m vbt_amd.cli eval MODELS... [--img_dir data/test] [--annotations_dir data/test] [--iou_threshold 0.5]
                           [--detections_df dfs/eval_detections.pkl.gz] [--replace_df] [--score_thresholds "[0.2, 0.5]"] [--curve_dir DIR] [--rgb]
                           [--jpeg_decode auto|gpu|host] [--fig_dir DIR] [--fig_size 1120x640] [--fig_scale 2] [--fig_format jpg|ppm] [--fig_quality 90]
                           [--coco [--coco_dump DIR]]
      reference eval.py:471-521: VOC annotations, every image through each model at threshold 0 (.jpg files decoded on the GPU
      straight to the network input, mixed sizes in one batch; --jpeg_decode host: with PIL as before), Hungarian
      matching and the PR / ROC curves on the GPU; writes (or, when it exists and --replace_df is not given, reads) the detections
      DataFrame, prints AP and AUC per model as the reference's legends show them and, for each --score_thresholds value, the
      closest curve point; --curve_dir writes the curve points as CSV.  --fig_dir writes, after the lines, the reference's figures
      (eval.py:218-468), rendered and encoded on the GPU: precision_recall_iou_{t} and roc_iou_{t} with every model and, with
      --score_thresholds, precision_recall_{m}_iou_{t} and roc_{m}_iou_{t} per model, annotated at the closest curve points.
      --coco prints, after all that, one line `model: {'AP': ..., ..., 'AP_/barbell': ...}` per model: the twelve COCO detection metrics
      and the per-class AP that model.evaluate prints at the end of the reference's training logs (train.py:64,70), matched and
      accumulated on the GPU; it always runs the models (the stored DataFrame has neither boxes nor unmatched detections).  --coco_dump DIR
      writes instances.json and {model}_detections.json for a cross-check with pycocotools on a machine that has it.
Option names (including the reference's `treshold` / `qualysis` spellings) and defaults follow the reference.
"""
import contextlib
import math
import os
import re

import click
import numpy as np

FILENAME_RE = re.compile(r"(\S*)_id(\d+)_(\S*)\.pkl\.gz")           # reference plot.py:19-25
DEFAULT_MODEL = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "models", "efficientdet_lite0_synth.vbtm")


@click.group()
def main():
    pass


def _rep_line(i, p):
    return f"  rep {i}: t {p.time_start:.4f}-{p.time_end:.4f} s  ROM {p.rom:.6f} m  ACV {p.rom / p.duration:.6f} m/s"


def _report_lines(phases, metrics, stop_loss=0.0):
    """--report: (the extended rep lines, the set line, the SetReport) of one id's phases and their rep metrics"""
    from .velocity import RM_PV, RM_ROM_Y, RM_T_PV, RM_X_DEV, Phase, set_report
    rep = set_report(phases, metrics, stop_loss)
    lines = []
    for k, (p, m) in enumerate(((p, m) for p, m in zip(phases, metrics) if p.type == Phase.CONCENTRIC), 1):
        lines.append(_rep_line(k, p) + f"  PV {m[RM_PV]:.6f} m/s  TTP {m[RM_T_PV] - p.time_start:.4f} s  vROM {m[RM_ROM_Y]:.6f} m"
                                       f"  xdev {m[RM_X_DEV]:.6f} m  loss {rep.loss_pct[k - 1]:.2f} %")
    return lines, _set_line(rep), rep


def _set_line(rep):
    return (f"  set: {rep.n_reps} reps  best ACV {rep.best_mv:.6f} m/s (rep {rep.best_rep})  mean ACV {rep.mean_mv:.6f} m/s  mean PV {rep.mean_pv:.6f} m/s"
            f"  max PV {rep.max_pv:.6f} m/s  loss {rep.loss_last_pct:.2f} %  concentric {rep.concentric_s:.4f} s  eccentric {rep.eccentric_s:.4f} s"
            f"  mean xdev {rep.mean_x_dev:.6f} m")


REPORT_CSV_COLUMNS = ("video", "id", "rep", "time_start", "time_end", "rom", "acv", "pv", "t_pv", "time_to_peak", "rom_y", "rom_x", "pv_y", "x_dev",
                      "n_steps", "loss_pct")


def _report_csv_rows(video, tid, phases, metrics, rep):
    """--report_csv: one row per concentric rep; floats as repr() writes them, so that they read back exactly"""
    from .velocity import RM_MV, RM_N_STEPS, RM_PV, RM_PV_Y, RM_ROM_X, RM_ROM_Y, RM_T_PV, RM_X_DEV, Phase
    rows = []
    for k, (p, m) in enumerate(((p, m) for p, m in zip(phases, metrics) if p.type == Phase.CONCENTRIC), 1):
        vals = [p.time_start, p.time_end, p.rom, m[RM_MV], m[RM_PV], m[RM_T_PV], m[RM_T_PV] - p.time_start, m[RM_ROM_Y], m[RM_ROM_X], m[RM_PV_Y],
                m[RM_X_DEV], m[RM_N_STEPS], rep.loss_pct[k - 1]]
        rows.append([video, tid, k] + [repr(float(v)) for v in vals])
    return rows


class _LiveReps:
    """track --live: the concentric reps of the clip's leader as they complete (see the module docstring).  report: the extended rep
    line of `analyze --report` (the records then carry rep metrics); stop_loss > 0: one STOP line at the first rep whose velocity loss
    reaches it (and again should a revision move it)."""

    def __init__(self, name, report=False, stop_loss=None):
        self.name, self.shown, self.warned = name, [], False
        self.report, self.stop_loss, self.stop_shown = report, stop_loss, None
        self.rep_metrics = report or stop_loss is not None        # what track_frames reads

    def __call__(self, rec, final):
        from .velocity import Phase
        if rec.overflow:
            if not self.warned:
                click.echo(f"{self.name}: live analysis overflow (flags {rec.overflow}); live reps stop here", err=True)
                self.warned = True
            return
        lines = [_rep_line(i, p) for i, p in enumerate((p for p in rec.phases if p.type == Phase.CONCENTRIC), 1)]
        stop = None
        if self.rep_metrics:
            ext, _, rep = _report_lines(rec.phases, rec.metrics, self.stop_loss or 0.0)
            if self.report:
                lines = ext
            if rep.stop_rep:
                stop = f"  STOP: rep {rep.stop_rep} lost {rep.loss_pct[rep.stop_rep - 1]:.2f} % (threshold {self.stop_loss:g} %)"
        k = 0
        while k < min(len(lines), len(self.shown)) and lines[k] == self.shown[k]:
            k += 1
        if k < len(self.shown):
            click.echo(f"  revised: id {rec.leader}, from rep {k + 1}")
        for ln in lines[k:]:
            click.echo(ln)
        self.shown = lines
        if stop is not None and stop != self.stop_shown:
            click.echo(stop)
            self.stop_shown = stop


ANALYZE_COLUMNS = ("time", "x", "y", "dx", "dy", "norm_plate_height", "norm_plate_width")


def _id_phases(df, tid, plate_diameter, metrics=False):
    """The phases of id `tid` of an exported DataFrame (reference plot.py:73-95): what `analyze` prints and what --hud shows.
    metrics: (phases, their rep metrics [P,8])"""
    from .velocity import analyze_rows
    df = df.query(f"id == {tid}").drop(columns=["id"])
    return analyze_rows(np.stack([df[c].to_numpy(np.float64) for c in ANALYZE_COLUMNS], axis=1), plate_diameter, preprocess=True, metrics=metrics)


def _hud_options(f):
    """--hud and what goes with it, for `track` and `overlay`"""
    for opt in (click.option("--hud_pos", default="16,16", show_default=True, type=str, help="X,Y of the rep panel's top left corner (even for nv12 / i420)."),
                click.option("--hud_scale", default=3, show_default=True, type=click.IntRange(1, 64), help="Pixels per cell of the rep panel (52 x 50 cells)."),
                click.option("--plate_diameter", default=0.45, show_default=True, type=float, help="Diameter of the weight plate used in meters (for --hud)."),
                click.option("--hud", is_flag=True, default=False,
                             help="Draw the rep panel on the exported frames: rep count, ROM / ACV of the last rep, a bar per rep, phase timeline (needs --video_dir).")):
        f = opt(f)
    return f


def _hud_params(hud, video_dir, hud_scale, hud_pos):
    """None without --hud, else the panel's parameters for overlay.render"""
    if not hud:
        return None
    if video_dir is None:
        raise click.UsageError("--hud draws on the exported frames: give --video_dir")
    m = re.fullmatch(r"\s*(\d+)\s*,\s*(\d+)\s*", hud_pos)
    if not m:
        raise click.BadParameter(f"expected X,Y (two non-negative integers), got {hud_pos!r}", param_hint="--hud_pos")
    return dict(x=int(m.group(1)), y=int(m.group(2)), scale=int(hud_scale))


def _display_option(f):
    """--display_image_height, for `track` and `overlay`"""
    return click.option("--display_image_height", default=None, type=int,
                        help="Height in lines of the exported frames: each is drawn at full size, then resized on the GPU, the width following the "
                             "source's aspect ratio (needs --video_dir; even for nv12 / i420).  Default: the source's own size - the reference's "
                             "default of 720 applied to the window it shows, not to a file.")(f)


def _check_display_height(display_image_height, video_dir, pix_fmt):
    """the refusals of --display_image_height that need no source, before anything is opened or written"""
    from .rawvideo import is_yuv
    if display_image_height is None:
        return
    if video_dir is None:
        raise click.UsageError("--display_image_height is the size of the exported frames: give --video_dir")
    if not 1 <= display_image_height <= 16384:
        raise click.UsageError(f"--display_image_height {display_image_height} is outside 1..16384")
    if is_yuv(pix_fmt) and display_image_height % 2:
        raise click.UsageError(f"--display_image_height {display_image_height} is odd: {pix_fmt} frames have an even height")


def _display_hw(frames, pix_fmt, display_image_height):
    """None without --display_image_height, else (h, w) of the export of this source (scale.display_size); a width outside 1..16384
    is a usage error, raised while nothing has been written for the source yet"""
    if display_image_height is None:
        return None
    from ._lib import VbtArgError
    from .rawvideo import source_hw
    from .scale import display_size
    H, W = source_hw(frames, pix_fmt)
    try:
        return display_size(H, W, pix_fmt, display_image_height)
    except VbtArgError as e:
        raise click.UsageError(f"--display_image_height: {e}")


def _open_source(s, pix_fmt, size, mjpeg_entropy="auto"):
    """One SRC of `track` as the clip array of its pixel format: a .npy stack (no --size) or a headerless raw video file."""
    from .rawvideo import open_raw
    if not os.path.isfile(s):
        raise FileNotFoundError(s)                                       # reference track.py:89-90
    if mjpeg_entropy != "auto" and not _is_avi(s):
        raise click.UsageError(f"{s}: --mjpeg_entropy {mjpeg_entropy} is about decoding an .avi source and does not apply to this one")
    if _is_avi(s):
        if size is not None or pix_fmt != "rgb24":
            raise click.UsageError(f"{s}: an .avi source carries its own frame size and decodes to RGB: --size and --pix_fmt {pix_fmt} do not apply")
        from ._lib import VbtError
        from .mjpeg import AviClip
        try:
            return AviClip(s, entropy=mjpeg_entropy)
        except (ValueError, VbtError) as e:
            raise click.ClickException(str(e))
    if size is not None:
        try:
            return open_raw(s, pix_fmt, size)
        except ValueError as e:
            raise click.ClickException(str(e))
    frames = np.load(s, mmap_mode="r")
    if frames.ndim != 4 or frames.shape[3] != 3 or frames.dtype != np.uint8:
        raise click.ClickException(f"{s}: expected uint8 [T,H,W,3], got {frames.dtype} {frames.shape}")
    return frames


def _is_avi(s):
    return str(s).lower().endswith(".avi")


def _fps_given():
    """was --fps on the command line?  (an .avi source otherwise brings its own rate / scale)"""
    from click.core import ParameterSource
    return click.get_current_context().get_parameter_source("fps") == ParameterSource.COMMANDLINE


def _source_fps(frames, fps, given):
    return fps if given or not hasattr(frames, "fps") else float(frames.fps)


def _check_colour_options(src, pix_fmt, color_matrix, color_range, exports):
    """The usage errors of the formats and colour descriptions that are tracked but not drawn, before anything is opened.
    exports: option name -> was it given, for every option that draws, scales or encodes frames."""
    from .rawvideo import is_new_format, is_yuv
    given = [f"{o} {v}" for o, v, d in (("--color_matrix", color_matrix, "bt601"), ("--color_range", color_range, "limited")) if v != d]
    if given and not is_yuv(pix_fmt):
        raise click.UsageError(f"{' '.join(given)} describes a YUV source: --pix_fmt {pix_fmt} frames carry no colour description")
    avi = [s for s in src if _is_avi(s)]
    if given and avi:
        raise click.UsageError(f"{' '.join(given)} does not apply to {avi[0]}: a JPEG carries its own colour description")
    what = ([f"--pix_fmt {pix_fmt}"] if is_new_format(pix_fmt) else []) + given
    asked = [o for o, on in exports.items() if on]
    if what and asked:
        raise click.UsageError(f"{' '.join(what)} is tracked but not drawn: exporting frames ({', '.join(asked)}) takes rgb24, nv12 or i420 "
                               "sources under bt601 / limited only")


def _raw_size(pix_fmt, size):
    """--size as (W, H), or None for .npy sources; the combinations `track` refuses"""
    from .rawvideo import frame_shape, is_yuv, parse_size
    if size is None:
        if is_yuv(pix_fmt):
            raise click.UsageError(f"--pix_fmt {pix_fmt} reads headerless raw video: give the frame size with --size WIDTHxHEIGHT")
        return None
    try:
        wh = parse_size(size)
        frame_shape(pix_fmt, wh[1], wh[0])
    except ValueError as e:
        raise click.BadParameter(str(e), param_hint="--size")
    return wh


@main.command()
@click.argument("src", type=str, nargs=-1)
@click.option("--model", default=DEFAULT_MODEL, show_default=True, type=str, help="VBTM model container.")
@click.option("--detection_treshold", default=0.5, show_default=True, type=float, help="Object detection threshold.")
@click.option("--df_dir", default=None, show_default=True, help="Directory for exporting the dataframes.")
@click.option("--fps", default=30.0, show_default=True, type=float, help="Frame rate of the source (cap.get(CAP_PROP_FPS) in the reference).")
@click.option("--frame_stride", default=1, show_default=True, type=int, help="16 reproduces `frame_count %% 16` of reference track.py:166.")
@click.option("--time_batch", default=64, show_default=True, type=int, help="Consecutive frames of the clip per detector batch (1 = one frame per step).")
@click.option("--live", is_flag=True, default=False, help="Print each concentric rep (ROM, ACV) as soon as it is complete.")
@click.option("--report", is_flag=True, default=False,
              help="With --live: the extended rep line of `analyze --report` (peak velocity, time to peak, vertical ROM, sideways excursion, loss).")
@click.option("--stop_loss", default=None, type=float,
              help="With --live: print one STOP line at the first rep whose velocity loss against the best rep so far reaches this percentage.")
@click.option("--tracker", default="ocsort", show_default=True, type=click.Choice(["ocsort", "sort"]),
              help="ocsort: OCSort(max_age=30, asso_func='diou', iou_threshold=0.1) of reference track.py:157; sort: SortTracker(max_age=30), its "
                   "commented-out alternative (track.py:156), which made the reference's dfs/ frames.  Every other option works with either.")
@click.option("--concurrent", default=1, show_default=True, type=int,
              help="Clips tracked side by side in one pipeline (a finished clip's tracker slot takes the next file); 1 = one pipeline per file.")
@click.option("--pix_fmt", default="rgb24", show_default=True, type=click.Choice(["rgb24", "nv12", "i420", "yuyv422", "uyvy422", "p010le"]),
              help="Pixel format of the sources; nv12 / i420 (YUV 4:2:0, as a decoder emits it), yuyv422 / uyvy422 (packed 4:2:2, webcams and "
                   "capture cards) and p010le (10-bit 4:2:0) need --size.  The last three are tracked, not drawn: no --video_dir with them.")
@click.option("--color_matrix", default="bt601", show_default=True, type=click.Choice(["bt601", "bt709"]),
              help="Matrix of a YUV source (HD material is bt709); not for rgb24 or .avi sources, not with --video_dir.")
@click.option("--color_range", default="limited", show_default=True, type=click.Choice(["limited", "full"]),
              help="Range of a YUV source (ffmpeg's yuvj420p is i420 with full); not for rgb24 or .avi sources, not with --video_dir.")
@click.option("--size", default=None, type=str, help="WIDTHxHEIGHT of headerless raw video sources, e.g. 1920x1080; without it SRC is a .npy stack.")
@click.option("--video_dir", default=None, show_default=True,
              help="Directory for exporting the frames with tracked objects and bar path ({video}.npy, or raw {video}.rgb / .yuv with --size).")
@click.option("--video_format", default="raw", show_default=True, type=click.Choice(["raw", "mjpeg"]),
              help="raw: the drawn frames as they are; mjpeg: {video}.avi, JPEG-encoded on the GPU, playing at fps / frame_stride.")
@click.option("--video_quality", default=85, show_default=True, type=click.IntRange(1, 100), help="JPEG quality of --video_format mjpeg.")
@click.option("--mjpeg_entropy", default="auto", show_default=True, type=click.Choice(["auto", "interval", "sync"]),
              help="Entropy decoding of .avi sources: one lane per restart interval, subsequences that synchronise, or auto by interval length.")
@click.option("--one_pass", is_flag=True, default=False,
              help="Draw and write each batch of frames right after it is tracked, from the tracker's row log on the GPU, instead of in a second pass "
                   "over the clip (needs --video_dir; same files; not with --hud or --concurrent above 1).")
@click.option("--live_hud", is_flag=True, default=False,
              help="With --one_pass: the rep panel fed by the live rep analysis on the GPU - the reps appear on the video as they complete "
                   "(uses --plate_diameter, --hud_scale, --hud_pos; not with --hud or --concurrent above 1).")
@_display_option
@_hud_options
def track(src, model, detection_treshold, df_dir, fps, frame_stride, time_batch, live, report, stop_loss, tracker, concurrent, pix_fmt, color_matrix, color_range, size,
          video_dir, video_format, video_quality, mjpeg_entropy, one_pass, live_hud, hud, plate_diameter, hud_scale, hud_pos, display_image_height):
    from ._lib import VbtArgError
    from .track import export_dataframe, track_frames
    size = _raw_size(pix_fmt, size)
    _check_colour_options(src, pix_fmt, color_matrix, color_range,
                          {"--video_dir": video_dir is not None, "--one_pass": one_pass, "--hud": hud, "--live_hud": live_hud,
                           "--display_image_height": display_image_height is not None})
    colour = dict(color_matrix=color_matrix, color_range=color_range)
    _check_display_height(display_image_height, video_dir, pix_fmt)
    fps_given = _fps_given()
    hud_params = _hud_params(hud, video_dir, hud_scale, hud_pos)
    if stop_loss is not None and not live:
        raise click.UsageError("--stop_loss watches the reps as they complete: give --live")
    if stop_loss is not None and not (math.isfinite(stop_loss) and stop_loss > 0):
        raise click.UsageError(f"--stop_loss {stop_loss} must be a finite percentage above 0")
    if report and not live:
        raise click.UsageError("--report extends the rep lines of --live: give --live (a finished DataFrame: analyze --report)")

    def live_reps(s):
        return _LiveReps(s, report, stop_loss) if live else None
    if concurrent < 1:
        raise click.UsageError("--concurrent must be at least 1")
    hud_live = None
    if live_hud:
        if hud:
            raise click.UsageError("--live_hud and --hud are two different panels (the reps so far / the finished analysis): give one of them")
        if video_dir is None:
            raise click.UsageError("--live_hud draws on the exported frames: give --video_dir")
        if not one_pass:
            raise click.UsageError("--live_hud draws while the clip is tracked: give --one_pass")
        if concurrent > 1:
            raise click.UsageError("--live_hud works with --concurrent 1 only")
        hud_live = dict(_hud_params(True, video_dir, hud_scale, hud_pos), plate_diameter=plate_diameter)
    if one_pass:
        if video_dir is None:
            raise click.UsageError("--one_pass is a way to write the exported frames: give --video_dir")
        if hud:
            raise click.UsageError("--one_pass cannot draw --hud: the rep panel shows the phases of the analysed clip, which exist only after its last frame")
        if concurrent > 1:
            raise click.UsageError("--one_pass works with --concurrent 1 only: clips tracked side by side are rendered as each one finishes")
    if concurrent > 1:
        if live:
            raise click.UsageError("--live works with --concurrent 1 only")
        return _track_concurrent(src, model, detection_treshold, df_dir, fps, frame_stride, time_batch, concurrent, pix_fmt, size, video_dir,
                                 video_format, video_quality, fps_given, mjpeg_entropy, hud_params, plate_diameter, tracker, display_image_height,
                                 colour)
    default_fps = fps
    for s in src:
        frames = _open_source(s, pix_fmt, size, mjpeg_entropy)
        fps = _source_fps(frames, default_fps, fps_given)
        display_hw = _display_hw(frames, pix_fmt, display_image_height)   # before any output file exists
        if hud_params is not None:                                       # the panel shows the finished analysis: render after tracking
            data = track_frames(frames, model, fps=fps, detection_treshold=detection_treshold, frame_stride=frame_stride, time_batch=time_batch,
                                live=live_reps(s), pix_fmt=pix_fmt, tracker=tracker, **colour)
            line, phases = _export_line(data, s, model, df_dir, plate_diameter)
            _render_video(video_dir, video_format, video_quality, s, frames, data, fps, frame_stride, time_batch, pix_fmt, size, phases, hud_params,
                          display_hw)
            click.echo(line)
            continue
        if hud_live is not None:
            _check_live_hud_fits(frames, pix_fmt, hud_live)                # before any output file exists
        mjpeg = video_dir is not None and video_format == "mjpeg"
        video = None if mjpeg else _video_out(video_dir, s, frames, frame_stride, pix_fmt, size, display_hw)
        with (_avi_out(video_dir, s, frames, fps, frame_stride, pix_fmt, display_hw) if mjpeg else contextlib.nullcontext()) as sink:   # closed on an error too
            try:
                data = track_frames(frames, model, fps=fps, detection_treshold=detection_treshold, frame_stride=frame_stride, time_batch=time_batch,
                                    live=live_reps(s), pix_fmt=pix_fmt, video_out=video, video_sink=sink,
                                    video_quality=video_quality, one_pass=one_pass, hud_live=hud_live, tracker=tracker, display_hw=display_hw,
                                    **colour)
            except VbtArgError as e:                                     # a panel the library refuses (outside the frame, odd origin in a YUV frame)
                if hud_live is None or "vbt_overlay_hud_follow" not in str(e):
                    raise
                raise click.UsageError(f"--live_hud: {e}")
        _video_done(video)
        if not data["id"]:
            click.echo(f"{s}: no tracked rows")
            continue
        df, best, path = export_dataframe(data, s, model, df_dir=df_dir, write=df_dir is not None)
        click.echo(f"{s}: {len(df)} rows, {df['id'].nunique()} ids, export id {best}" + (f" -> {path}" if df_dir is not None else ""))


def _check_live_hud_fits(frames, pix_fmt, hud_live):
    """--live_hud: the panel the library would refuse for this source (vbt_overlay_hud_follow: outside the frame, odd origin in a YUV
    frame) is a usage error here, while nothing has been written yet"""
    from .rawvideo import is_yuv, source_hw
    H, W = source_hw(frames, pix_fmt)
    x, y, s = hud_live["x"], hud_live["y"], hud_live["scale"]
    if is_yuv(pix_fmt) and (x | y) & 1:
        raise click.UsageError(f"--live_hud: a {pix_fmt} panel starts at even coordinates, got --hud_pos {x},{y}")
    if x + 52 * s > W or y + 50 * s > H:
        raise click.UsageError(f"--live_hud: the {52 * s} x {50 * s} panel at ({x}, {y}) does not lie inside the {W} x {H} frame "
                               "(--hud_scale, --hud_pos)")


def _export_line(data, s, model, df_dir, plate_diameter=None):
    """Export of a tracked clip: (the line `track` prints, with a plate_diameter (--hud) the phases of the export id - none for a clip
    without rows)"""
    from .track import export_dataframe
    if not data["id"]:
        return f"{s}: no tracked rows", []
    df, best, path = export_dataframe(data, s, model, df_dir=df_dir, write=df_dir is not None)
    line = f"{s}: {len(df)} rows, {df['id'].nunique()} ids, export id {best}" + (f" -> {path}" if df_dir is not None else "")
    return line, (_id_phases(df, best, plate_diameter) if plate_diameter is not None else None)


def _video_out(video_dir, s, frames, frame_stride, pix_fmt, size, display_hw=None):
    """The writable map of --video_dir for source `s` (None without --video_dir, or when no frame is kept): DIR/{video}.npy
    (numpy.lib.format.open_memmap, so a long clip never sits in memory) or, for --size sources, raw DIR/{video}.rgb / .yuv.
    display_hw: the (h, w) of --display_image_height; the frames then have that size."""
    if video_dir is None:
        return None
    os.makedirs(video_dir, exist_ok=True)                                # reference track.py:85-86
    stem = os.path.basename(s).split(".")[0]                             # reference track.py:97
    from .rawvideo import frame_shape
    shape = (int(frames.shape[0]) // max(int(frame_stride), 1),) + (tuple(frames.shape[1:]) if display_hw is None else frame_shape(pix_fmt, *display_hw))
    if size is None:
        path = os.path.join(video_dir, stem + ".npy")
        if shape[0] == 0:
            np.save(path, np.zeros(shape, np.uint8))
            return None
        return np.lib.format.open_memmap(path, mode="w+", dtype=np.uint8, shape=shape)
    path = os.path.join(video_dir, stem + (".rgb" if pix_fmt == "rgb24" else ".yuv"))
    if shape[0] == 0:
        open(path, "wb").close()
        return None
    return np.memmap(path, dtype=np.uint8, mode="w+", shape=shape)


def _avi_out(video_dir, s, frames, fps, frame_stride, pix_fmt, display_hw=None):
    """The mjpeg.AviWriter of --video_format mjpeg for source `s`: DIR/{video}.avi at fps / frame_stride, its header with the
    (h, w) of --display_image_height when there is one"""
    from .mjpeg import AviWriter, frame_rate
    from .rawvideo import source_hw
    os.makedirs(video_dir, exist_ok=True)
    H, W = source_hw(frames, pix_fmt) if display_hw is None else display_hw
    rate, scale = frame_rate(fps, frame_stride)
    path = os.path.join(video_dir, os.path.basename(s).split(".")[0] + ".avi")
    if os.path.exists(path) and os.path.samefile(path, s):
        raise click.UsageError(f"--video_dir {video_dir}: the export {path} would overwrite its own source; choose another directory")
    return AviWriter(path, W, H, rate, scale)


def _video_done(video):
    if video is not None:
        video.flush()


def _render_video(video_dir, video_format, video_quality, s, frames, data, fps, frame_stride, batch, pix_fmt, size, hud=None, hud_params=None,
                  display_hw=None):
    """The export of a finished clip from its rows: DIR/{video}.avi (mjpeg) or the raw map of _video_out.  Returns the frames written.
    hud_params (--hud): the rep panel of the phases `hud` on every frame; a panel the library refuses (outside the frame, odd origin
    in a YUV frame) is a usage error."""
    from ._lib import VbtArgError
    from .overlay import render
    panel = {} if hud_params is None else dict(hud=hud, hud_params=hud_params)
    if display_hw is not None:
        panel["display_hw"] = display_hw
    try:
        if video_format == "mjpeg":
            with _avi_out(video_dir, s, frames, fps, frame_stride, pix_fmt, display_hw) as sink:   # closed, hence a valid file, on an error too
                return render(frames, data, fps, frame_stride=frame_stride, pix_fmt=pix_fmt, batch=batch, sink=sink, quality=video_quality, **panel)
        video = _video_out(video_dir, s, frames, frame_stride, pix_fmt, size, display_hw)
        if video is None:
            return 0
        render(frames, data, fps, frame_stride=frame_stride, pix_fmt=pix_fmt, batch=batch, out=video, **panel)
    except VbtArgError as e:
        if hud_params is None or "vbt_overlay_set_hud" not in str(e):
            raise
        raise click.UsageError(f"--hud: {e}")
    _video_done(video)
    return len(video)


def _track_concurrent(src, model, detection_treshold, df_dir, fps, frame_stride, time_batch, concurrent, pix_fmt="rgb24", size=None, video_dir=None,
                      video_format="raw", video_quality=85, fps_given=True, mjpeg_entropy="auto", hud_params=None, plate_diameter=0.45, tracker="ocsort",
                      display_image_height=None, colour=None):
    """track --concurrent N: the files through ONE pipeline (track.track_many); files, DataFrames and lines as with N = 1.  A clip's
    DataFrame is written as soon as it finishes; its line waits for the clips before it (input order).  The files up to the first one
    that cannot be read are tracked and printed, then that file's error is raised - as N = 1 does."""
    from .track import track_many
    sources, error = [], None
    for s in src:
        try:
            sources.append(_open_source(s, pix_fmt, size, mjpeg_entropy))
        except (FileNotFoundError, click.ClickException) as e:
            error = e
            break
    lines, nxt = {}, 0
    fps = [_source_fps(a, fps, fps_given) for a in sources] or fps
    display_hw = [_display_hw(a, pix_fmt, display_image_height) for a in sources]    # before any output file exists
    for i, data in track_many(sources, model, concurrent, fps=fps, detection_treshold=detection_treshold, frame_stride=frame_stride,
                              time_batch=time_batch, pix_fmt=pix_fmt, tracker=tracker, **(colour or {})):
        s = src[i]
        if hud_params is None and video_dir is not None:                 # the clip is finished: its rows are all the renderer needs
            _render_video(video_dir, video_format, video_quality, s, sources[i], data, fps[i], frame_stride, time_batch, pix_fmt, size,
                          display_hw=display_hw[i])
        lines[i], phases = _export_line(data, s, model, df_dir, plate_diameter if hud_params is not None else None)
        if hud_params is not None:                                       # (--hud: the panel needs the export id's phases first)
            _render_video(video_dir, video_format, video_quality, s, sources[i], data, fps[i], frame_stride, time_batch, pix_fmt, size, phases, hud_params,
                          display_hw[i])
        while nxt in lines:
            click.echo(lines.pop(nxt))
            nxt += 1
    if error is not None:
        raise error


@main.command()
@click.argument("src", type=str)
@click.argument("dataframe", type=str)
@click.option("--fps", default=30.0, show_default=True, type=float, help="Frame rate the DataFrame was tracked at (its times are frame numbers / fps).")
@click.option("--frame_stride", default=1, show_default=True, type=int, help="The --frame_stride the DataFrame was tracked with: the frames that are kept.")
@click.option("--pix_fmt", default="rgb24", show_default=True, type=click.Choice(["rgb24", "nv12", "i420"]),
              help="Pixel format of the source; nv12 / i420 need --size.")
@click.option("--size", default=None, type=str, help="WIDTHxHEIGHT of a headerless raw video source; without it SRC is a .npy stack.")
@click.option("--video_dir", default=".", show_default=True, help="Directory for the drawn frames ({video}.npy, or raw {video}.rgb / .yuv with --size).")
@click.option("--video_format", default="raw", show_default=True, type=click.Choice(["raw", "mjpeg"]),
              help="raw: the drawn frames as they are; mjpeg: {video}.avi, JPEG-encoded on the GPU, playing at fps / frame_stride.")
@click.option("--video_quality", default=85, show_default=True, type=click.IntRange(1, 100), help="JPEG quality of --video_format mjpeg.")
@click.option("--mjpeg_entropy", default="auto", show_default=True, type=click.Choice(["auto", "interval", "sync"]),
              help="Entropy decoding of .avi sources: one lane per restart interval, subsequences that synchronise, or auto by interval length.")
@_display_option
@_hud_options
def overlay(src, dataframe, fps, frame_stride, pix_fmt, size, video_dir, video_format, video_quality, mjpeg_entropy, hud, plate_diameter, hud_scale,
            hud_pos, display_image_height):
    """Draw the boxes, ids and bar paths of a stored DataFrame into the frames of its clip (what `track --video_dir` writes)."""
    import pandas as pd
    size = _raw_size(pix_fmt, size)
    _check_display_height(display_image_height, video_dir, pix_fmt)
    hud_params = _hud_params(hud, video_dir, hud_scale, hud_pos)
    m = FILENAME_RE.match(os.path.basename(dataframe))
    if hud and not m:
        raise click.UsageError(f"--hud takes the panel's id from the DataFrame's file name: '{dataframe}' is not {{video}}_id{{N}}_{{model}}.pkl.gz")
    if frame_stride < 1:
        raise click.UsageError("--frame_stride must be at least 1")
    if not os.path.isfile(dataframe):
        raise FileNotFoundError(dataframe)
    frames = _open_source(src, pix_fmt, size, mjpeg_entropy)
    fps = _source_fps(frames, fps, _fps_given())
    df = pd.read_pickle(dataframe)
    phases = _id_phases(df, int(m.group(2)), plate_diameter) if hud else None
    n = _render_video(video_dir, video_format, video_quality, src, frames, df, fps, frame_stride, 64, pix_fmt, size, phases, hud_params,
                      _display_hw(frames, pix_fmt, display_image_height))
    click.echo(f"{src}: {n} frames, {len(df)} rows of {df['id'].nunique()} ids -> {video_dir}")


@main.command()
@click.argument("src", type=str, nargs=-1)
@click.option("--plate_diameter", default=0.45, show_default=True, type=float, help="Diameter of the weight plate used in meters.")
@click.option("--report", is_flag=True, default=False,
              help="Per rep also peak velocity (PV), time to peak (TTP), vertical ROM, sideways excursion and velocity loss; then a line for the set.")
@click.option("--report_csv", default=None, type=str, help="With --report: write one row per concentric rep to this CSV file.")
def analyze(src, plate_diameter, report, report_csv):
    import pandas as pd
    from .velocity import Phase
    if report_csv is not None and not report:
        raise click.UsageError("--report_csv writes the rows of --report: give --report")
    csv_rows = []
    for s in src:
        if not os.path.isfile(s):
            raise FileNotFoundError(s)                                   # reference plot.py:67-68
        m = FILENAME_RE.match(os.path.basename(s))
        if not m:
            click.echo(f"Couldn't create a plot for file '{s}'.")        # reference plot.py:81-85
            continue
        video, tid, model = m.groups()
        if report:
            phases, metrics = _id_phases(pd.read_pickle(s), tid, plate_diameter, metrics=True)
            lines, set_line, rep = _report_lines(phases, metrics)
            click.echo(f"{video} (id {tid}, {model}): {len(phases)} phases, {rep.n_reps} concentric reps")
            for ln in lines + [set_line]:
                click.echo(ln)
            csv_rows += _report_csv_rows(video, tid, phases, metrics, rep)
            continue
        phases = _id_phases(pd.read_pickle(s), tid, plate_diameter)
        reps = [p for p in phases if p.type == Phase.CONCENTRIC]
        click.echo(f"{video} (id {tid}, {model}): {len(phases)} phases, {len(reps)} concentric reps")
        for i, p in enumerate(reps, 1):
            click.echo(_rep_line(i, p))
    if report_csv is not None:
        import csv
        with open(report_csv, "w", newline="") as f:
            w = csv.writer(f)
            w.writerow(REPORT_CSV_COLUMNS)
            w.writerows(csv_rows)


def _analyze_lines(video, tid, model, phases):
    from .velocity import Phase
    reps = [p for p in phases if p.type == Phase.CONCENTRIC]
    click.echo(f"{video} (id {tid}, {model}): {len(phases)} phases, {len(reps)} concentric reps")
    for i, p in enumerate(reps, 1):
        click.echo(_rep_line(i, p))


@main.command()
@click.argument("src", type=str, nargs=-1)
@click.option("--plate_diameter", default=0.45, show_default=True, type=float, help="Diameter of the weight plate used in meters.")
@click.option("--fig_dir", default=None, help="Directory for saving the figures (required: there is no display to show them on).")
@click.option("--fig_size", default="1280x800", show_default=True, type=str, help="WIDTHxHEIGHT of a figure in pixels.")
@click.option("--fig_scale", default=2, show_default=True, type=click.IntRange(1, 64), help="Pixels per cell of the figure's text and margins.")
@click.option("--fig_format", default="jpg", show_default=True, type=click.Choice(["jpg", "ppm"]),
              help="jpg: baseline JPEG encoded on the GPU; ppm: the raw RGB frame behind a P6 header, lossless.")
@click.option("--fig_quality", default=90, show_default=True, type=click.IntRange(1, 100), help="JPEG quality of --fig_format jpg.")
def plot(src, plate_diameter, fig_dir, fig_size, fig_scale, fig_format, fig_quality):
    if fig_dir is None:
        raise click.UsageError("plot writes the figures: give --fig_dir (there is no display for --show_fig)")
    m = re.fullmatch(r"\s*(\d+)\s*[xX]\s*(\d+)\s*", fig_size)
    if not m:
        raise click.BadParameter(f"expected WIDTHxHEIGHT, got {fig_size!r}", param_hint="--fig_size")
    from . import figure

    def on_file(s, loaded):
        if loaded is None:
            click.echo(f"Couldn't create a plot for file '{s}'.")        # reference plot.py:81-85
            return
        _analyze_lines(*FILENAME_RE.match(os.path.basename(s)).groups(), loaded[1])
    try:
        figure.plot_many(src, fig_dir, plate_diameter, fig_format, fig_quality, on_file=on_file, width=int(m.group(1)), height=int(m.group(2)),
                         scale=fig_scale)
    except ValueError as e:                                              # (VbtArgError: a figure size the layout refuses)
        raise click.UsageError(str(e))


@main.command()
@click.option("--kinovea_dir", default=None, help="Directory containing the kinovea exports (*.txt).")
@click.option("--qualysis_dir", default=None, help="Directory containing the qualysis exports (*.tsv).")
@click.option("--df_dir", default="dfs", show_default=True, help="Directory containing the dfs.")
@click.option("--plate_diameter", default=0.45, show_default=True, type=float, help="Diameter of the weight plate used in meters.")
@click.option("--fig_dir", default=None, show_default=True,
              help="Directory for saving the figures ({video}_id{id}_{model}.jpg|ppm). With it, numbers and figures come from one batch on the GPU. "
                   "There is no --show_fig (no display), no LaTeX table and no p-values.")
@click.option("--fig_format", default="jpg", show_default=True, type=click.Choice(["jpg", "ppm"]),
              help="jpg: baseline JPEG encoded on the GPU; ppm: the raw RGB frame behind a P6 header, lossless.")
@click.option("--fig_quality", default=90, show_default=True, type=click.IntRange(1, 100), help="JPEG quality of --fig_format jpg.")
def validate(kinovea_dir, qualysis_dir, df_dir, plate_diameter, fig_dir, fig_format, fig_quality):
    import glob
    import pandas as pd
    from . import validate as V
    if (kinovea_dir is None) == (qualysis_dir is None):
        raise click.UsageError("give exactly one of --kinovea_dir / --qualysis_dir")
    source = "kinovea" if kinovea_dir is not None else "qualisys"
    exports = sorted(glob.glob(os.path.join(kinovea_dir, "*.txt") if source == "kinovea" else os.path.join(qualysis_dir, "*.tsv")))
    df_files = sorted(glob.glob(os.path.join(df_dir, "*.pkl.gz")))
    rows_out, pairs = [], []

    def line(video, r):
        click.echo(f"{video}: MSEx {r['mse_x']:.4f}  MSEy {r['mse_y']:.4f}  r_x {r['r_x']:.4f}  r_y {r['r_y']:.4f}")
    for ex in exports:
        stem = os.path.basename(ex).split(".")[0]
        match = next((x for x in df_files if os.path.basename(x).startswith(stem)), None)
        if match is None:
            click.echo(f"No matching df file found for: {ex}")                    # reference kinovea.py:62-64
            continue
        m = FILENAME_RE.match(os.path.basename(match))
        if not m:
            continue
        video, tid, model = m.groups()
        df = pd.read_pickle(match).query(f"id == {tid}").sort_values(by="time")
        rows = np.stack([df[c].to_numpy(np.float64) for c in ("time", "x", "y", "norm_plate_height", "norm_plate_width")], axis=1)
        ref = V.read_kinovea(ex) if source == "kinovea" else V.read_qualisys(ex)
        if fig_dir is not None:                                                   # the whole corpus in one batch, below
            pairs.append((ref, rows, f"{video}_id{tid}_{model}", video))          # reference kinovea.py:195-197: that name, as .pdf
            continue
        r = V.validate_pair(ref, rows, plate_diameter, source)
        rows_out.append((video, r))
        line(video, r)
    if fig_dir is not None:
        try:
            results, _ = V.validate_many([p[:3] for p in pairs], source, plate_diameter, fig_dir, fig_format, fig_quality)
        except ValueError as e:                                                   # (VbtArgError: a pair the set refuses)
            raise click.UsageError(str(e))
        for (_, _, _, video), r in zip(pairs, results):
            rows_out.append((video, r))
            line(video, r)
    click.echo(f"Total MSEx = {sum(r['mse_x'] for _, r in rows_out)}, MSEy = {sum(r['mse_y'] for _, r in rows_out)}")


@main.command(name="eval")
@click.argument("models", type=str, nargs=-1)
@click.option("--img_dir", default="data/test", show_default=True, help="Directory containing the test images (.jpg / .png / .npy).")
@click.option("--annotations_dir", default="data/test", show_default=True, help="Directory containing the XML annotation files.")
@click.option("--iou_threshold", default=0.5, show_default=True, type=float,
              help="Intersection over union threshold to label detections as correct or not against the ground truth bounding boxes.")
@click.option("--detections_df", default="dfs/eval_detections.pkl.gz", show_default=True, help="Path for storing/reading the detection results dataframe.")
@click.option("--replace_df", is_flag=True, help="If exists, replace the detections dataframe.")
@click.option("--score_thresholds", default="[]", show_default=True, help='List of score thresholds to locate on the curves, e.g. "[0.2, 0.5]".')
@click.option("--curve_dir", default=None, show_default=True, help="Directory for the curve points as CSV. If not set they are not written.")
@click.option("--rgb", is_flag=True, help="Feed RGB to the network (the reference's eval.py feeds cv2's BGR unswapped; that is the default).")
@click.option("--jpeg_decode", default="auto", show_default=True, type=click.Choice(["auto", "gpu", "host"]),
              help="Where .jpg test images are decoded. auto: baseline files on the GPU, straight to the network input, and files its decoder "
                   "refuses (progressive, CMYK, ...) on the host; gpu: such a file is an error; host: every file on the host (PIL).")
@click.option("--fig_dir", default=None, show_default=True, help="Directory for saving the figures. If not set the figures won't be saved.")
@click.option("--fig_size", default="1120x640", show_default=True, type=str,
              help="WIDTHxHEIGHT of the combined figures in pixels; the per-model figures are three quarters as high.")
@click.option("--fig_scale", default=2, show_default=True, type=click.IntRange(1, 64), help="Pixels per cell of the figures' text and margins.")
@click.option("--fig_format", default="jpg", show_default=True, type=click.Choice(["jpg", "ppm"]),
              help="jpg: baseline JPEG encoded on the GPU; ppm: the raw RGB frame behind a P6 header, lossless.")
@click.option("--fig_quality", default=90, show_default=True, type=click.IntRange(1, 100), help="JPEG quality of --fig_format jpg.")
@click.option("--coco", is_flag=True, help="After the lines above, print per model the twelve COCO detection metrics and the per-class AP as the "
                                           "reference's training logs end (model.evaluate). Always runs the models.")
@click.option("--coco_dump", default=None, show_default=True, help="With --coco: directory for instances.json and {model}_detections.json, to "
                                                                   "cross-check the numbers with pycocotools elsewhere.")
def evaluate(models, img_dir, annotations_dir, iou_threshold, detections_df, replace_df, score_thresholds, curve_dir, rgb, jpeg_decode, fig_dir, fig_size,
             fig_scale, fig_format, fig_quality, coco, coco_dump):
    import ast
    import pandas as pd
    from . import evaluate as E
    try:
        score_thresholds = list(ast.literal_eval(score_thresholds))                # reference eval.py:26-39
    except (ValueError, SyntaxError, TypeError):
        raise click.BadParameter(score_thresholds)
    size = re.fullmatch(r"\s*(\d+)\s*[xX]\s*(\d+)\s*", fig_size)
    if not size:
        raise click.BadParameter(f"expected WIDTHxHEIGHT, got {fig_size!r}", param_hint="--fig_size")
    if coco_dump is not None and not coco:
        raise click.UsageError("--coco_dump needs --coco")
    if not os.path.exists(detections_df) or replace_df:                            # reference eval.py:506-512
        click.echo(f"Creating dataframe '{detections_df}'.")
        annotations = E.read_annotations(annotations_dir)
        try:
            df = E.create_detections_df(models, img_dir, annotations, detections_df, rgb=rgb, jpeg_decode=jpeg_decode)
        except E.JpegRefused as e:                                                 # (a .jpg that --jpeg_decode gpu refuses: another mode takes it)
            raise click.UsageError(str(e))
        except E.JpegDamaged as e:                                                 # (bad data, not bad usage: exit code 1)
            raise click.ClickException(str(e))
    else:
        click.echo(f"Loading dataframe '{detections_df}'.")
        df = pd.read_pickle(detections_df)
    if curve_dir is not None:
        os.makedirs(curve_dir, exist_ok=True)
    curves = E.curves(df, iou_threshold)
    for m, c in curves.items():
        click.echo(f"{m}, AP_{iou_threshold * 100:0.0f}={c.ap:.4f}, AUC={c.auc:.4f}  ({c.n_rows} rows, {c.n_pos} correct)")   # eval.py:261,388
        if c.flags:
            click.echo(f"{m}: " + " and ".join(t for b, t in ((E.NO_POSITIVES, "no correct detection"), (E.NO_NEGATIVES, "no incorrect detection"))
                                              if c.flags & b) + " at this IoU threshold: the rates without a denominator are NaN", err=True)
        for v in score_thresholds:
            if len(c.pr_thresholds):
                i = E.closest_point(c.pr_thresholds, v)                            # reference eval.py:313-321
                click.echo(f"  PR  threshold {c.pr_thresholds[i]:.4f}: precision {c.precision[i]:.4f}  recall {c.recall[i]:.4f}")
            j = E.closest_point(c.roc_thresholds, v)                               # reference eval.py:443-451
            click.echo(f"  ROC threshold {c.roc_thresholds[j]:.4f}: FP rate {c.fpr[j]:.4f}  TP rate {c.tpr[j]:.4f}")
        if curve_dir is not None:
            thr = np.r_[c.pr_thresholds, c.pr_thresholds[-1:]] if len(c.pr_thresholds) else np.full(len(c.precision), np.nan)   # eval.py:235
            pd.DataFrame({"Precision": c.precision, "Recall": c.recall, "Threshold": thr, "Model": m}).to_csv(
                os.path.join(curve_dir, f"precision_recall_{m}_iou_{iou_threshold}.csv"), index=False)
            pd.DataFrame({"FP Rate": c.fpr, "TP Rate": c.tpr, "Threshold": c.roc_thresholds, "Model": m}).to_csv(
                os.path.join(curve_dir, f"roc_{m}_iou_{iou_threshold}.csv"), index=False)
    if fig_dir is not None:                                                        # reference eval.py:517-521
        try:
            for draw in (E.plot_precision_recall, E.plot_roc):
                draw(curves, fig_dir, iou_threshold, score_thresholds, fig_format, fig_quality, width=int(size.group(1)), height=int(size.group(2)),
                     scale=fig_scale)
        except ValueError as e:                                                    # (VbtArgError: a figure size the layout refuses)
            raise click.UsageError(str(e))
    if coco:                                                                       # reference train.py:64,70: the dict model.evaluate prints
        annotations = E.read_annotations(annotations_dir)
        images = [(name, E.find_image(img_dir, name)) for name in annotations]
        try:
            srt = E.SortedImages(images, jpeg_decode)
            dets, sizes = {}, {}
            for model in models:
                res, _, det = E.coco_evaluate(model, images, annotations, rgb=rgb, jpeg_decode=jpeg_decode, sorted_images=srt)
                line = {k: float(str(np.float32(v))) for k, v in res.metrics().items()}      # through float32, as the log's values
                click.echo(f"{E.model_name(model)}: {line}")
                dets[E.model_name(model)] = det
        except E.JpegRefused as e:
            raise click.UsageError(str(e))
        except E.JpegDamaged as e:
            raise click.ClickException(str(e))
        if coco_dump is not None:
            for name, path in images:
                sizes[name] = srt.heads[name][:2] if name in srt.heads else E.image_size(path)
            E.coco_dump(coco_dump, annotations, sizes, dets)


if __name__ == "__main__":
    main()
