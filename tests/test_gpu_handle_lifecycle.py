"""The paths of a handle's life on which one of its buffers is replaced or re-pointed (the handles hold their device buffers, pinned
buffers and events in the owners of vbt_amd/csrc/dev_mem.h and hip_handles.h): a staging buffer of the pipeline that grows while steps
are in flight, the slot-close buffers enabled twice, a pipeline destroyed and another created; the stills decoder's compressed-byte
buffers growing; the overlay's rows and panel going back and forth between their sources; the evaluator's staging slots on two
streams, across a reset.  Every result is compared bit for bit with the statement the handle's own tests use."""
import ctypes
import gc

import numpy as np
import pytest

from conftest import MODEL_LITE0

pytestmark = pytest.mark.gpu

NO_AUTOTUNE = 8          # VBT_MODEL_NO_AUTOTUNE (include/vbt_hip_diag.h)


# ---------------------------------------------------------------------------------------------- pipeline
SMALL, LARGE, STEPS = (48, 64), (96, 128), 6       # 6 steps go once round the 4 staging buffers (depth + 2) and on


def _sources(hw, seed0):
    """STEPS host-fed steps of two clips at source size hw: synthetic frames, every k-th row and column"""
    from vbt_amd import synth
    ri, ci = (np.arange(hw[0]) * 320) // hw[0], (np.arange(hw[1]) * 320) // hw[1]
    clips = [synth.clip_frames(seed0 + c, 9 * c, STEPS)[:, ri][:, :, ci] for c in range(2)]
    return [np.ascontiguousarray(np.stack([clips[c][t] for c in range(2)])) for t in range(STEPS)]


def _pipeline(**kw):
    from vbt_amd.track import Pipeline
    return Pipeline(MODEL_LITE0, 2, max_frames=2 * STEPS, fps=30.0, rows_per_frame=25, depth=2, **kw)


def _rows_equal(got, want, what):
    assert got["id"] == want["id"], what
    for k in want:
        assert np.array_equal(np.asarray(got[k]), np.asarray(want[k])), (what, k)


def test_pipeline_staging_grows_in_flight_close_enable_twice_and_a_second_pipeline(monkeypatch):
    from vbt_amd import _lib
    monkeypatch.setenv("VBT_FUSION_FLAGS", str(NO_AUTOTUNE))
    small, large = _sources(SMALL, 60), _sources(LARGE, 70)
    # four tracker clips on two slots: the small steps are frames 1.. of clips 0 and 1, the large ones frames 1.. of clips 2 and 3, so
    # that nothing has to be read - or waited for - between the two sizes
    pipe = _pipeline(tracker_clips=4, slot_close=True)
    assert (pipe.n, pipe.depth, pipe.group) == (2, 2, 1)
    for t in range(STEPS):
        pipe.step(small[t], src_hw=SMALL, clip_map=[0, 1], frame_idx=[t + 1, t + 1])
    for t in range(STEPS):                           # every staging buffer is too small now: each is replaced behind steps in flight
        pipe.step(large[t], src_hw=LARGE, clip_map=[2, 3], frame_idx=[t + 1, t + 1])
    mixed = [pipe.rows(c) for c in range(4)]
    assert pipe.info().h2d_bytes == STEPS * 2 * 3 * (SMALL[0] * SMALL[1] + LARGE[0] * LARGE[1])
    _lib.check(_lib.lib().vbt_pipeline_close_clips_enable(pipe._h))          # enabled at creation already: nothing to do
    pipe.close_clips([3])
    best, rows3, _, overflow = pipe.closed(3)
    _rows_equal(rows3, mixed[3], "the closed clip")
    assert overflow == 0
    del pipe
    gc.collect()                                     # destroyed: its streams are back in the pool
    for name, src, hw, first in (("small", small, SMALL, 0), ("large", large, LARGE, 2)):
        fresh = _pipeline()                          # the second and third pipeline of the process
        for t in range(STEPS):
            fresh.step(src[t], src_hw=hw, clip_map=[0, 1], frame_idx=[t + 1, t + 1])
        for c in range(2):
            want = fresh.rows(c)
            _rows_equal(mixed[first + c], want, (name, c))
        del fresh
    assert all(len(m["id"]) > 0 for m in mixed)      # every clip, at either size, was detected and tracked


# ---------------------------------------------------------------------------------------------- stills decoder
DESC_BYTES_MAX = 4608                                # >= sizeof(JpegDesc) (vbt_amd/csrc/jpeg_core.h: four Huffman tables of 904 bytes)


def test_stills_compressed_byte_buffers_grow_behind_a_small_batch():
    import mjpeg_dec_ref as D
    from test_gpu_jpeg_stills import run_full
    from test_gpu_mjpeg_decode import assert_same_frame
    from test_jpeg_stills_host import layout_blocks
    from vbt_amd.stills import JpegStills
    tiny = D.vectors()["own-16x16"]
    big = D.pil_jpeg(D.noise((112, 144, 3), 5), quality=100, subsampling=0)
    budget = layout_blocks(big)
    assert budget >= 2 * layout_blocks(tiny)
    # conditions on the inputs: the second batch outgrows the device buffer the first one allocated (vbt_jpeg_stills_decode: max_batch
    # descriptors, table entries and 4096 bytes each, 16 bytes per block of the budget) and the first batch's staging buffer
    packed_init = 2 * (DESC_BYTES_MAX + 32 + 4096) + 16 * budget
    first_total = 2 * (DESC_BYTES_MAX + 32) + 2 * (D.parse(tiny)["scan"][1] + 16)
    assert D.parse(big)["scan"][1] > packed_init and D.parse(big)["scan"][1] > 2 * first_total
    dec = JpegStills(max_batch=2, block_budget=budget)
    frames, st, _ = run_full([tiny, tiny], dec=dec)
    assert not st.any()
    for f in frames:
        assert_same_frame(f, D.expected("own-16x16"), "own-16x16")
    frames, st, _ = run_full([big], dec=dec)         # staging buffer 1 is new, the device buffer is replaced
    assert not st.any()
    assert_same_frame(frames[0], D.decode(big), "the large file")
    frames, st, _ = run_full([big], dec=dec)         # staging buffer 0, the first batch's, is replaced
    assert not st.any() and dec.uploaded_bytes() > packed_init
    assert_same_frame(frames[0], D.decode(big), "the large file again")
    frames, st, _ = run_full([tiny, tiny], dec=dec)
    assert not st.any()
    assert_same_frame(frames[1], D.expected("own-16x16"), "own-16x16 in the grown buffers")


# ---------------------------------------------------------------------------------------------- overlay
OV_FPS, FG, BG = 30.0, (252, 3, 115), (10, 200, 30)
HUD = dict(x=3, y=5, scale=1, bg=BG)
FRAME0 = 15


def _three_rows():
    import overlay_ref as R
    d = {k: [] for k in R.COLUMNS}
    for f, x, y in ((13, 0.30, 0.35), (14, 0.42, 0.48), (15, 0.55, 0.60)):
        for k, v in zip(R.COLUMNS, (4, f / OV_FPS, x, y, 0.0, 0.0, 0.3, 0.25)):
            d[k].append(v)
    return d


def _live_tracker():
    """a one-clip tracker with live analysis that saw a plate go up and down for 10 s: a few phases"""
    from vbt_amd.ocsort import MultiClipTracker
    T = 300
    f = np.arange(1, T + 1, dtype=np.float64)
    y = 0.5 + 0.14 * np.sin(2 * np.pi * f / (1.5 * OV_FPS))
    dets = np.zeros((T, 1, 25, 6))
    dets[:, 0, 0] = np.stack([np.full(T, 0.36), y - 0.08, np.full(T, 0.64), y + 0.08, np.full(T, 0.9), np.zeros(T)], 1)
    mc = MultiClipTracker(1, 8192, max_age=30, asso_func="diou", iou_threshold=0.1)
    mc.enable_live(path_cap=4096, phase_cap=128)
    mc.update_frames(dets, np.ones((T, 1), np.int32), (f / OV_FPS).reshape(T, 1))
    return mc


def test_overlay_rows_and_panel_change_their_source_and_back():
    import overlay_follow_util as U
    import overlay_hud_ref as HR
    import overlay_ref as R
    from test_gpu_overlay import assert_same, noise
    from test_gpu_overlay_follow import DeviceLog
    from vbt_amd import _lib
    from vbt_amd.mem import DeviceBuffer
    from vbt_amd.overlay import Overlay
    H = W = 64
    frame = noise((1, H, W, 3), 21)
    rows, none = _three_rows(), {k: [] for k in R.COLUMNS}
    two = {k: v[1:] for k, v in rows.items()}
    ov = Overlay(H, W, "rgb24", rgb=FG)

    def drawn():
        buf = DeviceBuffer.from_host(frame)
        ov.draw(buf.ptr, 1, FRAME0)
        _lib.check(_lib.lib().vbt_stream_synchronize(None))
        return buf.to_host(frame.shape, np.uint8)

    with_rows = R.draw(frame, rows, OV_FPS, frame0=FRAME0, rgb=FG)
    assert (with_rows != frame).any()
    ov.set_rows(rows, OV_FPS)
    assert_same(drawn(), with_rows)
    ov.set_rows(none, OV_FPS)                        # no rows: nothing allocated, nothing drawn
    assert_same(drawn(), frame)
    log = U.emission_log(rows)
    dl = DeviceLog(8)
    ov.follow(dl.rows.ptr, dl.count.ptr, dl.cap, 40, 4, OV_FPS)
    assert_same(drawn(), frame)                      # following, no row consumed yet
    dl.append(log)
    ov.follow_update()
    assert ov.follow_status() == (3, 0)
    assert_same(drawn(), with_rows)
    ov.set_rows(two, OV_FPS)                         # back to rows from the host: the follow allocation goes
    with_two = R.draw(frame, two, OV_FPS, frame0=FRAME0, rgb=FG)
    assert (with_two != with_rows).any()
    assert_same(drawn(), with_two)
    # ---- the panel: a table of its own, the followed table inside the follow allocation, off, a table of its own again
    ph2 = np.array([[1 / OV_FPS, 8 / OV_FPS, 0.4, 0.6, 0.5, 0.0], [9 / OV_FPS, 20 / OV_FPS, 0.6, 0.4, 0.5, 1.0]])
    ov.set_hud(ph2, OV_FPS, **HUD)
    assert np.array_equal(ov.hud_table(), HR.table(ph2, OV_FPS))
    assert_same(drawn(), HR.draw(frame, two, OV_FPS, ph2, frame0=FRAME0, hud_params=HUD, rgb=FG))
    mc = _live_tracker()
    ov.hud_follow(mc, 0, OV_FPS, **HUD)
    ov.hud_follow_update()
    live = mc.live()[0]
    followed = HR.table(live.phases, OV_FPS)
    assert len(followed) >= 2 and live.overflow == 0
    assert np.array_equal(ov.hud_table(), followed)
    want = with_two.copy()
    want[0] = HR.paint_panel(want[0], HR.panel_mask(followed, FRAME0, 1, 1, 200), 3, 5, "rgb24", FG, BG)
    assert_same(drawn(), want)
    ov.set_hud(None)
    assert_same(drawn(), with_two)
    ph1 = ph2[:1]
    ov.set_hud(ph1, OV_FPS, **HUD)
    assert np.array_equal(ov.hud_table(), HR.table(ph1, OV_FPS))
    assert_same(drawn(), HR.draw(frame, two, OV_FPS, ph1, frame0=FRAME0, hud_params=HUD, rgb=FG))
    with pytest.raises(_lib.VbtError, match="follows no live analysis"):
        ov.hud_follow_update()


# ---------------------------------------------------------------------------------------------- evaluator
def test_eval_staging_slots_on_two_streams_across_a_reset():
    import eval_ref
    from test_gpu_eval import _check_curves, _check_table, _crafted_images, _restated_table
    from vbt_amd import _lib
    from vbt_amd.evaluate import Evaluator
    from vbt_amd.mem import DeviceBuffer
    L = _lib.lib()
    images = _crafted_images()
    first, second = images[:12], images[12:24]       # six calls each: more than the four staging slots, every slot is used again
    streams = [ctypes.c_void_p(), ctypes.c_void_p()]
    for s in streams:
        _lib.check(L.vbt_stream_create(0, ctypes.byref(s)))
    ev = Evaluator(len(first) * 25, max_batch=2)
    keep = []

    def add(part):
        for i0 in range(0, len(part), 2):
            two = part[i0:i0 + 2]
            bufs = [DeviceBuffer.from_host(np.stack([np.asarray(im[k], dt).reshape(shp) for im in two]))
                    for k, dt, shp in ((0, np.float32, (25, 4)), (1, np.float32, (25,)), (2, np.int32, ()))]
            keep.append(bufs)
            ev.add(bufs[0].ptr, bufs[1].ptr, bufs[2].ptr, [(im[3], im[4]) for im in two], [im[5] for im in two], stream=streams[(i0 // 2) % 2])

    add(first)
    _check_table(ev.table(), _restated_table(first))
    ev.reset()
    assert len(ev.table()["score"]) == 0
    add(second)
    want = _restated_table(second)
    _check_table(ev.table(), want)
    ref = eval_ref.curves(want["score"], want["iou"], 0.5)
    got = ev.curves(0.5)
    assert (got.n_rows, got.n_pos, got.n_neg, got.flags) == (ref.n_rows, ref.n_pos, ref.n_neg, ref.flags)
    _check_curves(got, ref, "after the reset")
    del ev
    for s in streams:
        _lib.check(L.vbt_stream_destroy(s))
