"""The SORT tracker on the CPU: the numpy restatement (tests/sort_ref.py) against the reference's committed SORT frames (reference
dfs/*.pkl.gz -> tests/golden/dfs_sort.npz, tools/make_golden_sort.py), and what the C ABI refuses before any device call.

`sort-track` is not vendored, so these frames are the evidence for the algorithm.  The detections come from the OC-SORT fixture
(every emitted OC-SORT row carries the detector's box); on 12 of the 34 clips that fixture holds every detection SORT saw, and
there the replay's (id - id offset, time) key set IS the reference's: time, dx, dy and the ids are then bit-exact on every row,
x and y within half an ulp (TOL_XY), w and h within the 1e-6 that OC-SORT's convert_bbox_to_z left in a track's first recovered
detection (sort_cases.py).  The other 22 clips diverge where OC-SORT's min_hits hid detections from the fixture: unpinned."""
import ctypes

import numpy as np
import pytest

import sort_cases as sc
import sort_ref


def test_fixture_holds_the_fully_matching_clips():
    fx = sc.fixture()
    assert tuple(sorted(fx)) == sc.FULL_CLIPS                    # no clip dropped from the list silently
    assert len(fx) >= 12 and sum(len(g["id"]) for g, _, _ in fx.values()) >= 19000
    for clip, (g, offset, export_id) in fx.items():
        assert g["id"].min() == offset + 1 and export_id in g["id"], clip        # the clip's ids start right above its offset
    # the package's id counter runs through the whole corpus: offsets grow with the clip number, the last clip's file id is 93
    offs = [fx[c][1] for c in sc.FULL_CLIPS]
    assert offs == sorted(offs) and offs[0] == 9 and fx["033"][2] == 93


def test_reference_replay_equals_the_sort_frames():
    rows = 0
    for clip in sc.FULL_CLIPS:
        rep, stats = sc.clip_replay(clip)
        rows += sc.check_against_dfs(clip, rep)
        assert stats["nan_removals"] == 0, clip
    assert rows >= 19000


def test_replay_is_sensitive_to_what_the_fit_pins():
    """Two choices the data pins.  With the boxes rounded to float32 first (it changes only a clip's first, state-derived box) the
    velocities of clip 010 stop being bit-exact.  With OC-SORT's 1e-6 in r the velocities stay (r is a filter of its own) but the
    posterior w and h leave the late-row tolerance."""
    g, offset, _ = sc.fixture()["010"]
    frames, times = sc.clip_detections("010")

    def replay(fr, patch=None):
        saved = sort_ref.convert_bbox_to_z
        if patch:
            sort_ref.convert_bbox_to_z = patch
        try:
            rows, _ = sort_ref.track_boxes(fr, times)
        finally:
            sort_ref.convert_bbox_to_z = saved
        return {k: np.asarray(v) for k, v in rows.items()}

    def exact_dx(rows):
        ref = dict(zip(zip(g["id"] - offset, g["time"]), g["dx"]))
        return sum(ref.get((i, t)) == v for i, t, v in zip(rows["id"], rows["time"], rows["dx"]))

    from oracle import ocsort_np as oc
    assert exact_dx(replay(frames)) == len(g["id"])
    f32 = [np.concatenate([f[:, :4].astype(np.float32).astype(np.float64), f[:, 4:]], 1) for f in frames]
    assert exact_dx(replay(f32)) < len(g["id"])
    eps = replay(frames, oc.convert_bbox_to_z)
    assert exact_dx(eps) == len(g["id"])
    with pytest.raises(AssertionError, match="norm_plate"):
        sc.check_against_dfs("010", eps)


def test_reference_counters_and_id_base():
    frames, tm = sc.random_scene(3)
    rows, stats = sort_ref.track_boxes(frames, tm, max_age=sc.SCENE_MAX_AGE, iou_threshold=0.3)
    assert stats["assignment_frames"] > 0 and stats["late_births"] > 0 and stats["deaths"] > 0 and stats["nan_removals"] == 0
    based, _ = sort_ref.track_boxes(frames, tm, max_age=sc.SCENE_MAX_AGE, iou_threshold=0.3, id_base=93)
    assert min(based["id"]) == 94 and [i - 93 for i in based["id"]] == rows["id"] and based["dx"] == rows["dx"]
    # a zero-height detection: r = inf, the posterior box is NaN, the track leaves on the next frame's predict
    t = sort_ref.SortTracker(max_age=30)
    out = t.update(np.array([[0.1, 0.1, 0.2, 0.2, 0.9, 0.0], [0.5, 0.5, 0.6, 0.5, 0.9, 0.0]]))
    assert len(out) == 2 and np.isnan(out[0, :4]).any() and not np.isnan(out[1]).any()
    t.update(np.array([[0.1, 0.1, 0.2, 0.2, 0.9, 0.0]]))
    assert t.stats["nan_removals"] == 1 and [k.id for k in t.trackers] == [0]


# ---- the C ABI's refusals (include/vbt_hip.h, vbt_tracker_create_sort): argument checks come before any device call ----

def _lib_built():
    import __graft_entry__ as ge
    ge.build()
    from vbt_amd import _lib
    return _lib, _lib.lib()


@pytest.mark.parametrize("bad", [dict(max_age=-1), dict(min_hits=-1), dict(iou_threshold=float("nan")), dict(iou_threshold=float("inf")),
                                 dict(iou_threshold=float("-inf")), dict(id_base=-1), dict(id_base=0x40000000)])
def test_create_sort_refuses_bad_parameters(bad):
    _l, L = _lib_built()
    kw = dict(max_age=30, min_hits=3, id_base=0, iou_threshold=0.3)
    kw.update(bad)
    p = _l.SortParams(kw["max_age"], kw["min_hits"], kw["id_base"], kw["iou_threshold"])
    h = ctypes.c_void_p(0x1234)
    assert L.vbt_tracker_create_sort(1, 64, ctypes.byref(p), 0, ctypes.byref(h)) == -1          # VBT_ERR_ARG
    assert h.value is None and L.vbt_last_error()                                                # *out cleared, a message left
    assert L.vbt_pipeline_use_sort(None, ctypes.byref(p)) == -1


def test_create_sort_refuses_null_pointers_and_sizes():
    _l, L = _lib_built()
    p = _l.SortParams(30, 3, 0, 0.3)
    h = ctypes.c_void_p()
    assert L.vbt_tracker_create_sort(1, 64, None, 0, ctypes.byref(h)) == -1
    assert L.vbt_tracker_create_sort(1, 64, ctypes.byref(p), 0, None) == -1
    assert L.vbt_tracker_create_sort(0, 64, ctypes.byref(p), 0, ctypes.byref(h)) == -1
    assert L.vbt_tracker_create_sort(1, 0, ctypes.byref(p), 0, ctypes.byref(h)) == -1
    assert L.vbt_pipeline_use_sort(None, ctypes.byref(p)) == -1 and L.vbt_pipeline_use_sort(None, None) == -1
    assert ctypes.sizeof(_l.SortParams) == 24 and _l.SortParams.iou_threshold.offset == 16      # vbt_sort_params as the compiler lays it out


def test_python_wrappers_refuse_before_the_library():
    _lib, _ = _lib_built()
    from vbt_amd.sort import MultiClipSortTracker, sort_params
    from vbt_amd.track import Pipeline, track_frames
    with pytest.raises(ValueError):
        sort_params(max_age=1.5)
    with pytest.raises(_lib.VbtArgError):
        MultiClipSortTracker(1, 64, max_age=-1)
    with pytest.raises(ValueError, match="tracker must be one of"):
        Pipeline("no_such_model", 1, 1, tracker="bytetrack")
    with pytest.raises(ValueError, match="tracker must be one of"):
        track_frames(np.zeros((1, 8, 8, 3), np.uint8), "no_such_model", tracker="deepsort")


def test_sort_has_no_cpu_fallback():
    """valid parameters reach the device: without one the creation fails loudly (not an argument error), with one it works"""
    import torch
    _l, L = _lib_built()
    p = _l.SortParams(30, 3, 0, 0.3)
    h = ctypes.c_void_p()
    rc = L.vbt_tracker_create_sort(1, 64, ctypes.byref(p), 0, ctypes.byref(h))
    if torch.cuda.is_available():
        assert rc == 0 and h.value
        L.vbt_tracker_destroy(h)
    else:
        assert rc not in (0, -1) and h.value is None and L.vbt_last_error()
