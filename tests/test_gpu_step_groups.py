"""Step groups of the native pipeline (vbt_pipeline_params.group): `group` consecutive step() calls share one forward of
group x n images and one time-batched OC-SORT walk, while the network entry still runs inside every call.  Nothing may change:
every scenario runs on a group=3 and a group=1 pipeline over the same frames and detections, rows, ids and phases must be equal
bit for bit.  3 clips x 7 frames of the synthetic Lite0 model; the two pipelines are built once and reset between tests."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
N, T = 3, 7


@pytest.fixture(scope="module")
def frames():
    from vbt_amd import synth
    return np.stack([np.stack([synth.render(synth.background(21 + c), 7 * c + t) for c in range(N)]) for t in range(T)])


@pytest.fixture(scope="module")
def frames_dev(frames):
    import torch
    return torch.from_numpy(frames).to("cuda:0")


@pytest.fixture(scope="module")
def pipes(model_path):
    """(group=1, group=3) on the same model and settings; a test resets them before use"""
    from vbt_amd.track import Pipeline
    p1 = Pipeline(model_path, N, max_frames=64, fps=60.0, slot_close=True, group=1)
    p3 = Pipeline(model_path, N, max_frames=64, fps=60.0, slot_close=True, group=3)
    assert p1.group == 1 and p3.group == 3 and p3.info().defer == 0
    return p1, p3


def _stream():
    import torch
    return torch.cuda.current_stream().cuda_stream


def _result(pipe):
    """what a clip close gives, and every clip's row log"""
    best, rows_n, nph, ovf, ph = pipe.close(cap=64)
    counts, rows = pipe.rows_all()
    return {"best": best, "rows_n": rows_n, "nph": nph, "ovf": ovf, "ph": ph, "counts": counts,
            "rows": [rows[c, :counts[c]].copy() for c in range(pipe.n_trk)]}


def _same(a, b, what=""):
    if isinstance(a, dict):
        assert a.keys() == b.keys(), what
        for k in a:
            _same(a[k], b[k], f"{what}.{k}")
    elif isinstance(a, (list, tuple)):
        assert len(a) == len(b), what
        for i, (x, y) in enumerate(zip(a, b)):
            _same(x, y, f"{what}[{i}]")
    elif isinstance(a, np.ndarray) and a.dtype.names:
        assert a.shape == b.shape, what
        for f in a.dtype.names:
            assert np.array_equal(a[f], b[f], equal_nan=a[f].dtype.kind == "f"), f"{what}.{f}"
    elif isinstance(a, np.ndarray):
        assert np.array_equal(a, b), what
    else:
        assert a == b, what


def _seven_steps(pipe, frames_dev):
    pipe.reset()
    for t in range(T):
        pipe.step(frames_dev[t].data_ptr(), _stream())
    return _result(pipe)


@pytest.fixture(scope="module")
def ref7(pipes, frames_dev):
    """the seven plain steps on the ungrouped pipeline, every frame in a buffer of its own"""
    r = _seven_steps(pipes[0], frames_dev)
    assert int(r["counts"].sum()) > 0          # rows were emitted: the comparisons below are not vacuous
    return r


def test_seven_steps_two_groups_and_a_partial_one(pipes, frames_dev, ref7):
    """3 + 3 + 1: the last step is still held back when close() flushes it"""
    p3 = pipes[1]
    _same(_seven_steps(p3, frames_dev), ref7)
    b, s, c, k = p3.detections()               # after the close: still the last step's n detections
    p1 = pipes[0]
    _seven_steps(p1, frames_dev)
    _same([b, s, c, k], list(p1.detections()))
    assert b.shape == (N, 25, 4)


def test_one_device_buffer_overwritten_after_every_step(pipes, frames_dev, ref7):
    """The caller keeps ONE frame buffer: once the step's entry has run on the detector stream the caller's stream overwrites it.
    A pipeline that deferred the entry to the end of the group would read the overwritten frames."""
    import torch
    for pipe in pipes:
        pipe.reset()
        buf = torch.empty_like(frames_dev[0])
        cur = torch.cuda.current_stream()
        for t in range(T):
            buf.copy_(frames_dev[t])
            k = int(pipe.info().next_slot)
            pipe.step(buf.data_ptr(), cur.cuda_stream)
            det = torch.cuda.ExternalStream(pipe._det_streams[k].cuda_stream, device=buf.device)
            cur.wait_event(det.record_event())     # everything step() enqueued that reads the buffer
            buf.fill_(255 if t % 2 else 0)
        _same(_result(pipe), ref7, f"group={pipe.group}")


def test_one_pinned_host_buffer_overwritten_after_every_step(pipes, frames, ref7):
    """The same from pinned host memory: the upload runs on the copy stream inside the call, so the buffer is free once that stream is idle."""
    from vbt_amd.mem import pinned_empty
    for pipe in pipes:
        pipe.reset()
        host = pinned_empty(frames[0].shape, np.uint8)
        for t in range(T):
            host[...] = frames[t]
            pipe.step(host)
            pipe._copy_stream.synchronize()
            host[...] = 255 if t % 2 else 0
        _same(_result(pipe), ref7, f"group={pipe.group}")


def test_detections_read_in_mid_group(pipes, frames_dev, ref7):
    got = []
    for pipe in pipes:
        pipe.reset()
        dets = []
        for t in range(T):
            pipe.step(frames_dev[t].data_ptr(), _stream())
            if t in (1, 4, 5):
                dets.append(list(pipe.detections()))
        got.append(dets)
        _same(_result(pipe), ref7, f"group={pipe.group}")      # reading flushes the group early and changes nothing
    _same(got[1], got[0])
    assert all(d[3].shape == (N,) for d in got[1])


def test_skip_frames_and_close_clips_in_mid_group(pipes, frames_dev):
    got = []
    for pipe in pipes:
        pipe.reset()
        st = _stream()
        pipe.step(frames_dev[0].data_ptr(), st)
        pipe.step(frames_dev[1].data_ptr(), st)
        pipe.skip_frames(2)                         # frames 3 and 4 are dropped: the next step is frame 5
        pipe.step(frames_dev[2].data_ptr(), st)
        pipe.step(frames_dev[3].data_ptr(), st)
        pipe.close_clips([1])                       # clip 1 ends here, a new clip starts in its slot at frame 1
        pipe.step(frames_dev[4].data_ptr(), st)
        closed = pipe.closed(1, wait=True)
        pipe.step(frames_dev[5].data_ptr(), st)
        pipe.step(frames_dev[6].data_ptr(), st)
        got.append({"closed": list(closed), "end": _result(pipe), "frame_count": pipe.frame_count})
    _same(got[1], got[0])
    assert got[0]["frame_count"] == 9 and len(got[0]["closed"][1]["id"]) > 0


def test_run_of_detector_only_steps(pipes, frames_dev):
    got = []
    for pipe in pipes:
        pipe.reset()
        dets = []
        for t in range(T):
            pipe.step(frames_dev[t].data_ptr(), _stream(), track=t not in (2, 3, 4))
            if t == 4:
                dets = list(pipe.detections())
        got.append({"dets": dets, "end": _result(pipe)})
    _same(got[1], got[0])
    assert int(got[0]["end"]["counts"].sum()) > 0


def test_active_mask_differs_between_the_steps_of_a_group(pipes, frames_dev):
    masks = [[1, 1, 1], [1, 0, 1], [0, 1, 1], [1, 1, 0], [1, 1, 1], [0, 0, 1], [1, 1, 1]]
    got = []
    for pipe in pipes:
        pipe.reset()
        for t in range(T):
            pipe.step(frames_dev[t].data_ptr(), _stream(), active=masks[t])
        got.append(_result(pipe))
    _same(got[1], got[0])
    assert int(got[0]["counts"].sum()) > 0


def test_clip_map_differs_between_the_steps_of_a_group(pipes, frames_dev):
    maps = [[0, 1, 2], [2, 0, 1], [2, 0, -1], [1, 2, 0], [0, 1, 2], [0, -1, 2], [1, 0, 2]]
    got = []
    for pipe in pipes:
        pipe.reset()
        seen = [0] * N
        for t in range(T):
            idx = []
            for c in maps[t]:
                if c >= 0:
                    seen[c] += 1
                idx.append(seen[c] if c >= 0 else 0)
            pipe.step(frames_dev[t].data_ptr(), _stream(), clip_map=maps[t], frame_idx=idx)
        got.append(_result(pipe))
    _same(got[1], got[0])
    assert int(got[0]["counts"].sum()) > 0


def test_reset_with_a_group_pending(pipes, frames_dev, ref7):
    for pipe in pipes:
        pipe.reset()
        pipe.step(frames_dev[5].data_ptr(), _stream())
        pipe.step(frames_dev[6].data_ptr(), _stream())      # group=3: both still held back
        _same(_seven_steps(pipe, frames_dev), ref7, f"group={pipe.group}")


def test_step_groups_with_the_tracker_on_its_own_stream(model_path, frames_dev, ref7):
    """depth 2 puts the OC-SORT walk on the tracker stream: it waits there for the group's forward and for the walk before it"""
    from vbt_amd.track import Pipeline
    pipe = Pipeline(model_path, N, max_frames=64, fps=60.0, slot_close=True, group=3, depth=2)
    info = pipe.info()
    assert pipe.group == 3 and info.depth == 2 and info.tracker_inline == 0
    _same(_seven_steps(pipe, frames_dev), ref7)


def test_step_runs_between_plain_steps(pipes, frames_dev):
    """Frame 3 arrives as a time-batched step: on the grouped pipeline it closes the group of frames 1 and 2 and runs a forward of its own"""
    got = []
    for pipe in pipes:
        pipe.reset()
        st = _stream()
        pipe.step(frames_dev[0].data_ptr(), st)
        pipe.step(frames_dev[1].data_ptr(), st)
        pipe.step_runs(frames_dev[2], [(c, c, 1, 3) for c in range(N)], st)
        pipe.skip_frames(1)                         # the run step does not count frames: frame 3 is counted here
        for t in range(3, T):
            pipe.step(frames_dev[t].data_ptr(), st)
        got.append(_result(pipe))
    _same(got[1], got[0])
    assert int(got[0]["counts"].sum()) > 0
