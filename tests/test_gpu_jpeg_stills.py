"""JPEG stills on the GPU (include/vbt_hip.h, "JPEG stills"): ONE batch whose frames differ in size and sampling.  Straight to the network
input, every frame must EQUAL preprocess_image (oracle/preprocess.py) of the numpy statement's frame (tests/mjpeg_dec_ref.py); as
full-size frames, the numpy statement's frame.  Integer and pinned float32 on both sides: array_equal everywhere, no tolerance.
The sizes are the small ones at which it can go wrong: W <= 4 (the replicate rule), odd sizes (the dw / dh edge rules under a tap at
W - 1 / H - 1), 1 x 1 upscaled (all four taps clamp), sources smaller than, at, and far larger than the target (16 x 2064 -> 32 wide:
scale 64.5), and neighbours of different size, so that a wrong per-frame offset shows as the neighbour's pixels."""
import numpy as np
import pytest

import mjpeg_dec_ref as D
from oracle.preprocess import preprocess_image
from test_gpu_mjpeg_decode import assert_same_frame, gpu_decode, mixed_batch
from test_jpeg_stills_host import TARGETS, edge_vectors, layout_blocks

pytestmark = pytest.mark.gpu

# all 15 vectors, interleaved: no two neighbours share size and sampling
ORDER = ["own-16x16", "pil-24x40-444", "pil-40x56-420-optimize", "pil-9x23-grey", "pil-40x56-no-restarts", "own-1x1", "pil-40x56-restart-rows-1",
         "pil-17x33-422", "pil-40x56-restart-blocks-1", "own-16x2064-one-interval", "own-32x48-q1", "own-17x33", "own-32x48-q100",
         "own-160x32-noise-q95", "own-17x33-no-dht"]
PATTERN = 0xA5


def batch():
    return [D.vectors()[n] for n in ORDER]


def sizes(jpegs):
    return [(d["H"], d["W"]) for d in map(D.parse, jpegs)]


_want = {}


def want_resized(jpeg, hw, swap):
    """computed once per (file, target, order), shared, read-only"""
    key = (jpeg, hw, bool(swap))
    if key not in _want:
        _want[key] = preprocess_image(D.decode(jpeg), hw, swap_rb=bool(swap))[0]
        _want[key].setflags(write=False)
    return _want[key]


def run_resized(jpegs, hw, swap, dec=None, entropy="auto"):
    """-> (uint8 [B, h, w, 3], status, handle)"""
    from vbt_amd.mem import DeviceBuffer
    from vbt_amd.stills import JpegStills
    dec = dec or JpegStills(max_batch=len(jpegs), block_budget=sum(map(layout_blocks, jpegs)), entropy=entropy)
    buf = DeviceBuffer.from_host(np.full((len(jpegs), hw[0], hw[1], 3), PATTERN, np.uint8))
    dec.decode_resized(jpegs, buf.ptr, hw[0], hw[1], swap_rb=swap)
    st = dec.status()
    return buf.to_host((len(jpegs), hw[0], hw[1], 3), np.uint8), st, dec


def run_full(jpegs, dec=None, entropy="auto", gap=0):
    """-> ([frame uint8 [H_i, W_i, 3]], status, the whole buffer): the frames packed one behind the other, `gap` bytes between them"""
    from vbt_amd.mem import DeviceBuffer
    from vbt_amd.stills import JpegStills
    dec = dec or JpegStills(max_batch=len(jpegs), block_budget=sum(map(layout_blocks, jpegs)), entropy=entropy)
    hw = sizes(jpegs)
    off = np.zeros(len(jpegs) + 1, np.uint64)
    off[1:] = np.cumsum([H * W * 3 + gap for H, W in hw])
    buf = DeviceBuffer.from_host(np.full(int(off[-1]), PATTERN, np.uint8))
    dec.decode(jpegs, buf.ptr, off)
    st = dec.status()
    raw = buf.to_host((int(off[-1]),), np.uint8)
    return [raw[int(o):int(o) + H * W * 3].reshape(H, W, 3) for o, (H, W) in zip(off, hw)], st, raw


def test_the_batch_is_what_it_claims():
    assert sorted(ORDER) == sorted(D.vectors()) and len(ORDER) == 15
    kinds = [(d["H"], d["W"], d["comps"][0][:2], len(d["comps"])) for d in map(D.parse, batch())]
    assert all(a != b for a, b in zip(kinds, kinds[1:]))
    hw = {k[:2] for k in kinds}
    assert {(16, 16), (1, 1), (17, 33), (160, 32), (16, 2064), (24, 40), (9, 23), (40, 56), (32, 48)} == hw
    e = sizes(list(edge_vectors().values()))
    assert set(TARGETS) <= set(e) and sum(W <= 4 for _, W in e) == 3


@pytest.mark.parametrize("swap", (0, 1))
@pytest.mark.parametrize("hw", TARGETS)
def test_mixed_batch_straight_to_the_network_input(hw, swap):
    jpegs = batch()
    got, st, _ = run_resized(jpegs, hw, swap)
    assert not st.any(), st
    for i, (name, j) in enumerate(zip(ORDER, jpegs)):
        assert_same_frame(got[i], want_resized(j, hw, swap), f"{name} -> {hw}, swap {swap}")


@pytest.mark.parametrize("hw", TARGETS)
def test_identity_small_widths_and_upscaling(hw):
    """sources exactly at the target, W <= 4 at 4:2:0 and 4:2:2, 2 x 2: the cases the 15 vectors leave out"""
    e = edge_vectors()
    names = sorted(e)
    got, st, _ = run_resized([e[n] for n in names], hw, 0)
    assert not st.any()
    for i, n in enumerate(names):
        assert_same_frame(got[i], want_resized(e[n], hw, 0), f"{n} -> {hw}")
    same = [n for n in names if sizes([e[n]])[0] == hw]
    assert len(same) == 1 and np.array_equal(got[names.index(same[0])], D.decode(e[same[0]]))       # identity: the decoded frame itself


def test_mixed_batch_as_full_size_frames():
    jpegs = batch()
    frames, st, raw = run_full(jpegs, gap=5)
    assert not st.any(), st
    for name, f in zip(ORDER, frames):
        assert_same_frame(f, D.expected(name), name)
    used = sum(f.size for f in frames)
    assert (raw == PATTERN).sum() >= raw.size - used and all((raw[int(o) - 5:int(o)] == PATTERN).all() for o in np.cumsum([f.size + 5 for f in frames]))


def test_interval_and_sync_give_the_same_bytes():
    jpegs = batch()
    out = {}
    for mode in ("interval", "sync"):
        got, st, dec = run_resized(jpegs, (20, 28), 0, entropy=mode)
        frames, st2, _ = run_full(jpegs, dec=dec)
        assert not st.any() and not st2.any() and dec.entropy_info()["path"] == {"interval": 1, "sync": 2}[mode]
        out[mode] = (got, frames)
    assert np.array_equal(out["interval"][0], out["sync"][0])
    assert all(np.array_equal(a, b) for a, b in zip(out["interval"][1], out["sync"][1]))
    assert_same_frame(out["sync"][1][9], D.expected(ORDER[9]), ORDER[9])
    _, _, dec = run_resized(jpegs[:3], (20, 28), 0)                                     # AUTO: short scans take INTERVAL ...
    assert dec.entropy[0] == "auto" and dec.entropy_info()["path"] == 1
    long_scan = D.pil_jpeg(D.noise((96, 128, 3), 5), quality=95, subsampling=0)             # ... one interval above the threshold takes SYNC
    assert D.parse(long_scan)["scan"][1] >= dec.entropy[2]
    mixed = [jpegs[0], long_scan, jpegs[3]]
    got, st, dec = run_resized(mixed, (32, 32), 1)
    assert not st.any() and dec.entropy_info()["path"] == 2
    for i, j in enumerate(mixed):
        assert_same_frame(got[i], want_resized(j, (32, 32), 1), f"auto / sync, frame {i}")


def test_a_damaged_scan_spoils_its_own_frame_only():
    v = D.vectors()
    bad = D.damaged_frame(v["pil-40x56-restart-rows-1"])
    img, status = D.decode(bad, with_status=True)
    assert status != 0
    jpegs = [v["own-17x33"], bad, v["pil-24x40-444"]]
    for mode in ("interval", "sync"):
        got, st, dec = run_resized(jpegs, (20, 28), 0, entropy=mode)
        assert st.tolist() == [0, status, 0], (mode, st)
        assert_same_frame(got[0], want_resized(jpegs[0], (20, 28), 0), "the frame before")
        assert_same_frame(got[2], want_resized(jpegs[2], (20, 28), 0), "the frame behind")
        frames, st, _ = run_full(jpegs, dec=dec)
        assert st.tolist() == [0, status, 0]
        assert_same_frame(frames[0], D.expected("own-17x33"), "the full-size frame before")
        assert_same_frame(frames[2], D.expected("pil-24x40-444"), "the full-size frame behind")


def test_refused_batches_leave_the_output_untouched():
    from vbt_amd import _lib
    from vbt_amd.mem import DeviceBuffer
    from vbt_amd.stills import JpegStills
    jpegs = batch()[:4]
    need = sum(map(layout_blocks, jpegs))
    dec = JpegStills(max_batch=4, block_budget=need)
    got, st, _ = run_resized(jpegs, (20, 28), 0, dec=dec)                                   # the handle works, and has its scratch
    assert not st.any()
    buf = DeviceBuffer.from_host(np.full((5, 20, 28, 3), PATTERN, np.uint8))
    over = jpegs[:3] + [D.vectors()["pil-40x56-no-restarts"]]                               # 72 blocks where 6 were
    assert sum(map(layout_blocks, over)) > need
    progressive = jpegs[:2] + [D.pil_jpeg(D.smooth(24, 40, 1), quality=85, progressive=True)]
    for files, reason in ((over, "the handle's budget is"), (progressive, "frame 2 of the batch: SOF2 (progressive)"), (jpegs + jpegs[:1], "5 frames, the handle was created for 4")):
        with pytest.raises(_lib.VbtError, match=reason.replace("(", r"\(").replace(")", r"\)")):
            dec.decode_resized(files, buf.ptr, 20, 28)
        with pytest.raises(_lib.VbtError, match=reason.replace("(", r"\(").replace(")", r"\)")):
            dec.decode(files, buf.ptr, np.arange(len(files) + 1, dtype=np.uint64) * 56 * 40 * 3)
    _lib.check(_lib.lib().vbt_stream_synchronize(None))
    assert (buf.to_host((5, 20, 28, 3), np.uint8) == PATTERN).all()
    assert dec.status().tolist() == [0, 0, 0, 0]                                           # the last batch decoded is still the good one
    got2, st, _ = run_resized(jpegs, (20, 28), 0, dec=dec)
    assert not st.any() and np.array_equal(got, got2)


def test_smaller_and_larger_batches_on_one_handle():
    from vbt_amd.stills import JpegStills
    jpegs = batch()
    dec = JpegStills(max_batch=15, block_budget=sum(map(layout_blocks, jpegs)))
    for first, n in ((0, 15), (9, 2), (5, 1), (3, 7), (0, 15)):
        got, st, _ = run_resized(jpegs[first:first + n], (32, 32), 0, dec=dec)
        assert not st.any()
        for k in range(n):
            assert_same_frame(got[k], want_resized(jpegs[first + k], (32, 32), 0), f"{n} frames from {first}, frame {k}")
    assert dec.uploaded_bytes() > sum(map(len, jpegs)) // 2 and dec.plan(jpegs) == [(0, 15)]


def test_the_video_handle_still_gives_its_frames():
    """the kernels are shared: a uniform batch through vbt_mjpeg_decode, table filled uniformly, equals the numpy statement as before"""
    jpegs = mixed_batch()
    frames, status = gpu_decode(jpegs, max_batch=8)
    assert not status.any()
    for k, j in enumerate(jpegs):
        assert_same_frame(frames[k], D.decode(j), f"frame {k}")
    v = D.vectors()
    family = [v[n] for n in ("pil-40x56-420-optimize", "pil-40x56-no-restarts", "pil-40x56-restart-rows-1", "pil-40x56-restart-blocks-1")]
    frames, status = gpu_decode(family)
    assert not status.any() and all(np.array_equal(f, D.expected("pil-40x56-no-restarts")) for f in frames[1:])
    assert_same_frame(frames[0], D.expected("pil-40x56-420-optimize"))
