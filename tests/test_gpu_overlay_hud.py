"""Rep panel of the tracking overlay on the GPU, bit for bit against the numpy statement of its contract (tests/overlay_hud_ref.py),
on random noise frames so that an untouched or a wrongly touched byte cannot pass by accident."""
import os

import numpy as np
import pytest
from click.testing import CliRunner

import overlay_hud_ref as HR
import overlay_ref as R

pytestmark = pytest.mark.gpu

H, W, FPS = 120, 160, 30.0
COLOR0 = (252, 3, 115)
BG = (10, 200, 30)
# frame0, frame_step of the batches of 6 frames
EARLY = (8, 1)            # frames 8..13: n = 0 at 8 and 9, rep 0 ends at frame 10 exactly; most timeline columns are frames < 1
SCROLL = (58, 4)          # frames 58, 62, .., 78: n = 8, 9, 9, 10, 11, 11
FAR = (2147483640, 1)     # frames far past the last phase, at the end of int32


def synthetic_phases():
    """23 phases of 3 frames each from frame 4 on: eccentric and concentric in turn, 11 reps, one hold of 3 frames after rep 5.
    Rep r ends at frame 10 + 6 r (r <= 5) or 13 + 6 r (r >= 6).  ROMs: rep 2 has ACV 5 m/s (above the 200 cm/s full scale), rep 7
    0.1 m/s (12 s * 10 / 200 floors to 0 px at s = 1: the stub), rep 9 has ROM 1.115 m (v * 100.0 next to a tie), rep 10 has 250 m
    (both of its integers saturate at 9999)."""
    roms = [0.21, 0.1, 0.5, 0.17, 0.123, 0.08, 0.2, 0.01, 0.15, 1.115, 250.0]
    ph, f = [], 4
    for r in range(11):
        ph.append((f / FPS, (f + 3) / FPS, 0.3, 0.6, roms[r] * 0.9, HR.ECCENTRIC))
        ph.append(((f + 3) / FPS, (f + 6) / FPS, 0.6, 0.3, roms[r], HR.CONCENTRIC))
        f += 6
        if r == 5:
            ph.append((f / FPS, (f + 3) / FPS, 0.3, 0.3, 0.0, HR.HOLD))
            f += 3
    return np.asarray(ph, np.float64)


def crossing_rows():
    """Id 3 on frames 1..13 and 58..78: its box, label, marker and trail run through the top left quarter of the frame, where the panels sit"""
    d = {k: [] for k in R.COLUMNS}
    for f in list(range(1, 14)) + list(range(58, 79)):
        for k, v in zip(R.COLUMNS, (3, f / FPS, 0.18 + 0.012 * (f % 29), 0.55 - 0.011 * (f % 31), 0.0, 0.0, 0.3, 0.22)):
            d[k].append(v)
    return d


def noise(shape, seed):
    return np.random.default_rng(seed).integers(0, 256, shape, dtype=np.uint8)


def gpu_draw(frames, data, phases, batch, pix_fmt="rgb24", hud_params=None, times=1, then_off=False, **params):
    """frames through the device: rows `data` (None: no set_rows at all), the panel of `phases`; (frames back, handle)"""
    from vbt_amd import _lib
    from vbt_amd.mem import DeviceBuffer
    from vbt_amd.overlay import Overlay
    frames = np.ascontiguousarray(frames)
    buf = DeviceBuffer.from_host(frames)
    ov = Overlay(H, W, pix_fmt, **params)
    if data is not None:
        ov.set_rows(data, FPS)
    ov.set_hud(phases, FPS, **(hud_params or {}))
    if then_off:
        ov.set_hud(None)
    for _ in range(times):
        ov.draw(buf.ptr, len(frames), batch[0], batch[1])
    _lib.check(_lib.lib().vbt_stream_synchronize(None))
    return buf.to_host(frames.shape, np.uint8), ov


def assert_same(got, want):
    bad = np.argwhere(got != want)
    assert len(bad) == 0, f"{len(bad)} bytes differ, first at {bad[:5].tolist()}: got {got[tuple(bad[0])]}, want {want[tuple(bad[0])]}"


@pytest.fixture(scope="module")
def phases():
    ph = synthetic_phases()
    ph.setflags(write=False)
    return ph


@pytest.fixture(scope="module")
def rows():
    return crossing_rows()


def test_scenario_holds_what_it_promises(phases):
    """the synthetic phases really contain the cases the tests are about (checked on the reference's integers)"""
    t = HR.table(phases, FPS)
    assert len(t) == 23 and t[-1, 5] == 11 and (t[:, 4] == HR.HOLD).sum() == 1 and t[-1, 1] == 73
    ends = t[t[:, 4] == HR.CONCENTRIC, 1].tolist()
    assert ends == [10 + 6 * r for r in range(6)] + [13 + 6 * r for r in range(6, 11)]
    n = lambda f: len(HR.completed(t, f))
    assert [n(EARLY[0] + i * EARLY[1]) for i in range(6)] == [0, 0, 1, 1, 1, 1]               # frame 10 = fe of rep 0, 9 the one before
    assert [n(SCROLL[0] + i * SCROLL[1]) for i in range(6)] == [8, 9, 9, 10, 11, 11]
    assert n(FAR[0]) == 11
    acv = t[t[:, 4] == HR.CONCENTRIC, 3].tolist()
    assert acv[2] == 500 and acv[7] == 10 and acv[10] == 9999 and t[t[:, 4] == HR.CONCENTRIC, 2][9] == int(np.rint(1.115 * 100.0))
    assert HR.bar_heights(t, 58, 1, 200)[2] == 12 and HR.bar_heights(t, 58, 1, 200)[7] == 1   # above full scale; floors to 0 -> the stub
    assert HR.bar_heights(t, 78, 1, 200)[7] == 12 and HR.bar_heights(t, 78, 1, 200)[4] == 1   # the window has scrolled by three
    assert EARLY[0] - 46 * EARLY[1] < 1 and SCROLL[0] - (47 * 2 - 1) * SCROLL[1] < 1          # timeline columns with fc < 1


@pytest.mark.parametrize("batch", [EARLY, SCROLL, FAR], ids=["early", "scroll", "far"])
@pytest.mark.parametrize("hud_params", [dict(scale=1, x=17, y=9), dict(scale=2, x=W - 104, y=H - 100, bg=BG, full_scale_cm=333)],
                         ids=["s1-odd-x", "s2-corner"])
def test_rgb24_panel_is_bit_exact(phases, batch, hud_params):
    frames = noise((6, H, W, 3), 11)
    want = HR.draw(frames, None, FPS, phases, batch[0], batch[1], hud_params=hud_params, rgb=COLOR0)
    got, _ = gpu_draw(frames, None, phases, batch, hud_params=hud_params, rgb=COLOR0)
    assert_same(got, want)
    s, x, y = hud_params["scale"], hud_params["x"], hud_params["y"]
    outside = np.ones((H, W), bool)
    outside[y:y + 50 * s, x:x + 52 * s] = False
    assert np.array_equal(got[:, outside], frames[:, outside]) and (got[:, ~outside] != frames[:, ~outside]).any()


@pytest.mark.parametrize("fmt", ["nv12", "i420"])
@pytest.mark.parametrize("batch", [EARLY, SCROLL], ids=["early", "scroll"])
def test_yuv_panel_is_bit_exact(phases, fmt, batch):
    frames = noise((6, H * 3 // 2, W), 12)
    for hud_params in (dict(scale=1, x=18, y=10, bg=BG), dict(scale=2, x=W - 104, y=H - 100)):
        want = HR.draw(frames, None, FPS, phases, batch[0], batch[1], pix_fmt=fmt, hud_params=hud_params, rgb=COLOR0)
        got, _ = gpu_draw(frames, None, phases, batch, pix_fmt=fmt, hud_params=hud_params, rgb=COLOR0)
        assert_same(got, want)
    Yf, Uf, Vf = R.yuv_colour(COLOR0)
    assert Uf != Vf and (got[0][:H] == Yf).any()


@pytest.mark.parametrize("fmt", ["rgb24", "nv12"])
def test_rows_cross_the_panel_and_the_panel_wins(phases, rows, fmt):
    shape = (6, H, W, 3) if fmt == "rgb24" else (6, H * 3 // 2, W)
    frames = noise(shape, 13)
    hp = dict(scale=1, x=16, y=10)
    for batch in (EARLY, SCROLL):
        rows_only = R.draw(frames, rows, FPS, frame0=batch[0], frame_step=batch[1], pix_fmt=fmt)
        want = HR.draw(frames, rows, FPS, phases, batch[0], batch[1], pix_fmt=fmt, hud_params=hp)
        luma = (rows_only != frames)[:, :H].reshape(6, H, W, -1).any(axis=3)
        assert luma[:, 10:60, 16:68].any() and luma[:, 60:, :].any()                            # the rows draw inside the panel and outside it
        got, _ = gpu_draw(frames, rows, phases, batch, pix_fmt=fmt, hud_params=hp)
        assert_same(got, want)
        if fmt == "rgb24":
            outside = np.ones((H, W), bool)
            outside[10:60, 16:68] = False
            assert np.array_equal(got[:, outside], rows_only[:, outside])                       # outside the panel: the rows-only bytes


def test_panel_without_rows_idempotence_and_switch_off(phases, rows):
    frames = noise((6, H, W, 3), 14)
    hp = dict(scale=1, x=16, y=10)
    want = HR.draw(frames, None, FPS, phases, *SCROLL, hud_params=hp)
    got, _ = gpu_draw(frames, None, phases, SCROLL, hud_params=hp)                              # a handle that never saw set_rows
    assert_same(got, want)
    got, _ = gpu_draw(frames, {k: [] for k in R.COLUMNS}, phases, SCROLL, hud_params=hp)        # and one with zero rows
    assert_same(got, want)
    want = HR.draw(frames, rows, FPS, phases, *SCROLL, hud_params=hp)
    got, _ = gpu_draw(frames, rows, phases, SCROLL, hud_params=hp, times=2)                     # drawing twice = drawing once
    assert_same(got, want)
    got, ov = gpu_draw(frames, rows, phases, SCROLL, hud_params=hp, then_off=True)              # set_hud(None): the rows-only bytes again
    assert_same(got, R.draw(frames, rows, FPS, frame0=SCROLL[0], frame_step=SCROLL[1]))
    assert ov.hud_table().shape == (0, 6)
    got, _ = gpu_draw(frames, None, np.zeros((0, 6)), SCROLL, hud_params=hp)                    # P = 0 with params: "REP    0", blank fields
    want = HR.draw(frames, None, FPS, np.zeros((0, 6)), *SCROLL, hud_params=hp)
    assert_same(got, want)
    assert (want[0, 10:60, 16:68] == 255).any() and np.array_equal(want[0, 10:60, 16:68], want[5, 10:60, 16:68])


def test_hud_table_equals_the_reference_integers(phases):
    from vbt_amd.overlay import Overlay
    from vbt_amd.velocity import Phase
    ov = Overlay(H, W)
    ov.set_hud(phases, FPS, scale=2, x=0, y=0)
    tab = ov.hud_table()
    ref = HR.table(phases, FPS)
    assert tab.dtype == np.int32 and tab.shape == (23, 6)
    for k, name in enumerate(HR.TABLE):
        assert np.array_equal(tab[:, k], ref[:, k]), name
    ov.set_hud([Phase(*r[:5], int(r[5])) for r in phases], FPS, scale=1)                        # a list of Phase objects is the same table
    assert np.array_equal(ov.hud_table(), tab)


def test_set_hud_refuses_bad_geometry_and_keeps_the_panel(phases):
    from vbt_amd import _lib
    from vbt_amd.overlay import Overlay
    ov = Overlay(H, W, "nv12")
    ov.set_hud(phases, FPS, scale=1, x=16, y=10)
    for kw, word in ((dict(scale=1, x=17, y=10), "even"), (dict(scale=1, x=16, y=11), "even"), (dict(scale=1, x=W - 50, y=0), "inside"),
                     (dict(scale=1, x=0, y=H - 48), "inside"), (dict(scale=3, x=16, y=16), "inside")):
        with pytest.raises(_lib.VbtArgError, match=word):
            ov.set_hud(phases, FPS, **kw)
    assert ov.hud_table().shape == (23, 6)                                                      # a refused call leaves the panel as it was
    Overlay(H, W, "nv12").set_hud(phases, FPS, scale=2, x=W - 104, y=H - 100)                   # flush against the corner is inside
    Overlay(H, W, "rgb24").set_hud(phases, FPS, scale=1, x=17, y=11)                            # odd is fine for RGB24
    with pytest.raises(TypeError):
        ov.set_hud(phases, FPS, colour=(1, 2, 3))


# ---- end to end: the commands on a tiny synthetic clip with the shipped model

STRIDE, CLIP_FPS, HUD = 4, 60.0, ["--hud", "--hud_scale", "2", "--hud_pos", "8,6"]
HUD_PARAMS = dict(scale=2, x=8, y=6)


@pytest.fixture(scope="module")
def tracked(tmp_path_factory, model_path):
    """`track --video_dir --hud` at --concurrent 1 on 460 frames (two and a bit reps of the synthetic squat), every 4th kept"""
    from vbt_amd import synth
    from vbt_amd.cli import main
    tmp = tmp_path_factory.mktemp("hud")
    frames = synth.clip_frames(12, 0, 460)
    src = tmp / "demo.npy"
    np.save(str(src), frames)
    common = ["--model", model_path, "--fps", str(CLIP_FPS), "--detection_treshold", "0.3", "--frame_stride", str(STRIDE)]
    res = CliRunner().invoke(main, ["track", str(src), "--df_dir", str(tmp / "dfs"), "--video_dir", str(tmp / "c1")] + common + HUD)
    assert res.exit_code == 0, res.output
    files = os.listdir(tmp / "dfs")
    assert len(files) == 1, res.output
    return dict(tmp=tmp, frames=frames, src=str(src), common=common, df=str(tmp / "dfs" / files[0]), out=np.load(str(tmp / "c1" / "demo.npy")))


def _analyzed(df_path):
    """the phases `cli analyze` prints for the DataFrame: the rows of the file name's id through analyze_rows(preprocess=True)"""
    import pandas as pd
    from vbt_amd.cli import FILENAME_RE
    from vbt_amd.velocity import analyze_rows
    tid = int(FILENAME_RE.match(os.path.basename(df_path)).group(2))
    df = pd.read_pickle(df_path)
    one = df.query(f"id == {tid}").drop(columns=["id"])
    cols = ["time", "x", "y", "dx", "dy", "norm_plate_height", "norm_plate_width"]
    return df, analyze_rows(np.stack([one[c].to_numpy(np.float64) for c in cols], axis=1), 0.45, preprocess=True)


def test_track_hud_draws_the_reps_analyze_gives(tracked):
    from vbt_amd.overlay import Overlay
    from vbt_amd.velocity import Phase
    df, phases = _analyzed(tracked["df"])
    reps = [p for p in phases if p.type == Phase.CONCENTRIC]
    assert len(reps) >= 1 and reps[0].time_end * CLIP_FPS <= 460                               # a rep completes inside the clip
    out, kept = tracked["out"], 460 // STRIDE
    assert out.shape == (kept, 320, 320, 3)
    for i in list(range(9, kept, 15)) + [kept - 1]:                                            # whole frames, rows and panel, a few of them
        f = (i + 1) * STRIDE
        want = HR.draw(tracked["frames"][f - 1:f], df, CLIP_FPS, phases, frame0=f, frame_step=STRIDE, hud_params=HUD_PARAMS)
        assert_same(out[i:i + 1], want)
    ref = HR.table(phases, CLIP_FPS)
    x, y, s = HUD_PARAMS["x"], HUD_PARAMS["y"], HUD_PARAMS["scale"]
    for i in range(kept):                                                                      # the panel of every frame
        mask = HR.panel_mask(ref, (i + 1) * STRIDE, STRIDE, s, 200)
        assert np.array_equal(out[i, y:y + 50 * s, x:x + 52 * s], np.repeat(np.where(mask, 255, 0).astype(np.uint8)[:, :, None], 3, axis=2)), i
    ov = Overlay(320, 320)
    ov.set_hud(phases, CLIP_FPS, **HUD_PARAMS)
    tab = ov.hud_table()
    con = tab[tab[:, 4] == 0]
    assert con[:, 2].tolist() == [HR.centi(p.rom) for p in reps] and con[:, 3].tolist() == [HR.centi(p.rom / p.duration) for p in reps]
    assert np.array_equal(tab, ref)
    assert HR.text_lines(tab, 460)[1:] == ["ROM" + HR.field(1, int(con[-1, 2])), "ACV" + HR.field(1, int(con[-1, 3]))] and con[-1, 2] > 0


def test_track_hud_concurrent_writes_the_same_frames(tracked):
    from vbt_amd.cli import main
    out = tracked["tmp"] / "c2"
    res = CliRunner().invoke(main, ["track", tracked["src"], "--concurrent", "2", "--video_dir", str(out)] + tracked["common"] + HUD)
    assert res.exit_code == 0, res.output
    assert_same(np.load(str(out / "demo.npy")), tracked["out"])


def test_overlay_hud_reproduces_the_frames_from_the_dataframe(tracked):
    from vbt_amd.cli import main
    out = tracked["tmp"] / "o"
    res = CliRunner().invoke(main, ["overlay", tracked["src"], tracked["df"], "--fps", str(CLIP_FPS), "--frame_stride", str(STRIDE), "--video_dir", str(out)] + HUD)
    assert res.exit_code == 0, res.output
    assert_same(np.load(str(out / "demo.npy")), tracked["out"])


def test_hud_usage_errors(tracked, tmp_path):
    import shutil
    from vbt_amd.cli import main
    res = CliRunner().invoke(main, ["track", tracked["src"], "--hud"] + tracked["common"])
    assert res.exit_code == 2 and "--video_dir" in res.output
    other = tmp_path / "frame.pkl.gz"                                                          # a name FILENAME_RE does not match
    shutil.copy(tracked["df"], other)
    res = CliRunner().invoke(main, ["overlay", tracked["src"], str(other), "--hud", "--video_dir", str(tmp_path / "o")])
    assert res.exit_code == 2 and "file name" in res.output
    res = CliRunner().invoke(main, ["overlay", tracked["src"], tracked["df"], "--hud", "--hud_scale", "7", "--video_dir", str(tmp_path / "o")])
    assert res.exit_code == 2 and "inside" in res.output                                       # 364 x 350 does not fit 320 x 320
