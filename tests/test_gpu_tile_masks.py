"""The expand stage of the fused MBConv tile kernels without halo-mask work on interior tiles (fused_block.h: the out-of-image mask is built
only on tiles whose halo leaves the image, the expand loop has a flavour without the select for the others, the tail lanes of the last pixel
group are found by `p < NPh`; vbt_amd/csrc/halo_geom.h) against the oracle.

The cases are those of test_gpu_fused_params.py, whose child process they run: a written plan that puts b1-b4 on the tile kernels
profiles/plan_lite0.b256.f0 pins (9 57 9 57) and b5 on the generic matrix-pipe tile kernel (variant 1); every materialised tensor and the
detections must equal the oracle's.  What differs is the frames: uniform noise, an all-0 and an all-255 frame.  On the constant frames every
interior pixel of a map holds one value and the out-of-image halo pixels hold the zero points - a border pixel that is not forced to the
expand's zero point, or an interior pixel that is, changes the first row or column of the map.

These maps are the smallest the shipped models offer and hold what can go wrong: interior and border tiles on every side (b1: 81 of 100
tiles interior; b4: 3 of 15), a one-lane tail group (b1: 289 halo pixels = 18 x 16 + 1), part-filled tiles (b4: 40 wide on 16-wide tiles;
Lite2's 56), both padding conventions (stride 2 SAME on an even map, stride 1)."""
import numpy as np
import pytest

from test_gpu_band_chain import _oracle
from test_gpu_fused_params import LITE0_ON, _only, _run_case
from test_gpu_mbconv_toeplitz import clamped  # noqa: F401  (fixture: the narrowed-range model and the oracle's run of it on `frames`)
from test_gpu_plan_space import LITE2, _lite2_frames, _noise_and_checkerboard

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def frames():
    return np.concatenate([_noise_and_checkerboard(320, 47)[:1], np.zeros((1, 320, 320, 3), np.uint8), np.full((1, 320, 320, 3), 255, np.uint8)])


@pytest.fixture(scope="module")
def oracle_run(oracle_lib, model_path, frames):
    return _oracle(oracle_lib, model_path, frames)


def test_lite0_three_frames(tmp_path, model_path, frames, oracle_run):
    """Three frames at max_batch 4: the chunk parameters through LDS (the kernels of k_fused_mbconv_params.hip)."""
    assert _run_case(tmp_path, model_path, frames, oracle_run, 4) == LITE0_ON


def test_lite0_params_from_global_memory(tmp_path, model_path, frames, oracle_run):
    """VBT_FUSED_PARAMS=0: the same tiles on the kernels of k_fused_mbconv_tail.hip."""
    assert _run_case(tmp_path, model_path, frames, oracle_run, 4, {"VBT_FUSED_PARAMS": "0"}) == _only(())


def test_lite0_block_major(tmp_path, model_path, frames, oracle_run):
    """VBT_PROJ_TAIL=0: the block-major instantiations (b2 then takes its parameters from global memory)."""
    got = _run_case(tmp_path, model_path, frames, oracle_run, 4, {"VBT_PROJ_TAIL": "0"})
    assert got == [(v, n, 0, on and i != 1) for i, (v, n, _, on) in enumerate(LITE0_ON)]


def test_without_biased_accumulators(tmp_path, model_path, frames, oracle_run):
    """VBT_NO_KBIAS=1: the converting requantisation flavours of the expand loop, with and without the select."""
    assert _run_case(tmp_path, model_path, frames, oracle_run, 4, {"VBT_NO_KBIAS": "1"}) == LITE0_ON


def test_explicit_clamps(tmp_path, frames, clamped):  # noqa: F811
    """The clamped model: the explicitly clamped flavours."""
    path, oracle = clamped
    assert _run_case(tmp_path, path, frames, oracle, 4) == LITE0_ON


def test_single_frame(tmp_path, model_path, frames, oracle_run):
    """One frame (the all-255 one) at max_batch 1."""
    outs, tensors = oracle_run
    assert _run_case(tmp_path, model_path, frames[2:], (outs[2:], tensors[2:]), 1) == LITE0_ON


def test_lite2_bit_exact(tmp_path, oracle_lib):
    """Lite2 at two frames on 9 57 57 9 57 57: 112 x 112 and 56 x 56 maps (56 = three and a half 16-wide tiles)."""
    f2 = _lite2_frames()
    ran = _run_case(tmp_path, LITE2, f2, _oracle(oracle_lib, LITE2, f2), len(f2), None, (9, 57, 57, 9, 57, 57))
    assert [(v, n) for v, n, _, _ in ran[:6]] == [(9, 24), (57, 24), (57, 24), (9, 48), (57, 48), (57, 48)], ran
