"""The all-blocks form of the large-K pointwise conv (pw_f_kernel, variants 7 / 8 of pw_conv_mfma_i8): a workgroup owns its 64 or 128
pixels for every 64-channel output block.  Forced through VBT_PW_VARIANT (read once per process, hence a child process per case) and
compared with the oracle tensor by tensor; the plan space must offer the form exactly where it has something to share."""
import os
import pickle
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu

LITE2 = os.path.join(ROOT, "models", "efficientdet_lite2_synth.vbtm")

CHILD = (
    "import pickle, sys, numpy as np\n"
    "from vbt_amd.interpreter import Interpreter\n"
    "model, frames = pickle.load(open(sys.argv[1], 'rb'))\n"
    "B = len(frames)\n"
    "it = Interpreter(model, max_batch=B, flags=8)\n"
    "det = it.detect(frames)\n"
    "ten = {t: it.read_tensor(t, B) for t in range(1, it.num_tensors() - 1) if it.materialized(t)}\n"
    "plan = [(e['family'], e['variant'], e['first_op']) for e in it.plan_space() if e['chosen']]\n"
    "pickle.dump((det, ten, plan), open(sys.argv[2], 'wb'))\n")


@pytest.fixture(scope="module")
def frames():
    from vbt_amd import synth
    return np.concatenate([synth.clip_frames(s, 11 * s, 2) for s in range(3)])   # 6 frames, 3 clips: M = 600 and 2400 pixels


@pytest.fixture(scope="module")
def oracle_run(oracle_lib, model_path, frames):
    det = oracle_lib.OracleDetector(model_path)
    outs, tensors = [], []
    for f in frames:
        outs.append(det.run(f))
        tensors.append([det.tensor(t) for t in range(1, det.num_tensors - 1)])
    return outs, tensors


def _forced(tmp_path, model, frames, variant):
    """(detections, materialised tensors, chosen steps) of one forward in a child process under VBT_PW_VARIANT=variant"""
    src, dst = str(tmp_path / "in.pkl"), str(tmp_path / "out.pkl")
    with open(src, "wb") as f:
        pickle.dump((model, frames), f)
    subprocess.run([sys.executable, "-c", CHILD, src, dst], check=True, cwd=ROOT, env={**os.environ, "VBT_PW_VARIANT": str(variant)}, timeout=300)
    return pickle.load(open(dst, "rb"))


def _check(got, outs, tensors, n, what):
    (boxes, scores, classes, counts), ten, _ = got
    assert len(ten) > 60
    for tid, t in ten.items():
        for b in range(n):
            assert np.array_equal(t[b], tensors[b][tid - 1]), f"tensor {tid} of frame {b} differs under {what}"
    for b in range(n):
        ob, os_, oc, on = outs[b]
        assert counts[b] == on and np.array_equal(scores[b], os_) and np.array_equal(boxes[b], ob) and np.array_equal(classes[b], oc), (what, b)


def _pw_shapes(arch):
    """graph op -> (K, N) of every conv of the graph"""
    from vbt_amd import spec
    g = spec.build_graph(arch)
    return {i: (g.tensors[op.inputs[0]].c, g.tensors[op.output].c) for i, op in enumerate(g.ops) if op.inputs}


@pytest.mark.parametrize("variant", [7, 8])
def test_forced_all_blocks_bit_exact(tmp_path, model_path, frames, oracle_run, variant):
    """Lite0, six frames: M = 600 on the 10x10 maps and 2400 on the 20x20 ones, neither a multiple of 128, so the last workgroup is
    partial and its prefetch clamped.  The projections of b6-b15 cover N = 80 (a quarter of the last block live), 112, 192 and 320 (five
    blocks), K = 480, 672 and 1152, and both epilogues (residual: b7, b9, b10, b12-b14).  Every materialised tensor and every detection
    equals the oracle's."""
    outs, tensors = oracle_run
    _check(_forced(tmp_path, model_path, frames, variant), outs, tensors, len(frames), f"VBT_PW_VARIANT={variant}")


@pytest.mark.parametrize("variant", [7, 8])
def test_forced_all_blocks_single_frame(tmp_path, model_path, frames, oracle_run, variant):
    """One frame: M = 100 < 128, a single partial workgroup on the 10x10 maps."""
    outs, tensors = oracle_run
    _check(_forced(tmp_path, model_path, frames[:1], variant), outs, tensors, 1, f"VBT_PW_VARIANT={variant}, one frame")


def test_all_blocks_offered_where_there_is_something_to_share(model_path):
    """Every pw_conv_mfma_i8 step of Lite0 with K > 256 and more than one 64-channel output block offers 7 and 8; the single-block ones
    (the 320 -> 64 laterals) and the K <= 256 ones do not."""
    from vbt_amd.interpreter import Interpreter
    shapes = _pw_shapes(0)
    offered, withheld = 0, 0
    for flags in (0, 8 | 32768):   # every alternative; the laterals as launches of their own
        space = Interpreter(model_path, max_batch=8, flags=flags).plan_space()
        for e in space:
            if e["family"] != "pw_conv_mfma_i8":
                continue
            K, N = shapes[e["first_op"]]
            if K > 256 and N > 64:
                assert 7 in e["variants"] and 8 in e["variants"], (e, K, N)
                offered += 1
            else:
                assert 7 not in e["variants"] and 8 not in e["variants"], (e, K, N)
                withheld += K > 256
    assert offered >= 10 and withheld >= 1


def test_forced_all_blocks_lite2_bit_exact(tmp_path, oracle_lib):
    """Lite2 (448x448, N up to 352 = six output blocks, K up to 2112 = 33 K-steps) is supported: two frames, the 128-pixel form, whose
    six-block instantiation holds the most accumulators."""
    from vbt_amd import synth
    frames = np.stack([synth.render(synth.background(70 + c, 448), 6 * c) for c in range(2)])
    det = oracle_lib.OracleDetector(LITE2)
    outs, tensors = [], []
    for f in frames:
        outs.append(det.run(f))
        tensors.append([det.tensor(t) for t in range(1, det.num_tensors - 1)])
    got = _forced(tmp_path, LITE2, frames, 8)
    shapes = _pw_shapes(2)
    assert any(fam == "pw_conv_mfma_i8" and shapes[op][0] > 256 and shapes[op][1] > 320 for fam, _, op in got[2]), "no six-block projection ran"
    _check(got, outs, tensors, 2, "VBT_PW_VARIANT=8 on Lite2")
