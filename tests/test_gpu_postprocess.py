"""Decode + NMS (`postprocess_kernel`, family decode_nms) driven directly: crafted int8 head bytes are written into the ten input tensors
of the post-process op (Interpreter.write_tensor), the plan's last step runs alone (Interpreter.run_postprocess) and the four outputs
must equal the numpy reference of tests/postprocess_ref.py bit for bit.  The frames are the scenarios of tests/postprocess_cases.py,
whose coverage conditions (which sort, how many rounds and slices, where the 25th survivor lies) tests/test_postprocess_ref_host.py
asserts on the CPU.  Six models: Lite0 (every scenario), Lite2 (more than 64 KB of LDS, anchors beyond the register slots) and
TinyModel(S=32) with 1, 2, 3 and 4 class columns (C == 1 staging, C == 2 pair loads, the generic column loop).  Eight scenarios share a
batch, and every batch runs with its frames rolled by 0..3 slots: the byte offset of a small level inside a frame slot decides between the
aligned load and the patched dword."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import postprocess_cases as pc  # noqa: E402

pytestmark = pytest.mark.gpu
MAX_BATCH = 8


@pytest.fixture(scope="module")
def files(tmp_path_factory, model_path):
    return pc.model_files(tmp_path_factory.mktemp("post"), model_path)


def _interpreter(path, m, max_batch):
    from vbt_amd.interpreter import Interpreter
    it = Interpreter(model_path=path, max_batch=max_batch, flags=8)       # no autotuning: the plan does not change this kernel
    last = [e for e in it.plan_space() if e["chosen"]][-1]
    assert last["family"] == "decode_nms" and last["last_op"] == m.op_index
    assert all(it.materialized(t) for t in m.inputs)
    return it


def _run(it, m, frames):
    """frames: cases, one per frame slot -> asserts the kernel's outputs against each case's reference."""
    B = len(frames)
    per = [m.to_levels(c.cls, c.box) for c in frames]
    for k, tid in enumerate(m.inputs):
        it.write_tensor(tid, np.stack([p[k] for p in per]))
    boxes, scores, classes, counts = it.run_postprocess(B)
    for b, c in enumerate(frames):
        r = c.ref
        tag = (c.name, "slot", b, "of", B)
        assert counts[b] == r.count, (tag, int(counts[b]), r.count)
        assert np.array_equal(scores[b], r.scores), tag                   # rows [count, 25) included: the kernel zero-fills them
        assert np.array_equal(boxes[b], r.boxes), tag
        assert np.array_equal(classes[b], r.classes), tag


@pytest.mark.parametrize("name", pc.MODELS)
def test_postprocess_equals_reference(files, name):
    path, kind = files[name]
    m, cases = pc.build(path, kind)
    it = _interpreter(path, m, MAX_BATCH)
    for b0 in range(0, len(cases), MAX_BATCH):
        batch = cases[b0:b0 + MAX_BATCH]
        batch = batch + cases[:MAX_BATCH - len(batch)]                    # the last batch is filled up from the front
        for roll in range(4):
            _run(it, m, batch[-roll:] + batch[:-roll] if roll else batch)


@pytest.mark.parametrize("name", pc.MODELS)
def test_postprocess_single_frame_and_prefix(files, name):
    """B = 1 on a model created for one frame, and a B = 3 prefix of a model created for eight (slots 3..7 hold other frames' bytes)."""
    path, kind = files[name]
    m, cases = pc.build(path, kind)
    deep = [c for c in cases if c.name in ("mixed_ranks", "low_plateau", "plateau_all")]
    one = _interpreter(path, m, 1)
    for c in deep + [cases[0]]:
        _run(one, m, [c])
    it = _interpreter(path, m, MAX_BATCH)
    _run(it, m, cases[-MAX_BATCH:])
    _run(it, m, deep[:3] if len(deep) >= 3 else (deep + cases[:3])[:3])


def test_write_tensor_checks_its_arguments(files):
    from vbt_amd import _lib
    path, kind = files["tiny_c2"]
    m, cases = pc.build(path, kind)
    it = _interpreter(path, m, 2)
    t = m.to_levels(cases[0].cls, cases[0].box)[0]
    it.write_tensor(m.inputs[0], np.stack([t, t]))
    assert np.array_equal(it.read_tensor(m.inputs[0], 2)[1], t)
    buf = np.zeros(4 * t.size, np.int8)
    L = _lib.lib()
    assert L.vbt_model_write_tensor(it.handle, -1, 1, buf.ctypes.data) == -1                     # VBT_ERR_ARG
    assert L.vbt_model_write_tensor(it.handle, it.num_tensors(), 1, buf.ctypes.data) == -1
    assert L.vbt_model_write_tensor(it.handle, m.inputs[0], 1, None) == -1
    assert L.vbt_model_write_tensor(it.handle, m.inputs[0], 3, buf.ctypes.data) == L.vbt_model_read_tensor(it.handle, m.inputs[0], 3, buf.ctypes.data) != 0
    fused = [t for t in range(1, it.num_tensors()) if not it.materialized(t)]
    if fused:
        assert L.vbt_model_write_tensor(it.handle, fused[0], 1, buf.ctypes.data) == L.vbt_model_read_tensor(it.handle, fused[0], 1, buf.ctypes.data) != 0
    with pytest.raises(ValueError):
        it.write_tensor(m.inputs[0], t)
