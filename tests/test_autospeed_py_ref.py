"""The Python AutoSpeed wrapper's CPU pin: tests/autospeed_py_ref.py -- the restatement of Models/inference/auto_speed_infer.py around a raw detector
tensor -- reproduces tests/golden/autospeed_py.npz, the results of the reference class's OWN method bodies (tools/pin_autospeed_py.py asserted distance
0.0 between the two when it wrote the file); its letterbox is the project's Pillow restatement; the library's host geometry is Python's."""
import os
import sys

import numpy as np
import pytest
from PIL import Image

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import autospeed_py_cases as cases  # noqa: E402
import autospeed_py_ref as ref  # noqa: E402
from autoware_vision_pilot_amd import synthetic  # noqa: E402
from oracle import pre_post  # noqa: E402

G = np.load(cases.GOLDEN)


def _image(h, w, seed):
    return Image.fromarray(np.ascontiguousarray(synthetic.synthetic_frame(h, w, seed)[:, :, ::-1]))


def test_fixture_letterbox_and_conditions():
    """Geometry and the tensor sample at 0.0 (Pillow and one division: nothing depends on the machine); one frame pads left / right, one top / bottom;
    the thresholds are recorded; a kept box is clamped."""
    pads = []
    for fi, (h, w, seed) in enumerate(G["frames"]):
        x, geom = ref.letterbox_pil(_image(int(h), int(w), int(seed)))
        assert x.shape == (3, 512, 1024) and x.dtype == np.float32
        assert np.array_equal(np.array(geom, np.float64), G[f"geom_{fi}"])
        assert np.array_equal(x.ravel()[::int(G["tensor_step"])].view(np.uint32), G[f"tensor_{fi}"].view(np.uint32))
        pads.append((geom[1] > 0, geom[2] > 0))
    assert pads == [(True, False), (False, True)]
    assert float(G["conf"]) == ref.CONF and 0.3 <= float(G["iou"]) <= 0.7
    rows = np.concatenate([G["rows_0"], G["rows_1"]])
    assert (rows[:, :2] == 0).any() or any((G[f"rows_{fi}"][:, 2] == G["frames"][fi][1]).any() or (G[f"rows_{fi}"][:, 3] == G["frames"][fi][0]).any() for fi in range(2))


def test_restatement_reproduces_the_reference_wrappers_rows():
    """The decode of the reference module's own raw columns (every box near or above the threshold): the kept set, its order, the classes and the
    coordinates at 0.0; the score goes through torch's sigmoid, whose vector code may differ in the last bit between CPUs (1e-6)."""
    for raw, conf, iou, geom, ow, oh, want in cases.fixture_cases():
        score_gap, iou_gap, n = ref.candidate_iou_gap(raw, conf, iou)
        assert score_gap > 2e-3 and iou_gap > 2e-3 and 20 <= n <= 2000
        got = ref.decode(raw, geom, ow, oh, conf, iou)
        assert got.shape == want.shape and len(want) >= 3
        assert np.array_equal(got[:, 5], want[:, 5]) and len(set(want[:, 5])) > 1
        assert np.array_equal(got[:, :4], want[:, :4])
        assert float(np.abs(got[:, 4] - want[:, 4]).max()) <= 1e-6
        every = ref.post_process(raw, conf, 2.0).numpy()
        assert len(every) == n > len(want)                        # something was suppressed


def test_hand_built_cases_keep_what_the_rules_say():
    for name, raw, conf, iou, geom, ow, oh, cap, kept in cases.decode_cases():
        lb = ref.post_process(raw, conf, iou).numpy()
        idx = [int(np.flatnonzero(raw[0] + raw[1] * 1000 == (r[0] + r[2]) / 2 + (r[1] + r[3]) / 2 * 1000)[0]) for r in lb]
        assert idx == kept, name
        rows = ref.decode(raw, geom, ow, oh, conf, iou)
        assert rows.shape == (len(kept), 6) and (rows[:, [0, 2]] <= ow).all() and (rows[:, [1, 3]] <= oh).all() and (rows[:, :4] >= 0).all()
        if name == "clamped":
            assert tuple(rows[0, :2]) == (0.0, 0.0) and tuple(rows[1, 2:4]) == (float(ow), float(oh))
        if name == "cross-class suppression":
            assert list(rows[:, 5]) == [0.0, 3.0]


@pytest.mark.parametrize("size", [(1, 1), (37, 53), (1920, 1080), (500, 1000)])
def test_letterbox_pil_is_the_projects_pillow_restatement(size):
    """letterbox_pil (Pillow itself) against oracle/pre_post.py resize_pil_u8 -- the arithmetic whose tables the device kernels use -- pasted on 114s
    and divided by 255: equal on ragged (width, height) sizes."""
    w, h = size
    f = cases.frame(h, w, w + h)
    got, (scale, pad_x, pad_y) = ref.letterbox_pil(Image.fromarray(f))
    _, new_w, new_h, px, py = ref.letterbox_geometry(w, h)
    assert (px, py) == (pad_x, pad_y)
    canvas = np.full((512, 1024, 3), 114, np.uint8)
    canvas[pad_y:pad_y + new_h, pad_x:pad_x + new_w] = pre_post.resize_pil_u8(f, new_h, new_w, pre_post.PIL_BILINEAR)
    want = canvas.astype(np.float32).transpose(2, 0, 1) / np.float32(255)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))


def test_to_tensor_table():
    """ToTensor is one fp32 division: np.float32(v) / np.float32(255) for all 256 bytes -- and NOT v * fl(1 / 255), which differs for some of them."""
    import torch

    v = np.arange(256, dtype=np.uint8)
    img = Image.fromarray(np.repeat(v[None, :, None], 3, axis=2))
    x, _ = ref.letterbox_pil(img, (256, 1))
    want = v.astype(np.float32) / np.float32(255)
    assert np.array_equal(x[0, 0].view(np.uint32), want.view(np.uint32))
    assert np.array_equal(torch.from_numpy(v).to(torch.float32).div(255).numpy().view(np.uint32), want.view(np.uint32))
    assert (v.astype(np.float32) * np.float32(1.0 / 255.0) != want).any()


def test_host_geometry_is_pythons():
    """vp_detect_geometry_pil against int() and // on a sweep of sizes, among them every width whose w * scale comes within 1e-9 of an integer without
    being one in exact arithmetic's place (1024 / w * w rounds below 1024 for some w: the truncation then gives 1023)."""
    from autoware_vision_pilot_amd import lib

    sizes = [(w, 1) for w in range(1, 4097)] + [(1, h) for h in range(1, 2049)]
    rng = np.random.default_rng(3)
    sizes += [(int(a), int(b)) for a, b in rng.integers(1, 5000, (3000, 2))]
    sizes += [(1280, 720), (1920, 1080), (1024, 512), (2048, 1024), (53, 37), (100, 90), (1, 1)]
    near = 0
    for w, h in sizes:
        scale, new_w, new_h, pad_x, pad_y = ref.letterbox_geometry(w, h)
        for v in (w * scale, h * scale):
            near += abs(v - round(v)) < 1e-9 and v != round(v)
        if new_w < 1 or new_h < 1:
            with pytest.raises(ValueError):
                lib.detect_geometry_pil(512, 1024, h, w)
            continue
        assert lib.detect_geometry_pil(512, 1024, h, w) == (scale, new_w, new_h, pad_x, pad_y), (w, h)
    assert near >= 10
    assert ref.letterbox_geometry(49, 1)[1] == int(49 * (1024 / 49))
