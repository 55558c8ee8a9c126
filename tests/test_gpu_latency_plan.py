"""The latency kernel plan (creation flag VP_PLAN_LATENCY; what adapters/hip_backend.hpp creates by default) through the whole networks on the
device.  tests/test_gpu_networks.py, the shared-head tests and the parity sweep run the default plan only (the session fixture `engines` cannot
pass the flag); this module holds the latency plan to the same bars for the same quantities, imported from where they are defined:

  * against the CPU oracle: input tensor bit-exact, the five backbone taps and the logits within 1e-3 in the parity mode, FP16_TOL in fp16, the
    full_<kind>.npz samples within 1e-3; class maps under test_class_map_parity's strict rule, decodes bit-exact on the engine's own logits;
  * against the default plan on the same frame (include/vp_hip.h: the plans' "results differ only in fp32 summation order"): every activation
    produced before the first launch that differs between the plans -- the whole encoder and the context block among them -- bit-identical;
  * mixed plans on a shared prefix ("a shared-prefix engine may choose differently from its base"): a head of one plan on a base of the other;
  * graph replay bit-stable, no plan state leaking between a latency and a default engine interleaved in one process;
  * the eight frames of the parity sweep on each network's base weight seed, at the plain bar.

Which launches differ is pinned on the CPU (tests/test_engine_emulated.py::test_latency_plan_is_the_committed_one); their kernels run alone against
fp64 in tests/test_gpu_decoder_kernels.py (LATENCY_CONVS).  The worst errors per network are printed at the end of the module."""
import os

import numpy as np
import pytest
import torch

from test_gpu_networks import FP16_TOL, KINDS, PREFIX_BB, _rel, _tensor_by_name
from test_gpu_parity_sweep import BASE_SEED, FRAMES, _decode

pytestmark = pytest.mark.gpu

_worst = {}


def _record(what, kind, err):
    _worst[(what, kind)] = max(_worst.get((what, kind), 0.0), float(err))


@pytest.fixture(scope="module", autouse=True)
def _worst_table():
    yield
    if _worst:
        print("\nlatency plan, worst error per network (parity: |err| / max(1, |ref|); fp16: max |err| / max |ref|):")
        for (what, kind), err in sorted(_worst.items()):
            print(f"  {what:<28} {kind:<10} {err:.3e}")


@pytest.fixture(scope="module")
def latency_engines(state_dicts):
    """engines per (kind, precision) created with VP_PLAN_LATENCY, cached for this module"""
    from autoware_vision_pilot_amd import lib, weights as vw

    cache = {}

    def get(kind, precision):
        key = (kind, precision)
        if key not in cache:
            cache[key] = lib.Engine(kind, vw.pack_state_dict(state_dicts(kind)), precision=precision, plan_latency=True)
        return cache[key]

    yield get
    for e in cache.values():
        e.close()


def _launches(eng):
    return [(n, k, l) for (n, _, _), k, l in zip(eng.layers(), eng.layer_kernels(), eng.layer_launches())]


@pytest.mark.parametrize("kind", KINDS)
def test_latency_network_parity_fp16x3(latency_engines, oracle_runs, frame720, kind):
    """test_network_parity_fp16x3 and test_golden_fixture of tests/test_gpu_networks.py, on the latency plan"""
    eng = latency_engines(kind, "fp16x3")
    assert any(k.startswith("conv3x3_map<co32,px800") for k in eng.layer_kernels()) and not any(k.startswith("conv3x3_map2<") for k in eng.layer_kernels())
    ref_out, inter, x = oracle_runs(kind)
    eng.infer(frame720)
    assert np.array_equal(eng.input_tensor(), x)
    P = PREFIX_BB[kind]
    bb = {P + "0": 0, P + "2.1.block.3": 1, P + "3.1.block.3": 2, P + "4.2.block.3": 3, P + "8": 4}
    for name, fi in bb.items():
        got = _tensor_by_name(eng, name)
        assert _rel(got, inter["feats"][fi][0].numpy()) <= 1e-3, f"{kind} {name}"
    got = eng.logits()
    assert got.shape == ref_out.shape
    err = _rel(got, ref_out)
    _record("fp16x3 logits vs oracle", kind, err)
    assert err <= 1e-3, f"{kind} logits rel err {err:.3e}"
    g = np.load(os.path.join(os.path.dirname(__file__), "golden", f"full_{kind}.npz"))
    assert _rel(got.ravel()[g["samples_idx"]], g["samples"]) <= 1e-3


@pytest.mark.parametrize("kind", KINDS)
def test_latency_network_parity_fp16(latency_engines, oracle_runs, frame720, kind):
    eng = latency_engines(kind, "fp16")
    neck = [k for (n, _, _), k in zip(eng.layers(), eng.layer_kernels()) if n.endswith(("decode_layer_1", "decode_layer_3", "decode_layer_5"))]
    assert len(neck) == 3 and all(k.startswith("conv3x3_halo<co64,px128,x1") for k in neck), neck   # below 160 tiles the fp16 latency plan keeps the halo kernel
    ref_out, _, _ = oracle_runs(kind)
    eng.infer(frame720)
    got = eng.logits()
    err = np.abs(got - ref_out).max() / np.abs(ref_out).max()
    _record("fp16 logits vs oracle", kind, err)
    assert err <= FP16_TOL, f"{kind}: fp16 max err / max|ref| = {err:.3e}"


def test_latency_class_maps(latency_engines, oracle_runs, frame720):
    """SceneSeg's class-index map under the strict rule of test_class_map_parity (zero flips outside twice the measured logit error, that band
    <= 2e-3); every decode is integer work, bit-exact against the oracle decode of the engine's own logits"""
    from autoware_vision_pilot_amd import lib
    from oracle import pre_post

    ref_out, _, _ = oracle_runs("sceneseg")
    ref_cls = pre_post.argmax_classes(ref_out)
    srt = np.sort(ref_out, axis=0)
    margin = srt[-1] - srt[-2]
    eng = latency_engines("sceneseg", "fp16x3")
    eng.set_decode_mode(lib.VP_DECODE_CLASS_INDEX)
    try:
        eng.infer(frame720)
        cls = eng.mask().astype(np.int64)
        assert np.array_equal(cls, pre_post.argmax_classes(eng.logits()))
        flips = cls != ref_cls
        band = 2.0 * float(np.abs(eng.logits() - ref_out).max()) + 1e-12
        assert band <= 2e-3
        assert (margin[flips] <= band).all(), f"{flips.sum()} flips, one outside the tolerance band {band:.3e}: max margin {margin[flips].max():.3e}"
    finally:
        eng.set_decode_mode(lib.VP_DECODE_SEG_MASK)
    eng.infer(frame720)
    assert np.array_equal(eng.mask(), pre_post.seg_mask_u8(eng.logits()))
    ego = latency_engines("egolanes", "fp16x3")
    ego.infer(frame720)
    assert ego.logits().shape == (3, 80, 160)
    assert np.array_equal(ego.mask(), pre_post.egolanes_priority_mask(ego.logits()))
    ego.set_decode_mode(lib.VP_DECODE_LANE_LABEL)
    try:
        ego.infer(frame720)
        assert np.array_equal(ego.mask(), pre_post.egolanes_priority_mask(ego.logits()))
    finally:
        ego.set_decode_mode(lib.VP_DECODE_SEG_MASK)
    dom = latency_engines("domainseg", "fp16x3")
    dom.infer(frame720)
    assert np.array_equal(dom.mask(), pre_post.seg_mask_u8(dom.logits()))


@pytest.mark.parametrize("precision", ["fp16x3", "fp16"])
@pytest.mark.parametrize("kind", KINDS)
def test_latency_prefix_is_bit_identical_to_the_default_plan(engines, latency_engines, frame720, kind, precision):
    """the two plans differ in a handful of decoder launches (the CPU pin states which); everything computed before the first of them -- the
    whole encoder, the context block, the first composed up-sampling stage -- runs the same kernels on the same data, so its activations are
    bit-identical between a default and a latency engine.  If they are not, something besides the known dispatch branches depends on the flag."""
    d, l = engines(kind, precision), latency_engines(kind, precision)
    ld, ll = _launches(d), _launches(l)
    assert [r[0] for r in ld] == [r[0] for r in ll]
    first = next(i for i, (a, b) in enumerate(zip(ld, ll)) if a != b)
    assert ld[:first] == ll[:first] and first > 30, (kind, precision, first)
    assert ll[first][0].endswith("decode_layer_1"), ll[first]
    td, tl = d.tensors(), l.tensors()
    assert td == tl
    names = [t[0] for t in tl]
    stop = names.index(ll[first][0])           # the first tensor a differing launch writes
    assert any("context" in n for n in names[:stop]) and sum("encoder" in n for n in names[:stop]) >= 20
    d.infer(frame720)
    l.infer(frame720)
    assert np.array_equal(d.input_tensor(), l.input_tensor())
    different = [names[i] for i in range(stop) if not np.array_equal(d.tensor_read(i).view(np.uint32), l.tensor_read(i).view(np.uint32))]
    assert not different, f"{kind}/{precision}: {len(different)} of {stop} tensors before {names[stop]} differ between the plans: {different[:6]}"
    assert np.isfinite(l.tensor_read(stop)).all()


@pytest.fixture(scope="module")
def mixed_setup(state_dicts, frame720):
    """SceneSeg + Scene3D on SceneSeg's encoder (oracle.weights.share_backbone), in the parity mode: a base and a head of each plan, the
    standalone Scene3D engine of each plan, and the oracle's Scene3D output"""
    from autoware_vision_pilot_amd import lib, weights as vw
    from oracle import nets, pre_post, weights

    sd_seg = state_dicts("sceneseg")
    sd_3d = weights.share_backbone(dict(state_dicts("scene3d")), "scene3d", sd_seg, "sceneseg")
    x = torch.from_numpy(pre_post.preprocess(frame720, input_is_bgr=True, planes_rgb=False))
    ref = nets.forward("scene3d", nets.to_torch(sd_3d), x)[0].numpy()
    blob_seg, blob_3d = vw.pack_state_dict(sd_seg), vw.pack_state_dict(sd_3d)
    made = []

    def mk(*a, **kw):
        made.append(lib.Engine(*a, precision="fp16x3", **kw))
        return made[-1]

    out = {}
    for base_latency in (False, True):
        base = mk("sceneseg", blob_seg, plan_latency=base_latency)
        out[("base", base_latency)] = base
        for head_latency in (False, True):
            out[("head", base_latency, head_latency)] = mk("scene3d", blob_3d, base=base, plan_latency=head_latency)
    for latency in (False, True):
        out[("alone", latency)] = mk("scene3d", blob_3d, plan_latency=latency)
    yield ref, out
    for e in reversed(made):
        e.close()


@pytest.mark.parametrize("base_latency,head_latency", [(False, True), (True, False)], ids=["latency-head-on-default-base", "default-head-on-latency-base"])
def test_mixed_plans_on_a_shared_prefix(mixed_setup, frame720, base_latency, head_latency):
    """a Scene3D head of one plan on a SceneSeg base of the other: the shared level of the unmixed pair; the head's launches are the tail of a
    standalone Scene3D engine of the HEAD's plan; its logits are bit-identical to that engine's (sharing and mixing change the execution
    plan, not a kernel) and within 1e-3 of the oracle -- through vp_infer_multi and through vp_infer + vp_infer_shared"""
    ref, e = mixed_setup
    base, head, alone = e[("base", base_latency)], e[("head", base_latency, head_latency)], e[("alone", head_latency)]
    unmixed = e[("head", base_latency, base_latency)]
    assert base.shared_level() == 0 and head.shared_level() == unmixed.shared_level() == 1
    lh, la = _launches(head), _launches(alone)
    own = [r for r in lh if "encoder" not in r[0] and r[0] != "preprocess"]
    assert len(own) > 12 and own == la[len(la) - len(own):], [(a, b) for a, b in zip(own, la[len(la) - len(own):]) if a != b][:4]
    assert len(lh) == len(_launches(unmixed)) and lh != _launches(unmixed)          # ... and not the base's plan
    alone.infer(frame720)
    want = alone.logits().copy()
    base.infer_multi([head], frame720)
    got_multi = head.logits().copy()
    base.infer(frame720)
    head.infer_shared()
    got_shared = head.logits().copy()
    for how, got in (("vp_infer_multi", got_multi), ("vp_infer + vp_infer_shared", got_shared)):
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), f"{how}: max |diff| to the standalone engine {np.abs(got - want).max():.3e}"
        err = _rel(got, ref)
        _record("fp16x3 mixed-plan head", "scene3d", err)
        assert err <= 1e-3, f"{how}: {err:.3e}"


@pytest.mark.parametrize("kind,precision", [("sceneseg", "fp16"), ("sceneseg", "fp16x3"), ("egolanes", "fp16x3")])
def test_latency_graph_replay_is_deterministic(latency_engines, frame720, kind, precision):
    """as test_graph_replay_is_deterministic: eager pass, capture, replays of one frame -- the same bits (the split-K slabs of this plan's map and
    halo launches are re-initialised and summed in a fixed order)"""
    eng = latency_engines(kind, precision)
    eng.use_graph(False)
    try:
        eng.infer(frame720)
        a = eng.logits().copy()
    finally:
        eng.use_graph(True)
    outs = []
    for _ in range(4):
        eng.infer(frame720)
        outs.append(eng.logits().copy())
    assert all(np.array_equal(a.view(np.uint32), o.view(np.uint32)) for o in outs)


@pytest.mark.parametrize("precision", ["fp16x3", "fp16"])
def test_latency_and_default_engines_interleaved(engines, latency_engines, frame720, precision):
    """a latency and a default engine of one network, enqueued alternately in one process: each reproduces its own solo result bit for bit
    (the plan is a property of the engine; no option is set here)"""
    from oracle import pre_post

    d, l = engines("sceneseg", precision), latency_engines("sceneseg", precision)
    other = pre_post.synthetic_frame(720, 1280, 77)
    d.infer(frame720)
    solo_d = d.logits().copy()
    l.infer(frame720)
    solo_l = l.logits().copy()
    d.infer(other)
    l.infer(other)
    d.upload_frame(frame720)
    l.upload_frame(frame720)
    for _ in range(3):
        d.enqueue()
        l.enqueue()
    d.fetch_outputs()
    l.fetch_outputs()
    assert np.array_equal(d.logits().view(np.uint32), solo_d.view(np.uint32))
    assert np.array_equal(l.logits().view(np.uint32), solo_l.view(np.uint32))
    assert _launches(d) != _launches(l)


@pytest.mark.parametrize("kind", KINDS)
def test_latency_parity_sweep_base_seeds(kind):
    """the eight frames of tests/test_gpu_parity_sweep.py on the network's BASE weight seed, parity mode, latency engine.  On the base seeds that
    module's report asserts that every default-plan pass meets the plain bar, so the same holds here with no fp64 re-judging:
    |error| <= 1e-3 x max(1, |ref|), the engine's decode bit-exact on its own logits, zero flips outside twice the measured error."""
    from autoware_vision_pilot_amd import lib, weights as vw
    from oracle import nets, pre_post, weights

    sd = weights.make_state_dict(kind, BASE_SEED[kind])
    sdt = nets.to_torch(sd)
    eng = lib.Engine(kind, vw.pack_state_dict(sd), precision="fp16x3", plan_latency=True)
    mode = {"sceneseg": lib.VP_DECODE_CLASS_INDEX, "egolanes": None}.get(kind, lib.VP_DECODE_SEG_MASK)
    if mode is not None:
        eng.set_decode_mode(mode)
    rgb = kind == "egolanes"
    eng.set_input_format(lib.VP_BGR8, lib.VP_PLANES_RGB if rgb else lib.VP_PLANES_BGR)
    fails, worst_pass = [], (0.0, None)
    try:
        for (h, w), fseed, smooth in FRAMES:
            frame = pre_post.synthetic_frame(h, w, fseed, smooth=smooth)
            x = pre_post.preprocess(frame, input_is_bgr=True, planes_rgb=rgb)
            ref = nets.forward(kind, sdt, torch.from_numpy(x))[0].numpy()
            eng.infer(frame)
            got = eng.logits()
            assert np.array_equal(eng.input_tensor(), x)
            assert np.isfinite(got).all()
            err_abs = float(np.abs(got - ref).max())
            err_rel = _rel(got, ref)
            ref_cls, margin = _decode(kind, ref)
            got_cls, _ = _decode(kind, got)
            if kind == "sceneseg":
                assert np.array_equal(eng.mask().astype(np.int64), got_cls)
            elif kind == "domainseg":
                assert np.array_equal(eng.mask() > 0, got_cls > 0)
            elif kind == "egolanes":
                assert np.array_equal(eng.mask(), pre_post.egolanes_priority_mask(got))
            flips = got_cls != ref_cls
            nflip = int(flips.sum())
            worst = float(margin[flips].max()) if nflip else 0.0
            if err_rel > worst_pass[0]:
                worst_pass = (err_rel, f"{h}x{w} frame seed {fseed}, max |err| {err_abs:.3e}, {nflip} flips")
            if err_rel > 1e-3:
                fails.append(f"{kind} frame {fseed}: logits rel err {err_rel:.3e}")
            if kind != "scene3d" and not (nflip == 0 or worst <= 2.0 * err_abs):
                fails.append(f"{kind} frame {fseed}: {nflip} flips, largest oracle margin {worst:.3e} vs max logit error {err_abs:.3e}")
    finally:
        eng.close()
    print(f"\nlatency sweep, {kind} weight seed {BASE_SEED[kind]}: worst of {len(FRAMES)} frames {worst_pass[0]:.3e} ({worst_pass[1]})")
    _record("fp16x3 sweep of 8 frames", kind, worst_pass[0])
    assert not fails, fails
