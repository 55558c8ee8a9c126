"""The whole engine on the CPU: csrc/ compiled for the host on the HIP-on-CPU shim (tests/emul), driven through the C ABI
exactly as on the GPU -- weight blob, plan, every kernel incl. the MFMA convolutions (emulated wave-level MFMA), graph
capture / replay as closure lists.  AutoDrive (8 GFLOP, ~8 s emulated) is pinned end to end: tests/golden/autodrive.npz holds the outputs of the reference's OWN nn.Module
(oracle/pin_autodrive.py), so this checks engine == reference without a GPU.  EgoLanes runs whole in the parity mode and SceneSeg (the headline network) in the benchmark's
fp16 mode, ~1 min each; other kinds / modes by hand with tests/emul/run_network.py."""
import ctypes as ct
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "emul"))
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "autodrive.npz")


@pytest.fixture(scope="module")
def emu_lib():
    import build as emul_build

    from autoware_vision_pilot_amd import lib

    if not os.path.exists(emul_build.CLANG):
        pytest.skip("host clang++ of the ROCm toolchain not found")
    so = ct.CDLL(emul_build.build(), mode=os.RTLD_LOCAL | os.RTLD_NOW)     # never RTLD_GLOBAL: same symbol names as libvp_hip.so
    for name, (res, args) in lib._SIGS.items():
        fn = getattr(so, name)
        fn.restype, fn.argtypes = res, args
    saved = lib._lib
    lib._lib = so
    yield lib
    lib._lib = saved


def test_autodrive_engine_end_to_end_on_cpu(emu_lib):
    from autoware_vision_pilot_amd import synthetic, weights as vw
    from oracle import pre_post

    g = np.load(GOLDEN)
    frames = [synthetic.synthetic_frame(1080, 1920, int(s)) for s in g["frame_seeds"]]
    eng = emu_lib.Engine("autodrive", vw.pack_state_dict(synthetic.make_autodrive_state_dict(int(g["weight_seed"]))), precision="fp16x3")
    try:
        eng.infer_pair(frames[0], frames[1])                     # eager pass + graph capture
        got = eng.logits().reshape(3)
        assert np.abs(got - g["fp32_out"]).max() <= 1e-3, (got, g["fp32_out"])      # the GPU parity bar (measured 2.5e-6)
        want_in = pre_post.preprocess(frames[1], input_is_bgr=True, planes_rgb=True, out_h=512, out_w=1024, resize="pil_bilinear")   # the reference's frame path: PIL's antialiased BILINEAR
        assert np.array_equal(eng.input_tensor(), want_in)
        p5 = None
        for i, (n, c, h, w) in enumerate(eng.tensors()):
            if n == "backbone.p5.3.cv2":
                p5 = eng.tensor_read(i)
        ref = g["fp32_p5"]
        assert p5 is not None and np.abs(p5.ravel()[g["fp32_p5_idx"]] - ref).max() <= 1e-3 * max(1.0, float(np.abs(ref).max()))
    finally:
        eng.close()


def test_autodrive_attention_block_kernel_matches_per_query_kernel(emu_lib, vp_opts):
    """kernels_autodrive.hip: the four-queries-per-workgroup attention (round 4; the plan's default for C2PSA's dk = 32, dv = 64) against the
    one-query-per-workgroup kernel it replaces (VP_ATTN_BLOCK=0) on the same network and frames: the attention output and the copy of v, both
    (hi, lo) planes -- same arithmetic order per output except the order of the softmax denominator's sum."""
    from autoware_vision_pilot_amd import synthetic, weights as vw

    g = np.load(GOLDEN)
    frames = [synthetic.synthetic_frame(1080, 1920, int(s)) for s in g["frame_seeds"]]
    blob = vw.pack_state_dict(synthetic.make_autodrive_state_dict(int(g["weight_seed"])))

    def run():
        eng = emu_lib.Engine("autodrive", blob, precision="fp16x3")
        try:
            eng._ck(eng._lib.vp_use_graph(eng._h, 0))
            eng.infer_pair(frames[0], frames[1])
            t = {n: eng.tensor_read(i) for i, (n, c, h, w) in enumerate(eng.tensors()) if n.endswith(".conv1.attn") or n.endswith(".conv1.v")}
            return t, [k for k in _layer_kernels(eng) if k.startswith("attention")], eng.logits().reshape(3).copy()
        finally:
            eng.close()

    new, tags_new, out_new = run()
    vp_opts.setenv("VP_ATTN_BLOCK", "0")
    old, tags_old, out_old = run()
    assert tags_new == ["attention<q4>"] and tags_old == ["attention"]
    assert len(new) == 2 and set(new) == set(old)
    for n in new:
        scale = float(np.abs(old[n]).max())
        assert scale > 0 and float(np.abs(new[n] - old[n]).max()) <= 2e-6 * scale, n
    assert np.abs(out_new - out_old).max() <= 1e-5


def test_autodrive_fp8_storage_parity_mode_on_cpu(emu_lib):
    """BASELINE configs[4] with the fp8 weights as REAL storage (round 4): every conv / linear weight of the plan is one e4m3 byte + a row scale in
    HBM (conv_gemm / halo kernels and the FC kernel convert on the fly), activations in the parity mode -- against the reference module's outputs on
    the same fp8-dequantised weights, at the parity bar (the GPU test's contract, tests/test_gpu_autodrive.py)."""
    from autoware_vision_pilot_amd import synthetic, weights as vw

    g = np.load(GOLDEN)
    frames = [synthetic.synthetic_frame(1080, 1920, int(s)) for s in g["frame_seeds"]]
    eng = emu_lib.Engine("autodrive", vw.pack_state_dict(synthetic.make_autodrive_state_dict(int(g["weight_seed"]))), precision="fp16x3", weights_fp8=True)
    try:
        eng.infer_pair(frames[0], frames[1])
        got = eng.logits().reshape(3)
        assert np.abs(got - g["fp8_out"]).max() <= 1e-3, (got, g["fp8_out"])
        wb = eng.weight_bytes()
        # every matrix / FC weight of the plan is e4m3 bytes: 6.6 MB (exp0's Conv1d keeps only the centre tap of its three), no fp16 plane, no fp32 row
        assert wb["fp8"] > 6e6 and wb["fp16"] == 0 and wb["fp32"] == 0, wb
    finally:
        eng.close()


def test_autodrive_from_onnx_path_fp8_fp16_on_cpu(emu_lib, tmp_path):
    """vp_create on a `*.onnx` model_path (native reader, exporter-folded Conv+BN form), VP_WEIGHTS_FP8, the fp16 engine and
    the streaming vp_infer form -- BASELINE configs[4] as deployed -- against the reference-pinned fp8 golden outputs."""
    from pbwriter import onnx_model
    from test_gpu_onnx_folded import fold_like_exporter

    from autoware_vision_pilot_amd import synthetic

    g = np.load(GOLDEN)
    frames = [synthetic.synthetic_frame(1080, 1920, int(s)) for s in g["frame_seeds"]]
    path = tmp_path / "AutoDrive.onnx"
    path.write_bytes(onnx_model(fold_like_exporter(synthetic.make_autodrive_state_dict(int(g["weight_seed"])))))
    eng = emu_lib.Engine("autodrive", str(path), precision="fp16", weights_fp8=True)
    try:
        eng.infer(frames[0])            # streaming: the first frame pairs with itself
        eng.infer(frames[1])            # (frames[0], frames[1])
        got = eng.logits().reshape(3)
        # fp8 quantisation of FOLDED weights differs slightly from quantising conv and norm separately (the golden path):
        # the bar is the fp16 engine's (3e-2), not the 1e-3 of the parity mode
        assert np.abs(got - g["fp8_out"]).max() <= 3e-2, (got, g["fp8_out"])
    finally:
        eng.close()


def test_batched_encoder_taps_on_cpu(emu_lib):
    """Batched encoder (vp_create_batched, frames = 2): preprocess + EfficientNet backbone of two different camera frames in
    one pass -- stacked 1x1 GEMMs, the BATCH depthwise / squeeze-excite kernels, per-frame SE-gated projections -- against the
    oracle's backbone taps of each frame; then once more through graph replay with the frames swapped."""
    import torch

    from autoware_vision_pilot_amd import synthetic, weights as vw
    from oracle import nets, pre_post

    sd = synthetic.make_state_dict("sceneseg", 0)
    frames = [synthetic.synthetic_frame(360, 640, s) for s in (11, 12)]
    tsd = nets.to_torch(sd)
    want = []
    for f in frames:
        x = torch.from_numpy(pre_post.preprocess(f, input_is_bgr=True, planes_rgb=False))
        want.append([t[0].numpy() for t in nets.backbone(tsd, "Backbone.encoder.", x)])
    enc = emu_lib.Engine("sceneseg", vw.pack_state_dict(sd), precision="fp16x3", frames=2)
    try:
        assert enc.frames() == 2
        taps = ("Backbone.encoder.0", "Backbone.encoder.2.1.block.3", "Backbone.encoder.3.1.block.3", "Backbone.encoder.4.2.block.3", "Backbone.encoder.8")
        for order in ((0, 1), (1, 0)):                   # second pass: graph replay, frames swapped between the slots
            for slot, fi in enumerate(order):
                enc.upload_frame(frames[fi], index=slot)
            enc.enqueue()
            enc.sync()
            names = [n for n, *_ in enc.tensors()]
            for ti, name in enumerate(taps):
                t = enc.tensor_read(names.index(name))  # C x (2 * H) x W: the two frames stacked along H
                c, h2, w = t.shape
                for slot, fi in enumerate(order):
                    got, ref = t[:, slot * (h2 // 2):(slot + 1) * (h2 // 2)], want[fi][ti]
                    assert got.shape == ref.shape, name
                    err = float((np.abs(got - ref) / np.maximum(1.0, np.abs(ref))).max())
                    assert err <= 1e-3, f"{name} slot {slot} frame {fi}: {err:.2e}"
        with pytest.raises(emu_lib.VpError, match="no outputs"):
            enc._ck(enc._lib.vp_fetch_outputs(enc._h))
    finally:
        enc.close()


@pytest.mark.parametrize("kind,seed", [("egolanes", 2)])  # ("sceneseg", 0) passes too (2 min): run_network.py; its fp16 mode is below
def test_scene_network_end_to_end_on_cpu(emu_lib, kind, seed):
    """Whole scene networks through the production plan on the CPU (1 - 1.5 min each, emulated): preprocess, EfficientNet
    encoder, (EgoLanes: five-tap feature fusion), context, neck with the fused ConvTranspose + skip GEMMs, head, decode.
    SceneSeg is the headline network (367 GFLOP), EgoLanes the smallest (197 GFLOP).  Same bar as the GPU parity tests: input
    tensor bit-exact, logits within 1e-3, decoded mask identical outside the float tolerance band."""
    import torch

    from autoware_vision_pilot_amd import synthetic, weights as vw
    from oracle import nets, pre_post

    sd = synthetic.make_state_dict(kind, seed)
    frame = synthetic.synthetic_frame(720, 1280, 9)
    x = pre_post.preprocess(frame, input_is_bgr=True, planes_rgb=False)
    ref = nets.forward(kind, nets.to_torch(sd), torch.from_numpy(x))[0].numpy()
    eng = emu_lib.Engine(kind, vw.pack_state_dict(sd), precision="fp16x3")
    try:
        if kind == "egolanes":
            eng.set_decode_mode(emu_lib.VP_DECODE_LANE_LABEL)
            eng.set_lane_ring(True)                          # the AutoSteer hand-over (vp_set_lane_ring): checked below
        eng._ck(eng._lib.vp_use_graph(eng._h, 0))          # one eager pass is enough here
        eng.infer(frame)
        assert np.array_equal(eng.input_tensor(), x)
        got = eng.logits()
        want_mask = pre_post.egolanes_priority_mask(ref) if kind == "egolanes" else pre_post.seg_mask_u8(ref)
        differ = eng.mask() != want_mask
        if differ.any():  # only where two logits (or a logit and the threshold) are closer than the tolerance
            top2 = np.sort(ref, axis=0)[-2:]
            margin = np.abs(ref).min(axis=0) if kind == "egolanes" else top2[1] - top2[0]
            assert margin[differ].max() <= 1e-3 * np.abs(ref).max()
        if kind == "egolanes":
            # after ONE frame the ring is [zeros | logits] and reports one valid frame: the reference skips AutoSteer until two are in
            # (main.cpp:521); a second frame shifts: [logits(t-1) | logits(t)], bit for bit the engine's own logits
            ring, nvalid = eng.lane_ring()
            assert nvalid == 1 and not ring[:3].any() and np.array_equal(ring[3:], got)
            eng.infer(synthetic.synthetic_frame(360, 640, 10))
            ring, nvalid = eng.lane_ring()
            assert nvalid == 2 and np.array_equal(ring[:3], got) and np.array_equal(ring[3:], eng.logits()) and not np.array_equal(ring[3:], got)
    finally:
        eng.close()


def test_sceneseg_fp16_benchmark_mode_on_cpu(emu_lib):
    """The precision bench.py reports (VP_FP16: single fp16 plane, fp16 activation variants, register epilogues, the composed
    up-sampling stages on 64-channel chunks) through the whole SceneSeg network on the CPU; the GPU test's bar: max |error| within
    3e-2 of the largest logit, >= 99.5 % class agreement."""
    import torch

    from autoware_vision_pilot_amd import synthetic, weights as vw
    from oracle import nets, pre_post

    sd = synthetic.make_state_dict("sceneseg", 0)
    frame = synthetic.synthetic_frame(720, 1280, 9)
    ref = nets.forward("sceneseg", nets.to_torch(sd), torch.from_numpy(pre_post.preprocess(frame, input_is_bgr=True, planes_rgb=False)))[0].numpy()
    eng = emu_lib.Engine("sceneseg", vw.pack_state_dict(sd), precision="fp16")
    try:
        eng._ck(eng._lib.vp_use_graph(eng._h, 0))
        eng.infer(frame)
        got = eng.logits()
        assert float(np.abs(got - ref).max() / np.abs(ref).max()) <= 3e-2
        assert float((got.argmax(0) == ref.argmax(0)).mean()) >= 0.995
        kernels = {eng_k for eng_k in _layer_kernels(eng)}
        # the fp16-only paths ran (round 6: the composed up-sampling stages' fp16 form took the ConvTranspose launches' place)
        assert any(k.startswith("upconv_x1") for k in kernels) and any("regepi" in k for k in kernels) and any(k.startswith("head_conv3x3") for k in kernels)
        assert not any(k.startswith("convt_rs") or k.startswith("gemm_dma") for k in kernels)
    finally:
        eng.close()


def _layer_kernels(eng):
    out = []
    for i in range(eng._ck(eng._lib.vp_layer_count(eng._h))):
        tag = ct.c_char_p()
        eng._ck(eng._lib.vp_layer_kernel(eng._h, i, ct.byref(tag)))
        out.append(tag.value.decode())
    return out


def test_range_guard_is_loud_on_cpu(emu_lib):
    """The parity mode has fp32-class significand but fp16 EXPONENT range.  (1) A folded weight beyond 65504 fails engine construction
    with VP_ERR_RANGE (VpRangeError) instead of loading as inf.  (2) Weights scaled so that activations pass 65504: the probe on the
    outputs turns the silent inf / NaN into VP_ERR_RANGE from the synchronous call -- once; the same engine then serves a frame again
    (the error is per frame, not a poisoned engine) and raises again.  (3) With the probe switched off the garbage comes back silently:
    that is what the guard is for."""
    from autoware_vision_pilot_amd import synthetic, weights as vw

    sd = synthetic.make_autodrive_state_dict(5)
    frame = synthetic.synthetic_frame(270, 480, 3)
    big = dict(sd)
    k = next(k for k in sd if k.endswith("p2.0.conv.weight"))
    big[k] = sd[k] * np.float32(1e7)
    with pytest.raises(emu_lib.VpRangeError, match="fp16 range"):
        emu_lib.Engine("autodrive", vw.pack_state_dict(big), precision="fp16x3")
    hot = dict(sd)
    for key in sd:                       # every BatchNorm scale x 60: a few layers in, |x| > 65504
        if key.endswith(".norm.weight"):
            hot[key] = sd[key] * np.float32(60.0)
    eng = emu_lib.Engine("autodrive", vw.pack_state_dict(hot), precision="fp16x3")
    try:
        for _ in range(2):
            with pytest.raises(emu_lib.VpRangeError, match="non-finite"):
                eng.infer(frame)
        eng.set_finite_check(False)
        eng.infer(frame)
        assert not np.isfinite(eng.logits()).all()
    finally:
        eng.close()


def vw_blob(kind, seed):
    from autoware_vision_pilot_amd import synthetic, weights as vw

    return vw.pack_state_dict(synthetic.make_state_dict(kind, seed))


def test_kernel_plan_is_the_committed_one(emu_lib, monkeypatch):
    """WHICH kernel every layer of every network gets (vp_layer_kernel), both precisions, against tests/golden/kernel_plan.json: the
    dispatch rules of csrc/engine_dispatch.cpp (choose_conv: tile shapes, split-K, the pipelined / register-stationary / LDS-DMA kernels, fused decode) are host
    code and untested as rules otherwise -- a wrong predicate silently picks a slower kernel.  Deliberate rule changes regenerate the file
    with tools/dump_kernel_plan.py and show up as a reviewable diff."""
    import json

    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
    from dump_kernel_plan import kernel_plan

    want = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "kernel_plan.json")))
    # a HOSTILE environment: every knob the dispatch rules used to read from it (round 3) set to its most disruptive value -- the plan
    # below must still be the committed one, because the library no longer reads the environment (csrc/options.cpp)
    for k, v in {"VP_X3_TILE": "0", "VP_MAP3X3": "0", "VP_MBCONV_FUSE": "0", "VP_MBCONV_BACK": "0", "VP_CONV3X3": "v1", "VP_HEAD_CONV": "0", "VP_CONVT_RS": "0",
                 "VP_GEMM_DMA": "0", "VP_FUSE_SKIP": "0", "VP_FUSE_DECODE": "0", "VP_NSPLIT_FORCE": "1", "VP_PROJ_SPLIT": "0", "VP_CONVT_TILE": "2", "VP_X3_C64": "1"}.items():
        monkeypatch.setenv(k, v)
    got = kernel_plan(emu_lib)
    assert sorted(got) == sorted(want)
    for key in want:
        diff = [(a, b) for a, b in zip(got[key], want[key]) if list(a) != list(b)]
        assert len(got[key]) == len(want[key]) and not diff, f"{key}: {diff[:6]}"
    # the rules this round relies on, spelled out (SceneSeg, parity mode)
    seg = dict(tuple(r) for r in got["sceneseg/fp16x3"])
    # round 6: every up-sampling stage of the parity mode is ONE composed launch (ConvTranspose [+ skip link] + the 3x3 behind it, kernels_upconv.hip):
    # 8-row patches where the map's rows leave a 16-row patch mostly empty or the K loop is short, K slices on the two small maps
    assert seg["SceneNeck.upsample_layer_0+skip_link_layer_0+decode_layer_0"] == "upconv_x3w8<co128,px256>+splitk"
    assert seg["SceneNeck.upsample_layer_1+skip_link_layer_1+decode_layer_2"] == "upconv_x3w4<co128,px128>+splitk"
    assert seg["SceneNeck.upsample_layer_2+skip_link_layer_2+decode_layer_4"] == "upconv_x3w4<co128,px128>"
    assert seg["SceneSegHead.upsample_layer_3+skip_link_layer_3+decode_layer_6"] == "upconv_x3w8<co128,px256>"
    assert seg["SceneSegHead.upsample_layer_4+decode_layer_8"] == "upconv_x3w4<co128,px128>"
    assert seg["SceneNeck.decode_layer_5"] == "conv3x3_x3w8<co128,px256>" and seg["SceneSegHead.decode_layer_9"] == "conv3x3_x3w4<co64,px128>"
    assert seg["SceneSegHead.decode_layer_10"].startswith("head_conv3x3<c64,x3>+decode")
    # the fp16 engines take the same composed stages on 64-channel chunks (X1 form of the kernel); VP_UPCONV=0 / VP_UPCONV_F16=0 keep the three-op form
    seg16 = dict(tuple(r) for r in got["sceneseg/fp16"])
    assert seg16["SceneSegHead.upsample_layer_4+decode_layer_8"].startswith("upconv_x1w") and "SceneSegHead.upsample_layer_4" not in seg16
    assert seg16["SceneNeck.upsample_layer_2+skip_link_layer_2+decode_layer_4"].startswith("upconv_x1w")
    emu_lib.set_option("VP_UPCONV_F16", "0")
    try:
        e16 = emu_lib.Engine("sceneseg", vw_blob("sceneseg", 0), precision="fp16")
        k16 = dict(zip([n for n, _, _ in e16.layers()], e16.layer_kernels()))
        e16.close()
    finally:
        emu_lib.clear_options()
    assert k16["SceneSegHead.upsample_layer_4"] == "convt_rs<k128,x1>" and "SceneNeck.upsample_layer_2+skip_link_layer_2" in k16
    # the same knobs through vp_set_option DO change the plan -- and its hash, which bench.py records
    from autoware_vision_pilot_amd import synthetic, weights as vw

    blob = vw.pack_state_dict(synthetic.make_state_dict("egolanes", 2))
    eng = emu_lib.Engine("egolanes", blob, precision="fp16x3")
    h0, k0 = eng.plan_hash(), eng.layer_kernels()
    eng.close()
    emu_lib.set_option("VP_MAP3X3", "0")
    try:
        eng = emu_lib.Engine("egolanes", blob, precision="fp16x3")
        h1, k1 = eng.plan_hash(), eng.layer_kernels()
        eng.close()
    finally:
        emu_lib.clear_options()
    assert h0 != 0 and h0 != h1 and any("conv3x3_map" in k for k in k0) and not any("conv3x3_map" in k for k in k1)
    # round 5: the one option meant for hosts.  Default plan = CU-time rules (decode_layer_5 on the 8-wave pipelined shape, the neck on 64-channel slabs);
    # VP_PLAN_TARGET=latency = the round-4 choices for a host that runs one network on one camera, one frame at a time
    assert sum(1 for k in k0 if k.startswith("conv3x3_map2<")) == 2      # decode_layer_1 / 3 (round 6: decode_layer_0 / 2 live inside the composed stages)
    emu_lib.set_option("VP_PLAN_TARGET", "latency")
    try:
        eng = emu_lib.Engine("egolanes", blob, precision="fp16x3")
        h2, k2, names = eng.plan_hash(), eng.layer_kernels(), [n for n, _, _ in eng.layers()]
        eng.close()
    finally:
        emu_lib.clear_options()
    assert h2 not in (h0, h1) and not any(k.startswith("conv3x3_map2<") for k in k2) and sum(1 for k in k2 if k.startswith("conv3x3_map<co32,px800")) == 2
    d5 = [k for n, k in zip(names, k2) if n.endswith("decode_layer_5")]
    assert d5 == ["conv3x3_halo<co64,px128,x3>"] and [k for n, k in zip(names, k0) if n.endswith("decode_layer_5")] == ["conv3x3_x3w8<co128,px256>"]


# The launches whose (kernel tag, launch geometry) differ between a default-plan and a latency-plan engine: per precision, layer name suffix ->
# ((default tag, launch), (latency tag, launch)).  Every network has the three neck layers; decode_layer_6 at 80x160 is EgoLanes' head alone
# (the other heads' decode_layer_6 lives inside a composed up-sampling stage).  Written out, not derived: a rule change that moves another
# layer, or moves one of these elsewhere, fails test_latency_plan_is_the_committed_one and gets reviewed.
LATENCY_DIFFERENCE = {
    "fp16x3": {"decode_layer_1": (("conv3x3_map2<co64,px800,x3>+splitk", "nsplit=10 wgs=120"), ("conv3x3_map<co32,px800,x3>+splitk", "nsplit=10")),
               "decode_layer_3": (("conv3x3_map2<co64,px800,x3>+splitk", "nsplit=4 wgs=128"), ("conv3x3_map<co32,px800,x3>+splitk", "nsplit=3")),
               "decode_layer_5": (("conv3x3_x3w8<co128,px256>", ""), ("conv3x3_halo<co64,px128,x3>", "")),
               "decode_layer_6": (("conv3x3_x3w8<co128,px256>", ""), ("conv3x3_halo<co64,px128,x3>", ""))},
    "fp16": {"decode_layer_1": (("conv3x3_x1w4<co128,px128,k64>+splitk", "nsplit=4"), ("conv3x3_halo<co64,px128,x1>+splitk", "nsplit=4")),
             "decode_layer_3": (("conv3x3_x1w8<co128,px256,k64>", ""), ("conv3x3_halo<co64,px128,x1>+splitk", "nsplit=3")),
             "decode_layer_5": (("conv3x3_x1w8<co128,px256,k64>", ""), ("conv3x3_halo<co64,px128,x1,regepi>", "")),
             "decode_layer_6": (("conv3x3_x1w8<co128,px256,k64>", ""), ("conv3x3_halo<co64,px128,x1,regepi>", ""))},
}
LATENCY_DIFFERENCE_LAYERS = {"sceneseg": ("decode_layer_1", "decode_layer_3", "decode_layer_5"), "scene3d": ("decode_layer_1", "decode_layer_3", "decode_layer_5"),
                             "domainseg": ("decode_layer_1", "decode_layer_3", "decode_layer_5"),
                             "egolanes": ("decode_layer_1", "decode_layer_3", "decode_layer_5", "decode_layer_6")}


def test_latency_plan_is_the_committed_one(emu_lib):
    """The kernel plan of an engine created with VP_PLAN_LATENCY -- what adapters/hip_backend.hpp creates by default -- for the four scene networks
    in both precisions against tests/golden/kernel_plan_latency.json, entry by entry: name, kernel tag AND launch geometry (vp_layer_launch; the
    K split of this plan's map kernel is the engine's own rule, and tests/test_gpu_decoder_kernels.py takes it from that file).  Then what
    include/vp_hip.h says of the two plans: the creation flag and the developer option select the same plan; the plan hash tells the plans apart;
    and the difference between them is the written-out set above, nothing in the encoder, the context block or a composed up-sampling stage."""
    import json

    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
    from dump_kernel_plan import NETWORKS

    want = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "kernel_plan_latency.json")))
    assert sorted(want) == sorted(f"{kind}/{prec}" for kind, _ in NETWORKS for prec in ("fp16x3", "fp16"))

    def plan(kind, seed, prec, **kw):
        eng = emu_lib.Engine(kind, vw_blob(kind, seed), precision=prec, **kw)
        try:
            return [[n, k, l] for (n, _, _), k, l in zip(eng.layers(), eng.layer_kernels(), eng.layer_launches())], eng.plan_hash()
        finally:
            eng.close()

    for kind, seed in NETWORKS:
        for prec in ("fp16x3", "fp16"):
            key = f"{kind}/{prec}"
            rows_d, hash_d = plan(kind, seed, prec)
            rows_l, hash_l = plan(kind, seed, prec, plan_latency=True)
            diff = [(a, b) for a, b in zip(rows_l, want[key]) if list(a) != list(b)]
            assert len(rows_l) == len(want[key]) and not diff, f"{key}: {diff[:6]}"
            assert hash_l != hash_d and hash_l != 0, key
            if key in ("sceneseg/fp16x3", "egolanes/fp16"):        # the flag and the option: the same plan, launch for launch, and the same hash
                emu_lib.set_option("VP_PLAN_TARGET", "latency")
                try:
                    rows_o, hash_o = plan(kind, seed, prec)
                    rows_both, hash_both = plan(kind, seed, prec, plan_latency=True)
                finally:
                    emu_lib.clear_options()
                assert rows_o == rows_l and hash_o == hash_l, key
                assert rows_both == rows_l and hash_both == hash_l, key
            # the difference set, stated
            assert [r[0] for r in rows_d] == [r[0] for r in rows_l], key
            moved = {d[0]: ((d[1], d[2]), (l[1], l[2])) for d, l in zip(rows_d, rows_l) if d[1:] != l[1:]}
            stated = LATENCY_DIFFERENCE[prec]
            assert sorted(n.split(".")[-1] for n in moved) == sorted(LATENCY_DIFFERENCE_LAYERS[kind]), f"{key}: {moved}"
            for name, pair in moved.items():
                assert pair == stated[name.split(".")[-1]], f"{key} {name}: {pair}"
                assert "encoder" not in name and "context" not in name and "upsample" not in name, name
            first = min(i for i, (d, l) in enumerate(zip(rows_d, rows_l)) if d[1:] != l[1:])
            assert all("decode_layer" in r[0] or r[0] in ("finite_probe", "lane_ring") for r in rows_l[first:]), key   # all behind the context block


def test_plan_under_every_option_is_the_committed_one(emu_lib):
    """The plan hash (every launch's name, kernel tag and launch string) under every developer option the rules of csrc/engine_dispatch.cpp read, one
    setting at a time, against tests/golden/plan_options.json (tools/dump_plan_options.py: the settings, the engines and why SceneSeg takes them on top
    of VP_UPCONV=0) -- the branches tools/plan_search.py and the A/B profiles run through, which the default-option plan files cannot see.  A setting
    under which creation throws must throw the same message.  On a mismatch: the launches that differ from the engine's base plan under that setting."""
    import json

    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
    import dump_plan_options as dpo

    want = json.load(open(dpo.GOLDEN))
    engines = dpo.engines()
    assert sorted(want) == sorted(e[0] for e in engines)
    bad = []
    for key, kind, prec, kw, blob in engines:
        settings = dpo.settings_of(kind, prec)
        assert sorted(want[key]) == sorted(dpo.setting_key(o) for o in settings), key
        for o in settings:
            got = dpo.plan_under(emu_lib, kind, blob(kind), prec, kw, o)
            if got != want[key][dpo.setting_key(o)]:
                base = dpo.plan_under(emu_lib, kind, blob(kind), prec, kw, settings[0], rows=True)
                rows = dpo.plan_under(emu_lib, kind, blob(kind), prec, kw, o, rows=True)
                moved = [r for r in rows or [] if r not in base]
                bad.append((key, dpo.setting_key(o), got, want[key][dpo.setting_key(o)]))
                print(f"{key} {dpo.setting_key(o)}: {got} != {want[key][dpo.setting_key(o)]}; launches that differ from {dpo.setting_key(settings[0])}:")
                for r in moved:
                    print("   ", r)
    assert not bad, bad
