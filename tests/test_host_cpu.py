"""CPU suite, part 2: the host logic and the C-ABI surface (no compute calls: there is no GPU here).

* libvp_hip.so loads and exports exactly the symbols include/vp_hip.h declares;
* the product fails LOUDLY without a GPU / with bad weights (no CPU fallback exists);
* weight-blob writer layout; Python operator API argument checks;
* multi-camera sharding + record gather under a world_size-2 gloo process group;
* the product package never imports the oracle.
"""
import os
import re
import struct
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_abi_exports_every_declared_symbol():
    """the header, the binding and the library's dynamic symbol table name the same entries: nothing else leaves the library"""
    import abi
    from autoware_vision_pilot_amd import lib

    declared = sorted(abi.declared_symbols())
    assert len(declared) >= 30
    assert sorted(lib.EXPORTED_SYMBOLS) == declared, set(declared) ^ set(lib.EXPORTED_SYMBOLS)
    so = lib.load()  # binds all of them; AttributeError if one is missing
    exported = abi.exported_symbols()   # every defined dynamic symbol, of any type
    expected = set(declared)
    if not exported & set(lib._COMM_SIGS):   # built with VP_NO_COMM=1: a library without the multi-camera exchange (vp_comm_*, vp_gather)
        expected -= set(lib._COMM_SIGS)
    assert exported == expected, exported ^ expected
    assert so.vp_version().startswith(b"libvp_hip")


@pytest.mark.skipif(torch.cuda.is_available(), reason="checks the no-GPU failure mode")
def test_no_cpu_fallback():
    from autoware_vision_pilot_amd import lib, weights as vw

    blob = vw.pack_state_dict({"a.weight": np.zeros((2, 3), np.float32)})
    with pytest.raises(lib.VpError, match="no HIP device|no CPU fallback"):
        lib.Engine("sceneseg", blob)


def test_bad_weights_are_rejected():
    from autoware_vision_pilot_amd import lib

    with pytest.raises(lib.VpError, match="magic|truncated"):
        lib.Engine("sceneseg", b"XXXX" + b"\0" * 64)
    with pytest.raises((lib.VpError, ValueError)):
        lib.Engine("sceneseg", "/nonexistent/file.vpw")
    with pytest.raises(ValueError):
        lib.Engine("sceneseg", "")


def test_weight_blob_layout_roundtrip():
    from autoware_vision_pilot_amd import weights as vw

    sd = {"x.weight": np.arange(24, dtype=np.float32).reshape(2, 3, 4), "x.num_batches_tracked": np.array(7),
          "y.bias": torch.ones(5)}
    blob = vw.pack_state_dict(sd)
    assert blob[:4] == b"VPW1" and struct.unpack("<I", blob[4:8])[0] == 2
    p, got = 8, {}
    for _ in range(2):
        (nl,) = struct.unpack("<H", blob[p:p + 2])
        name = blob[p + 2:p + 2 + nl].decode()
        p += 2 + nl
        nd = blob[p]
        dims = struct.unpack(f"<{nd}I", blob[p + 1:p + 1 + 4 * nd])
        p += 1 + 4 * nd
        n = int(np.prod(dims))
        got[name] = np.frombuffer(blob, dtype="<f4", count=n, offset=p).reshape(dims)
        p += 4 * n
    assert p == len(blob)
    assert np.array_equal(got["x.weight"], sd["x.weight"]) and np.array_equal(got["y.bias"], np.ones(5, np.float32))


def test_python_operator_api_argument_checks():
    from autoware_vision_pilot_amd import infer

    with pytest.raises(ValueError, match="checkpiont"):  # message copied from scene_seg_infer.py:33 (typo included)
        infer.SceneSegNetworkInfer("")
    x = infer.image_loader(np.full((320, 640, 3), 255, np.uint8))
    assert x.shape == (1, 3, 320, 640) and x.dtype == np.float32
    assert np.allclose(x[0, :, 0, 0], (1.0 - np.array([0.485, 0.456, 0.406])) / np.array([0.229, 0.224, 0.225]), atol=1e-6)
    with pytest.raises(ValueError):
        infer.image_loader(np.zeros((320, 640), np.uint8))


def test_product_never_imports_oracle():
    pkg = os.path.join(ROOT, "autoware_vision_pilot_amd")
    for dirpath, _, files in os.walk(pkg):
        for f in files:
            if f.endswith((".py", ".cpp", ".hpp", ".hip", ".h")):
                src = open(os.path.join(dirpath, f)).read()
                assert not re.search(r"^\s*(from|import)\s+oracle", src, flags=re.M), f
                assert "import_module(\"oracle" not in src and "dlopen(\"oracle" not in src, f


def test_camera_sharding_map():
    from autoware_vision_pilot_amd import multicam

    assert multicam.cameras_for_rank(8, 3, 8) == [3]
    assert multicam.cameras_for_rank(8, 1, 2) == [1, 3, 5, 7]
    assert sorted(sum((multicam.cameras_for_rank(5, r, 3) for r in range(3)), [])) == list(range(5))
    with pytest.raises(ValueError):
        multicam.cameras_for_rank(8, 8, 8)
    r = multicam.ResultRecord(3, 17, np.arange(6, dtype=np.uint8).reshape(2, 3))
    q = multicam.ResultRecord.unpack(r.pack())
    assert (q.camera, q.frame) == (3, 17) and np.array_equal(q.mask, r.mask)


_WORKER = r"""
import os, sys
sys.path.insert(0, {root!r})
import numpy as np, torch, torch.distributed as dist
from autoware_vision_pilot_amd import multicam
dist.init_process_group(backend="gloo", init_method="env://")
rank, world = dist.get_rank(), dist.get_world_size()
cams = multicam.cameras_for_rank(world, rank, world)
assert cams == [rank]
mask = np.full((80, 160), 10 * rank + 1, dtype=np.uint8); mask[rank, :] = 255
recs = multicam.gather_records(multicam.ResultRecord(cams[0], 42, mask), dist)
assert [r.camera for r in recs] == list(range(world)) and all(r.frame == 42 for r in recs)
for r in recs:
    assert (r.mask[r.camera] == 255).all() and r.mask[79, 0] == 10 * r.camera + 1
t = multicam.max_over_ranks(1.0 + rank, dist)
assert t == float(world)
dist.barrier(); dist.destroy_process_group()
print("rank", rank, "ok")
"""


def test_gather_world_size_2_gloo(tmp_path):
    script = tmp_path / "worker.py"
    script.write_text(_WORKER.format(root=ROOT))
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT="29617", WORLD_SIZE="2")
    procs = [subprocess.Popen([sys.executable, str(script)], env=dict(env, RANK=str(r), LOCAL_RANK=str(r)),
                              stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True) for r in range(2)]
    outs = [p.communicate(timeout=180)[0] for p in procs]
    for p, o in zip(procs, outs):
        assert p.returncode == 0, o
        assert "ok" in o


from pbwriter import _onnx_tensor, _pb_ld, _pb_varint  # noqa: E402  (tests/pbwriter.py)


def test_onnx_initializer_reader_roundtrip(tmp_path):
    """N2: the self-contained protobuf reader recovers named initializers (raw_data, packed float_data, fp16,
    non-float tensors skipped by the packer) from an ONNX ModelProto laid out like the exporter's."""
    from autoware_vision_pilot_amd import weights as vw

    rng = np.random.default_rng(0)
    tensors = {"SceneNeck.decode_layer_0.weight": rng.standard_normal((4, 3, 3, 3)).astype(np.float32),
               "SceneNeck.decode_layer_0.bias": rng.standard_normal((4,)).astype(np.float32),
               "half.weight": rng.standard_normal((2, 5)).astype(np.float16),
               "Backbone.encoder.0.1.num_batches_tracked": np.array([7], dtype=np.int64)}
    graph = b"".join(_pb_ld(5, _onnx_tensor(k, v, raw=(i % 2 == 0) or v.dtype != np.float32)) for i, (k, v) in enumerate(tensors.items()))
    graph = _pb_ld(2, b"main_graph") + graph                      # GraphProto.name = 2, .initializer = 5
    model = _pb_varint((1 << 3) | 0) + _pb_varint(8) + _pb_ld(2, b"pytorch") + _pb_ld(7, graph)  # ir_version, producer_name, graph
    path = tmp_path / "m.onnx"
    path.write_bytes(model)
    got = vw.load_onnx_initializers(str(path))
    assert set(got) == set(tensors)
    for k, v in tensors.items():
        assert got[k].shape == v.shape and np.array_equal(got[k], v)
    out = vw.export_onnx(str(path), str(tmp_path / "m.vpw"))
    blob = open(out, "rb").read()
    assert blob[:4] == b"VPW1" and int.from_bytes(blob[4:8], "little") == 3   # int64 counter dropped, fp16 widened
    # an exporter-folded weight can only be named from its node's module scope: a scope-less node is refused, loudly
    anon = _pb_ld(5, _onnx_tensor("onnx::Conv_123", tensors["SceneNeck.decode_layer_0.weight"]))
    node = _pb_ld(1, _pb_ld(1, b"x") + _pb_ld(1, b"onnx::Conv_123") + _pb_ld(2, b"y") + _pb_ld(3, b"Conv_0") + _pb_ld(4, b"Conv"))
    (tmp_path / "f.onnx").write_bytes(_pb_ld(7, node + anon))
    with pytest.raises(ValueError, match="cannot name"):
        vw.export_onnx(str(tmp_path / "f.onnx"), str(tmp_path / "f.vpw"))
    (tmp_path / "g.onnx").write_bytes(_pb_ld(7, anon))           # anonymous tensor no node consumes: nothing to load
    with pytest.raises(ValueError, match="no floating-point weights"):
        vw.export_onnx(str(tmp_path / "g.onnx"), str(tmp_path / "g.vpw"))


def test_onnx_reader_names_exporter_folded_convs():
    """N2: tests/golden/tiny_export.onnx was made by torch.onnx.export with the reference's exporter settings
    (tests/golden/make_tiny_onnx.py): Conv+BatchNorm pairs arrive folded under anonymous names.  The reader must name them
    from the node scopes (torchvision-style `encoder.1.0.block.0.0`, reference-style `stage.conv`), keep the named tensors
    verbatim, transpose the bias-free Linear back, and drop the second invocation of the trunk."""
    from autoware_vision_pilot_amd import weights as vw

    here = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
    ref = dict(np.load(os.path.join(here, "tiny_export.npz")))
    got = vw.load_onnx_state_dict(os.path.join(here, "tiny_export.onnx"))
    convs = {}
    for n in {k[:-len(".running_var")] for k in ref if k.endswith(".running_var")}:
        head, leaf = n.rsplit(".", 1)
        convs[head + (".conv" if leaf == "norm" else ".0")] = (n, 1e-3 if leaf == "norm" else 1e-5)
    assert len(convs) == 8
    want = {k for k in ref if not any(k.startswith(n + ".") for n, _ in convs.values())} | {c + ".bias" for c in convs}
    assert set(got) == want
    for c, (n, eps) in convs.items():
        s = ref[n + ".weight"] / np.sqrt(ref[n + ".running_var"] + np.float32(eps))
        w = ref[c + ".weight"] * s[:, None, None, None]
        b = ref[n + ".bias"] - ref[n + ".running_mean"] * s
        assert np.allclose(got[c + ".weight"], w, rtol=1e-5, atol=1e-7), c
        assert np.allclose(got[c + ".bias"], b, rtol=1e-5, atol=1e-7), c
    for k in ("plain.weight", "plain.bias", "up.weight", "up.bias", "fc.weight", "fc.bias", "proj.weight"):
        assert got[k].shape == ref[k].shape and np.array_equal(got[k], ref[k]), k
    assert vw._scope_prefix("/backbone/p5/p5.3/middle_block/conv2/conv2.0/conv/Conv") == "backbone.p5.3.middle_block.conv2.0.conv"


def test_native_onnx_reader_matches_python_reader(tmp_path):
    """csrc/onnx_reader.cpp (what vp_create runs on a `*.onnx` model_path) against weights.load_onnx_state_dict, tensor by
    tensor, on the exporter-made fixture; host only -- vp_convert_onnx needs no HIP device.  Also the hand-laid-out file of
    the reader round-trip test (fp16 raw_data, packed float_data, an int64 tensor to skip) and the two refusals."""
    from autoware_vision_pilot_amd import lib, weights as vw

    here = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
    out = lib.convert_onnx(os.path.join(here, "tiny_export.onnx"), str(tmp_path / "tiny.vpw"))
    got = vw.unpack_blob(open(out, "rb").read())
    want = vw.load_onnx_state_dict(os.path.join(here, "tiny_export.onnx"))
    assert set(got) == set(want)
    for k, v in want.items():
        assert got[k].shape == v.shape and np.array_equal(got[k], v.astype(np.float32)), k
    assert vw.unpack_blob(vw.pack_state_dict(want)).keys() == got.keys()

    rng = np.random.default_rng(1)
    tensors = {"a.weight": rng.standard_normal((4, 3, 3, 3)).astype(np.float32), "a.bias": rng.standard_normal((4,)).astype(np.float32),
               "half.weight": rng.standard_normal((2, 5)).astype(np.float16), "sub.weight": np.array([6e-8, -3e-6, 65504.0], dtype=np.float16),
               "n.num_batches_tracked": np.array([7], dtype=np.int64)}
    graph = b"".join(_pb_ld(5, _onnx_tensor(k, v, raw=(i % 2 == 0) or v.dtype != np.float32)) for i, (k, v) in enumerate(tensors.items()))
    (tmp_path / "m.onnx").write_bytes(_pb_ld(7, _pb_ld(2, b"main_graph") + graph))
    got = vw.unpack_blob(open(lib.convert_onnx(str(tmp_path / "m.onnx"), str(tmp_path / "m.vpw")), "rb").read())
    assert set(got) == {"a.weight", "a.bias", "half.weight", "sub.weight"}
    for k in got:
        assert np.array_equal(got[k], tensors[k].astype(np.float32)), k

    anon = _pb_ld(5, _onnx_tensor("onnx::Conv_123", tensors["a.weight"]))
    node = _pb_ld(1, _pb_ld(1, b"x") + _pb_ld(1, b"onnx::Conv_123") + _pb_ld(2, b"y") + _pb_ld(3, b"Conv_0") + _pb_ld(4, b"Conv"))
    (tmp_path / "f.onnx").write_bytes(_pb_ld(7, node + anon))
    with pytest.raises(lib.VpError, match="cannot name"):
        lib.convert_onnx(str(tmp_path / "f.onnx"), str(tmp_path / "f.vpw"))
    (tmp_path / "t.onnx").write_bytes(_pb_ld(7, graph)[:-9])      # truncated file
    with pytest.raises(lib.VpError):
        lib.convert_onnx(str(tmp_path / "t.onnx"), str(tmp_path / "t.vpw"))
    with pytest.raises(lib.VpError, match="cannot open"):
        lib.convert_onnx(str(tmp_path / "missing.onnx"), str(tmp_path / "x.vpw"))


def test_weights_cli_converts_pth_and_onnx(tmp_path):
    """`python -m autoware_vision_pilot_amd.weights src dst`: .pth state_dict (AutoDrive-style {"model": sd} wrapper too)
    and exporter-made .onnx both end in the same VPW1 container."""
    from autoware_vision_pilot_amd import weights as vw

    sd = {"a.weight": torch.randn(4, 3, 3, 3), "a.bias": torch.randn(4), "bn.num_batches_tracked": torch.tensor(3)}
    torch.save({"model": sd}, tmp_path / "m.pth")
    assert vw.main([str(tmp_path / "m.pth"), str(tmp_path / "m.vpw")]) == 0
    got = vw.unpack_blob((tmp_path / "m.vpw").read_bytes())
    assert set(got) == {"a.weight", "a.bias"} and np.array_equal(got["a.weight"], sd["a.weight"].numpy())
    here = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
    r = subprocess.run([sys.executable, "-m", "autoware_vision_pilot_amd.weights", os.path.join(here, "tiny_export.onnx"), str(tmp_path / "t.vpw")],
                       capture_output=True, text=True, cwd=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    assert r.returncode == 0, r.stderr
    assert set(vw.unpack_blob((tmp_path / "t.vpw").read_bytes())) == set(vw.load_onnx_state_dict(os.path.join(here, "tiny_export.onnx")))


def test_viridis_table_in_engine_matches_published_data():
    """csrc/viridis_lut.inc (compiled into the engine) against matplotlib's published viridis data, the
    source OpenCV's COLORMAP_VIRIDIS embeds; and the oracle's depth visualisation on a hand-checked ramp."""
    pytest.importorskip("matplotlib")
    from oracle import pre_post

    inc = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "autoware_vision_pilot_amd", "csrc", "viridis_lut.inc")
    vals = [int(v) for line in open(inc) if not line.startswith("//") for v in line.replace(",", " ").split()]
    table = np.array(vals, dtype=np.uint8).reshape(256, 3)
    assert np.array_equal(table, pre_post.viridis_lut_bgr())
    assert tuple(table[0]) == (84, 1, 68) and tuple(table[255]) == (37, 231, 253)
    ramp = np.linspace(-2.0, 3.0, 256, dtype=np.float32).reshape(16, 16)
    out = pre_post.visualize_depth(ramp)
    assert out.shape == (16, 16, 3) and np.array_equal(out.reshape(256, 3), table)      # 256 evenly spaced values -> every entry once
    assert np.array_equal(pre_post.visualize_depth(np.full((4, 5), 7.5, np.float32)), np.broadcast_to(table[0], (4, 5, 3)))


def test_weight_planes_reconstruct_to_2e_minus_21_of_the_row_maximum():
    """The (hi, lo) fp16 planes the engine makes of a weight matrix (vp_split_weight_rows = engine.cpp row_prescale + split_half, the host
    code every packing site uses) carry each fp32 weight to within 2^-21 of its ROW MAXIMUM -- for the decoder's real distributions
    (kaiming std at K = 11520 / 2304 / 288, where the UNSCALED lo plane is an fp16 subnormal: VERDICT round 3), trained-checkpoint-like
    tiny rows, rows mixing 2^-20 ... 1, and weights up to the fp16 range; and 2^-s * (hi + lo) reproduces the weight to fp32-class
    relative accuracy on the large-K rows.  The unscaled split (round 3) fails the same bound by 30x on the first case."""
    from autoware_vision_pilot_amd import lib

    rng = np.random.default_rng(0)
    cases = {
        "decode_layer_0 (K = 11520)": rng.standard_normal((8, 11520)).astype(np.float32) * np.float32(np.sqrt(2.0 / 11520)),
        "K = 2304": rng.standard_normal((8, 2304)).astype(np.float32) * np.float32(np.sqrt(2.0 / 2304)),
        "tiny rows (1e-5)": rng.standard_normal((8, 1152)).astype(np.float32) * np.float32(1e-5),
        "wide dynamic range": (rng.standard_normal((8, 512)) * np.exp2(rng.integers(-20, 1, (8, 512)))).astype(np.float32),
        "large (to 6e4)": rng.uniform(-6e4, 6e4, (4, 256)).astype(np.float32),
        "zero row + one value": np.concatenate([np.zeros((1, 64), np.float32), np.full((1, 64), 3e-7, np.float32)]),
    }
    for name, w in cases.items():
        hi, lo, post = lib.split_weight_rows(w)
        amax = np.abs(w).max(axis=1, keepdims=True)
        assert np.isfinite(hi.astype(np.float32)).all() and np.isfinite(lo.astype(np.float32)).all(), name
        s = np.log2(post.astype(np.float64))
        assert np.array_equal(s, np.round(s)), name                                   # powers of two: the epilogue's product is exact
        rec = (hi.astype(np.float64) + lo.astype(np.float64)) * post.astype(np.float64)[:, None]
        err = np.abs(rec - w.astype(np.float64))
        bound = np.maximum(amax.astype(np.float64), 1e-300) * 2.0 ** -21
        assert (err <= bound).all(), (name, float((err / bound).max()))
        nz = amax[:, 0] > 0
        scaled_max = amax[nz, 0].astype(np.float64) / post[nz].astype(np.float64)
        assert ((scaled_max >= 2.0 ** 13) & (scaled_max < 2.0 ** 14)).all(), name     # row maximum lands in [2^13, 2^14)
    # the measured claim: rms reconstruction error on N(0, 0.0132^2) weights, prescaled vs the round-3 split
    w = cases["decode_layer_0 (K = 11520)"]
    hi, lo, post = lib.split_weight_rows(w)
    rec = (hi.astype(np.float64) + lo.astype(np.float64)) * post.astype(np.float64)[:, None]
    h0 = w.astype(np.float16)
    l0 = (w - h0.astype(np.float32)).astype(np.float16)
    rms = lambda r: float(np.sqrt(np.mean((r - w.astype(np.float64)) ** 2)) / w.std())
    assert rms(rec) < 1e-7 and rms(h0.astype(np.float64) + l0.astype(np.float64)) > 5e-7
    with pytest.raises(lib.VpRangeError):
        lib.split_weight_rows(np.array([[1.0, 7e4]], np.float32))


def test_library_ignores_a_hostile_environment():
    """Up to round 3 ~25 VP_* environment variables changed which kernels an engine ran.  The library no longer reads the environment
    (no getenv in the product sources), the knobs are vp_set_option keys, an unknown key is refused, and vp_version() reports what is set."""
    from autoware_vision_pilot_amd import lib

    csrc = os.path.join(ROOT, "autoware_vision_pilot_amd", "csrc")
    for f in sorted(os.listdir(csrc)) + ["../lib.py", "../infer.py", "../multicam.py", "../weights.py", "../../adapters/hip_backend.hpp", "../../adapters/egolanes_hip_engine.hpp"]:
        p = os.path.join(csrc, f)
        if os.path.isfile(p) and f.endswith((".cpp", ".hip", ".hpp", ".py")):
            text = open(p).read()
            assert "getenv" not in text, f
            if f.endswith(".py") and f != "../lib.py":
                assert "environ" not in text, f
    assert lib.get_option("VP_MAP3X3") is None and "options: none" in lib.version()
    os.environ["VP_MAP3X3"] = "0"
    try:
        assert lib.get_option("VP_MAP3X3") is None                    # the environment is not an input
        lib.set_option("VP_MAP3X3", "0")
        assert lib.get_option("VP_MAP3X3") == "0" and "VP_MAP3X3=0" in lib.version()
        with pytest.raises(ValueError):
            lib.set_option("VP_NO_SUCH_KNOB", "1")
    finally:
        del os.environ["VP_MAP3X3"]
        lib.clear_options()
    assert lib.get_option("VP_MAP3X3") is None and "options: none" in lib.version()


def test_fp8_codes_reproduce_the_quantised_weights():
    """VP_WEIGHTS_FP8 storage, host side (vp_fp8_encode_rows = engine_internal.hpp e4m3_encode + fp8_row_scale): every one of the 254 finite OCP e4m3
    codes survives decode -> encode; rows that came out of the per-row quantiser (oracle/autodrive.py quantize_fp8_e4m3) and were re-scaled
    afterwards as BatchNorm folding does (incl. a sign flip) come back as code x scale to fp32 rounding, with no code off by one."""
    from autoware_vision_pilot_amd import lib
    from oracle import autodrive

    def decode(c):
        c = np.asarray(c, np.int64)
        e, m = (c >> 3) & 15, c & 7
        mag = np.where(e > 0, (1.0 + m / 8.0) * np.exp2(e.astype(np.float64) - 7.0), m * 2.0 ** -9)
        return np.where(c & 0x80, -mag, mag)

    finite = np.array([c for c in range(256) if (c & 0x7F) != 0x7F], np.uint8)
    vals = decode(finite).astype(np.float32)
    row = np.concatenate([vals, np.array([448.0], np.float32)])[None]          # the row maximum 448 pins the scale to 1
    codes, scale = lib.fp8_encode_rows(row)
    assert scale[0] == 1.0
    back = decode(codes[0][:-1])
    assert np.array_equal(back, vals.astype(np.float64))                      # (+0 and -0 both decode to 0)
    rng = np.random.default_rng(5)
    w = (rng.standard_normal((64, 1152)) * 0.03).astype(np.float32)
    w[3] *= np.float32(1e-4)
    wq = autodrive.quantize_fp8_e4m3({"x.weight": w})["x.weight"]
    fold = ((0.3 + rng.random(64)) * np.where(rng.random(64) < 0.3, -1.0, 1.0)).astype(np.float32)
    wf = (wq * fold[:, None]).astype(np.float32)
    codes, scale = lib.fp8_encode_rows(wf)
    rec = decode(codes) * scale.astype(np.float64)[:, None]
    assert np.abs(rec - wf).max() <= 4e-7 * np.abs(wf).max()
    assert (np.abs(decode(codes)).max(axis=1) == 448.0).all()                 # every row's maximum is the largest code, as the quantiser made it


def test_autosteer_angle_is_the_reference_postprocess():
    """vp_autosteer_angle (host arithmetic, no device): AutoSteerOnnxEngine::postProcess, autosteer_engine.cpp:160-185 -- strict '>' arg-max from class 0
    over the 61 logits of the head's second output (the FIRST maximum wins; a NaN never wins), angle = class - 30.  Against a line-by-line Python
    restatement on random logits, ties, a NaN, a maximum at either end; NULL / empty input gives the reference's failure value 0."""
    from autoware_vision_pilot_amd import lib

    def ref(v):
        best, best_v = 0, v[0]
        for i in range(1, len(v)):
            if v[i] > best_v:
                best, best_v = i, v[i]
        return float(best - 30)

    rng = np.random.default_rng(61)
    cases = [rng.standard_normal(61).astype(np.float32) for _ in range(20)]
    t = np.zeros(61, np.float32); t[[7, 40]] = 3.0; cases.append(t)                      # tie: class 7 wins
    t = rng.standard_normal(61).astype(np.float32); t[12] = np.nan; t[50] = 9.0; cases.append(t)
    t = np.full(61, -1.0, np.float32); t[60] = 0.0; cases.append(t)                       # +30 degrees
    t = np.full(61, -1.0, np.float32); t[0] = 0.0; cases.append(t)                        # -30 degrees
    cases.append(np.array([np.nan] + [0.0] * 60, np.float32))                             # NaN first: nothing is '>' NaN -> class 0
    for v in cases:
        assert lib.autosteer_angle(v) == ref(v)
    assert lib.load().vp_autosteer_angle(None, 61) == 0.0
    assert lib.autosteer_angle(np.array([5.0], np.float32)) == -30.0
