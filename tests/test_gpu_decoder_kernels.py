"""Device cases of the decoder kernels (the bodies of tests/decoder_checks.py through the product library's vp_op_conv2d / vp_op_upconv): every
decoder kernel tag of the eight production plans (tests/golden/kernel_plan.json: four networks x fp16x3 / fp16) at the 320x640 input, with the
channel counts of synthetic.model_spec and the tile / shape / K split of the plan forced; uniform rows and spread rows with a dead one at the
production shapes, the value edges (x 2^-12, x 2^8) on smaller maps of the same channel counts; three launches of every split-K path,
bit-identical; the register-stationary and LDS-DMA ConvTranspose kernels the current plans no longer pick, at small shapes.

The latency plans (tests/golden/kernel_plan_latency.json: the same eight engines created with VP_PLAN_LATENCY, the drop-in adapters' default)
send four decoder layers to other instantiations; LATENCY_CONVS holds one row per such launch, tile / K split / tag taken from that pin, and
runs through the same production, value-edge and split-K tests."""
import json
import os

import numpy as np
import pytest

from decoder_checks import check_conv, check_upconv

pytestmark = pytest.mark.gpu

PLAN = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "kernel_plan.json")))
LATENCY_PLAN = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "kernel_plan_latency.json")))   # [name, tag, launch] per launch
DECODER_KERNELS = ("conv_gemm", "conv3x3_", "upconv_", "head_conv3x3", "convt_rs", "gemm_dma")
PREC = {1: "x3", 0: "x1"}

# name, cin, cout, H, W, ks, act, res_mode, {precision: (tile, bk, nsplit, plan tag)}
CONVS = [
    ("encoder.8", 320, 1280, 10, 20, 1, 2, 0, {1: (2, 64, -1, "conv_gemm<bk64,co64,px64,x3>"), 0: (2, 64, -1, "conv_gemm<bk64,co64,px64,x1,regepi2>")}),
    ("context_layer_4", 128, 256, 10, 20, 3, 1, 0, {1: (111, -1, -1, "conv3x3_map<co32,px200,x3>+splitk"), 0: (111, -1, -1, "conv3x3_map<co32,px200,x1,k32>+splitk")}),
    ("context_layer_5", 256, 512, 10, 20, 3, 1, 0, {1: (111, -1, -1, "conv3x3_map<co32,px200,x3>+splitk"), 0: (111, -1, -1, "conv3x3_map<co32,px200,x1,k32>+splitk")}),
    ("context_layer_6", 512, 1280, 10, 20, 3, 1, 2, {1: (111, -1, -1, "conv3x3_map<co32,px200,x3>+splitk"), 0: (111, -1, -1, "conv3x3_map<co32,px200,x1,k32>+splitk")}),
    ("context_layer_6/egolanes", 512, 1456, 10, 20, 3, 1, 2, {1: (111, -1, -1, "conv3x3_map<co32,px200,x3>+splitk"), 0: (111, -1, -1, "conv3x3_map<co32,px200,x1,k32>+splitk")}),
    ("decode_layer_1", 768, 768, 20, 40, 3, 1, 0, {1: (112, -1, -1, "conv3x3_map2<co64,px800,x3>+splitk"), 0: (107, -1, 4, "conv3x3_x1w4<co128,px128,k64>+splitk")}),
    ("decode_layer_3", 512, 512, 40, 80, 3, 1, 0, {1: (112, -1, -1, "conv3x3_map2<co64,px800,x3>+splitk"), 0: (106, -1, 1, "conv3x3_x1w8<co128,px256,k64>")}),
    ("decode_layer_5", 512, 256, 80, 160, 3, 1, 0, {1: (106, -1, 1, "conv3x3_x3w8<co128,px256>"), 0: (106, -1, 1, "conv3x3_x1w8<co128,px256,k64>")}),
    ("decode_layer_6/egolanes", 256, 256, 80, 160, 3, 1, 0, {1: (106, -1, 1, "conv3x3_x3w8<co128,px256>"), 0: (106, -1, 1, "conv3x3_x1w8<co128,px256,k64>")}),
    ("decode_layer_7", 256, 128, 160, 320, 3, 1, 0, {1: (106, -1, 1, "conv3x3_x3w8<co128,px256>"), 0: (106, -1, 1, "conv3x3_x1w8<co128,px256,k64>")}),
    ("decode_layer_7/egolanes", 256, 128, 80, 160, 3, 1, 0, {1: (103, -1, 2, "conv3x3_halo<co64,px128,x3>+splitk"), 0: (103, -1, 2, "conv3x3_halo<co64,px128,x1>+splitk")}),
    ("decode_layer_9", 128, 64, 320, 640, 3, 1, 0, {1: (108, -1, 1, "conv3x3_x3w4<co64,px128>"), 0: (102, -1, 1, "conv3x3_halo<co64,px256,x1,regepi>")}),
    ("decode_layer_9/scene3d", 128, 128, 320, 640, 3, 1, 0, {1: (107, -1, 1, "conv3x3_x3w4<co128,px128>"), 0: (100, -1, 1, "conv3x3_halo<co128,px256,x1,regepi>")}),
]
# halo tile (vp_op_conv2d's `tile`) of the kernel tags the latency plans put in the default plans' place
TILE_OF_TAG = {"conv3x3_map<co32,px800,x3>": 111, "conv3x3_halo<co64,px128,x3>": 103, "conv3x3_halo<co64,px128,x1>": 103,
               "conv3x3_halo<co64,px128,x1,regepi>": 103}


def _pinned(plan, layer):
    """(tag, launch) the latency pin holds for the launch of `plan` ("sceneseg/fp16x3") whose name ends in `layer`"""
    hit = [(t, l) for n, t, l in LATENCY_PLAN[plan] if n == layer or n.endswith("." + layer) or n.endswith("+" + layer)]
    assert len(hit) == 1, (plan, layer, hit)
    return hit[0]


def _nsplit_of(launch):
    """K slices of a pinned launch string: "nsplit=10" -> 10, "" -> 1"""
    ns = [int(f[len("nsplit="):]) for f in launch.split() if f.startswith("nsplit=")]
    return ns[0] if ns else 1


def _latency_row(name, kind, cin, cout, H, W):
    """a CONVS row for decoder layer `name` of network `kind` under the latency plan: tile from the pinned tag, K split from the pinned launch"""
    cfg = {}
    for p, prec in ((1, "fp16x3"), (0, "fp16")):
        tag, launch = _pinned(f"{kind}/{prec}", name)
        cfg[p] = (TILE_OF_TAG[tag.replace("+splitk", "")], -1, _nsplit_of(launch), tag)
        assert ("+splitk" in tag) == (cfg[p][2] > 1 or cfg[p][0] == 111), (name, tag, launch)
    return (f"latency/{name}" + ("" if kind == "sceneseg" else "/" + kind), cin, cout, H, W, 3, 1, 0, cfg)


# the decoder launches whose (tag, launch) differ between the default and the latency engine (tests/test_engine_emulated.py::
# test_latency_plan_is_the_committed_one states that set), one row per distinct (channels, map, tag, launch), at the 320x640 input's shapes
LATENCY_CONVS = [_latency_row("decode_layer_1", "sceneseg", 768, 768, 20, 40), _latency_row("decode_layer_3", "sceneseg", 512, 512, 40, 80),
                 _latency_row("decode_layer_5", "sceneseg", 512, 256, 80, 160), _latency_row("decode_layer_6", "egolanes", 256, 256, 80, 160)]
ALL_CONVS = CONVS + LATENCY_CONVS
# the logits layers (mode 3, the engine's choice: head_conv3x3 for 64 / 128 input channels)
HEADS = [("decode_layer_10", 64, 3, 320, 640), ("decode_layer_10/domainseg", 64, 1, 320, 640), ("decode_layer_10/scene3d", 128, 1, 320, 640),
         ("decode_layer_8/egolanes", 128, 3, 80, 160)]
# name, cin, cm, cout, cs, H, W (low-resolution map), shape; the plan's K split is the engine's rule (nsplit 0), the compacted form its rule too
UPCONVS = [("neck_0", 1280, 1280, 768, 80, 10, 20, 6), ("neck_1", 768, 768, 512, 40, 20, 40, 7), ("neck_2", 512, 512, 512, 24, 40, 80, 7),
           ("head_3", 256, 256, 256, 32, 80, 160, 6), ("head_4", 128, 128, 128, 0, 160, 320, 7)]
UPCONV_SPLIT = {"neck_0", "neck_1"}      # "+splitk" in the plans


def _head_tag(cin, precision):
    return f"head_conv3x3<c{cin},{PREC[precision]}>"


def _upconv_tag(name, shape, precision):
    return (f"upconv_{PREC[precision]}" + ("w8<co128,px256" if shape == 6 else "w4<co128,px128") + (",k64>" if precision == 0 else ">") +
            ("+splitk" if name in UPCONV_SPLIT else ""))


def covered_tags():
    tags = {c[8][p][3] for c in CONVS for p in (0, 1)}
    tags |= {_head_tag(h[1], p) for h in HEADS for p in (0, 1)}
    tags |= {_upconv_tag(u[0], u[7], p) for u in UPCONVS for p in (0, 1)}
    return tags


def _layer_of(row_name):
    """CONVS / LATENCY_CONVS row name -> (layer name, the networks whose plans hold that shape)"""
    parts = [q for q in row_name.split("/") if q != "latency"]
    return parts[0], ([parts[1]] if len(parts) > 1 else ["sceneseg", "scene3d", "domainseg", "egolanes"])


def covered_launches():
    """(tag, launch string) pairs of the latency pin that a case here runs: a row that forces its K split covers that launch string; a row that
    leaves the K split to the engine's rule (nsplit <= 0) runs the operator entry's rule on the layer's own shape, which is the launch the pin
    holds for that layer where the pinned tag is the row's"""
    got = set()
    for row in ALL_CONVS:
        layer, kinds = _layer_of(row[0])
        for p, prec in ((1, "fp16x3"), (0, "fp16")):
            tile, bk, nsplit, tag = row[8][p]
            if nsplit > 0:
                got.add((tag, f"nsplit={nsplit}" if nsplit > 1 else ""))
                continue
            for kind in kinds:
                ptag, launch = _pinned(f"{kind}/{prec}", layer)
                if ptag == tag:
                    got.add((tag, launch))
    for name, cin, cm, cout, cs, H, W, shape in UPCONVS:      # nsplit 0: the engine's rule on the stage's own shape
        i = name.split("_")[1]
        for p, prec in ((1, "fp16x3"), (0, "fp16")):
            for kind in ("sceneseg", "scene3d", "domainseg", "egolanes"):
                for n, ptag, launch in LATENCY_PLAN[f"{kind}/{prec}"]:
                    if f"upsample_layer_{i}+" in n and ptag == _upconv_tag(name, shape, p):
                        got.add((ptag, launch))
    got |= {(_head_tag(h[1], p), "") for h in HEADS for p in (0, 1)}
    return got


_errs = {}


@pytest.fixture(scope="module", autouse=True)
def _error_table():
    yield
    if _errs:
        print("\nper kernel, the largest per-channel error (relative to the channel's largest magnitude) beyond the output's storage error / the bar:")
        for name, (err, bar) in sorted(_errs.items()):
            print(f"  {name:<48} {err:.3e} / {bar:.3e}")


def _table_key(name, tag):
    """the error table's line of a case: the kernel tag; a latency-plan row gets a line of its own per layer (its tag may be one the default plans use
    at another shape)"""
    return f"{tag} [{name}]" if name.startswith("latency/") else tag


def _note(tag, r):
    err, bar = _errs.get(tag, (0.0, 0.0))
    _errs[tag] = (max(err, r["err"]), max(bar, r["bar"]))
    return r


@pytest.fixture(scope="module")
def lib():
    from autoware_vision_pilot_amd import lib

    return lib


def test_plan_covers_the_decoder():
    """every decoder kernel tag of the eight production plans has a case here: a new kernel or a new instantiation cannot ship without one"""
    covered = covered_tags()
    missing = set()
    for plan, layers in PLAN.items():
        for name, tag in layers:
            base = tag.replace("+decode", "")
            if base.startswith(DECODER_KERNELS) and base not in covered:
                missing.add((plan, name, tag))
    assert not missing, sorted(missing)
    # the latency plans (the drop-in adapters' default): every decoder tag of the pin, and every distinct launch string of a tag
    covered_l = covered_launches()
    covered = covered | {c[8][p][3] for c in LATENCY_CONVS for p in (0, 1)}
    for plan, layers in LATENCY_PLAN.items():
        for name, tag, launch in layers:
            base = tag.replace("+decode", "")
            if base.startswith(DECODER_KERNELS) and (base not in covered or (base, launch) not in covered_l):
                missing.add((plan, name, tag, launch))
    assert not missing, sorted(missing)
    # ... and the rows of LATENCY_CONVS are exactly the decoder launches that differ from the default plan's tag
    differ = {(n.split(".")[-1], tl, ll) for plan in PLAN for (n, t), (_, tl, ll) in zip(PLAN[plan], LATENCY_PLAN[plan]) if t != tl}
    assert differ == {(_layer_of(r[0])[0], r[8][p][3], (f"nsplit={r[8][p][2]}" if r[8][p][2] > 1 else "")) for r in LATENCY_CONVS for p in (0, 1)}


@pytest.mark.parametrize("rows", ["uniform", "spread+dead"])
@pytest.mark.parametrize("precision", [1, 0], ids=["fp16x3", "fp16"])
@pytest.mark.parametrize("case", ALL_CONVS, ids=[c[0] for c in ALL_CONVS])
def test_conv_production(lib, case, precision, rows):
    name, cin, cout, H, W, ks, act, res_mode, plan = case
    tile, bk, nsplit, tag = plan[precision]
    _note(_table_key(name, tag), check_conv(lib, cin, cout, H, W, ks=ks, act=act, res_mode=res_mode, precision=precision, tile=tile, bk=bk, nsplit=nsplit, rows=rows,
                          seed=cin + cout + H))


@pytest.mark.parametrize("rows", ["uniform", "spread+dead"])
@pytest.mark.parametrize("precision", [1, 0], ids=["fp16x3", "fp16"])
@pytest.mark.parametrize("case", HEADS, ids=[h[0] for h in HEADS])
def test_head_production(lib, case, precision, rows):
    name, cin, cout, H, W = case
    _note(_head_tag(cin, precision), check_conv(lib, cin, cout, H, W, mode=3, precision=precision, rows=rows, seed=cin + cout))


@pytest.mark.parametrize("rows", ["uniform", "spread+dead", "spread_cm"])
@pytest.mark.parametrize("precision", ["fp16x3", "fp16"])
@pytest.mark.parametrize("case", UPCONVS, ids=[u[0] for u in UPCONVS])
def test_upconv_production(lib, case, precision, rows):
    name, cin, cm, cout, cs, H, W, shape = case
    p = 1 if precision == "fp16x3" else 0
    _note(_upconv_tag(name, shape, p), check_upconv(lib, cin, cm, cout, cs, H, W, shape=shape, nsplit=0, precision=precision, rows=rows, seed=cin + H))


@pytest.mark.parametrize("name", ["neck_0", "neck_1"])
def test_upconv_compacted_production(lib, vp_opts, name):
    """the compacted form forced on the neck's 10x20 and 20x40 stages (the engine's rule picks it there in the parity mode)"""
    _, cin, cm, cout, cs, H, W, shape = next(u for u in UPCONVS if u[0] == name)
    vp_opts.setenv("VP_UPCONV_COMPACT", "1")
    _note(_upconv_tag(name, shape, 1) + " compacted", check_upconv(lib, cin, cm, cout, cs, H, W, shape=shape, nsplit=0, rows="spread+dead", seed=cin))


# value edges: the production channel counts on smaller maps (the map kernels keep their region geometry)
EDGE_CONVS = [("encoder.8", 16, 32), ("context_layer_6", 10, 20), ("decode_layer_1", 20, 40), ("decode_layer_5", 32, 64),
              ("decode_layer_7/egolanes", 32, 64), ("decode_layer_9", 32, 64), ("decode_layer_9/scene3d", 32, 64)]
# the latency plan's rows: the 20x40-region map kernel keeps a 20x40 map (and its pinned K split)
EDGE_CONVS += [("latency/decode_layer_1", 20, 40), ("latency/decode_layer_3", 20, 40), ("latency/decode_layer_5", 32, 64),
               ("latency/decode_layer_6/egolanes", 32, 64)]
EDGE_UPCONVS = [("neck_0", 10, 20), ("neck_1", 20, 40), ("head_3", 16, 32), ("head_4", 16, 32)]


@pytest.mark.parametrize("scale", [2.0 ** -12, 2.0 ** 8])
@pytest.mark.parametrize("precision", [1, 0], ids=["fp16x3", "fp16"])
@pytest.mark.parametrize("name,H,W", EDGE_CONVS, ids=[e[0] for e in EDGE_CONVS])
def test_conv_value_edges(lib, name, H, W, precision, scale):
    _, cin, cout, _, _, ks, act, res_mode, plan = next(c for c in ALL_CONVS if c[0] == name)
    tile, bk, nsplit, tag = plan[precision]
    _note(_table_key(name, tag), check_conv(lib, cin, cout, H, W, ks=ks, act=act, res_mode=res_mode, precision=precision, tile=tile, bk=bk, nsplit=nsplit,
                          rows="spread+dead", scale=scale, seed=cout + H))


@pytest.mark.parametrize("scale", [2.0 ** -12, 2.0 ** 8])
@pytest.mark.parametrize("precision", [1, 0], ids=["fp16x3", "fp16"])
def test_head_value_edges(lib, precision, scale):
    for name, cin, cout, _, _ in HEADS[::2]:
        _note(_head_tag(cin, precision), check_conv(lib, cin, cout, 64, 128, mode=3, precision=precision, rows="spread+dead", scale=scale, seed=cin))


@pytest.mark.parametrize("scale", [2.0 ** -12, 2.0 ** 8])
@pytest.mark.parametrize("precision", ["fp16x3", "fp16"])
@pytest.mark.parametrize("name,H,W", EDGE_UPCONVS, ids=[e[0] for e in EDGE_UPCONVS])
def test_upconv_value_edges(lib, name, H, W, precision, scale):
    _, cin, cm, cout, cs, _, _, shape = next(u for u in UPCONVS if u[0] == name)
    p = 1 if precision == "fp16x3" else 0
    for rows in ("spread+dead", "spread_cm"):
        _note(_upconv_tag(name, shape, p), check_upconv(lib, cin, cm, cout, cs, H, W, shape=shape, nsplit=0 if name in UPCONV_SPLIT else 1,
                                                        precision=precision, rows=rows, scale=scale, seed=cin + H))


@pytest.mark.parametrize("precision", [1, 0], ids=["fp16x3", "fp16"])
def test_convt_kernels_off_plan(lib, vp_opts, precision):
    """the register-stationary ConvTranspose kernel (tile 5) and the LDS-DMA GEMM (tile 6, split-K, fused skip link): no current plan picks
    them, the operator entry still offers them"""
    kw = dict(mode=1, act=0, precision=precision, rows="spread+dead")
    _note(f"convt_rs<k128,{PREC[precision]}>", check_conv(lib, 128, 128, 32, 64, tile=5, nsplit=1, seed=51, **kw))
    vp_opts.setenv("VP_GEMM_DMA", "1")
    _note(f"gemm_dma<co256,px128,{PREC[precision]}>", check_conv(lib, 256, 256, 9, 15, tile=6, nsplit=1, seed=52, **kw))
    _note(f"gemm_dma<co256,px128,{PREC[precision]}>+splitk", check_conv(lib, 320, 512, 8, 16, tile=6, nsplit=3, seed=53, **kw))
    _note(f"gemm_dma<co256,px128,{PREC[precision]}> skip", check_conv(lib, 256, 256, 10, 16, mode=2, cs=24, precision=precision, rows="spread+dead",
                                                                      seed=54))


def _three_same(run):
    outs = [run()["out"] for _ in range(3)]
    for o in outs[1:]:
        assert np.array_equal(o.view(np.uint32), outs[0].view(np.uint32)), f"max |diff| {np.abs(o - outs[0]).max():.3e}"


@pytest.mark.parametrize("name", ["latency/decode_layer_1", "latency/decode_layer_3"])
@pytest.mark.parametrize("rows", ["uniform", "spread+dead"])
def test_latency_map_kernel_by_the_operator_rule(lib, vp_opts, name, rows):
    """the latency plan's 20x40-region map kernel with NOTHING forced: VP_PLAN_TARGET=latency, tile and K split left to the operator entry's own
    rules (which are the engine's).  Against fp64 at the same bar; and the split-K sum is deterministic, so the same K order on the same K
    slices gives the same bits as the run that forces what the pin names -- another K split (decode_layer_3: the default plan's four slices
    against this plan's three) or the halo kernel's tiles would not"""
    _, cin, cout, H, W, ks, act, res_mode, plan = next(c for c in LATENCY_CONVS if c[0] == name)
    tile, bk, nsplit, tag = plan[1]
    assert tile == 111 and tag == "conv3x3_map<co32,px800,x3>+splitk"
    kw = dict(ks=ks, act=act, res_mode=res_mode, precision=1, rows=rows, seed=cin + cout + H)
    forced = check_conv(lib, cin, cout, H, W, tile=tile, nsplit=nsplit, **kw)
    vp_opts.setenv("VP_PLAN_TARGET", "latency")
    rule_split = _note(_table_key(name, tag), check_conv(lib, cin, cout, H, W, tile=tile, nsplit=-1, **kw))
    rule_all = _note(_table_key(name, tag), check_conv(lib, cin, cout, H, W, tile=-1, nsplit=-1, **kw))
    for r in (rule_split, rule_all):
        assert np.array_equal(r["out"].view(np.uint32), forced["out"].view(np.uint32)), f"max |diff| {np.abs(r['out'] - forced['out']).max():.3e}"


@pytest.mark.parametrize("path", ["map", "map2", "x3_split", "halo_split", "upconv_split", "latency_map_px800", "latency_map_px800_4regions",
                                  "latency_halo_split_fp16_ns4", "latency_halo_split_fp16_ns3"])
def test_split_k_is_deterministic(lib, path):
    """three launches of each split-K path on the same operands: bit-identical outputs (the fp32 slabs are summed by the finish kernels in a
    fixed order)"""
    if path == "map":
        _three_same(lambda: check_conv(lib, 512, 1280, 10, 20, res_mode=2, precision=1, tile=111, nsplit=3, seed=61))
    elif path == "map2":
        _three_same(lambda: check_conv(lib, 768, 768, 20, 40, precision=1, tile=112, nsplit=3, seed=62))
    elif path == "x3_split":
        _three_same(lambda: check_conv(lib, 768, 768, 20, 40, precision=0, tile=107, nsplit=4, seed=63))
    elif path == "halo_split":
        _three_same(lambda: check_conv(lib, 256, 128, 80, 160, precision=1, tile=103, nsplit=2, seed=64))
    elif path == "upconv_split":
        _three_same(lambda: check_upconv(lib, 1280, 1280, 768, 80, 10, 20, shape=6, nsplit=3, seed=65))
    else:           # the latency plan's split-K launches, tile and K slices as pinned
        name, precision = {"latency_map_px800": ("latency/decode_layer_1", 1), "latency_map_px800_4regions": ("latency/decode_layer_3", 1),
                           "latency_halo_split_fp16_ns4": ("latency/decode_layer_1", 0), "latency_halo_split_fp16_ns3": ("latency/decode_layer_3", 0)}[path]
        _, cin, cout, H, W, ks, act, res_mode, plan = next(c for c in LATENCY_CONVS if c[0] == name)
        tile, bk, nsplit, tag = plan[precision]
        assert nsplit > 1 and "+splitk" in tag
        _three_same(lambda: check_conv(lib, cin, cout, H, W, precision=precision, tile=tile, nsplit=nsplit, seed=66 + precision))
