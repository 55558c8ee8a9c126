#!/usr/bin/env python3
"""Developer tool: (re)write tests/golden/plan_options.json -- the PLAN HASH (vp_plan_hash: every launch's name, kernel tag and launch string) an
engine gets under every developer option the dispatch rules of csrc/engine_dispatch.cpp read, and under the up-sampling switches that route layers
back into those rules, one option (or one stated combination) at a time, each at the values that flip a branch.  The four kernel_plan*.json files
pin the plans at default options; this file pins the option branches tools/plan_search.py and the A/B profiles in profiles/ run through.

  {"<network>/<precision>[+flags]": {"<OPTION>=<value>[,<OPTION>=<value>]": "<plan hash, hex>" | "error: <first line of the message>"}}

"default" is the engine without any option (SceneSeg: see THREE_OP below).  A setting under which engine creation throws is recorded with its message: it must throw the same one.
Taken from the CPU-emulated engine (tests/emul), like tools/dump_kernel_plan.py; VP_AUTOTUNE is left out (it times launches).
tests/test_engine_emulated.py::test_plan_under_every_option_is_the_committed_one compares.  Re-run after a DELIBERATE rule change and review the diff."""
import ctypes as ct
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests", "emul"))

GOLDEN = os.path.join(ROOT, "tests", "golden", "plan_options.json")

X3, F16 = ("fp16x3",), ("fp16",)      # a setting guarded by split() / !split() cannot move the other precision's plan
BOTH = X3 + F16
# SceneSeg takes every setting ON TOP OF VP_UPCONV=0, the three-op plan: there every decoder 3x3 and every ConvTranspose goes through the rules of
# engine_dispatch.cpp (the default plan composes five of the 3x3 layers and all ConvTranspose launches into stages those rules never see), and creation
# costs ~1 s of CPU against ~70 s with the composed stages (their fp64 weight products run on the emulated device).  The default plan at default options
# is what kernel_plan.json / kernel_plan_latency.json pin.  VP_UPCONV_F16=0 is the fp16 engines' own way back and is taken alone.
THREE_OP = {"VP_UPCONV": "0"}

# (options, precisions of the scene network it is taken in, also on the AutoDrive / AutoSpeed engines below)
SETTINGS = (
    ({}, BOTH, True),                      # SceneSeg: VP_UPCONV=0 alone; with fp16, SceneNeck.decode_layer_0 keeps the fp16 rule's four K slices on the map kernel
    ({"VP_X3_TILE": "0"}, X3, True), ({"VP_X3_TILE": "6"}, X3, True), ({"VP_X3_TILE": "7"}, X3, True),
    ({"VP_MAP3X3": "0"}, BOTH, True),
    ({"VP_CTX3": "0"}, BOTH, True),
    ({"VP_F16_BIG": "0"}, F16, False), ({"VP_F16_BIG": "6"}, F16, False), ({"VP_F16_BIG": "7"}, F16, False),
    ({"VP_F16_MAP": "0"}, F16, False), ({"VP_F16_MAP": "1"}, F16, False),
    ({"VP_F16_MIN_WGS": "100"}, F16, False),
    ({"VP_X3_MIN_WGS": "200"}, X3, True), ({"VP_X3_MIN_WGS": "36"}, X3, True),
    ({"VP_MAP2": "0"}, X3, True), ({"VP_MAP2": "1", "VP_PLAN_TARGET": "latency"}, X3, False),
    ({"VP_MAP2_MIN_REGIONS": "4"}, X3, False),
    ({"VP_MAP2_SLOTS": "64"}, X3, False),
    ({"VP_MAP2_CAP_MB": "14"}, X3, False),
    ({"VP_MAP_MAX_M": "800"}, BOTH, True),
    ({"VP_MAP_NSPLIT_PCT": "50"}, BOTH, True),
    ({"VP_NSPLIT_PCT": "50"}, BOTH, True),
    ({"VP_NSPLIT_FORCE": "2"}, BOTH, True),
    ({"VP_X3_C64": "0"}, X3, True), ({"VP_X3_C64": "1"}, X3, True),
    ({"VP_X3_T16": "1"}, X3, True),
    ({"VP_HEAD_CONV": "0"}, BOTH, True),
    ({"VP_HEAD_TILE5": "1"}, BOTH, True),
    ({"VP_CONV3X3": "v1"}, BOTH, True),
    ({"VP_CONVT_RS": "0"}, BOTH, True),
    ({"VP_CONVT_RS_GROUPS": "64"}, BOTH, False),
    ({"VP_CONVT_RS_GROUPS_K288": "64"}, BOTH, False),
    ({"VP_GEMM_DMA": "0"}, BOTH, False), ({"VP_GEMM_DMA": "1"}, BOTH, False),
    ({"VP_GEMM_DMA_NSPLIT": "2"}, BOTH, False),
    ({"VP_CONVT_TILE": "1"}, BOTH, False),
    ({"VP_CONVT_BK": "32"}, F16, False), ({"VP_CONVT_BK": "64"}, X3, False),
    ({"VP_FUSE_SKIP": "0"}, BOTH, False),
    ({"VP_FUSE_DECODE": "0"}, BOTH, True),
    ({"VP_PROJ_SPLIT": "0"}, BOTH, True),
    ({"VP_UPCONV_F16": "0"}, F16, False),
    ({"VP_PLAN_TARGET": "latency"}, BOTH, True),
    ({"VP_PLAN_OVERRIDE": "decode_layer_5=3"}, BOTH, False), ({"VP_PLAN_OVERRIDE": "decode_layer_5=7:2"}, BOTH, False),
)
# the fp8-storage branches (generic kernel's byte-weight tile, the halo clamp) and the VP_ACT_SCALE kernel gate of push_conv_op: parity-mode engines
OTHER_ENGINES = (("autodrive/fp16x3+fp8", "autodrive", {"weights_fp8": True}), ("autodrive/fp16x3+act_scale", "autodrive", {"act_scale": True}),
                 ("autospeed/fp16x3+act_scale", "autospeed", {"act_scale": True}))


def setting_key(opts):
    return ",".join(f"{k}={v}" for k, v in opts.items()) or "default"


def settings_of(kind, prec):
    """the option sets taken on that engine"""
    if kind != "sceneseg":
        return [o for o, _, others in SETTINGS if others]
    return [o if "VP_UPCONV_F16" in o else {**o, **THREE_OP} for o, precs, _ in SETTINGS if prec in precs]


def engines():
    """[(golden key, kind, precision, creation keywords, lambda: blob)]"""
    from autoware_vision_pilot_amd import synthetic, weights as vw

    make = {"sceneseg": lambda: synthetic.make_state_dict("sceneseg", 0), "autodrive": lambda: synthetic.make_autodrive_state_dict(0),
            "autospeed": lambda: synthetic.make_autospeed_state_dict(0)}
    cache = {}

    def blob(kind):
        if kind not in cache:
            cache[kind] = vw.pack_state_dict(make[kind]())
        return cache[kind]

    out = [(f"sceneseg/{p}", "sceneseg", p, {}, blob) for p in BOTH]
    return out + [(key, kind, "fp16x3", kw, blob) for key, kind, kw in OTHER_ENGINES]


def plan_under(lib, kind, blob, prec, kw, opts, rows=False):
    """plan hash (hex) of the engine created under `opts`, or "error: ..."; rows=True: its [name, tag, launch] list instead (None when creation throws)"""
    for k, v in opts.items():
        lib.set_option(k, v)
    try:
        eng = lib.Engine(kind, blob, precision=prec, **kw)
    except Exception as e:  # noqa: BLE001  (whatever vp_create reports is the record)
        return None if rows else "error: " + (str(e).splitlines() or [""])[0]
    finally:
        lib.clear_options()
    try:
        if rows:
            return [[n, k, l] for (n, _, _), k, l in zip(eng.layers(), eng.layer_kernels(), eng.layer_launches())]
        return "%016x" % eng.plan_hash()
    finally:
        eng.close()


def plan_options(lib):
    out = {}
    for key, kind, prec, kw, blob in engines():
        out[key] = {setting_key(o): plan_under(lib, kind, blob(kind), prec, kw, o) for o in settings_of(kind, prec)}
    return out


if __name__ == "__main__":
    import build as eb

    from autoware_vision_pilot_amd import lib

    so = ct.CDLL(eb.build(), mode=os.RTLD_LOCAL | os.RTLD_NOW)
    for name, (res, args) in lib._SIGS.items():
        fn = getattr(so, name)
        fn.restype, fn.argtypes = res, args
    lib._lib = so
    with open(GOLDEN, "w") as f:
        json.dump(plan_options(lib), f, indent=0, sort_keys=True)
        f.write("\n")
    print("written", GOLDEN)
