#!/usr/bin/env python3
"""Developer tool: (re)write tests/golden/kernel_plan.json -- the kernel tag the engine's dispatch rules (csrc/engine_dispatch.cpp choose_conv, csrc/engine_upconv.cpp) give EVERY layer of every
network in both precisions (vp_layer_kernel), taken from the CPU-emulated engine (tests/emul; the rules are host code and see the
MI355X's 256 CUs there too).  tests/test_engine_emulated.py::test_kernel_plan_is_the_committed_one compares against it, so a predicate
regression that silently picks another kernel fails the CPU suite.  Also writes tests/golden/kernel_plan_latency.json: the same eight
engines created with VP_PLAN_LATENCY (the drop-in adapters' default), one entry per launch [name, kernel tag, launch] -- the launch string
(vp_layer_launch: "nsplit=4", "groups=32", "") is recorded there because the latency plan's map-kernel K split is the engine's own rule and
tests/test_gpu_decoder_kernels.py reproduces it (test_latency_plan_is_the_committed_one compares).  Re-run after a DELIBERATE change of a
rule and review the diff.

`dump_kernel_plan.py autospeed` writes tests/golden/kernel_plan_autospeed.json instead: the detector network (VP_AUTOSPEED) in both precisions, default
and latency plan, and AutoDrive's plan beside it -- [name, tag, launch] per launch; the two share their backbone launches (Engine::build_ad_backbone),
which tests/test_autospeed_net_emulated.py checks entry by entry.  `dump_kernel_plan.py autosteer` writes tests/golden/kernel_plan_autosteer.json:
the AutoSteer 2.0 lane-perception network (VP_AUTOSTEER) in the same four forms (tests/test_autosteer_net_emulated.py compares, and checks its
backbone launches against AutoDrive's).  Without an argument only the two scene-network files are written."""
import ctypes as ct
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests", "emul"))


NETWORKS = (("sceneseg", 0), ("scene3d", 1), ("domainseg", 3), ("egolanes", 2))


def kernel_plan(lib, latency=False):
    """default plans: [name, tag] per launch (the committed format); latency plans: [name, tag, launch]"""
    from autoware_vision_pilot_amd import synthetic, weights as vw

    out = {}
    for kind, seed in NETWORKS:
        blob = vw.pack_state_dict(synthetic.make_state_dict(kind, seed))
        for prec in ("fp16x3", "fp16"):
            eng = lib.Engine(kind, blob, precision=prec, plan_latency=latency)
            rows = zip(eng.layers(), eng.layer_kernels(), eng.layer_launches())
            out[f"{kind}/{prec}"] = [[n, k, l] if latency else [n, k] for (n, _, _), k, l in rows]
            eng.close()
    return out


def autospeed_plan(lib):
    """{"autospeed/<precision>[/latency]": [[name, tag, launch], ...], "autodrive/<precision>": [...]}"""
    from autoware_vision_pilot_amd import synthetic, weights as vw

    out = {}
    for kind, blob in (("autospeed", vw.pack_state_dict(synthetic.make_autospeed_state_dict(0))), ("autodrive", vw.pack_state_dict(synthetic.make_autodrive_state_dict(0)))):
        for prec in ("fp16x3", "fp16"):
            for latency in ((False, True) if kind == "autospeed" else (False,)):
                eng = lib.Engine(kind, blob, precision=prec, plan_latency=latency)
                rows = zip(eng.layers(), eng.layer_kernels(), eng.layer_launches())
                out[f"{kind}/{prec}" + ("/latency" if latency else "")] = [[n, k, l] for (n, _, _), k, l in rows]
                eng.close()
    return out


def autosteer_plan(lib):
    """{"autosteer/<precision>[/latency]": [[name, tag, launch], ...]}"""
    from autoware_vision_pilot_amd import synthetic, weights as vw

    out = {}
    blob = vw.pack_state_dict(synthetic.make_autosteer_state_dict(0))
    for prec in ("fp16x3", "fp16"):
        for latency in (False, True):
            eng = lib.Engine("autosteer", blob, precision=prec, plan_latency=latency)
            rows = zip(eng.layers(), eng.layer_kernels(), eng.layer_launches())
            out[f"autosteer/{prec}" + ("/latency" if latency else "")] = [[n, k, l] for (n, _, _), k, l in rows]
            eng.close()
    return out


if __name__ == "__main__":
    import build as eb

    from autoware_vision_pilot_amd import lib

    so = ct.CDLL(eb.build(), mode=os.RTLD_LOCAL | os.RTLD_NOW)
    for name, (res, args) in lib._SIGS.items():
        fn = getattr(so, name)
        fn.restype, fn.argtypes = res, args
    lib._lib = so
    if sys.argv[1:] == ["autospeed"]:
        path = os.path.join(ROOT, "tests", "golden", "kernel_plan_autospeed.json")
        with open(path, "w") as f:
            json.dump(autospeed_plan(lib), f, indent=0)
        print("written", path)
        sys.exit(0)
    if sys.argv[1:] == ["autosteer"]:
        path = os.path.join(ROOT, "tests", "golden", "kernel_plan_autosteer.json")
        with open(path, "w") as f:
            json.dump(autosteer_plan(lib), f, indent=0)
        print("written", path)
        sys.exit(0)
    for fname, latency in (("kernel_plan.json", False), ("kernel_plan_latency.json", True)):
        path = os.path.join(ROOT, "tests", "golden", fname)
        with open(path, "w") as f:
            json.dump(kernel_plan(lib, latency), f, indent=0)
        print("written", path)
