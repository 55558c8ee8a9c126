"""TEST INFRASTRUCTURE: build tests/emul/_build/device/libvp_harness_device.so -- the kernel entry points of harness_entries.hpp
compiled by hipcc for gfx950 (harness_device.cpp) and linked against the product's OWN kernel objects
(autoware_vision_pilot_amd/csrc/build/*.o, made by the product Makefile), so a device test runs the machine code libvp_hip.so
ships.  Linked with -Bsymbolic and meant to be dlopen-ed RTLD_LOCAL, like the emulated library: it exports the same symbols as
libvp_hip.so.  Cross-compiles on a machine without a GPU."""
import os
import subprocess

from build import CSRC, HERE, OUT, UNITS

HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
READELF = "/opt/rocm/lib/llvm/bin/llvm-readelf"
ARCH = "gfx950"
DEV_OUT = os.path.join(OUT, "device")
TIMEOUT = 1800     # seconds per subprocess: a cold product build of every kernel unit is the long one


def product_objects():
    """the product Makefile's objects of the units the emulated library is built from (build.UNITS)"""
    return [os.path.join(CSRC, "build", u.rsplit(".", 1)[0] + ".o") for u in UNITS]


def _run(cmd, what):
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=TIMEOUT)
    if r.returncode:
        raise RuntimeError("%s failed:\n%s" % (what, (r.stdout + r.stderr)[-4000:]))


def build(force=False):
    # the product's objects first (a no-op when they are current): what ships is what is linked here
    _run(["make", "-C", CSRC, "-j16"] + [os.path.relpath(o, CSRC) for o in product_objects()], "product kernel build (make -C csrc)")
    lib = os.path.join(DEV_OUT, "libvp_harness_device.so")
    srcs = [os.path.join(HERE, f) for f in ("harness_device.cpp", "harness_entries.hpp", "build.py", "build_device.py")]
    deps = srcs + product_objects()
    if not force and os.path.exists(lib) and all(os.path.getmtime(lib) >= os.path.getmtime(s) for s in deps):
        return lib
    os.makedirs(DEV_OUT, exist_ok=True)
    obj = os.path.join(DEV_OUT, "harness_device.o")
    _run([HIPCC, "-O3", "-std=c++17", "-fPIC", "--offload-arch=" + ARCH, "-Wall", "-Wno-unused-function", "-I", CSRC, "-x", "hip", "-c",
          os.path.join(HERE, "harness_device.cpp"), "-o", obj], "device harness compile")
    _run([HIPCC, "--offload-arch=" + ARCH, "-shared", "-fPIC", "-pthread", "-Wl,-Bsymbolic", "-o", lib, obj] + product_objects() + ["-ldl"],
         "device harness link")
    return lib


def exported_entry_points(lib):
    """names of the emu_* kernel entry points a shared library defines (dynamic symbol table); emu_switch, the emulation core's
    fiber switch (harness.cpp), is not one"""
    r = subprocess.run([READELF, "--dyn-syms", "-W", lib], capture_output=True, text=True, timeout=120)
    if r.returncode:
        raise RuntimeError("llvm-readelf failed on %s:\n%s" % (lib, r.stderr[-2000:]))
    names = set()
    for line in r.stdout.splitlines():
        f = line.split()
        # Num: Value Size Type Bind Vis Ndx Name
        if len(f) >= 8 and f[3] == "FUNC" and f[4] == "GLOBAL" and f[6] != "UND" and f[7].startswith("emu_") and f[7] != "emu_switch":
            names.add(f[7])
    return names


if __name__ == "__main__":
    print(build(force=True))
