"""The device build of the kernel entry points (tests/emul/build_device.py: hipcc --offload-arch=gfx950, linked against the product's
kernel objects) builds without a GPU, and exports exactly the entry points of the emulated build, so the two cannot drift apart."""
import os
import sys

import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "emul"))


def test_device_harness_builds_and_matches_the_emulated_entry_points():
    import build as emul_build
    import build_device

    if not os.path.exists(emul_build.CLANG) or not os.path.exists(build_device.HIPCC):
        pytest.skip("ROCm toolchain not found")
    dev = build_device.build()
    emu = emul_build.build()
    got, want = build_device.exported_entry_points(dev), build_device.exported_entry_points(emu)
    assert len(want) >= 25, sorted(want)                      # the list really was read
    assert got == want, f"device only: {sorted(got - want)}, emulated only: {sorted(want - got)}"
