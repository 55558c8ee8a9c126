"""The device half of tests/test_kernels_emulated.py: every test of that module -- the same test body, the same assertions and bars --
run on the MI355X, with the `emu` fixture bound to the device backend (tests/emul/backends.py DeviceBackend: the entry points of
tests/emul/harness_entries.hpp compiled by hipcc for gfx950 and linked against the product's own kernel objects, every array staged
through a torch.cuda buffer).  The tests are taken from that module by name, so a test added there runs on both backends."""
import os
import sys

import pytest

import test_kernels_emulated as _bodies

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "emul"))

pytestmark = pytest.mark.gpu

globals().update({name: fn for name, fn in vars(_bodies).items() if name.startswith("test_") and callable(fn)})


@pytest.fixture(scope="module")
def emu():
    import backends

    return backends.load("device")
