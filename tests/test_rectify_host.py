"""vp_frame rectification without a GPU: the host map builder against the numpy restatement (tests/rectify_cases.py), the invariants of the definition,
the refusals, the ABI -- and, on the HIP-on-CPU emulation of the real kernel and frame code (tests/emul), the kernel through vp_op_remap_bgr8 and the
frame path.  Every comparison is bit for bit; the homography helper alone is compared at 1e-12 (it calls trigonometric functions)."""
import ctypes as ct
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "emul"))
import abi  # noqa: E402
import rectify_cases as rc  # noqa: E402

NEW_SYMBOLS = ("vp_frame_set_rectify", "vp_frame_get_rectify", "vp_rectify_map", "vp_rectify_homography", "vp_op_remap_bgr8")


@pytest.fixture(scope="module")
def lib():
    from autoware_vision_pilot_amd import lib as _lib

    return _lib


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


@pytest.fixture(scope="module")
def emu_autodrive(emu_lib):
    """two AutoDrive fp16 engines on the same weights (the kind tests/test_frame_host.py feeds from a frame)"""
    from autoware_vision_pilot_amd import synthetic, weights as vw

    blob = vw.pack_state_dict(synthetic.make_autodrive_state_dict(0))
    engs = [emu_lib.Engine("autodrive", blob, precision="fp16") for _ in range(2)]
    yield engs
    for e in engs:
        e.close()


# ---- 1. host only: the ABI, the maps, the invariants, the refusals
def test_new_symbols_are_declared_exported_and_bound(lib):
    src = abi.header_source()
    declared, exported = abi.declared_symbols(), abi.exported_symbols()
    for s in NEW_SYMBOLS:
        assert s in declared, s
        assert s in exported, s
        assert s in lib.EXPORTED_SYMBOLS, s
    for name, v in (("VP_RECTIFY_TWO_PASS", lib.VP_RECTIFY_TWO_PASS), ("VP_RECTIFY_ONE_PASS", lib.VP_RECTIFY_ONE_PASS), ("VP_BORDER_CONSTANT", lib.VP_BORDER_CONSTANT),
                    ("VP_BORDER_REPLICATE", lib.VP_BORDER_REPLICATE)):
        assert f"{name} = {v}" in src
    assert ct.sizeof(lib.Rectify) == 23 * 8 + 3 * 4 + 4 and ct.sizeof(lib.CameraPose) == 4 * 8 + 9 * 8 + 2 * 4 + 8     # the C layouts: doubles first, no hidden padding but the tail's


def test_cases_show_their_properties_on_the_restatement_alone():
    h, w = rc.SRC_HW
    t = rc.tap_state(*rc.undistort_map(rc.K, rc.PINCUSHION, h, w), h, w)
    assert (t == 0).mean() > 0.10 and ((t > 0) & (t < 4)).mean() > 0.02          # CONSTANT is live: pixels all outside, pixels straddling the border
    assert (rc.tap_state(*rc.undistort_map(rc.K, rc.BARREL, h, w), h, w) == 4).all()
    t = rc.tap_state(*rc.warp_map(rc.H_WARP, *rc.OUT_HW), h, w)
    assert 0.35 < (t < 4).mean() < 0.60 and ((t > 0) & (t < 4)).any()               # REPLICATE is live on about half the destination
    src = rc.random_picture(h, w, 3)
    for X, Y, _ in (rc.named_map("undistort", rc.PINCUSHION), rc.named_map("warp", rc.BARREL)):
        assert not np.array_equal(rc.remap(src, X, Y, rc.CONSTANT), rc.remap(src, X, Y, rc.REPLICATE))


@pytest.mark.parametrize("which,dist_name", rc.MAP_CASES, ids=["-".join(c) for c in rc.MAP_CASES])
def test_map_equals_restatement_bit_for_bit(lib, which, dist_name):
    X, Y, _ = rc.named_map(which, rc.DISTS[dist_name])
    xy, frac = lib.rectify_map(rc.K, rc.DISTS[dist_name], rc.H_WARP, rc.OUT_HW, rc.SRC_HW, which)
    want_xy, want_frac = rc.to_exchange(X, Y)
    assert xy.shape == want_xy.shape and np.array_equal(xy, want_xy), np.argwhere(xy != want_xy)[:4]
    assert np.array_equal(frac, want_frac), np.argwhere(frac != want_frac)[:4]


def test_map_saturates_as_the_restatement_does(lib):
    """a homography whose W crosses 0 inside the destination and a distortion that throws the corners far out: both clamps, W == 0 handled"""
    H = np.array([[1.0 / 4096, 0.0, 0.0], [0.0, 1.0, 0.0], [1.0 / 65536, 0.0, 1.0]])      # its inverse: X0 = 4096 x, W = 1 - x / 16, exactly 0 at x = 16
    dist = (900.0, 0.0, 0.0, 0.0, 4.0e5)
    for which, (X, Y) in ((0, rc.undistort_map(rc.K, dist, *rc.SRC_HW)), (1, rc.warp_map(H, *rc.OUT_HW)), (2, rc.one_pass_map(rc.K, dist, H, *rc.OUT_HW, *rc.SRC_HW))):
        xy, frac = lib.rectify_map(rc.K, dist, H, rc.OUT_HW, rc.SRC_HW, which)
        want_xy, want_frac = rc.to_exchange(X, Y)
        assert np.array_equal(xy, want_xy) and np.array_equal(frac, want_frac), which
        if which < 2:
            assert X.min() == rc.LO and X.max() == rc.HI, which


def test_invariants_of_the_definition(lib):
    h, w = rc.SRC_HW
    jj, ii = np.meshgrid(np.arange(w), np.arange(h))
    xy, frac = lib.rectify_map(rc.K, rc.ZERO, rc.H_WARP, rc.OUT_HW, rc.SRC_HW, "undistort")
    assert np.array_equal(xy[..., 0], jj) and np.array_equal(xy[..., 1], ii) and not frac.any()          # dist = 0: the identity
    src = rc.random_picture(h, w, 3)
    one = rc.from_exchange(*lib.rectify_map(rc.K, rc.ZERO, rc.H_WARP, rc.OUT_HW, rc.SRC_HW, "one_pass"))
    warp = rc.from_exchange(*lib.rectify_map(rc.K, rc.ZERO, rc.H_WARP, rc.OUT_HW, rc.SRC_HW, "warp"))
    assert np.array_equal(rc.remap(src, *one, rc.CONSTANT), rc.remap(src, *warp, rc.REPLICATE))             # one-pass with dist = 0: the warp-only picture
    for dist in rc.DISTS.values():                                                                       # one-pass with H = I at the raw size: the undistort map
        a = lib.rectify_map(rc.K, dist, np.eye(3), rc.SRC_HW, rc.SRC_HW, "one_pass")
        b = lib.rectify_map(rc.K, dist, np.eye(3), rc.SRC_HW, rc.SRC_HW, "undistort")
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    X = np.arange(-64, 64, dtype=np.int64)[None, :] * 32                                                  # frac = 0 samples the pixel itself: a skipped pass is exact
    Y = np.full_like(X, 32 * 4)
    assert np.array_equal(rc.remap(src, X, Y, rc.REPLICATE)[0, 64:], src[4, :64])


def test_refusals(lib):
    good = dict(K=rc.K, dist=rc.PINCUSHION, H=rc.H_WARP, out_hw=rc.OUT_HW, src_hw=rc.SRC_HW, which=0)

    def refused(**kw):
        with pytest.raises(ValueError):
            lib.rectify_map(**{**good, **kw})

    lib.rectify_map(**good)
    for bad in (np.nan, np.inf):
        for key, shape in (("K", (3, 3)), ("dist", (5,)), ("H", (3, 3))):
            a = np.array(good[key], np.float64).reshape(shape).copy()
            a.flat[0] = bad
            refused(**{key: a})
    refused(K=rc.k_matrix(0.0, 118.7, 80.2, 44.9))
    refused(K=rc.k_matrix(120.3, 0.0, 80.2, 44.9))
    for idx in ((0, 1), (1, 0), (2, 0), (2, 1)):
        a = rc.K.copy()
        a[idx] = 1e-3
        refused(K=a)
    a = rc.K.copy()
    a[2, 2] = 2.0
    refused(K=a)
    refused(H=np.array([[1.0, 2.0, 3.0], [2.0, 4.0, 6.0], [0.0, 0.0, 1.0]]))          # det H = 0
    for out_hw in ((1, 128), (64, 1), (64, 16385), (16385, 128)):
        refused(out_hw=out_hw)
    refused(mode=2)
    refused(which=3)
    refused(src_hw=(1, 161))
    refused(src_hw=(90, 16385))


def test_homography_equals_the_restated_protocol(lib):
    """|H - H_ref| <= 1e-12 max|H_ref|, every entry: entries that cancel towards 0 carry the rounding of the operands they are formed from"""
    standard = {"pitch": 0.0, "yaw": 0.0, "roll": 0.0, "camera_height": 1.45, "img_width": 1024, "img_height": 512, "hfov": 50.4}
    for inference in ({"pitch": 2.3, "yaw": -1.1, "roll": 0.7, "camera_height": 2.1, "intrinsic_matrix": [[2055.6, 0, 939.7], [0, 2055.6, 641.1], [0, 0, 1]]},
                      {"pitch": 0.0, "yaw": 0.0, "roll": 0.0, "camera_height": 1.45, "intrinsic_matrix": rc.K},
                      {"pitch": -4.0, "yaw": 12.5, "roll": -3.0, "camera_height": 1.2, "intrinsic_matrix": rc.FRAME_K}):
        for std in (standard, {**standard, "pitch": 1.5, "yaw": 0.4, "roll": -0.2}):
            want = rc.homography(inference, std)
            got = lib.rectify_homography(inference, std)
            assert np.abs(got - want).max() <= 1e-12 * np.abs(want).max()
            lib.rectify_map(inference["intrinsic_matrix"], rc.ZERO, got, (512, 1024), (1280, 1920), "warp")     # and it is a setting the library takes
    for bad in ({"camera_height": 0.0}, {"pitch": np.nan}, {"intrinsic_matrix": rc.k_matrix(0.0, 1.0, 0.0, 0.0)}):
        with pytest.raises(ValueError):
            lib.rectify_homography({"pitch": 0.0, "yaw": 0.0, "roll": 0.0, "camera_height": 1.0, "intrinsic_matrix": rc.K, **bad}, standard)
    for bad in ({"hfov": 0.0}, {"hfov": 180.0}, {"img_width": 0}):
        with pytest.raises(ValueError):
            lib.rectify_homography({"pitch": 0.0, "yaw": 0.0, "roll": 0.0, "camera_height": 1.0, "intrinsic_matrix": rc.K}, {**standard, **bad})


def test_one_pass_differs_from_two_passes_by_the_definition(capsys):
    """The difference is a property of the definition, not of the device.  On rectify_cases.smooth_picture (at most 15 levels per pixel along x, 11 along y)
    under the barrel case and the test homography: d = |two_pass - one_pass| per byte over the INTERIOR -- the destination pixels whose four taps lie
    inside the source in the warp map and in the one-pass map (the barrel undistort map has every tap inside), so no border rule takes part.
    Bound, from the definition: two roundings to a byte against one (0.5 + 0.5 + 0.5 levels), the coordinates of three maps rounded to 1/32 pixel
    (1/64 pixel each way: (15 + 11) / 64 levels per map, the warp's magnified by the undistort pass's slope, below 1.3: 1.6 levels in all), and two
    bilinear interpolations of a picture whose second derivative is at most 100 * 0.15^2 = 2.25 levels per pixel^2 against one (3 * 2.25 / 8 < 0.9):
    below 5 levels.  Measured on the restatement: max 2 levels, mean 0.21 levels, on the 50 % of the destination that is interior."""
    h, w = rc.SRC_HW
    pic = rc.smooth_picture(h, w)
    gx = np.abs(np.diff(pic.astype(np.int64), axis=1)).max()
    assert 13 <= gx <= 16
    two = rc.rectify(pic, rc.K, rc.BARREL, rc.H_WARP, rc.OUT_HW).astype(np.int64)
    one = rc.rectify(pic, rc.K, rc.BARREL, rc.H_WARP, rc.OUT_HW, "one_pass").astype(np.int64)
    interior = (rc.tap_state(*rc.warp_map(rc.H_WARP, *rc.OUT_HW), h, w) == 4) & (rc.tap_state(*rc.one_pass_map(rc.K, rc.BARREL, rc.H_WARP, *rc.OUT_HW, h, w), h, w) == 4)
    d = np.abs(two - one)[interior]
    with capsys.disabled():
        print(f"\none-pass vs two-pass on the smooth picture: interior {interior.mean():.3f} of the destination, max |d| = {d.max()} levels, mean |d| = {d.mean():.4f}")
    assert interior.mean() > 0.25
    assert 1 <= d.max() <= 5


# ---- 2. the kernel through vp_op_remap_bgr8, emulated
@pytest.mark.parametrize("which,dist_name", rc.MAP_CASES, ids=["-".join(c) for c in rc.MAP_CASES])
def test_kernel_case_emulated(emu_lib, which, dist_name):
    rc.check_kernel_case(emu_lib, which, dist_name)


def test_kernel_table_emulated(emu_lib):
    rc.check_kernel_table(emu_lib)


def test_kernel_edges_emulated(emu_lib):
    rc.check_kernel_edges(emu_lib)


def test_kernel_widths_and_padding_emulated(emu_lib):
    rc.check_kernel_widths_and_padding(emu_lib)


def test_kernel_wide_emulated(emu_lib):
    rc.check_kernel_wide(emu_lib)


def test_op_refusals_emulated(emu_lib):
    rc.check_op_refusals(emu_lib)


# ---- 3. the frame path, emulated
@pytest.mark.parametrize("mode", ["two_pass", "one_pass"])
@pytest.mark.parametrize("fmt", rc.FRAME_FORMATS)
def test_frame_rectified_emulated(emu_lib, fmt, mode):
    rc.check_frame_rectified(emu_lib, fmt, mode)


def test_frame_single_passes_emulated(emu_lib):
    rc.check_frame_single_passes(emu_lib)


@pytest.mark.parametrize("fmt", rc.FRAME_FORMATS)
def test_frame_identity_setting_is_todays_picture_emulated(emu_lib, fmt):
    rc.check_frame_identity_setting(emu_lib, fmt)


def test_setting_applies_to_later_uploads_emulated(emu_lib):
    rc.check_setting_applies_to_later_uploads(emu_lib)


def test_geometry_change_rebuilds_the_maps_emulated(emu_lib):
    rc.check_geometry_change_rebuilds_the_maps(emu_lib)


def test_consumer_of_rectified_frame_equals_host_path_emulated(emu_lib, emu_autodrive):
    rc.check_consumer_of_rectified_frame(emu_lib, emu_autodrive[0])


def test_canvas_has_out_geometry_emulated(emu_lib):
    rc.check_canvas_has_out_geometry(emu_lib)


def test_reupload_keeps_the_ordering_emulated(emu_lib, emu_autodrive):
    rc.check_reupload_keeps_the_ordering(emu_lib, emu_autodrive[0], emu_autodrive[1], rc.FRAME_HW, rc.FRAME_OUT_HW, rc.FRAME_K, rc.FRAME_DIST, rc.FRAME_H, rounds=1)
