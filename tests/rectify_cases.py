"""Shared cases of the vp_frame rectification tests (tests/test_rectify_host.py on the host and on the emulated library, tests/test_gpu_rectify.py on the
MI355X).

The oracle is the numpy restatement below of what include/vp_hip.h states as the DEFINITION: the maps in IEEE double in the order written (numpy rounds
after every operation: no fused multiply-add), coordinates rounded half to even onto the 1/32-pixel grid, the sample as an integer blend of four taps.
Every comparison with the library is bit for bit; only the homography helper, which calls trigonometric functions, is compared at 1e-12."""
import numpy as np

import frame_cases as fc

LO, HI = -(1 << 20), (1 << 20) - 1
CONSTANT, REPLICATE = 0, 1


# ---- the definition
def rne_clamp(v):
    """round half to even, then the clamp to [-2^20, 2^20 - 1]; a NaN takes the lower clamp"""
    r = np.rint(np.asarray(v, dtype=np.float64))
    r = np.where(r >= LO, r, float(LO))
    r = np.where(r > HI, float(HI), r)
    return r.astype(np.int64)


def k_matrix(fx, fy, cx, cy):
    return np.array([[fx, 0.0, cx], [0.0, fy, cy], [0.0, 0.0, 1.0]], np.float64)


def distort(K, dist, x, y):
    fx, fy, cx, cy = float(K[0, 0]), float(K[1, 1]), float(K[0, 2]), float(K[1, 2])
    k1, k2, p1, p2, k3 = (float(d) for d in dist)
    r2 = x * x + y * y
    kr = 1.0 + ((k3 * r2 + k2) * r2 + k1) * r2
    xy2 = 2.0 * (x * y)
    xd = x * kr + p1 * xy2 + p2 * (r2 + 2.0 * (x * x))
    yd = y * kr + p1 * (r2 + 2.0 * (y * y)) + p2 * xy2
    return fx * xd + cx, fy * yd + cy


def undistort_map(K, dist, h, w):
    """(X, Y) int64 [h][w] in 1/32 pixel"""
    fx, fy, cx, cy = float(K[0, 0]), float(K[1, 1]), float(K[0, 2]), float(K[1, 2])
    j = np.arange(w, dtype=np.float64)[None, :] + np.zeros((h, 1))
    i = np.arange(h, dtype=np.float64)[:, None] + np.zeros((1, w))
    u, v = distort(K, dist, (j - cx) / fx, (i - cy) / fy)
    return rne_clamp(32.0 * u), rne_clamp(32.0 * v)


def inverse_homography(H):
    """adjugate over determinant, the nine cofactors spelled out as in the header"""
    H = [float(v) for v in np.asarray(H, dtype=np.float64).reshape(9)]
    a = [H[4] * H[8] - H[5] * H[7], H[2] * H[7] - H[1] * H[8], H[1] * H[5] - H[2] * H[4],
         H[5] * H[6] - H[3] * H[8], H[0] * H[8] - H[2] * H[6], H[2] * H[3] - H[0] * H[5],
         H[3] * H[7] - H[4] * H[6], H[1] * H[6] - H[0] * H[7], H[0] * H[4] - H[1] * H[3]]
    det = (H[0] * a[0] + H[1] * a[3]) + H[2] * a[6]
    return [v / det for v in a]


def _projective(H, out_h, out_w):
    M = inverse_homography(H)
    x = np.arange(out_w, dtype=np.float64)[None, :] + np.zeros((out_h, 1))
    y = np.arange(out_h, dtype=np.float64)[:, None] + np.zeros((1, out_w))
    return (M[0] * x + M[1] * y) + M[2], (M[3] * x + M[4] * y) + M[5], (M[6] * x + M[7] * y) + M[8]


def warp_map(H, out_h, out_w):
    X0, Y0, W = _projective(H, out_h, out_w)
    with np.errstate(all="ignore"):
        s = np.where(W != 0.0, 32.0 / W, 0.0)
        return rne_clamp(np.clip(X0 * s, -2.0 ** 31, 2.0 ** 31)), rne_clamp(np.clip(Y0 * s, -2.0 ** 31, 2.0 ** 31))


def one_pass_map(K, dist, H, out_h, out_w, h, w):
    fx, fy, cx, cy = float(K[0, 0]), float(K[1, 1]), float(K[0, 2]), float(K[1, 2])
    X0, Y0, W = _projective(H, out_h, out_w)
    with np.errstate(all="ignore"):
        px = np.where(W != 0.0, X0 / W, 0.0)
        py = np.where(W != 0.0, Y0 / W, 0.0)
    px = np.where(px >= 0.0, np.where(px > w - 1.0, w - 1.0, px), 0.0)
    py = np.where(py >= 0.0, np.where(py > h - 1.0, h - 1.0, py), 0.0)
    u, v = distort(K, dist, (px - cx) / fx, (py - cy) / fy)
    return rne_clamp(32.0 * u), rne_clamp(32.0 * v)


def tap_state(X, Y, h, w):
    """per destination pixel: how many of the four taps lie inside an h x w source"""
    ix, iy = X >> 5, Y >> 5
    n = np.zeros(X.shape, np.int64)
    for dy in (0, 1):
        for dx in (0, 1):
            n += ((ix + dx >= 0) & (ix + dx < w) & (iy + dy >= 0) & (iy + dy < h)).astype(np.int64)
    return n


def remap(src, X, Y, border):
    """the sample: src uint8 [h][w][3], (X, Y) int64 in 1/32 pixel -> uint8 [..., 3]"""
    src = np.asarray(src)
    h, w = src.shape[:2]
    s = src.astype(np.int64)
    ix, iy, fx, fy = X >> 5, Y >> 5, X & 31, Y & 31
    acc = np.zeros(X.shape + (3,), np.int64)
    for dy, wy in ((0, 32 - fy), (1, fy)):
        for dx, wx in ((0, 32 - fx), (1, fx)):
            x, y = ix + dx, iy + dy
            p = s[np.clip(y, 0, h - 1), np.clip(x, 0, w - 1)]
            if border == CONSTANT:
                p = p * ((x >= 0) & (x < w) & (y >= 0) & (y < h))[..., None]
            acc += (wx * wy)[..., None] * p
    return ((acc + 512) >> 10).astype(np.uint8)


def to_exchange(X, Y):
    """the exchange form of vp_rectify_map: int16 (ix, iy) pairs, uint16 frac = fy << 5 | fx"""
    return np.stack([X >> 5, Y >> 5], axis=-1).astype(np.int16), (((Y & 31) << 5) | (X & 31)).astype(np.uint16)


def from_exchange(xy, frac):
    xy, frac = xy.astype(np.int64), frac.astype(np.int64)
    return xy[..., 0] * 32 + (frac & 31), xy[..., 1] * 32 + (frac >> 5)


def is_identity_h(H):
    return np.array_equal(np.asarray(H, dtype=np.float64).reshape(3, 3), np.eye(3))


def rectify(bgr, K, dist, H, out_hw, mode="two_pass"):
    """the picture a vp_frame holds after uploading `bgr` [h][w][3] under the setting: the passes of include/vp_hip.h, identity passes skipped"""
    h, w = bgr.shape[:2]
    oh, ow = out_hw
    if mode == "one_pass":
        return remap(bgr, *one_pass_map(K, dist, H, oh, ow, h, w), CONSTANT)
    pic = bgr
    if any(float(d) != 0.0 for d in dist):
        pic = remap(pic, *undistort_map(K, dist, h, w), CONSTANT)
    if not (is_identity_h(H) and (oh, ow) == (h, w)):
        pic = remap(pic, *warp_map(H, oh, ow), REPLICATE)
    return np.ascontiguousarray(pic)


def homography(inference, standard):
    """calibration.py restated with numpy: Rodrigues of (pitch, yaw, roll), R_rel = R_s R_i^-1, K_s from the standard pose's size and HFoV, its [1][1] scaled by
    the ratio of the camera heights, H = K_s_mod R_rel K_i^-1"""
    def rot(p):
        v = np.radians(np.array([p["pitch"], p["yaw"], p["roll"]], np.float64))
        th = float(np.sqrt((v * v).sum()))
        if th == 0.0:
            return np.eye(3)
        k = v / th
        kx = np.array([[0.0, -k[2], k[1]], [k[2], 0.0, -k[0]], [-k[1], k[0], 0.0]])
        return np.cos(th) * np.eye(3) + (1.0 - np.cos(th)) * np.outer(k, k) + np.sin(th) * kx

    ws, hs = standard["img_width"], standard["img_height"]
    fs = (ws / 2) / np.tan(np.radians(standard["hfov"]) / 2)
    Ks = np.array([[fs, 0.0, ws / 2], [0.0, fs, hs / 2], [0.0, 0.0, 1.0]])
    Ks[1, 1] *= standard["camera_height"] / inference["camera_height"]
    R_rel = rot(standard) @ np.linalg.inv(rot(inference))
    return Ks @ R_rel @ np.linalg.inv(np.asarray(inference["intrinsic_matrix"], dtype=np.float64).reshape(3, 3))


# ---- the cases.  A 90 x 161 source (the width no multiple of 4); the pincushion coefficients push the border of the undistorted picture outside the raw
# one (CONSTANT is live), the barrel coefficients keep every tap inside; the homography leaves about half of the 64 x 128 destination outside the
# source (REPLICATE is live).
SRC_HW = (90, 161)
K = k_matrix(120.3, 118.7, 80.2, 44.9)
PINCUSHION = (0.25, 0.05, 0.001, -0.0007, 0.0)
BARREL = (-0.31, 0.12, 0.001, -0.0007, -0.02)
ZERO = (0.0, 0.0, 0.0, 0.0, 0.0)
OUT_HW = (64, 128)
H_WARP = np.array([[0.93, 0.06, 53.0], [-0.045, 0.88, 9.5], [0.0005, 0.0003, 1.0]], np.float64)
DISTS = {"pincushion": PINCUSHION, "barrel": BARREL}

# the ordering check on the device: a camera large enough for the passes to take a while (270 x 482 -> 256 x 448)
BIG_HW = (270, 482)
BIG_K = k_matrix(395.0, 388.0, 242.6, 136.1)
BIG_OUT_HW = (256, 448)
BIG_H = np.array([[0.9, 0.04, 30.0], [-0.03, 0.93, 6.5], [0.00008, 0.00004, 1.0]], np.float64)

# the frame path: a 60 x 86 camera (even both ways for the YUV formats, the width no multiple of 4) rectified to 50 x 70
FRAME_HW = (60, 86)
FRAME_K = k_matrix(70.5, 69.2, 43.3, 29.6)
FRAME_DIST = (0.12, 0.02, 0.001, -0.0007, 0.0)
FRAME_OUT_HW = (50, 70)
FRAME_H = np.array([[0.9, 0.04, 14.0], [-0.03, 0.86, 3.5], [0.0004, 0.0002, 1.0]], np.float64)
FRAME_FORMATS = ("bgr8", "nv12")


def random_picture(h, w, seed):
    return np.random.default_rng(seed).integers(0, 256, size=(h, w, 3), dtype=np.uint8)


def smooth_picture(h, w):
    """p[y][x][c] = round(127.5 + 100 sin(0.15 x + 0.3 c) cos(0.11 y)): at most 15 levels per pixel along x, 11 along y"""
    x = np.arange(w, dtype=np.float64)[None, :, None]
    y = np.arange(h, dtype=np.float64)[:, None, None]
    c = np.arange(3, dtype=np.float64)[None, None, :]
    return np.rint(127.5 + 100.0 * np.sin(0.15 * x + 0.3 * c) * np.cos(0.11 * y)).astype(np.uint8)


def named_map(which, dist, h=SRC_HW[0], w=SRC_HW[1]):
    """(X, Y, border) of the maps of the cases above"""
    if which == "undistort":
        return undistort_map(K, dist, h, w) + (CONSTANT,)
    if which == "warp":
        return warp_map(H_WARP, *OUT_HW) + (REPLICATE,)
    return one_pass_map(K, dist, H_WARP, OUT_HW[0], OUT_HW[1], h, w) + (CONSTANT,)


MAP_CASES = [("undistort", "pincushion"), ("undistort", "barrel"), ("warp", "barrel"), ("one_pass", "pincushion"), ("one_pass", "barrel")]


# ---- checks taking a `lib` (the binding on the shipped or on the emulated library)
def _strided(pic, extra, seed):
    """`pic` as a view into a parent with `extra` poison bytes behind every row"""
    h, w = pic.shape[:2]
    parent = np.random.default_rng(seed).integers(0, 256, size=(h, 3 * w + extra), dtype=np.uint8)
    parent[:, :3 * w] = pic.reshape(h, 3 * w)
    return parent[:, :3 * w].reshape(h, w, 3)


def check_kernel_case(lib, which, dist_name):
    """the maps of item 1 on seeded random bytes through vp_op_remap_bgr8, BOTH borders, a strided source"""
    X, Y, _ = named_map(which, DISTS[dist_name])
    src = random_picture(SRC_HW[0], SRC_HW[1], 11)
    xy, frac = to_exchange(X, Y)
    for border in (CONSTANT, REPLICATE):
        got = lib.op_remap_bgr8(_strided(src, 7, 12), xy, frac, border)
        want = remap(src, X, Y, border)
        assert np.array_equal(got, want), (which, dist_name, border, np.argwhere(got != want)[:4])


def check_kernel_table(lib):
    """a 2 x 2 source of 0 / 255 bytes under a map holding all 1024 fraction pairs, at the one position where all four taps are inside"""
    src = np.array([[[0, 255, 0], [255, 0, 255]], [[255, 255, 0], [0, 0, 255]]], np.uint8)
    fy, fx = np.meshgrid(np.arange(32), np.arange(32), indexing="ij")
    X, Y = fx.astype(np.int64), fy.astype(np.int64)
    want = remap(src, X, Y, REPLICATE)
    assert want.min() == 0 and want.max() == 255 and len(np.unique(want)) > 100
    xy, frac = to_exchange(X, Y)
    assert frac.reshape(-1).tolist() == list(range(1024))
    for border in (CONSTANT, REPLICATE):
        got = lib.op_remap_bgr8(src, xy, frac, border)
        assert np.array_equal(got, remap(src, X, Y, border)), border


def check_kernel_edges(lib):
    """coordinates saturated at both clamps and one pixel outside each edge, with and without a fraction, both borders"""
    h, w = 5, 7
    src = random_picture(h, w, 13)
    xs = [LO, LO + 13, -64, -32, -19, -1, 0, 17, 32 * (w - 1) - 1, 32 * (w - 1), 32 * (w - 1) + 9, 32 * w, 32 * w + 5, HI - 7, HI]
    ys = [LO, -32, -7, 0, 21, 32 * (h - 1), 32 * (h - 1) + 30, 32 * h, HI]
    Y, X = np.meshgrid(np.array(ys, np.int64), np.array(xs, np.int64), indexing="ij")
    xy, frac = to_exchange(X, Y)
    assert np.array_equal(np.stack(from_exchange(xy, frac)), np.stack([X, Y]))     # the exchange form holds both clamps
    for border in (CONSTANT, REPLICATE):
        got = lib.op_remap_bgr8(src, xy, frac, border)
        assert np.array_equal(got, remap(src, X, Y, border)), border


def check_kernel_widths_and_padding(lib):
    """out_w in {2, 5, 8, 161}: a row that ends inside, at the end of, and beyond one store block; a destination stride above the pitch shows the bytes
    behind the row's end (the entry fills the device picture with 0xFF first, so a zero there was WRITTEN), and bytes beyond the pitch stay untouched"""
    src = random_picture(SRC_HW[0], SRC_HW[1], 14)
    Xf, Yf, _ = named_map("undistort", PINCUSHION)
    for ow in (2, 5, 8, 161):
        X, Y = Xf[:9, :ow], Yf[:9, :ow]
        xy, frac = to_exchange(X, Y)
        pitch = 12 * ((ow + 3) // 4)
        for border in (CONSTANT, REPLICATE):
            want = remap(src, X, Y, border)
            raw = lib.op_remap_bgr8(_strided(src, 5, 15), xy, frac, border, dst_stride=pitch + 8)
            assert np.array_equal(raw[:, :3 * ow].reshape(9, ow, 3), want), (ow, border)
            assert (raw[:, 3 * ow:pitch] == 0).all(), (ow, border)
            assert (raw[:, pitch:] == 0xAA).all(), (ow, border)
            tight = lib.op_remap_bgr8(src, xy, frac, border, dst_stride=3 * ow + 1)      # below the pitch: the pixels alone
            assert np.array_equal(tight[:, :3 * ow].reshape(9, ow, 3), want) and (tight[:, 3 * ow:] == 0xAA).all(), (ow, border)


def check_kernel_wide(lib):
    """more than one 256-work-item block along a row (out_w = 1030 > 1024, the last block of the row half empty) under a map of random coordinates in
    and around a 6 x 1100 source: no order among the entries a work-item reads"""
    rng = np.random.default_rng(16)
    h, w, oh, ow = 6, 1100, 3, 1030
    src = random_picture(h, w, 17)
    X = rng.integers(-96, 32 * w + 96, size=(oh, ow), dtype=np.int64)
    Y = rng.integers(-96, 32 * h + 96, size=(oh, ow), dtype=np.int64)
    xy, frac = to_exchange(X, Y)
    for border in (CONSTANT, REPLICATE):
        got = lib.op_remap_bgr8(src, xy, frac, border)
        assert np.array_equal(got, remap(src, X, Y, border)), border


def check_op_refusals(lib):
    import pytest

    src = random_picture(4, 4, 1)
    xy, frac = np.zeros((2, 2, 2), np.int16), np.zeros((2, 2), np.uint16)
    with pytest.raises(ValueError, match="border"):
        lib.op_remap_bgr8(src, xy, frac, 2)
    with pytest.raises(ValueError, match="below 32"):
        lib.op_remap_bgr8(src, xy, np.full((2, 2), 1024, np.uint16), REPLICATE)
    with pytest.raises(ValueError, match="strides"):
        lib.op_remap_bgr8(src, xy, frac, REPLICATE, dst_stride=5)


def frame_planes(fmt, seed):
    h, w = FRAME_HW
    rb = fc.PX_BYTES[fmt] * w
    return fc.random_planes(fmt, h, w, (rb + 5, w + 3) if fmt == "nv12" else (rb + 5,), seed)


def frame_want(fmt, planes, mode="two_pass", dist=FRAME_DIST, H=FRAME_H, out_hw=FRAME_OUT_HW):
    return rectify(fc.to_bgr(fmt, planes, *FRAME_HW), FRAME_K, dist, H, out_hw, mode)


def check_frame_rectified(lib, fmt, mode):
    """fetch == the numpy passes over the frame tests' to_bgr picture; vp_frame_dims answers the out size; the setting reads back"""
    planes = frame_planes(fmt, 21)
    want = frame_want(fmt, planes, mode)
    assert want.shape == FRAME_OUT_HW + (3,) and len(np.unique(want)) > 100
    f = lib.Frame()
    try:
        assert f.get_rectify() is None
        f.set_rectify(FRAME_K, FRAME_DIST, FRAME_H, FRAME_OUT_HW, mode)
        back = f.get_rectify()
        assert np.array_equal(back["K"], FRAME_K) and np.array_equal(back["H"], FRAME_H) and back["dist"].tolist() == list(FRAME_DIST)
        assert back["out_hw"] == FRAME_OUT_HW and back["mode"] == lib.RECTIFY_MODES[mode]
        for _ in range(2):                                   # the second upload runs on the cached maps
            f.upload(planes, fmt, hw=FRAME_HW)
            assert f.hw() == FRAME_OUT_HW
            got = f.fetch_bgr8()
            assert np.array_equal(got, want), (fmt, mode, np.argwhere(got != want)[:4])
    finally:
        f.close()


def check_frame_single_passes(lib, fmt="nv12"):
    """two-pass with one identity pass: undistort alone (H = I at the raw size), warp alone (dist = 0), and the warp-only pass to ANOTHER size with H = I"""
    planes = frame_planes(fmt, 22)
    f = lib.Frame()
    try:
        for dist, H, out_hw in ((FRAME_DIST, np.eye(3), FRAME_HW), (ZERO, FRAME_H, FRAME_OUT_HW), (ZERO, np.eye(3), (FRAME_HW[0] + 3, FRAME_HW[1] - 5))):
            f.set_rectify(FRAME_K, dist, H, out_hw)
            f.upload(planes, fmt, hw=FRAME_HW)
            assert f.hw() == tuple(out_hw)
            assert np.array_equal(f.fetch_bgr8(), frame_want(fmt, planes, "two_pass", dist, H, tuple(out_hw)))
    finally:
        f.close()


def check_frame_identity_setting(lib, fmt):
    """zero dist and identity H at the raw size: today's picture, byte for byte"""
    planes = frame_planes(fmt, 23)
    f = lib.Frame()
    try:
        f.set_rectify(FRAME_K, ZERO, np.eye(3), FRAME_HW)
        f.upload(planes, fmt, hw=FRAME_HW)
        assert f.hw() == FRAME_HW
        assert np.array_equal(f.fetch_bgr8(), fc.to_bgr(fmt, planes, *FRAME_HW))
    finally:
        f.close()


def check_setting_applies_to_later_uploads(lib, fmt="nv12"):
    """a setting changed between two uploads applies to the second only; NULL switches it off again; a refused setting changes nothing"""
    import pytest

    A, B, Cc = (frame_planes(fmt, s) for s in (24, 25, 26))
    f = lib.Frame()
    try:
        f.upload(A, fmt, hw=FRAME_HW)
        f.set_rectify(FRAME_K, FRAME_DIST, FRAME_H, FRAME_OUT_HW)
        assert f.hw() == FRAME_HW and np.array_equal(f.fetch_bgr8(), fc.to_bgr(fmt, A, *FRAME_HW))     # the picture it holds stays
        f.upload(B, fmt, hw=FRAME_HW)
        assert f.hw() == FRAME_OUT_HW and np.array_equal(f.fetch_bgr8(), frame_want(fmt, B))
        f.set_rectify(FRAME_K, FRAME_DIST, FRAME_H, FRAME_OUT_HW, "one_pass")                              # same geometry, another setting: new maps
        f.upload(B, fmt, hw=FRAME_HW)
        assert np.array_equal(f.fetch_bgr8(), frame_want(fmt, B, "one_pass"))
        with pytest.raises(ValueError, match="det H"):
            f.set_rectify(FRAME_K, FRAME_DIST, np.zeros((3, 3)), FRAME_OUT_HW)
        assert f.get_rectify()["mode"] == lib.VP_RECTIFY_ONE_PASS
        f.set_rectify(None)
        assert f.get_rectify() is None
        assert f.hw() == FRAME_OUT_HW                                                                   # still the last upload's
        f.upload(Cc, fmt, hw=FRAME_HW)
        assert f.hw() == FRAME_HW and np.array_equal(f.fetch_bgr8(), fc.to_bgr(fmt, Cc, *FRAME_HW))
    finally:
        f.close()


def check_geometry_change_rebuilds_the_maps(lib, fmt="nv12"):
    """one setting, cameras of two sizes in turn: the maps belong to a raw geometry and are rebuilt when it changes (the buffers grow and shrink with it)"""
    f = lib.Frame()
    try:
        f.set_rectify(FRAME_K, FRAME_DIST, FRAME_H, FRAME_OUT_HW)
        for h, w, seed in ((40, 52, 41), FRAME_HW + (42,), (40, 52, 43)):
            planes = fc.random_planes(fmt, h, w, (w + 3, w + 1), seed)
            f.upload(planes, fmt, hw=(h, w))
            assert f.hw() == FRAME_OUT_HW
            assert np.array_equal(f.fetch_bgr8(), rectify(fc.to_bgr(fmt, planes, h, w), FRAME_K, FRAME_DIST, FRAME_H, FRAME_OUT_HW)), (h, w)
    finally:
        f.close()


def check_consumer_of_rectified_frame(lib, eng, fmt="nv12", region=(5, 7, 41, 29)):
    """a consumer fed a region of the rectified frame == the host path on the numpy-rectified picture passed as a strided view (frame_cases.
    check_consumer_equals_host with the passes in between), input tensor and logits bit for bit"""
    planes = frame_planes(fmt, 27)
    pic = np.ascontiguousarray(frame_want(fmt, planes))
    x0, y0, rw, rh = region
    fc.infer_view(lib, eng, pic, x0, y0, rw, rh)
    want_in, want = eng.input_tensor().copy(), eng.logits().copy()
    f = lib.Frame()
    try:
        f.set_rectify(FRAME_K, FRAME_DIST, FRAME_H, FRAME_OUT_HW)
        f.upload(planes, fmt, hw=FRAME_HW)
        eng.infer_frame(f, region)
        assert eng.frame_hw() == (rh, rw)
        assert np.array_equal(eng.input_tensor(), want_in)
        assert np.array_equal(eng.logits(), want)
        with __import__("pytest").raises(ValueError, match="frame region"):       # the region is checked against the OUT geometry
            eng.upload_from_frame(f, (0, 0, FRAME_HW[1], FRAME_HW[0]))
    finally:
        f.close()


def check_canvas_has_out_geometry(lib, fmt="nv12"):
    planes = frame_planes(fmt, 28)
    f, c = lib.Frame(), lib.Canvas()
    try:
        f.set_rectify(FRAME_K, FRAME_DIST, FRAME_H, FRAME_OUT_HW)
        f.upload(planes, fmt, hw=FRAME_HW)
        c.begin(f)
        assert c.hw() == FRAME_OUT_HW
        assert np.array_equal(c.fetch("bgr8"), frame_want(fmt, planes))
    finally:
        c.close()
        f.close()


def check_reupload_keeps_the_ordering(lib, e1, e2, raw_hw, out_hw, K_, dist, H, fmt="nv12", rounds=2):
    """upload A, consume, upload B, consume -- no host wait in between -- and each consumer sees its own rectified frame"""
    h, w = raw_hw
    A, B = (fc.random_planes(fmt, h, w, (w + 6, w + 2), s) for s in (31, 32))
    want = []
    for e, p in ((e1, A), (e2, B)):
        pic = rectify(fc.to_bgr(fmt, p, h, w), K_, dist, H, out_hw)
        for _ in range(2):               # twice: a streaming engine (AutoDrive) pairs a frame with the one before it, below always the same picture
            e.infer(pic)
        want.append(e.logits().copy())
    assert not np.array_equal(want[0], want[1])
    f = lib.Frame()
    try:
        f.set_rectify(K_, dist, H, out_hw)
        for _ in range(rounds):
            f.upload(A, fmt, hw=(h, w))
            e1.upload_from_frame(f)
            e1.enqueue()
            f.upload(B, fmt, hw=(h, w))
            e2.upload_from_frame(f)
            e2.enqueue()
            e1.fetch_outputs()
            e2.fetch_outputs()
            assert np.array_equal(e1.logits(), want[0])
            assert np.array_equal(e2.logits(), want[1])
    finally:
        f.close()
