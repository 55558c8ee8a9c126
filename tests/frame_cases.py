"""Shared cases of the vp_frame tests (tests/test_frame_host.py on the emulated library, tests/test_gpu_frame.py on the MI355X).

The oracle of the conversions is the numpy restatement below of the formula include/vp_hip.h states as the DEFINITION (integer BT.601 limited range,
20 fractional bits, no chroma interpolation); the other formats are permutations.  Every case builds its planes inside larger, randomly filled parent
arrays, so the bytes between a row's end and the next row are poison: a stride slip in the upload or the kernel shows in the result."""
import ctypes as C

import numpy as np

UV_GRID = (0, 1, 15, 16, 17, 64, 127, 128, 129, 192, 239, 240, 241, 254, 255)
PX_BYTES = {"bgr8": 3, "rgb8": 3, "bgra8": 4, "rgba8": 4, "gray8": 1, "nv12": 1, "yuy2": 2, "uyvy": 2}
YUV = ("nv12", "yuy2", "uyvy")


def yuv_raw(Y, U, V):
    """(R, G, B) before the clamp, int64: y = 1220542 * max(0, Y - 16); u = U - 128; v = V - 128; (y + c + 2^19) >> 20, arithmetic shift"""
    Y, U, V = (np.asarray(a).astype(np.int64) for a in (Y, U, V))
    y = 1220542 * np.maximum(0, Y - 16)
    u, v = U - 128, V - 128
    r = (y + 1673527 * v + (1 << 19)) >> 20
    g = (y - 852492 * v - 409993 * u + (1 << 19)) >> 20
    b = (y + 2116026 * u + (1 << 19)) >> 20
    return r, g, b


def yuv_to_bgr(Y, U, V):
    """uint8 [..., 3] in B, G, R order"""
    r, g, b = yuv_raw(Y, U, V)
    return np.stack([np.clip(c, 0, 255) for c in (b, g, r)], axis=-1).astype(np.uint8)


def to_bgr(fmt, planes, h, w):
    """the BGR8 image [h][w][3] a vp_frame holds after uploading `planes` (arrays whose rows may be longer than the row's bytes) as `fmt`"""
    p0 = np.asarray(planes[0]).reshape(planes[0].shape[0], -1)[:h, :PX_BYTES[fmt] * w]
    if fmt == "bgr8":
        return p0.reshape(h, w, 3).copy()
    if fmt == "rgb8":
        return p0.reshape(h, w, 3)[:, :, ::-1].copy()
    if fmt == "bgra8":
        return p0.reshape(h, w, 4)[:, :, :3].copy()
    if fmt == "rgba8":
        return p0.reshape(h, w, 4)[:, :, 2::-1].copy()
    if fmt == "gray8":
        return np.repeat(p0.reshape(h, w, 1), 3, axis=2)
    if fmt == "nv12":
        uv = np.asarray(planes[1])[:h // 2, :w].reshape(h // 2, w // 2, 2)
        U = uv[:, :, 0].repeat(2, axis=0).repeat(2, axis=1)
        V = uv[:, :, 1].repeat(2, axis=0).repeat(2, axis=1)
        return yuv_to_bgr(p0, U, V)
    q = p0.reshape(h, w // 2, 4)
    yo, co = (0, 1) if fmt == "yuy2" else (1, 0)
    Y = np.stack([q[:, :, yo], q[:, :, yo + 2]], axis=2).reshape(h, w)
    return yuv_to_bgr(Y, q[:, :, co].repeat(2, axis=1), q[:, :, co + 2].repeat(2, axis=1))


def random_planes(fmt, h, w, strides, seed):
    """planes of a random frame as views [rows][row bytes] into parents [rows][stride] filled with other random bytes"""
    rng = np.random.default_rng(seed)
    rows = [(h, PX_BYTES[fmt] * w)] + ([(h // 2, w)] if fmt == "nv12" else [])
    out = []
    for (n, rb), st in zip(rows, strides):
        parent = rng.integers(0, 256, size=(n, st), dtype=np.uint8)
        out.append(parent[:, :rb])
    return out


def table_planes(fmt):
    """The table frame of a YUV format: all 256 Y values across, each repeated to fill a chroma group (2 pixels wide; NV12: 2 x 2), one row group per
    (U, V) pair of UV_GRID squared -- both clamps of every channel and the Y < 16 floor.  Returns (planes, h, w)."""
    pairs = [(u, v) for u in UV_GRID for v in UV_GRID]
    w = 512
    Y = np.arange(256, dtype=np.uint8).repeat(2)
    if fmt == "nv12":
        h = 2 * len(pairs)
        yp = np.tile(Y, (h, 1))
        uv = np.empty((h // 2, w // 2, 2), np.uint8)
        for i, (u, v) in enumerate(pairs):
            uv[i, :, 0], uv[i, :, 1] = u, v
        return [yp, uv.reshape(h // 2, w)], h, w
    h = len(pairs)
    q = np.empty((h, w // 2, 4), np.uint8)
    yo, co = (0, 1) if fmt == "yuy2" else (1, 0)
    for i, (u, v) in enumerate(pairs):
        q[i, :, yo], q[i, :, yo + 2] = Y[0::2], Y[1::2]
        q[i, :, co], q[i, :, co + 2] = u, v
    return [q.reshape(h, 2 * w)], h, w


# (format, h, w, strides): the smallest shapes at which the upload and the kernel can still go wrong -- more than one chroma group per row and per
# column, a row that ends inside a four-pixel store block (w % 4 != 0), strides above the row's bytes
CONVERSION_CASES = [
    ("nv12", 4, 6, (8, 8)),
    ("yuy2", 3, 6, (16,)),
    ("uyvy", 3, 6, (16,)),
    ("bgra8", 3, 5, (24,)),
    ("rgba8", 3, 5, (20,)),
    ("rgb8", 3, 5, (17,)),
    ("gray8", 3, 5, (7,)),
    ("bgr8", 3, 5, (19,)),
]


def check_conversion(lib, fmt, h, w, strides, seed=0):
    planes = random_planes(fmt, h, w, strides, seed)
    want = to_bgr(fmt, planes, h, w)
    f = lib.Frame()
    try:
        f.upload(planes, fmt, hw=(h, w))
        assert f.hw() == (h, w)
        got = f.fetch_bgr8()
    finally:
        f.close()
    assert got.shape == want.shape
    assert np.array_equal(got, want), (fmt, np.argwhere(got != want)[:4])


def check_table(lib, fmt):
    planes, h, w = table_planes(fmt)
    want = to_bgr(fmt, planes, h, w)
    for c in range(3):   # the table does what it is for
        assert want[:, :, c].min() == 0 and want[:, :, c].max() == 255
    f = lib.Frame()
    try:
        f.upload(planes, fmt)
        got = f.fetch_bgr8()
    finally:
        f.close()
    assert np.array_equal(got, want), (fmt, np.argwhere(got != want)[:4])


def check_upload_refusals(lib):
    """VP_ERR_ARG with text: odd w for the 4:2:x formats, odd h for NV12, h or w below 2, a stride below the row's bytes, a wrong n_planes; VP_ERR_STATE before
    the first upload"""
    import pytest

    z = np.zeros((8, 64), np.uint8)
    f = lib.Frame()
    try:
        with pytest.raises(lib.VpError, match="never uploaded"):
            f._ck(f._lib.vp_frame_fetch_bgr8(f._h, z.ctypes.data_as(C.c_void_p), 64))
        h, w = C.c_int(), C.c_int()
        assert f._lib.vp_frame_dims(f._h, C.byref(h), C.byref(w)) == -4
        for fmt in YUV:
            with pytest.raises(ValueError, match="even width"):
                f.upload([z, z] if fmt == "nv12" else z, fmt, hw=(4, 5))
        with pytest.raises(ValueError, match="even height"):
            f.upload([z, z], "nv12", hw=(5, 6))
        with pytest.raises(ValueError, match="frame size"):
            f.upload(z, "gray8", hw=(1, 6))
        with pytest.raises(ValueError, match="frame size"):
            f.upload(z, "bgr8", hw=(4, 1))
        with pytest.raises(ValueError, match="below the row's"):
            f.upload(z, "bgra8", hw=(4, 17))          # 68 bytes a row, stride 64
        with pytest.raises(ValueError, match="below the row's"):
            f.upload([z, np.zeros((8, 8), np.uint8)], "nv12", hw=(4, 10))   # the UV plane: 10 bytes a row, stride 8
        with pytest.raises(ValueError, match="plane"):
            f.upload([z[:4]], "nv12", hw=(4, 6))       # one plane
        with pytest.raises(ValueError, match="plane"):
            f.upload([z, z], "yuy2", hw=(4, 6))
        with pytest.raises(ValueError, match="unknown format"):
            f.upload(z, 8, hw=(4, 6))
        with pytest.raises(lib.VpError):               # still nothing resident
            f.hw()
    finally:
        f.close()


def infer_view(lib, eng, parent, x0, y0, w, h):
    """vp_infer on the region of `parent` ([H][W][3] uint8, C-contiguous) passed as a STRIDED VIEW: the pointer of its first pixel, the parent's stride"""
    assert parent.flags.c_contiguous and parent.dtype == np.uint8
    ptr = C.c_void_p(parent.ctypes.data + y0 * parent.strides[0] + 3 * x0)
    eng._ck(lib.load().vp_infer(eng._h, ptr, h, w, parent.strides[0]))


def check_consumer_equals_host(lib, eng, fmt, h, w, region, seed=3, strides=None):
    """input tensor and logits of infer_frame on `region` (None: the whole frame) of a random `fmt` frame == vp_infer on the numpy-converted BGR8 slice passed
    as a strided view, bit for bit"""
    rb = PX_BYTES[fmt] * w
    planes = random_planes(fmt, h, w, strides or ((rb + 5, w + 3) if fmt == "nv12" else (rb + 5,)), seed)
    bgr = np.ascontiguousarray(to_bgr(fmt, planes, h, w))
    x0, y0, rw, rh = region if region is not None else (0, 0, w, h)
    infer_view(lib, eng, bgr, x0, y0, rw, rh)
    want_in, want = eng.input_tensor().copy(), eng.logits().copy()
    f = lib.Frame()
    try:
        f.upload(planes, fmt, hw=(h, w))
        eng.infer_frame(f, region)
        assert eng.frame_hw() == (rh, rw)
        assert np.array_equal(eng.input_tensor(), want_in)
        assert np.array_equal(eng.logits(), want)
    finally:
        f.close()
    return want
