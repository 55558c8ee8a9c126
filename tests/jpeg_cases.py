"""The cases of the JPEG tests (tests/test_jpeg_host.py, test_jpeg_emulated.py, test_gpu_jpeg.py) and the checks they share.  The reference of every
byte comparison is tests/jpeg_ref.py, the numpy / Python twin of the rules in include/vp_hip.h; streams are made once per process (stream_of)."""
import ctypes as C
import functools

import numpy as np
import pytest

import jpeg_ref as ref

QUALITIES = (1, 50, 75, 90, 100)


def picture(kind, h, w):
    """uint8 [h][w][3] BGR"""
    if kind == "frame":
        from oracle import pre_post

        return np.ascontiguousarray(pre_post.synthetic_frame(h, w, 5))
    if kind == "grey":
        return np.full((h, w, 3), 128, np.uint8)
    if kind == "noise":
        return np.random.default_rng(1000 * h + w).integers(0, 256, size=(h, w, 3), dtype=np.uint8)
    if kind == "checker":       # 8 x 8 squares of black and white: the largest DC differences; its lower half alternates per pixel: the largest AC values
        y, x = np.mgrid[0:h, 0:w]
        v = np.where(y < (h + 1) // 2, ((y >> 3) + (x >> 3)) & 1, (y + x) & 1)
        return np.repeat((v * 255).astype(np.uint8)[:, :, None], 3, axis=2)
    if kind == "ramp":
        y, x = np.mgrid[0:h, 0:w]
        return np.stack([(255 * x) // max(1, w - 1), (255 * y) // max(1, h - 1), (255 * (x + y)) // max(1, h + w - 2)], axis=2).astype(np.uint8)
    raise KeyError(kind)


# (picture, h, w, quality, restart_mcus).  2 x 2: everything is padding; 16 x 16: one MCU; 18 x 34: partial MCUs both ways; 48 x 64: 12 MCUs under Ri 1, 2, 3,
# 5 (does not divide 12), 65535 (one interval) and the default; 16 x 272: 17 intervals at Ri 1, the RST index wraps past 7; 176 x 320: more than one
# workgroup of every kernel at Ri 1 (220 MCUs, 28 groups of 8, 4 groups of 64 intervals)
CASES = (
    [("noise", 2, 2, q, 1) for q in QUALITIES]
    + [(p, 2, 2, 75, 0) for p in ("grey", "checker")]
    + [(p, 16, 16, q, 1) for p, q in (("frame", 75), ("grey", 50), ("noise", 100), ("checker", 100), ("ramp", 90), ("noise", 1))]
    + [(p, 18, 34, q, 1) for p, q in (("frame", 90), ("noise", 50), ("checker", 100), ("ramp", 1))]
    + [("frame", 48, 64, 75, ri) for ri in (1, 2, 3, 5, 65535, 0)]
    + [("noise", 48, 64, 100, 5), ("checker", 48, 64, 100, 3), ("grey", 48, 64, 75, 2), ("ramp", 48, 64, 50, 65535)]
    + [("frame", 16, 272, 75, 1), ("noise", 16, 272, 90, 1)]
    + [("frame", 176, 320, q, 1) for q in QUALITIES]
    + [("noise", 176, 320, 75, 0), ("checker", 176, 320, 100, 4), ("ramp", 176, 320, 90, 8), ("grey", 176, 320, 75, 1)]
)
SMALL_CASES = [c for c in CASES if c[1] * c[2] <= 48 * 64]     # what the emulation runs


def case_id(c):
    return "%s-%dx%d-q%d-ri%d" % c


@functools.lru_cache(maxsize=None)
def stream_of(case):
    """(the twin's stream, its statistics) of a case"""
    p, h, w, q, ri = case
    stats = {}
    return ref.encode(picture(p, h, w), q, ri, stats), stats


@functools.lru_cache(maxsize=None)
def coverage():
    """what the cases reach, summed over all of them: the case list cannot silently miss a path of the entropy coder"""
    total = {}
    for c in CASES:
        for k, v in stream_of(c)[1].items():
            total[k] = max(total.get(k, 0), v) if k == "dc_max" else total.get(k, 0) + v
    assert total.get("stuffed", 0) > 0, "no case has a stuffed FF 00"
    assert total.get("zrl", 0) > 0, "no case has a ZRL"
    assert total.get("no_eob", 0) > 0, "no case has a block without EOB"
    assert total.get("dc_max", 0) == 11, "no case has DC category 11"
    assert stream_of(("grey", 48, 64, 75, 2))[1].get("zrl", 0) == 0 and stream_of(("grey", 48, 64, 75, 2))[1].get("no_eob", 0) == 0   # EOB only
    return total


def first_difference(got, want):
    n = min(len(got), len(want))
    d = np.flatnonzero(np.frombuffer(got[:n], np.uint8) != np.frombuffer(want[:n], np.uint8))
    return (len(got), len(want), int(d[0]) if len(d) else None)


def check_operator(lib, case):
    """vp_op_jpeg_encode_bgr8 (from a packed picture, and from a view with a row stride of its own) equals the twin byte for byte"""
    p, h, w, q, ri = case
    bgr, want = picture(p, h, w), stream_of(case)[0]
    got = lib.jpeg_encode(bgr, q, ri)
    assert got == want, (case, first_difference(got, want))
    parent = np.random.default_rng(3).integers(0, 256, size=(h, w + 5, 3), dtype=np.uint8)
    parent[:, :w] = bgr
    got = lib.jpeg_encode(parent[:, :w], q, ri)
    assert got == want, (case, "strided", first_difference(got, want))
    assert len(want) <= lib.jpeg_bound(h, w, ri) == ref.bound(h, w, ri)


def raw_encode(lib, bgr, quality, ri, cap, fill=0xAA, null=()):
    """the raw entry on a buffer of `cap` bytes pre-filled with `fill`: (status, buffer, *n, text)"""
    buf = np.full(max(cap, 1), fill, np.uint8)
    n, err = C.c_size_t(0), C.create_string_buffer(512)
    h, w = bgr.shape[:2]
    P = lambda a: a.ctypes.data_as(C.c_void_p)   # noqa: E731
    rc = lib.load().vp_op_jpeg_encode_bgr8(0, None if "bgr" in null else P(bgr), h, w, 3 * w, quality, ri, None if "dst" in null else P(buf), cap,
                                           None if "n" in null else C.byref(n), err, len(err))
    return rc, buf, n.value, err.value.decode()


def check_operator_refusals(lib):
    """every refusal of the operator entry; `cap` one byte short leaves dst beyond the header untouched"""
    bgr = picture("noise", 16, 16)
    for q in (0, 101, -5):
        with pytest.raises(ValueError, match="quality"):
            lib.jpeg_encode(bgr, q, 1)
    for ri in (-1, 65536):
        with pytest.raises(ValueError, match="restart_mcus"):
            lib.jpeg_encode(bgr, 75, ri)
    for h, w, what in ((15, 16, "even height"), (16, 15, "even width"), (0, 16, "frame size")):
        rc, _, _, text = raw_encode(lib, np.zeros((max(h, 1), max(w, 1), 3), np.uint8)[:h] if h else np.zeros((0, 16, 3), np.uint8), 75, 1, 4096)
        assert rc == -1 and what in text, (h, w, rc, text)
    for null in ("bgr", "dst", "n"):
        rc, _, _, text = raw_encode(lib, bgr, 75, 1, 4096, null=(null,))
        assert rc == -1 and "null" in text, (null, rc, text)
    want = stream_of(("noise", 16, 16, 100, 1))[0]
    for cap in (len(want) - 1, ref.HEADER_BYTES + 1, ref.HEADER_BYTES, 10, 0):
        rc, buf, n, text = raw_encode(lib, bgr, 100, 1, cap)
        assert rc == -1 and str(len(want)) in text and n == len(want), (cap, rc, n, text)
        if cap >= ref.HEADER_BYTES:
            assert buf[:ref.HEADER_BYTES].tobytes() == want[:ref.HEADER_BYTES] and (buf[ref.HEADER_BYTES:] == 0xAA).all(), cap
        else:
            assert (buf == 0xAA).all(), cap
    rc, buf, n, _ = raw_encode(lib, bgr, 100, 1, len(want))      # the exact size is enough
    assert rc == 0 and n == len(want) and buf.tobytes() == want


def check_host_entries(lib):
    """vp_jpeg_header equals the twin's header byte for byte; vp_jpeg_bound is the twin's and holds every case; their refusals"""
    for h, w in ((2, 2), (16, 16), (18, 34), (720, 1280), (16384, 16384)):
        for q in (1, 25, 50, 75, 90, 100):
            for ri in (0, 1, 7, 65535):
                assert lib.jpeg_header(h, w, q, ri) == ref.header(h, w, q, ri), (h, w, q, ri)
        assert lib.jpeg_bound(h, w, 0) == ref.bound(h, w, 0) and lib.jpeg_bound(h, w, 1) == ref.bound(h, w, 1) >= ref.bound(h, w, 8)
    assert len(ref.header(2, 2, 1, 0)) == len(ref.header(16384, 16384, 100, 65535)) == ref.HEADER_BYTES
    for c in CASES:
        assert len(stream_of(c)[0]) <= lib.jpeg_bound(c[1], c[2], c[4]), c
        assert stream_of(c)[0].startswith(lib.jpeg_header(c[1], c[2], c[3], c[4])), c
    for call in (lambda: lib.jpeg_header(16, 16, 0), lambda: lib.jpeg_header(16, 16, 101)):
        with pytest.raises(ValueError, match="quality"):
            call()
    for call in (lambda: lib.jpeg_header(16, 16, 75, -1), lambda: lib.jpeg_bound(16, 16, 65536)):
        with pytest.raises(ValueError, match="restart_mcus"):
            call()
    for call in (lambda: lib.jpeg_bound(15, 16), lambda: lib.jpeg_header(16, 18000), lambda: lib.jpeg_bound(16, 7)):
        with pytest.raises(ValueError, match="even|frame size"):
            call()
    n, err = C.c_size_t(0), C.create_string_buffer(256)
    buf = np.full(700, 0xAA, np.uint8)
    assert lib.load().vp_jpeg_header(16, 16, 75, 1, buf.ctypes.data_as(C.c_void_p), 628, C.byref(n), err, len(err)) == -1 and n.value == 629 and (buf == 0xAA).all()
    assert lib.load().vp_jpeg_header(16, 16, 75, 1, None, 700, C.byref(n), err, len(err)) == -1 and b"null" in err.value
    assert lib.load().vp_jpeg_bound(16, 16, 1, None, err, len(err)) == -1 and b"null" in err.value


# ---- the canvas entries
CANVAS_HW = (48, 80)
MASK_REGION = (4, 2, 60, 40)


def drawn_canvas(lib, oc):
    """begin + blend_mask_u8 + draw_points, with no synchronisation of the caller's"""
    oc.canvas.begin(oc.frame)
    mask = np.random.default_rng(2).integers(0, 3, size=(20, 30), dtype=np.uint8)
    oc.canvas.blend_mask_u8(mask, 0, MASK_REGION)
    oc.canvas.draw_points([(10, 10), (70, 40), (79, 47)], 3, (0, 255, 0))


def check_canvas(lib):
    import canvas_cases as cc

    bgr0 = picture("frame", *CANVAS_HW)
    with cc.OnCanvas(lib, bgr0) as oc:
        c = oc.canvas
        drawn_canvas(lib, oc)
        got = c.fetch_jpeg(75, 1)                      # the first call behind the draws: no fetch, no sync before it
        shown = c.fetch("bgr8")
        assert not np.array_equal(shown, bgr0)         # the draws are in the picture
        assert got == lib.jpeg_encode(shown, 75, 1) == ref.encode(shown, 75, 1)
        c.set_color("bt601", "full", "mean")           # the samples' anchor: the twin fed the I420 fetch gives the same stream
        assert ref.encode_planes(c.fetch("i420"), 75, 1) == got
        for setting in (("bt709", "limited", "even"), ("bt601", "limited", "mean"), ("bt709", "full", "even")):
            c.set_color(*setting)                      # the canvas's own setting does not change the JPEG
            assert c.fetch_jpeg(75, 1) == got, setting
        assert np.array_equal(c.fetch("bgr8"), shown)  # the canvas is unchanged
        assert c.fetch_jpeg(75, 1) == got              # and the stream is the same on every call
        for q, ri in ((90, 0), (100, 3), (1, 65535)):
            assert c.fetch_jpeg(q, ri) == ref.encode(shown, q, ri), (q, ri)
        assert c.fetch_jpeg() == ref.encode(shown, 90, 0)
        small = c.fetch("bgr8", size=(30, 52))         # the resized picture: partial MCUs both ways
        assert c.fetch_jpeg(90, 1, size=(30, 52)) == lib.jpeg_encode(small, 90, 1) == ref.encode(small, 90, 1)
        assert np.array_equal(c.fetch("bgr8"), shown)
        c.draw_points([(40, 20)], 5, (255, 0, 0))      # a later draw is seen
        shown2 = c.fetch("bgr8")
        assert c.fetch_jpeg(75, 2) == ref.encode(shown2, 75, 2) != ref.encode(shown, 75, 2)
        other = picture("noise", 34, 18)               # a second begin at another geometry
        oc.frame.upload(other, "bgr8")
        c.begin(oc.frame)
        assert c.fetch_jpeg(50, 1) == ref.encode(other, 50, 1)
        bigger = picture("frame", 64, 96)
        oc.frame.upload(bigger, "bgr8")
        c.begin(oc.frame)
        assert c.fetch_jpeg(75, 0) == ref.encode(bigger, 75, 0)


def check_canvas_refusals(lib):
    import canvas_cases as cc

    c = lib.Canvas()
    try:
        with pytest.raises(lib.VpError, match="no picture"):
            c.fetch_jpeg()
        with pytest.raises(lib.VpError, match="no picture"):
            c.fetch_jpeg(size=(16, 16))
    finally:
        c.close()
    bgr = picture("noise", 16, 18)
    with cc.OnCanvas(lib, bgr) as oc:
        c = oc.canvas
        want = ref.encode(bgr, 100, 1)
        for q in (0, 101):
            with pytest.raises(ValueError, match="quality"):
                c.fetch_jpeg(q)
            with pytest.raises(ValueError, match="quality"):
                c.fetch_jpeg(q, size=(16, 16))
        for ri in (-1, 65536):
            with pytest.raises(ValueError, match="restart_mcus"):
                c.fetch_jpeg(75, ri)
        for size, what in (((15, 16), "even height"), ((16, 15), "even width"), ((0, 16), "frame size"), ((16, 16386), "frame size")):
            with pytest.raises(ValueError, match=what):
                c.fetch_jpeg(75, 1, size=size)
        n = C.c_size_t(0)
        buf = np.full(len(want) + 8, 0xAA, np.uint8)
        P = buf.ctypes.data_as(C.c_void_p)
        assert c._lib.vp_canvas_fetch_jpeg(c._h, 100, 1, None, buf.size, C.byref(n)) == -1 and "null" in c._lib.vp_canvas_last_error(c._h).decode()
        assert c._lib.vp_canvas_fetch_jpeg(c._h, 100, 1, P, buf.size, None) == -1
        assert c._lib.vp_canvas_fetch_jpeg_resized(c._h, 16, 16, 100, 1, None, buf.size, C.byref(n)) == -1
        assert c._lib.vp_canvas_fetch_jpeg(None, 100, 1, P, buf.size, C.byref(n)) == -1
        assert (buf == 0xAA).all()
        assert c._lib.vp_canvas_fetch_jpeg(c._h, 100, 1, P, len(want) - 1, C.byref(n)) == -1     # one byte short
        text = c._lib.vp_canvas_last_error(c._h).decode()
        assert str(len(want)) in text and n.value == len(want), text
        assert buf[:ref.HEADER_BYTES].tobytes() == want[:ref.HEADER_BYTES] and (buf[ref.HEADER_BYTES:] == 0xAA).all()
        assert c._lib.vp_canvas_fetch_jpeg(c._h, 100, 1, P, len(want), C.byref(n)) == 0 and buf[:len(want)].tobytes() == want and (buf[len(want):] == 0xAA).all()
        assert np.array_equal(c.fetch("bgr8"), bgr)        # refused calls changed nothing
