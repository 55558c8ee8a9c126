"""Shared bodies of the decoder-kernel tests: one convolution through vp_op_conv2d (3x3 / 1x1, ConvTranspose2d(k2, s2) with and without the
fused skip link, a head's logits) or one composed up-sampling stage through vp_op_upconv, with the kernel chosen explicitly, against torch in
fp64 on the operands as the engine stores them.  tests/test_conv_emulated.py and tests/test_upconv_emulated.py run them at small shapes on
the HIP-on-CPU emulator; tests/test_gpu_decoder_kernels.py runs them at the production shapes on the MI355X.

Operand axes:
  rows   "uniform"      He-scaled weights, every output row of the same magnitude (the family of the older tests);
         "spread"       output row r scaled by 2^k_r, k_r uniform in [-10, 6] with both ends present, its bias and residual rows likewise: the
                        engine's per-row prescale (engine.cpp row_prescale) then differs from row to row, so every epilogue's
                        fmaf(acc, wscale[co], bias[co]) has to read its own row's scale;
         "spread+dead"  as "spread", plus one all-zero weight row (prescale 0 next to non-zero neighbours) and one row with a single non-zero weight;
         "spread_cm"    (up-sampling stage only) the ConvTranspose's and the skip link's middle channels spread independently, so the composed
                        (phase, channel) rows and the x and skip parts inside one row differ in magnitude.
  scale  1, 2^-12 (every activation's lo plane is subnormal, below 2^-14 the hi plane too) or 2^8, on inputs, biases and residuals.

Judging: per output channel, max |got - ref| relative to that channel's largest |ref|, against a bar that models the arithmetic (BAR_*); at a
value edge or with spread rows (channels down to 2^-10 of the rest) the output format's own storage error for that channel is added."""
import numpy as np
import torch
import torch.nn.functional as F

ROWS = ("uniform", "spread", "spread+dead")
SCALES = (1.0, 2.0 ** -12, 2.0 ** 8)
K_LO, K_HI = -10, 6                   # row exponents of the spread families

BAR_X3 = 1e-4
"""parity mode (fp16x3), error model: per product the dropped lo*lo term (2^-22 of |x w|), fp32 accumulation over K = taps * Cin terms
(~sqrt(K) * 2^-24 of the partial sums), the (hi, lo) split of the weights and of the output (2^-22 each); the emulator measures 0.6e-5 - 2.1e-5
with spread rows, so the bar leaves 5x"""
BAR_F16 = 1e-3
"""fp16 engines, error model: the reference convolves the operands as stored (fp16 activations, fp16 weight rows after the prescale), so what
remains is fp32 accumulation (< 1e-5, as above), GELU_F16's approximation (7e-6 of |x|) and the single fp16 output plane: round to nearest,
at most 2^-11 = 4.9e-4 of the channel's maximum"""
BAR_F16_UPCONV = 2e-3
"""fp16 form of the composed stage: BAR_F16 plus the composed weights rounded to fp16 (2^-12 of each weight, the reference composes the
un-rounded ones in fp64): random signs give ~2^-12 / sqrt(3) = 1.4e-4 of the channel's spread, 6e-4 at four sigma"""


def split16(x):
    """fp32 -> the (hi, lo) fp16 planes of the engine's activation and weight format"""
    hi = x.astype(np.float16)
    return hi, (x - hi.astype(np.float32)).astype(np.float16)


def as_stored(a, precision):
    """what the engine's planes hold of fp32 values `a` (precision 1: hi + lo, 0: one fp16 plane), as fp64"""
    a = np.asarray(a, np.float32)
    if precision == 1:
        h, l = split16(a)
        return h.astype(np.float64) + l.astype(np.float64)
    return a.astype(np.float16).astype(np.float64)


def prescale_exp(amax):
    """engine.cpp prescale_exp, per element: the s that puts amax * 2^s in [2^13, 2^14), clamped to [-8, 60]; 0 for an all-zero row"""
    amax = np.asarray(amax, np.float32)
    e = np.frexp(amax)[1]
    return np.where((amax > 0) & np.isfinite(amax), np.clip(14 - e, -8, 60), 0).astype(np.int64)


def rows_as_stored(m, precision):
    """a weight matrix [rows][K] as the engine holds it: each row times its 2^s, split into planes, times 2^-s again (fp64)"""
    m = np.asarray(m, np.float32)
    s = prescale_exp(np.abs(m).max(axis=1))[:, None]
    return as_stored(np.ldexp(m, s), precision) * np.ldexp(1.0, -s)


def row_factors(rng, n, rows):
    """2^k_r per row: all 1 for "uniform", else k_r uniform in [K_LO, K_HI] with both ends present"""
    if rows == "uniform":
        return np.ones(n, np.float32)
    k = rng.integers(K_LO, K_HI + 1, n)
    if n >= 2:
        k[rng.permutation(n)[:2]] = (K_LO, K_HI)
    return np.ldexp(np.float32(1.0), k).astype(np.float32)


def kill_rows(rng, w, axis=0):
    """"spread+dead": one all-zero row and one row with a single non-zero weight along `axis` (indices returned)"""
    n = w.shape[axis]
    if n < 3:                                 # (a one-row logits layer keeps its row)
        return None
    dead, single = rng.permutation(n)[:2]
    v = np.moveaxis(w, axis, 0)
    keep = v[single].flat[v[single].size // 2] or np.float32(0.5)
    v[dead] = 0
    v[single] = 0
    v[single].flat[v[single].size // 2] = keep
    return int(dead), int(single)


def edge_weight_factor(rows, scale):
    """at 2^8 the outputs have to stay inside the fp16 range (65504): spread rows (weights, biases, residuals) are taken down by 2^-K_HI, so no
    row exceeds He scale"""
    return np.float32(2.0 ** -K_HI) if scale > 1.0 and rows != "uniform" else np.float32(1.0)


def _judge(got, ref, precision, base, rows, scale, stored_out, what):
    """per-channel error of got [C][...] against ref (fp64) and the bar; asserts; returns the body's result"""
    assert got.shape == ref.shape and np.isfinite(got).all(), what
    C = ref.shape[0]
    r = ref.reshape(C, -1)
    chmax = np.maximum(np.abs(r).max(axis=1), 1e-30)
    err = np.abs(got.reshape(C, -1).astype(np.float64) - r).max(axis=1) / chmax
    bar = np.full(C, base)
    if stored_out and (scale != 1.0 or rows != "uniform"):
        bar += np.abs(as_stored(r.astype(np.float32), precision) - r).max(axis=1) / chmax
    worst = int(np.argmax(err / bar))
    assert (err <= bar).all(), f"{what}: channel {worst} err {err[worst]:.3e} > bar {bar[worst]:.3e} (channel max {chmax[worst]:.3e})"
    # for the error table: the largest error beyond the output's storage error, against the arithmetic bar
    return {"out": got, "ref": ref, "err_c": err, "bar_c": bar, "err": float(np.maximum(err - (bar - base), 0.0).max()), "bar": base}


ACT = {0: lambda t: t, 1: F.gelu, 2: F.silu}


def check_conv(lib, cin, cout, h, w, ks=3, mode=0, act=1, res_mode=0, precision=1, tile=-1, bk=-1, nsplit=-1, rows="spread", scale=1.0, seed=0,
               cs=0):
    """vp_op_conv2d with an explicit kernel choice against torch fp64.  mode 0: conv ks x ks (+ act, + residual: 1 add, 2 mul-add);
    1: ConvTranspose2d(k2, s2), rows spread along its output-channel axis ([cin][cout][2][2], axis 1); 2: the same + Conv2d 1x1 of a
    cs-channel skip tensor, whose weight rows get factors of their own (spread separately from the ConvTranspose's); 3: a head's logits
    (fp32 NCHW out: no output storage error).  The mul-add residual multiplies the convolution: its rows keep unit scale (and at 2^8 unit
    magnitude), so y * r + r stays inside fp16 at every row factor."""
    rng = np.random.default_rng(seed)
    f32 = np.float32
    act = act if mode in (0, 1) else 0        # the skip-link form and the logits carry no activation
    fac = row_factors(rng, cout, rows) * edge_weight_factor(rows, scale)
    x = (rng.standard_normal((cin, h, w)) * scale).astype(f32)
    b = (rng.standard_normal(cout) * 0.1 * scale * fac).astype(f32)
    if mode in (1, 2):
        wt = (rng.standard_normal((cin, cout, 2, 2)) * np.sqrt(1.0 / cin) * fac[None, :, None, None]).astype(f32)
        if rows == "spread+dead":
            kill_rows(rng, wt, axis=1)
    else:
        wt = (rng.standard_normal((cout, cin, ks, ks)) * np.sqrt(2.0 / (cin * ks * ks)) * fac[:, None, None, None]).astype(f32)
        if rows == "spread+dead":
            kill_rows(rng, wt, axis=0)
    oh, ow = (2 * h, 2 * w) if mode in (1, 2) else (h, w)
    res, rs = None, None
    if mode == 0 and res_mode == 1:
        res = (rng.standard_normal((cout, oh, ow)) * scale * fac[:, None, None]).astype(f32)
    elif mode == 0 and res_mode == 2:
        res = (rng.standard_normal((cout, oh, ow)) * min(scale, 1.0)).astype(f32)
    if res is not None:
        rs = torch.from_numpy(as_stored(res, precision))[None]
    xs = torch.from_numpy(as_stored(x, precision))[None]
    if mode in (1, 2):
        m = wt.reshape(cin, cout, 4).transpose(2, 1, 0).reshape(4 * cout, cin)      # GEMM rows (quadrant, output channel) over the input channels
        if mode == 2:
            gac = row_factors(rng, cout, rows) * edge_weight_factor(rows, scale)
            ws = (rng.standard_normal((cout, cs)) * np.sqrt(2.0 / cs) * gac[:, None]).astype(f32)
            bs = (rng.standard_normal(cout) * 0.1 * scale * gac).astype(f32)
            sk = (rng.standard_normal((cs, oh, ow)) * scale).astype(f32)
            m = np.concatenate([m, np.tile(ws, (4, 1))], axis=1)                      # one row's prescale covers both weight sets of its K axis
        st = rows_as_stored(m, precision)
        wst = torch.from_numpy(np.ascontiguousarray(st[:, :cin].reshape(4, cout, cin).transpose(2, 1, 0).reshape(cin, cout, 2, 2)))
        y = F.conv_transpose2d(xs, wst, torch.from_numpy(b.astype(np.float64)), stride=2)
        if mode == 2:
            wss = torch.from_numpy(np.ascontiguousarray(st[:cout, cin:]))[:, :, None, None]
            y = y + F.conv2d(torch.from_numpy(as_stored(sk, precision))[None], wss, torch.from_numpy(bs.astype(np.float64)))
    else:
        wst = torch.from_numpy(rows_as_stored(wt.reshape(cout, -1), precision).reshape(wt.shape))
        y = F.conv2d(xs, wst, torch.from_numpy(b.astype(np.float64)), padding=ks // 2)
    if mode != 3:
        y = ACT[act](y)
    if res_mode == 1 and mode == 0:
        y = y + rs
    elif res_mode == 2 and mode == 0:
        y = y * rs + rs
    ref = y[0].numpy()
    if mode == 2:
        got = lib.op_conv2d(x, np.concatenate([wt.ravel(), ws.ravel()]), np.concatenate([b, bs]), mode=2, res=sk, res_mode=cs, precision=precision)
    elif mode == 3:
        got = lib.op_conv2d(x, wt, b, ks=3, mode=3, precision=precision, tile=tile)
    else:
        got = lib.op_conv2d(x, wt, b, ks=ks, mode=mode, act=act, res=res, res_mode=res_mode if mode == 0 else 0, precision=precision, tile=tile,
                            bk=bk, nsplit=nsplit)
    what = f"conv {cin}->{cout} {h}x{w} k{ks} mode {mode} act {act} res {res_mode} prec {precision} tile {tile} nsplit {nsplit} {rows} x{scale}"
    return _judge(got, ref, precision, BAR_X3 if precision == 1 else BAR_F16, rows, scale, mode != 3, what)


def upconv_stage(rng, cin, cm, cout, cs, h, w, rows, scale):
    """operands of one composed stage (tests/test_upconv_emulated.py make_stage's family) with a row axis and a value edge"""
    f32 = np.float32
    wmul = edge_weight_factor(rows, scale)
    f3 = row_factors(rng, cout, rows if rows != "spread_cm" else "uniform") * (wmul if rows != "spread_cm" else 1)
    fm = row_factors(rng, cm, "spread" if rows == "spread_cm" else "uniform") * (wmul if rows == "spread_cm" else 1)
    t = dict(x=(rng.standard_normal((cin, h, w)) * scale).astype(f32),
             wt=(rng.standard_normal((cin, cm, 2, 2)) * np.sqrt(1.0 / cin) * fm[None, :, None, None]).astype(f32),
             bt=(rng.standard_normal(cm) * 0.1 * scale * fm).astype(f32),
             w3=(rng.standard_normal((cout, cm, 3, 3)) * np.sqrt(2.0 / (9 * cm)) * f3[:, None, None, None]).astype(f32),
             b3=(rng.standard_normal(cout) * 0.1 * scale * f3).astype(f32), skip=None, ws=None, bs=None)
    if rows == "spread+dead":
        kill_rows(rng, t["w3"], axis=0)
    if cs:
        gm = row_factors(rng, cm, "spread" if rows == "spread_cm" else "uniform") * (wmul / 8 if rows == "spread_cm" else 1)   # skip part ~3 binades under x's
        t.update(skip=(rng.standard_normal((cs, 2 * h, 2 * w)) * scale).astype(f32),
                 ws=(rng.standard_normal((cm, cs)) * np.sqrt(2.0 / cs) * gm[:, None]).astype(f32),
                 bs=(rng.standard_normal(cm) * 0.1 * scale * gm).astype(f32))
    return t


def check_upconv(lib, cin, cm, cout, cs, h, w, act=1, shape=-1, nsplit=0, precision="fp16x3", rows="spread", scale=1.0, seed=0):
    """vp_op_upconv (ConvTranspose2d(k2, s2) [+ 1x1 skip link] -> 3x3 [-> GELU], composed at load) with an explicit shape / K split against
    torch fp64 evaluating the reference's three-op form on the stored inputs.  rows: "uniform" / "spread" / "spread+dead" act on the 3x3's
    output rows (w3, b3); "spread_cm" on the middle channels of the ConvTranspose and, independently, of the skip link."""
    from test_upconv_emulated import three_op_fp64

    p = 1 if precision == "fp16x3" else 0
    t = upconv_stage(np.random.default_rng(seed), cin, cm, cout, cs, h, w, rows, scale)
    stored = dict(t, x=as_stored(t["x"], p), skip=as_stored(t["skip"], p) if cs else None)
    ref = three_op_fp64(stored, act)
    got = lib.op_upconv(t["x"], t["wt"], t["bt"], t["w3"], t["b3"], skip=t["skip"], ws=t["ws"], bs=t["bs"], act=act, shape=shape, nsplit=nsplit,
                        precision=precision)
    what = f"upconv {cin}->{cm}->{cout} skip {cs} {h}x{w} shape {shape} nsplit {nsplit} {precision} {rows} x{scale}"
    return _judge(got, ref, p, BAR_X3 if p == 1 else BAR_F16_UPCONV, rows, scale, True, what)
