"""The edge inputs of the post stack (bloom -> sharpen -> exposure + post_processor::process -> 8-bit, and analyze_framebuffer): frames, parameter
sets and cases, described once.  tests/golden/make_golden.py feeds them to the genuine post_processor / bloom_filter (`zenith_ref post_raw`) and stores
inputs and answers in tests/golden/post_edges.npz; tests/test_post_edges.py rebuilds them from here, checks that they are byte-identical to the stored
ones, and runs the CPU oracle and the device on them.

Everything here is exact arithmetic on doubles (integers, sums, products, powers of two) or correctly rounded (decimal), never a libm call, so the
frames are the same bytes wherever they are built.  Random content comes from a splitmix64 counter, not from numpy's generators.

A case of the beauty pass sees  frame * 2^exposure * exposure  (camera.hpp:741-748, color_processing.hpp:90), so NEUTRAL parameters are
exposure = 1.0f (a factor of exactly 2, frames hold half the value process() is to see), vignette 0, everything else off."""
import decimal

import numpy as np

SHAPES = [(2, 2), (2, 9), (9, 2), (3, 3), (5, 4), (255, 3), (256, 3), (257, 3), (3, 257), (64, 37)]   # (W, H)
RADII = [0, 1, 6, 300, 4096]          # fixtures; 4096 (the accepted maximum, 8193 taps per pixel) only on frames of at most MAX_PIXELS_R4096
MAX_PIXELS_R4096 = 300
SWEEP_RADII = [0, 1, 2, 3, 6, 17, 300]
SWEEP_SEEDS = [1, 2, 3]

FLOAT_FIELDS = ("exposure", "saturation", "contrast", "hue_shift", "vignette_intensity", "bloom_threshold", "bloom_intensity")


def f32(v):
    """the float the C ABI's field holds, as a Python float"""
    return float(np.float32(v))


def uniform(seed, n):
    """n doubles in [0, 1) with 53 random bits each: splitmix64 of (seed, index)"""
    base = np.uint64((int(seed) * 0xD1342543DE82EF95) & 0xFFFFFFFFFFFFFFFF)
    with np.errstate(over="ignore"):
        z = (np.arange(1, n + 1, dtype=np.uint64) + base) * np.uint64(0x9E3779B97F4A7C15)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        z = z ^ (z >> np.uint64(31))
    return (z >> np.uint64(11)).astype(np.float64) * 2.0 ** -53


def params(**kw):
    """a full parameter set (the keywords of capi.PostParams.defaults); unnamed fields are NEUTRAL"""
    p = dict(exposure=1.0, saturation=1.0, contrast=1.0, hue_shift=0.0, vignette_intensity=0.0, bloom_threshold=1.0, bloom_intensity=0.3, bloom_radius=4,
             color_balance=[1.0, 1.0, 1.0], sharpen_amount=0.2, use_aces_tone_mapping=0, use_bloom=0, use_sharpening=0, debug=[0, 0, 0, 0, 0])
    for k, v in kw.items():
        if k not in p:
            raise KeyError(k)
        p[k] = v
    for k in FLOAT_FIELDS:
        p[k] = f32(p[k])
    return p


def ref_arguments(p, is_data_pass, apply_gamma):
    """the 22 parameters of `zenith_ref post_raw`; floats in hexadecimal, so they arrive exactly"""
    a = [float(p[k]).hex() for k in FLOAT_FIELDS] + [str(int(p["bloom_radius"]))] + [float(x).hex() for x in p["color_balance"]]
    a += [float(p["sharpen_amount"]).hex(), str(int(p["use_aces_tone_mapping"])), str(int(p["use_bloom"])), str(int(p["use_sharpening"]))]
    return a + [str(int(x)) for x in p["debug"]] + [str(int(is_data_pass)), str(int(apply_gamma))]


# ---- frames ------------------------------------------------------------------------------------------------------------------
def shape_frame(W, H, seed=0):
    """Dim content (multiples of 1/4096 in [0.02, 0.35): below the bloom threshold of SHAPE_PARAMS after exposure) with bright pixels in two opposite
    corners, on two edges, in the interior position (1, 1) where there is one, and on both sides of flat index 256 where the frame is that long."""
    n = W * H
    u = uniform(1000 + seed, n * 3).reshape(H, W, 3)
    f = (np.floor(u * 1350.0) + 82.0) / 4096.0
    bright = np.array([[5.0, 2.5, 6.5], [0.5, 4.0, 1.0], [3.0, 3.0, 3.0], [9.0, 0.25, 0.5]]) * (1.0 + 0.125 * seed)
    spots = [(0, 0), (W - 1, H - 1), (W // 2, 0), (0, H // 2)]
    if W >= 3 and H >= 3:
        spots.append((1, 1))
    if n > 257:
        spots += [(255 % W, 255 // W), (256 % W, 256 // W)]
    for k, (x, y) in enumerate(spots):
        f[y, x] = bright[k % len(bright)]
    return f


SHAPE_PARAMS = dict(exposure=0.5, vignette_intensity=1.0, use_bloom=1, bloom_threshold=0.8, bloom_intensity=0.45, use_sharpening=1, sharpen_amount=0.25)

# colours process() is to see (the frame holds half of each): primaries, secondaries, two-channel ties at the top and at the bottom, grey, a colour whose
# max - min is one part in 10^7, black, a grey below the luma gate of 0.0001, one HDR colour
GATE_COLOURS = [(1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 0), (0, 1, 1), (1, 0, 1), (0.5, 0.5, 0.125), (0.25, 0.75, 0.75), (0.625, 0.125, 0.625), (0.75, 0.25, 0.25),
                (0.5, 0.5, 0.5), (0.5, 0.5, 0.5 + 5e-8), (0, 0, 0), (1e-5, 1e-5, 1e-5), (7.5, 2.0, 0.3125), (0.125, 0.5, 0.25)]
GATE_CONTRASTS = [1.0, 1.001, 1.0011]
GATE_SATURATIONS = [1.0, 1.001, 1.0011, 0.0, 2.0, -1.0]
GATE_HUES = [0.0, 0.001, 0.0011, -0.0011, 60.0, 120.0, 180.0, 300.0, 359.999, 360.0, -360.0, 720.0, -719.9]

BANDS = [0.02, 0.10, 0.40, 0.70, 0.95, 1.0]       # apply_debug_view's luminance bands (color_processing.hpp:243-264)
POISONS = [("pinf", np.inf), ("ninf", -np.inf), ("nan", np.nan), ("huge", 1e300), ("denormal", 1e-320), ("negzero", -0.0)]
THRESHOLD = 0.75                                   # the bloom threshold of the threshold cases: exact in float and in double


def gate_frame():
    return (np.array(GATE_COLOURS, dtype=np.float64) * 0.5).reshape(2, 8, 3)


def _byte_edges(gamma):
    """for k = 1..255 the inputs just below and just above the value whose byte is k: (k / 255.999)^2.2 (1 -+ 1e-12) through the gamma curve,
    k / 255.999 (1 -+ 1e-12) without it; correctly rounded.  Returns (values[510], expected bytes[510])."""
    ctx = decimal.Context(prec=50)
    vals, want = [], []
    for k in range(1, 256):
        t = ctx.divide(decimal.Decimal(k), decimal.Decimal("255.999"))
        if gamma:
            t = ctx.power(t, decimal.Decimal("2.2"))
        for s, b in ((-1, k - 1), (1, k)):
            vals.append(float(ctx.multiply(t, decimal.Decimal(1) + s * decimal.Decimal("1e-12"))))
            want.append(b)
    return np.array(vals, dtype=np.float64), np.array(want, dtype=np.uint8)


def byte_frame(gamma, scale=1.0):
    """510 edge values as the channels of 170 pixels (17 x 10), times `scale` (0.5 for the beauty pass at exposure 1)"""
    v, _ = _byte_edges(gamma)
    return (v * scale).reshape(10, 17, 3)


def byte_expected(gamma):
    return _byte_edges(gamma)[1].reshape(10, 17, 3)


def band_frame():
    """greys that process() sees at each band edge times (1 -+ 1e-9)"""
    g = np.array([b * s for b in BANDS for s in (1.0 - 1e-9, 1.0 + 1e-9)], dtype=np.float64) * 0.5
    return np.repeat(g[:, None], 3, axis=1).reshape(2, 6, 3)


def band_expected():
    """the debug colour of each pixel of band_frame() as bytes: below / above each of the six edges"""
    cols = [(0.1, 0.0, 0.2), (0.0, 0.0, 1.0), (0.0, 0.5, 0.0), (0.5, 0.5, 0.5), (1.0, 1.0, 0.0), (1.0, 0.0, 0.0), (1.0, 1.0, 1.0)]
    ctx = decimal.Context(prec=50)

    def byte(c):
        return 0 if c == 0 else int(decimal.Decimal("255.999") * ctx.power(decimal.Decimal(repr(c)), decimal.Decimal(1) / decimal.Decimal("2.2")))
    out = [[byte(c) for c in cols[i + j]] for i in range(6) for j in (0, 1)]
    return np.array(out, dtype=np.uint8).reshape(2, 6, 3)


def threshold_frame():
    """7 x 3, dark but for three greys on row 1 whose float luminance after exposure 1 is the float below THRESHOLD, THRESHOLD itself, the float above"""
    f = np.full((3, 7, 3), 0.03125)
    t = np.float32(THRESHOLD)
    for x, lum in zip((1, 3, 5), (np.nextafter(t, np.float32(0)), t, np.nextafter(t, np.float32(2)))):
        f[1, x] = float(lum) * 0.5
        e = f[1, x] * 2.0
        assert np.float32(0.2126 * e[0] + 0.7152 * e[1] + 0.0722 * e[2]) == lum
    return f


def signed_frame():
    """6 x 5 with values in [-1, 2): negative pixels for the sharpener"""
    return np.floor(uniform(77, 90) * 3072.0).reshape(5, 6, 3) / 1024.0 - 1.0


def vignette_frame():
    """5 x 4 bright greys: at intensity 2 the corners (distance 0.707 from the centre) clamp to zero"""
    return (np.floor(uniform(78, 60) * 256.0).reshape(4, 5, 3) + 128.0) / 1024.0


def poison_frame(value):
    """11 x 7 of finite content in [0, 1.5) (some of it above the bloom threshold) with `value` in one channel of three pixels, a different channel each"""
    f = np.floor(uniform(79, 231) * 1536.0).reshape(7, 11, 3) / 1024.0
    for c, (x, y) in enumerate([(1, 1), (5, 3), (9, 5)]):
        f[y, x, c] = value
    return f


def grey(lums):
    l = np.asarray(lums, dtype=np.float64)
    return np.repeat(l[:, None], 3, axis=1).reshape(1, -1, 3)


def loguniform_frame(n, seed):
    """n pixels with luminances spread over 2^-12 .. 2^11, colours not grey (channels are multiples of 1/256 of a power of two: the fixture stays small)"""
    u = uniform(seed, n * 4).reshape(n, 4)
    scale = 2.0 ** (np.floor(u[:, 0] * 24.0) - 12.0)
    return ((np.floor(u[:, 1:] * 256.0) / 256.0 + 0.5) * scale[:, None]).reshape(1, n, 3)


def bin_edge_luminances():
    """2^k (1 - 1e-4), 2^k, 2^k (1 + 1e-4) for k = -14..12: a grey of luminance 2^k has exactly that float luminance, and 2^k is where
    (log2 + 10) / 20 * 255 crosses an integer for k = -10, 10 and the clamps"""
    return np.array([2.0 ** k * s for k in range(-14, 13) for s in (1.0 - 1e-4, 1.0, 1.0 + 1e-4)], dtype=np.float64)


def stat_frames():
    """frames for analyze_framebuffer alone, (1, n, 3): name -> frame"""
    f = {}
    for n in (1, 5, 255, 256, 257, 513):
        f[f"count{n}"] = loguniform_frame(n, 300 + n)
    f["bin_edges"] = grey(bin_edge_luminances())
    f["specials"] = grey([0.0, -1.0, -0.0, 1e-4, 9.9e-5, 1e30])
    f["all_negative"] = -loguniform_frame(300, 91)            # more than one block, the first one full: the maximum stays at 0
    mixed = loguniform_frame(260, 92)                         # non-finite luminances among finite ones, in both blocks
    mixed[0, 3] = [np.inf, 0.5, 0.5]; mixed[0, 100] = [0.5, -np.inf, 0.5]; mixed[0, 200] = [0.5, 0.5, np.nan]
    mixed[0, 257] = [np.inf, np.inf, np.inf]; mixed[0, 258] = [np.inf, -np.inf, 0.0]; mixed[0, 259] = [-np.inf, 0.0, 0.0]
    f["nonfinite"] = mixed
    f["one_pinf"] = grey([np.inf]); f["one_nan"] = grey([np.nan]); f["one_ninf"] = grey([-np.inf])
    for name, fr in f.items():
        assert fr.shape[0] == 1 and fr.shape[2] == 3, name
    e = bin_edge_luminances()[1::3]
    assert np.array_equal((0.2126 * e + 0.7152 * e + 0.0722 * e).astype(np.float32), e.astype(np.float32))   # the exact powers stay exact
    return f


def post_frames():
    """frames of the post-stack cases, (H, W, 3) with W, H >= 2: name -> frame"""
    f = {f"shape_{W}x{H}": shape_frame(W, H) for W, H in SHAPES}
    f["gates"] = gate_frame()
    f["bytes_gamma"] = byte_frame(True); f["bytes_gamma_half"] = byte_frame(True, 0.5)
    f["bytes_linear"] = byte_frame(False)
    f["bands"] = band_frame()
    f["threshold"] = threshold_frame()
    f["signed"] = signed_frame()
    f["vignette"] = vignette_frame()
    for name, v in POISONS:
        f["poison_" + name] = poison_frame(v)
    return f


# ---- cases --------------------------------------------------------------------------------------------------------------------
def cases():
    """every post-stack case: (name, frame name, parameters, is_data_pass, apply_gamma)"""
    c = []

    def add(name, frame, p, data=False, gamma=True):
        c.append((name, frame, p, bool(data), bool(gamma)))
    for W, H in SHAPES:
        for r in RADII:
            if r == 4096 and W * H > MAX_PIXELS_R4096:
                continue
            add(f"shape_{W}x{H}_r{r}", f"shape_{W}x{H}", params(bloom_radius=r, **SHAPE_PARAMS))
    for r in (0, 1):    # an intensity of 4e6 turns the one float spacing above the threshold into a visible overlay
        add(f"threshold_r{r}", "threshold", params(use_bloom=1, bloom_threshold=THRESHOLD, bloom_intensity=4.0e6, bloom_radius=r))
    for tag, amount in (("zero", 0.0), ("negative", -0.5), ("above_one", 1.75)):
        add(f"sharpen_{tag}", "signed", params(use_sharpening=1, sharpen_amount=amount))
    for v in (0.0, 1.0, 2.0):
        add(f"vignette_{v:g}", "vignette", params(vignette_intensity=v))
    for tag, dbg in (("red", [1, 0, 0, 0, 0]), ("green", [0, 1, 0, 0, 0]), ("blue", [0, 0, 1, 0, 0]), ("luminance", [0, 0, 0, 1, 0]), ("bvh", [0, 0, 0, 0, 1]),
                     ("luminance_red", [1, 0, 0, 1, 0])):
        add(f"debug_{tag}", "gates", params(debug=dbg))
    for ci, con in enumerate(GATE_CONTRASTS):
        for si, sat in enumerate(GATE_SATURATIONS):
            for hi, hue in enumerate(GATE_HUES):
                add(f"gate_c{ci}_s{si}_h{hi}", "gates", params(contrast=con, saturation=sat, hue_shift=hue))
    add("bytes_data_gamma", "bytes_gamma", params(), data=True, gamma=True)
    add("bytes_data_linear", "bytes_linear", params(), data=True, gamma=False)
    add("bytes_gamma_frame_data_linear", "bytes_gamma", params(), data=True, gamma=False)
    add("bytes_beauty", "bytes_gamma_half", params())
    add("bands", "bands", params(debug=[0, 0, 0, 1, 0]))
    for name, _ in POISONS:
        for aces in (0, 1):
            for hsv in (0, 1):
                for bloom in (0, 1):
                    p = params(use_aces_tone_mapping=aces, use_bloom=bloom, bloom_threshold=0.8, bloom_intensity=0.5, bloom_radius=2,
                               saturation=1.3 if hsv else 1.0, hue_shift=40.0 if hsv else 0.0, exposure=0.25)
                    add(f"poison_{name}_a{aces}_h{hsv}_b{bloom}", "poison_" + name, p)
        add(f"poison_{name}_data_gamma", "poison_" + name, params(), data=True, gamma=True)
        add(f"poison_{name}_data_linear", "poison_" + name, params(), data=True, gamma=False)
    assert len({n for n, *_ in c}) == len(c)
    return c


# cases whose bytes are known without the reference: name -> expected image.  A broken fixture cannot pass these.
def known_bytes():
    return {"bytes_data_gamma": byte_expected(True), "bytes_data_linear": byte_expected(False), "bytes_beauty": byte_expected(True), "bands": band_expected()}


def sweep_cases(W, H, seed):
    """the generated device-against-oracle sweep on one frame: radii x bloom on / off x sharpening on / off"""
    for r in SWEEP_RADII:
        for bloom in (1, 0):
            for sharpen in (1, 0):
                p = dict(SHAPE_PARAMS, use_bloom=bloom, use_sharpening=sharpen, bloom_radius=r, use_aces_tone_mapping=(r + seed) % 2,
                         saturation=1.0 if seed == 1 else 1.25)
                yield f"r{r}_bloom{bloom}_sharpen{sharpen}", params(**p)


def first_difference(got, want, frame):
    """what a failure message needs: the first differing pixel, its channel, the input there and both outputs; None if equal"""
    got, want = np.asarray(got), np.asarray(want)
    if got.shape != want.shape:
        return f"shape {got.shape} against {want.shape}"
    bad = np.argwhere(got != want)
    if not len(bad):
        return None
    y, x, ch = (int(v) for v in bad[0])
    return (f"{len(bad)} of {want.size} bytes differ; first at pixel (x={x}, y={y}) channel {ch}: input {frame[y, x].tolist()!r}, "
            f"got {got[y, x].tolist()} want {want[y, x].tolist()}")
