"""A long-double model of the texel an HDR environment map is read at (camera.hpp:828-925 get_background_color in HDR_MAP mode, texture.hpp:50-78), and
the maps, rotations and directions the lookup tests run it on (test_lookup_model.py on the CPU oracle, test_lookup_edges.py on the device).

The lookup is a nearest-texel read, so its result is a discontinuous function of the direction: a direction whose texel coordinate lies within rounding
error of a texel boundary may legitimately land on either side.  The model therefore returns, per direction, the ADMISSIBLE texel set: every texel whose
cell [i, i + 1) x [j, j + 1) meets the interval the FP64 computation's coordinate can lie in.

The interval.  With u = 2^-53 and every component of a unit vector at most 1 in magnitude, the steps before atan2 / acos err by
  normalise   x / sqrt(x x + y y + z z): the sum of squares carries 3 roundings of products and 2 of sums (relative error <= 2.5 u), the square root halves
              that and adds 0.5 u, the division adds 0.5 u: at most 3 u per component;
  a rotation  c a +- s b with c, s the FP64 cos / sin of the angle (the model uses the same two doubles, so their own rounding is no error): input errors e
              become at most (|c| + |s|) e <= 1.42 e, plus two product roundings (0.5 u each) and the sum's (0.5 u of at most 1.42): 1.42 e + 2 u;
  yaw, tilt and roll each rotate two of the three components, so every component passes through two rotations: 1.42 (1.42 * 3 u + 2 u) + 2 u = 10.9 u.
DELTA = 16 u bounds that with room for a contracted multiply-add to round differently.  Propagated:
  u  phi = atan2(z, x) moves by at most (|x| dz + |z| dx) / (x x + z z) <= 1.42 * 10.9 u / hypot(x, z) < DELTA / hypot(x, z), i.e. DELTA / hypot(x, z) * W / (2 pi)
     texels; at a pole hypot(x, z) = 0 and every column is admissible;
  v  acos is monotonic, so the interval is [acos(y + DELTA), acos(y - DELTA)] / pi * H with y +- DELTA clamped to [-1, 1] (the square-root singularity at the
     poles is in there);
  and the steps after them — atan2 / acos themselves (a few ulp), + pi, / (2 pi), u - floor(u), * W — are a few u relative to a coordinate of at most W (H):
  DELTA * W (DELTA * H) texels more.
pi is the FP64 constant 3.14159265358979323846, as in the reference.  u wraps (u = W is column 0), v clamps.

A direction with one admissible texel has a known answer; the share of directions with more than one is a property of the inputs, capped per case by
test_lookup_model.py."""
import ctypes as C
import math

import numpy as np

LD = np.longdouble
DELTA = 16.0 * 2.0 ** -53
PI = LD(3.14159265358979323846)

ROTATIONS = [(0.0, 0.0, 0.0), (0.7, -0.3, 1.9), (math.pi, math.pi / 2, -math.pi / 2)]   # (hdri_rotation, hdri_tilt, hdri_roll)
OFFSETS = [0.0, 1e-12, 1e-9, 1e-6, 1e-4, 1e-3, 5e-3, 0.015, 0.019, 0.021, 0.025, 0.05, 0.5]   # texels from a boundary, on both sides of the fast path's 0.02

# (name, width, height, texture kind of the map): ZR_TEX_IMAGE_F32 = 3, ZR_TEX_IMAGE_U8 = 2
MAPS = [("16384x4", 16384, 4, 3), ("4x16384", 4, 16384, 3), ("16385x2", 16385, 2, 3), ("2x16385", 2, 16385, 3), ("32768x2", 32768, 2, 3),
        ("1000x500", 1000, 500, 3), ("64x32", 64, 32, 3), ("3x5", 3, 5, 3), ("1x1", 1, 1, 3), ("u8_256x128", 256, 128, 2)]
N_DIRECTIONS = 200000


def _trig(angles):
    """the six FP64 coefficients the environment rotates with: cos, sin of yaw, tilt, roll"""
    return [f(a) for a in angles for f in (math.cos, math.sin)]


def texel_coordinate(dirs, width, height, angles):
    """(fu, fv, hypot(x, z), y) in long double: the texel coordinate of every direction and what its error interval needs"""
    d = np.asarray(dirs, dtype=np.float64).astype(LD)
    d = d / np.sqrt((d * d).sum(1))[:, None]
    cy, sy, cp, sp, cr, sr = [LD(t) for t in _trig(angles)]
    x, y, z = d[:, 0], d[:, 1], d[:, 2]
    x1 = cy * x + sy * z; z1 = -sy * x + cy * z
    y2 = cp * y - sp * z1; z2 = sp * y + cp * z1
    x3 = cr * x1 - sr * y2; y3 = sr * x1 + cr * y2
    fu = (np.arctan2(z2, x3) + PI) / (2 * PI) * width
    fv = np.arccos(np.clip(y3, -1, 1)) / PI * height
    return fu, fv, np.hypot(x3, z2), y3


class Admissible:
    """per direction: columns {a_u .. b_u} modulo W (every column when all_u) and rows a_v .. b_v"""

    def __init__(self, dirs, width, height, angles):
        self.width, self.height = int(width), int(height)
        fu, fv, h, y = texel_coordinate(dirs, width, height, angles)
        self.fu, self.fv = fu, fv
        with np.errstate(divide="ignore", over="ignore", invalid="ignore"):
            eu = np.where(h > 0, LD(DELTA) / np.where(h > 0, h, 1) * width / (2 * PI), np.inf) + LD(DELTA) * width
        self.all_u = ~(eu < width)          # the interval is as wide as the map (the poles)
        eu = np.where(self.all_u, 0, eu)
        self.a_u = np.floor(fu - eu).astype(np.int64); self.b_u = np.floor(fu + eu).astype(np.int64)
        self.all_u |= (self.b_u - self.a_u + 1) >= width
        ev = LD(DELTA) * height
        lo = np.arccos(np.clip(y + LD(DELTA), -1, 1)) / PI * height - ev
        hi = np.arccos(np.clip(y - LD(DELTA), -1, 1)) / PI * height + ev
        self.a_v = np.clip(np.floor(lo), 0, height - 1).astype(np.int64); self.b_v = np.clip(np.floor(hi), 0, height - 1).astype(np.int64)

    def contains(self, i, j):
        i = np.asarray(i, dtype=np.int64); j = np.asarray(j, dtype=np.int64)
        in_u = self.all_u | (np.mod(i - self.a_u, self.width) <= self.b_u - self.a_u)
        return in_u & (i >= 0) & (i < self.width) & (j >= self.a_v) & (j <= self.b_v)

    def size(self):
        nu = np.where(self.all_u, self.width, np.minimum(self.b_u - self.a_u + 1, self.width))
        return nu * (self.b_v - self.a_v + 1)

    def boundary_distance(self):
        """texels from the coordinate to the nearest texel boundary, in u (every integer: u wraps) and in v (1 .. H - 1: v clamps); inf where there is none"""
        du = np.abs(self.fu - np.round(self.fu)).astype(np.float64) if self.width > 1 else np.full(len(self.fu), np.inf)
        dv = np.abs(self.fv - np.clip(np.round(self.fv), 1, self.height - 1)).astype(np.float64) if self.height > 1 else np.full(len(self.fv), np.inf)
        return du, dv


def map_texels(width, height, kind):
    """every texel names itself: F32 (column, row, 1); U8 (column mod 256, row mod 256, 255), read back as those over 255"""
    col, row = np.meshgrid(np.arange(width), np.arange(height))
    if kind == 3:
        return np.stack([col, row, np.ones_like(col)], -1).astype(np.float32)
    return np.stack([col % 256, row % 256, np.full_like(col, 255)], -1).astype(np.uint8)


def decode(rgb, kind):
    """(column, row) from a lookup's colour at intensity 1 (for a U8 map: modulo 256)"""
    if kind == 3:
        return rgb[:, 0].astype(np.int64), rgb[:, 1].astype(np.int64)
    return np.rint(rgb[:, 0] * 255).astype(np.int64), np.rint(rgb[:, 1] * 255).astype(np.int64)


def _unrotate(t, angles):
    """directions that the environment's yaw, tilt, roll take (up to FP64 rounding) to the rows of t"""
    if tuple(angles) == (0.0, 0.0, 0.0):
        return t.copy()   # exactly, signed zeros included
    cy, sy, cp, sp, cr, sr = _trig(angles)
    x3, y3, z2 = t[:, 0], t[:, 1], t[:, 2]
    x1 = cr * x3 + sr * y3; y2 = -sr * x3 + cr * y3
    y = cp * y2 + sp * z2; z1 = -sp * y2 + cp * z2
    x = cy * x1 - sy * z1; z = sy * x1 + cy * z1
    return np.stack([x, y, z], 1)


def _sphere(fu, fv, width, height):
    phi = fu / width * 2 * np.pi - np.pi; th = np.clip(fv / height, 0, 1) * np.pi
    return np.stack([np.sin(th) * np.cos(phi), np.cos(th), np.sin(th) * np.sin(phi)], 1)


def directions(width, height, angles, n=N_DIRECTIONS, seed=7):
    """n directions (un-normalised, in world space) for a width x height map under `angles`:
      90 %  aimed at texel boundaries +- OFFSETS: a third at a column boundary (the other coordinate anywhere), a third at a row boundary, a third at a corner;
            the boundary is the first, second, middle, last-but-one or last one (column 0 and column W are the seam, row 0 and row H the poles) or any
       5 %  anywhere
       5 %  by hand: the seam from both sides (z = +-0.0 and +-tiny with x < 0), both poles, |y| on both sides of 0.999 (as a double and as the float next to it),
            the six axes
    each scaled to a length between 1e-3 and 1e3."""
    rng = np.random.default_rng(seed + 1000003 * width + 7919 * height)
    w, h = width, height

    def boundary(size, count):
        named = np.array([0, 1, size // 2, max(size - 1, 0), size])
        return np.where(rng.random(count) < 0.5, named[rng.integers(0, len(named), count)], rng.integers(0, size + 1, count))
    nb = n * 9 // 10
    off = rng.choice(OFFSETS, nb) * rng.choice([-1.0, 1.0], nb)
    off2 = rng.choice(OFFSETS, nb) * rng.choice([-1.0, 1.0], nb)
    which = rng.integers(0, 3, nb)
    fu = np.where(which != 1, boundary(w, nb) + off, rng.uniform(0, w, nb))
    fv = np.where(which != 0, boundary(h, nb) + np.where(which == 2, off2, off), rng.uniform(0, h, nb))
    parts = [_sphere(fu, fv, w, h)]
    nr = n // 20
    parts.append(_sphere(rng.uniform(0, w, nr), rng.uniform(0, h, nr), w, h))
    hand = []
    for y in (0.0, 0.3, -0.8, 0.9989, -0.9991):
        s = math.sqrt(1 - y * y)
        for z in (0.0, -0.0, 1e-300, -1e-300, 1e-17, -1e-17, 1e-9, -1e-9, 1e-5, -1e-5):
            hand.append((-s, y, z))
    f999 = float(np.float32(0.999))
    for y0 in (0.999, f999, float(np.nextafter(np.float32(0.999), np.float32(0))), float(np.nextafter(np.float32(0.999), np.float32(1)))):
        for dy in (0.0, 1e-12, -1e-12, 1e-9, -1e-9, 1e-6, -1e-6, 1e-4, -1e-4):
            for sign in (1.0, -1.0):
                y = sign * (y0 + dy); s = math.sqrt(1 - y * y)
                for a in (0.1, 2.0, -2.5):
                    hand.append((s * math.cos(a), y, s * math.sin(a)))
    for y in (1.0, -1.0):
        hand += [(0.0, y, 0.0), (-0.0, y, -0.0), (1e-17, y, 0.0), (0.0, y, -1e-17), (1e-9, y, 1e-9), (-1e-7, y, 1e-8)]
    hand += [(1, 0, 0), (-1, 0, 0), (0, 0, 1), (0, 0, -1), (1, 0, -0.0), (-1, -0.0, 0.0)]
    hand = np.array(hand, dtype=np.float64)
    parts.append(hand[np.arange(n - nb - nr) % len(hand)])
    t = np.concatenate(parts)
    length = 10.0 ** rng.uniform(-3, 3, len(t))
    length[nb + nr:nb + nr + len(hand)] = 1.0   # the first copy of every hand-placed direction as it is
    return _unrotate(t, angles) * length[:, None]


def hdr_env(capi, tex, angles, intensity=1.0):
    e = capi.Env()
    e.mode, e.hdr_texture, e.intensity = 1, int(tex), intensity   # ZR_ENV_HDR_MAP
    e.hdri_rotation, e.hdri_tilt, e.hdri_roll = angles
    return e


class TextureSet:
    """A scene of one sphere and a table of textures over one texel blob; owns the ctypes arrays its SceneDesc points into.  add_image packs U8 images at
    whatever byte the blob has reached (pad_to_odd() first puts that on an odd byte) and F32 images at the next multiple of 4."""

    def __init__(self, capi):
        self.capi = capi
        self.texs, self.mats, self.blob = [], [], bytearray()
        self.solid((0.5, 0.5, 0.5))
        self.material(0, 0)

    def solid(self, c):
        self.texs.append(self.capi.Texture(0, 0, 0, 0, 0, 0, 0, 0.0, (C.c_double * 3)(*c)))
        return len(self.texs) - 1

    def checker(self, scale, odd, even):
        self.texs.append(self.capi.Texture(1, odd, even, 0, 0, 0, 0, 1.0 / scale, (C.c_double * 3)(0, 0, 0)))
        return len(self.texs) - 1

    def raw(self, kind, width, height, offset):
        """an image record as given, for records a commit must refuse"""
        self.texs.append(self.capi.Texture(kind, 0, 0, width, height, 0, offset, 0.0, (C.c_double * 3)(0, 0, 0)))
        return len(self.texs) - 1

    def pad_to_odd(self):
        if len(self.blob) % 2 == 0:
            self.blob += b"\x5a"

    def add_image(self, texels):
        texels = np.ascontiguousarray(texels)
        assert texels.ndim == 3 and texels.shape[2] == 3 and texels.dtype in (np.uint8, np.float32)
        kind = 3 if texels.dtype == np.float32 else 2
        if kind == 3:
            self.blob += b"\xa5" * (-len(self.blob) % 4)
        offset = len(self.blob)
        self.blob += texels.tobytes()
        return self.raw(kind, texels.shape[1], texels.shape[0], offset)

    def material(self, kind, tex, param=0.0, bump=0xFFFFFFFF, strength=1.0):
        self.mats.append(self.capi.Material(kind, tex, bump, 0, param, strength, (C.c_double * 3)(1, 1, 1)))
        return len(self.mats) - 1

    @property
    def desc(self):
        capi = self.capi
        self._keep = [(C.c_double * 4)(0.0, 0.0, 0.0, 1.0), (C.c_uint32 * 1)(0), (capi.Material * len(self.mats))(*self.mats),
                      (capi.Texture * len(self.texs))(*self.texs), (C.c_ubyte * max(1, len(self.blob))).from_buffer_copy(bytes(self.blob) or b"\0")]
        d = capi.SceneDesc()
        d.spheres, d.sphere_mat, d.n_spheres = [C.cast(a, C.c_void_p) for a in self._keep[:2]] + [1]
        d.materials, d.n_materials = C.cast(self._keep[2], C.c_void_p), len(self.mats)
        d.textures, d.n_textures = C.cast(self._keep[3], C.c_void_p), len(self.texs)
        d.texels, d.texel_bytes = C.cast(self._keep[4], C.c_void_p), len(self.blob)
        return d


def environment_set(capi):
    """the texture set of the environment cases: ({map name: (texture id, width, height, kind)}, TextureSet)"""
    ts = TextureSet(capi)
    ids = {}
    for name, w, h, kind in MAPS:
        ids[name] = (ts.add_image(map_texels(w, h, kind)), w, h, kind)
    # a checker reads its even child at p = (0, 0, 0): the 64 x 32 map through a texture that is not itself an image (the FP64 path), and a plain colour
    ids["checker_of_64x32"] = (ts.checker(0.5, ts.solid((9.0, 9.0, 9.0)), ids["64x32"][0]), 64, 32, 3)
    ids["solid"] = (ts.solid((0.25, 1.5, 3.0)), 0, 0, 0)
    return ids, ts


ENV_CASES = [(name, r) for name in [m[0] for m in MAPS] + ["checker_of_64x32"] for r in range(len(ROTATIONS))]
