"""Inputs and models of tests/test_shade_edges.py and of the fixture tests/golden/kat_kat2.npz (scene "kat2", scenes/zr_scenes_mix.inc).

Pure Python / numpy restatements, every one in the reference's own operation order (Python floats are IEEE doubles and never fuse a multiply into an add):
the RNG contract of include/zr_rng.h and random_unit_vector (vec3.hpp:184-191), dot / unit_vector (vec3.hpp:154-171), triangle::hit's interpolated normal
(triangle.hpp:17-82), sphere::hit (sphere.hpp:18-46) and dielectric::scatter's decisions and directions (material.hpp:192-241).  tests/golden/make_golden.py
kat2_inputs() places the rays with them; the tests evaluate the fixture's records with them."""
import math
from fractions import Fraction

import numpy as np

M64 = (1 << 64) - 1
GOLDEN = 0x9E3779B97F4A7C15
KAT_SEED, KAT_PIXEL = 0x5EED3001, 0x7ACE      # oracle/ref_harness.cpp `kat <scene> hits`: ray k draws from the stream (seed, pixel, k) at draw 0
GLASS_INDEX = (1.5, 1.0, 1.0 / 1.5, 2.4)      # zr_build_kat2's four dielectrics, in order
KNIFE = ("0", "+1ulp", "-1ulp", "+2ulp", "-2ulp", "+4ulp", "-4ulp")   # threshold offsets at which the reflect / refract decision may fall either way


# ---- include/zr_rng.h ---------------------------------------------------------------------------------------------------------------------
def mix64(z):
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def stream_key(seed, pixel, sample):
    return mix64((mix64((seed + GOLDEN * (pixel + 1)) & M64) + GOLDEN * (sample + 1)) & M64)


def draw(key, k):
    """draw k = 0, 1, ... of a main stream as random_double() returns it"""
    u = float(mix64((key + GOLDEN * (k + 1)) & M64)) * 2.0 ** -64
    return 0.99999999999999988897769753748434595763683319091796875 if u >= 1.0 else u


def kat_key(row):
    return stream_key(KAT_SEED, KAT_PIXEL, row)


def random_unit_vector(key, first=0):
    """vec3.hpp:184-191 on the stream `key` from draw `first`: (the vector, draws used)"""
    k = first
    while True:
        x, y, z = (-1.0 + (1.0 - -1.0) * draw(key, k + q) for q in range(3))
        k += 3
        l2 = x * x + y * y + z * z
        if 1e-160 < l2 <= 1:
            r = 1 / math.sqrt(l2)
            return np.array([r * x, r * y, r * z]), k - first


# ---- vec3.hpp -----------------------------------------------------------------------------------------------------------------------------
def dot(u, v):
    return float(u[0]) * float(v[0]) + float(u[1]) * float(v[1]) + float(u[2]) * float(v[2])


def cross(u, v):
    return np.array([u[1] * v[2] - u[2] * v[1], u[2] * v[0] - u[0] * v[2], u[0] * v[1] - u[1] * v[0]])


def unit(v):
    ln = math.sqrt(dot(v, v))
    if ln < 1e-8:
        return np.zeros(3)
    r = 1 / ln
    return np.array([r * float(v[0]), r * float(v[1]), r * float(v[2])])


def inexact_products(u, v):
    """does any product of dot(u, v) round?"""
    return any(Fraction(float(a)) * Fraction(float(b)) != Fraction(float(a) * float(b)) for a, b in zip(u, v))


# ---- the layout of "kat2" (scenes/zr_scenes_mix.inc zr_build_kat2) ---------------------------------------------------------------------------
def at(k):
    return np.array([8.0 * (k % 10) - 36.0, 8.0 * (k // 10) - 28.0, 8.0 * ((k % 10 + k // 10) % 11) - 40.0])


BENT, FLAT, OPPOSED, CANCEL = 0, 1, 2, 3
TRI_VERTS = {FLAT: ((-1, -1, 0), (1, -1, 0), (0, 1, 0))}
TRI_NB = {BENT: (1, 0, 0), FLAT: (0, 0, 1), OPPOSED: (0.6, 0, -0.8), CANCEL: (0, 0, -1)}   # vertex B's normal; A's and C's are (0, 0, 1)


def tri_local(shape):
    v = TRI_VERTS.get(shape, ((-1, -1, 0), (1, -1, 0), (-1, 1, 0)))
    return [np.array(p, float) for p in v], [np.array([0, 0, 1.0]), np.array(TRI_NB[shape], float), np.array([0, 0, 1.0])]


def triangles():
    """cell -> (shape, form, material kind) of every triangle of kat2; form 6 is translate(rotate_y(0.5))"""
    kinds = ("lambertian", "metal", "dielectric")
    t = {3 * f + j: (BENT, f, kinds[j]) for f in range(6) for j in range(3)}
    for g in range(4):
        t[18 + 2 * g] = (FLAT, 0, "dielectric"); t[19 + 2 * g] = (FLAT, 1, "dielectric")
    t.update({26: (FLAT, 0, "metal"), 27: (FLAT, 6, "metal"), 28: (FLAT, 3, "lambertian"), 29: (FLAT, 0, "light"),
              30: (OPPOSED, 0, "metal"), 31: (OPPOSED, 1, "metal"), 32: (OPPOSED, 2, "metal"), 33: (OPPOSED, 0, "dielectric"), 34: (OPPOSED, 1, "lambertian"),
              35: (CANCEL, 0, "dielectric"), 36: (CANCEL, 1, "metal"), 37: (CANCEL, 2, "lambertian"), 59: (FLAT, 0, "none")})
    return t


SPHERE_KINDS = ("lambertian", "metal", "metal", "metal", "dielectric", "dielectric", "dielectric", "dielectric")


def spheres():
    """cell -> (material kind, under a translate?) of every sphere of kat2 with a positive radius"""
    s = {40 + 2 * m + w: (SPHERE_KINDS[m], bool(w)) for m in range(8) for w in range(2)}
    s.update({56: ("light", False), 57: ("none", False)})
    return s


def baked(cell):
    """is the object of this cell stored in world space from under wrappers (the world-space bounds apply)?"""
    t = triangles()
    return t[cell][1] != 0 if cell in t else spheres().get(cell, ("", False))[1]


def cell_of(p):
    p = np.atleast_2d(p)
    return (np.rint((p[:, 1] + 28.0) / 8.0).astype(int) * 10 + np.rint((p[:, 0] + 36.0) / 8.0).astype(int))


# ---- triangle::hit and sphere::hit, as far as the face normal ---------------------------------------------------------------------------------
def triangle_face(verts, normals, o, d):
    """triangle.hpp:17-82 -> (t, p, interpolated normal, dot(d, normal)) or None"""
    v0, v1, v2 = verts
    normal = cross(v1 - v0, v2 - v0)
    ln = math.sqrt(dot(normal, normal))
    un = (1 / ln) * normal
    nd = dot(un, d)
    if abs(nd) < 1e-8:
        return None
    t = (dot(un, v0) - dot(un, o)) / nd
    p = o + t * d
    c0, c1, c2 = cross(v1 - v0, p - v0), cross(v2 - v1, p - v1), cross(v0 - v2, p - v2)
    if dot(normal, c0) < 0 or dot(normal, c1) < 0 or dot(normal, c2) < 0:
        return None
    area = dot(normal, normal)
    u, v = dot(normal, c2) / area, dot(normal, c0) / area
    w = 1.0 - u - v
    n = unit(w * normals[0] + u * normals[1] + v * normals[2])
    return t, p, n, dot(d, n)


def sphere_face(centre, radius, o, d):
    """sphere.hpp:18-46 for the interval (0.001, inf) -> (t, p, outward normal, dot(d, normal)) or None"""
    oc = centre - o
    a, h = dot(d, d), dot(d, oc)
    c = dot(oc, oc) - radius * radius
    disc = h * h - a * c
    if disc < 0:
        return None
    sq = math.sqrt(disc)
    root = (h - sq) / a
    if not 0.001 < root:
        root = (h + sq) / a
        if not 0.001 < root:
            return None
    p = o + root * d
    n = (1 / radius) * (p - centre)
    return root, p, n, dot(d, n)


# ---- dielectric::scatter ---------------------------------------------------------------------------------------------------------------------------
def dielectric(d, n, front, index, u):
    """material.hpp:192-241 with rec.normal = n, rec.front_face = front and the draw u: a dict of every intermediate value, the decision and both
    candidate directions (reflect: vec3.hpp:204-206, refract: vec3.hpp:209-214)"""
    ri = (1.0 / index) if front else index
    ud = unit(d)
    raw = dot(-ud, n)
    ct = min(raw, 1.0)
    st = math.sqrt(1.0 - ct * ct)
    cannot = ri * st > 1.0
    r0 = (1 - ri) / (1 + ri)
    r0 = r0 * r0
    rf = r0 + (1 - r0) * math.pow(1 - ct, 5)
    k = 2 * dot(ud, n)
    refl = ud - k * np.asarray(n, float)
    perp = ri * (ud + ct * np.asarray(n, float))
    par = -math.sqrt(abs(1.0 - dot(perp, perp))) * np.asarray(n, float)
    return {"ri": ri, "raw": raw, "ct": ct, "st": st, "ri_st": ri * st, "cannot": cannot, "rf": rf, "reflects": cannot or rf > u, "draws": 0 if cannot else 1,
            "reflect": refl, "refract": perp + par}
