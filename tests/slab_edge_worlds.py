"""Worlds that drive EXTEND's box tests to their edges through the real builders and the real kernel (a helper of tests/test_slab_edges.py: no tests here).

The FP32 box tests decide which primitives are asked at all, so a box test that is wrong for one ray drops a hit silently.  These worlds put real trees where
the box arithmetic is under most strain, with rays whose answers are known without a tracer: triangle worlds through tests/triangle_edge_worlds.py's exact
classifier (fractions.Fraction over the double inputs: `tw.answers`), the sphere world by construction.

  S1  offset lattice    class A's cells (triangle_edge_worlds.lattice) translated to 2^20 (the 2^-4 lattice) and to 2^24 (the unit lattice): vertices that no float
                        holds, so both builders must round every box outwards.  Every ray from inside its cell, where every determinant is exact, and every sixteenth
                        also from 2^24 direction vectors further back (exactly representable: t grows by 2^24).
  S2  mixed scale       a fan of 196 triangles with 2^-10 legs beside two 2^20 ground triangles and one triangle out at 2^30: on a node's 8-bit grid the small
                        ones fill single cells.  Rays are aimed at lattice points of the small triangles (interior, edges, vertices, one step outside) from 1, 2
                        and 1024 direction vectors above; what misses the fan meets the ground.  Also as placed runs (fan, ground, outlier: one run each).
  S3  directions        class A+0's rays with a zero component as +0 and as -0 (rays along lattice planes), and rays with d scaled by 2^60 and by 2^-20.
                        triangle_t's parallel test det^2 < 1e-16 |N|^2 is not scale-free in d: far below |d| = 1e-8 every triangle is a miss and a world would
                        test nothing, so 2^-20 it is.
  S4  overflow          40 spheres of radius 1e11 on a 1e12 lattice out to 1e14, each with a material of its own, no two in one row, column or file.  One ray
                        per sphere aimed at its centre from 1e13 away, its largest |d_k| between 1e-23 and 1e-27, a second component 1e-3 of that, the third
                        3e-4 of it or exactly 0: |plane| / |d_k| is 1e37 ... 1e41 and more, t = (distance - r) / |d| runs from 1e36 to 1e40, on both sides of
                        the float range.  Triangles cannot reach this class (the parallel test again).  Miss rays pass between the spheres.
                        From 1e13 away |o / d_k| itself passes 2^120 and the axis is dropped for that alone; so each sphere also gets a ray from beside the
                        world's origin (|o| <= 4e6, largest |d_k| 1e-25 ... 1e-27), where only the plane products leave the float range.
"""
import numpy as np

import builder_worlds as bw
import triangle_edge_worlds as tw


FAR_EVERY = 16   # every sixteenth ray also from far away: the exact classifier works its longest on those


def offset_lattice(k, shift_exp, seed=11):
    """S1: lattice(k) translated by 2^shift_exp on every axis; labels["near"]: the origin lies inside the ray's cell"""
    a = tw.lattice(k, seed)
    T = np.full(3, 2.0 ** shift_exp)
    tv = a.tri_v + np.tile(T, 3)
    near = a.all.copy()
    near[:, :3] += T
    far = near[::FAR_EVERY].copy()
    far[:, :3] -= 2.0 ** 24 * far[:, 3:]
    assert np.array_equal(far[:, :3] + 2.0 ** 24 * far[:, 3:], near[::FAR_EVERY, :3])   # exactly representable
    labels = {n: np.concatenate([v, v[::FAR_EVERY]]) for n, v in a.labels.items()}
    labels["near"] = np.concatenate([np.ones(len(near), bool), np.zeros(len(far), bool)])
    w = tw._world(f"S1{k:+d}@2^{shift_exp}", tv, a.tri_n, a.tri_cell, np.concatenate([near, far]), np.concatenate([a.ray_cell, a.ray_cell[::FAR_EVERY]]), labels)
    w.scale = a.scale
    return w


S2_POINTS = ((1, 1), (2, 1), (2, 0), (0, 2), (2, 2), (0, 0), (4, 0), (0, 4), (-1, 1), (1, -1), (3, 2))   # interior, edges, vertices, one step outside each edge
S2_BACK = (1, 2, 1024)


def mixed_scale(seed=21):
    """S2: cell 0 = the fan (legs 4 h, h = 2^-12, on a 14 x 14 raster of pitch 8 h around (1, 1, 1)), cell 1 = the ground (y = 0, 2^20 across), cell 2 = the outlier"""
    rng = np.random.default_rng([seed])
    h = 2.0 ** -12
    tv, cell, rays, ray_cell, lab_point, lab_back = [], [], [], [], [], []
    for i in range(14):
        for j in range(14):
            v0 = np.array([1.0 + 8 * h * i, 1.0, 1.0 + 8 * h * j])
            g1, g2 = h * np.array([1.0, (i + j) % 3 - 1, 0.0]), h * np.array([0.0, (2 * i + j) % 3 - 1, 1.0])
            t = np.array([v0, v0 + 4 * g1, v0 + 4 * g2])
            if (i + j) % 2:
                t, g1, g2 = t[[0, 2, 1]], g2, g1
            tv.append(t.reshape(9))
            cell.append(0)
            for n, (a, b) in enumerate(S2_POINTS):
                P = t[0] + a * g1 + b * g2
                dv = h * np.array([rng.integers(-1, 2), -3.0, rng.integers(-1, 2)]) * int(rng.integers(1, 4))
                back = S2_BACK[(i + j + n) % 3]
                rays.append(np.concatenate([P - back * dv, dv]))
                ray_cell.append(0); lab_point.append(n); lab_back.append(back)
    S = 2.0 ** 19
    tv += [np.array([-S, 0, -S, S, 0, -S, -S, 0, S]), np.array([S, 0, -S, S, 0, S, -S, 0, S])]
    cell += [1, 1]
    far = 2.0 ** 30
    tv.append(np.array([far, far, far, far + 1, far, far, far, far, far + 1]))
    cell.append(2)
    tv = np.array(tv)
    w = tw._world("S2", tv, tw._normals(rng, tv, 0.15), cell, np.array(rays), ray_cell, {"point": np.array(lab_point), "back": np.array(lab_back)})
    w.scale = 1.0
    return w


S2_TRANSLATE = np.array([[128.0, -64.0, 256.0]])   # one whole-number translate for every run: the placed world is the bare one moved rigidly


def direction_extremes(seed=11):
    """S3: see the module's docstring; labels["what"]: "+0", "-0" (zero components of that sign), "up" (d x 2^60), "down" (d x 2^-20)"""
    a = tw.lattice(0, seed)
    zero = np.flatnonzero((a.all[:, 3:] == 0).any(axis=1))
    plus, minus = a.all[zero].copy(), a.all[zero].copy()
    minus[:, 3:] = np.where(minus[:, 3:] == 0, -0.0, minus[:, 3:])
    up, down = a.all[1::4].copy(), a.all[3::4].copy()
    up[:, 3:] *= 2.0 ** 60
    down[:, 3:] *= 2.0 ** -20
    what = np.array(["+0"] * len(plus) + ["-0"] * len(minus) + ["up"] * len(up) + ["down"] * len(down))
    pick = np.concatenate([zero, zero, np.arange(len(a.all))[1::4], np.arange(len(a.all))[3::4]])
    labels = {n: v[pick] for n, v in a.labels.items()}
    labels["what"] = what
    w = tw._world("S3", a.tri_v, a.tri_n, a.tri_cell, np.concatenate([plus, minus, up, down]), a.ray_cell[pick], labels)
    w.scale = a.scale
    return w


class Census:
    """S4: world (a bw.World), rays, want_mat (bw.MISS for a miss ray), want_t (0 for a miss ray)"""


S4_R, S4_PITCH, S4_BACK, S4_N = 1e11, 1e12, 1e13, 40


def overflow_spheres(seed=31):
    """S4: the answer of ray k, "material want_mat[k] at t = (|c - o| - r) / |d|", follows from the construction: no two spheres share a coordinate, a ray runs
    within 1.1e10 of an axis line through its target's centre over 1e13, and every other centre is 1e12 or more from that line in both other coordinates
    (asserted below, in plain float64: the margins are ten orders of magnitude above its rounding)"""
    rng = np.random.default_rng([seed])
    n = S4_N
    cells = np.stack([rng.permutation(101)[:n] for _ in range(3)], axis=1).astype(np.float64)   # distinct on every axis
    c = cells * S4_PITCH
    spheres = np.concatenate([c, np.full((n, 1), S4_R)], axis=1)
    w = bw.World("S4", n, spheres=spheres, sphere_mat=np.arange(n), objects=bw._objects(np.full(n, bw.SPHERE), np.arange(n)))

    def ray_towards(p, k):
        axis, sign = k % 3, 1.0 if (k // 3) % 2 else -1.0
        u = np.zeros(3)
        u[axis], u[(axis + 1) % 3], u[(axis + 2) % 3] = sign, 1e-3 * (1 if k % 2 else -1), (0.0, 3e-4, -3e-4)[k % 3]
        u /= np.linalg.norm(u)
        o = p - S4_BACK * u
        return o, u * 10.0 ** -(23 + 4 * (k % 8) / 7.0) / abs(u[axis])   # the largest |d_k|: 1e-23 ... 1e-27

    rays, want_t = [], []
    for k in range(n):
        o, d = ray_towards(c[k], k)
        rays.append(np.concatenate([o, d]))
        want_t.append((np.linalg.norm(c[k] - o) - S4_R) / np.linalg.norm(d))
    miss = []
    for k in range(n):   # between the spheres: half a pitch off the target's row in both other coordinates
        axis = k % 3
        p = c[k].copy()
        p[(axis + 1) % 3] += 0.5 * S4_PITCH
        p[(axis + 2) % 3] -= 0.5 * S4_PITCH
        miss.append(np.concatenate(ray_towards(p, k)))
    # ... and from beside the world's origin, |o| <= 4e6: there |o / d_k| stays below 2^120 while |plane| / |d_k| reaches 1e39 ... 1e41, so no guard on the
    # ray alone drops the axis — the plane products themselves leave the float range.  Largest |d_k| 1e-25 ... 1e-27.  A ray is kept when every sphere but
    # its target stays 2 r from its line.
    def ray_from_origin(p, k):
        o = 1e5 * np.array([k + 1.0, -(k + 2.0), k % 5 - 2.0])
        u = (p - o) / np.linalg.norm(p - o)
        return o, u * 10.0 ** -(25 + 2 * (k % 8) / 7.0) / np.abs(u).max()

    def clear_of_all_but(ray, target):
        u = ray[3:] / np.linalg.norm(ray[3:])
        off = np.linalg.norm(np.cross(c - ray[:3], u), axis=1)
        return off[np.arange(n) != target].min() > 2 * S4_R

    origin_rays, origin_mat, origin_t = [], [], []
    for k in range(n):
        r = np.concatenate(ray_from_origin(c[k], k))
        if clear_of_all_but(r, k):
            origin_rays.append(r); origin_mat.append(k)
            origin_t.append((np.linalg.norm(c[k] - r[:3]) - S4_R) / np.linalg.norm(r[3:]))
        m = np.concatenate(ray_from_origin(c[k] + S4_PITCH * np.array([0.5, -0.5, 0.5]), k))
        if clear_of_all_but(m, -1):
            origin_rays.append(m); origin_mat.append(bw.MISS); origin_t.append(0.0)
    assert sum(x != bw.MISS for x in origin_mat) >= 30 and sum(x == bw.MISS for x in origin_mat) >= 20
    s = Census()
    s.world, s.rays = w, np.array(rays + miss + origin_rays)
    s.want_mat = np.concatenate([np.arange(n), np.full(n, bw.MISS), origin_mat]).astype(np.uint32)
    s.want_t = np.concatenate([want_t, np.zeros(n), origin_t])
    s.from_origin = np.arange(len(s.rays)) >= 2 * n
    for k, r in enumerate(s.rays[:2 * n]):   # the construction's claim: every sphere but the target stays 2 r and more from the ray's line
        u = r[3:] / np.linalg.norm(r[3:])
        off = np.linalg.norm(np.cross(c - r[:3], u), axis=1)
        others = np.arange(n) != (k if k < n else -1)
        assert off[others].min() > 2 * S4_R, (k, off[others].min())
        if k < n:
            assert off[k] < 1e-3 * S4_R
    assert (s.want_t[:n] < 3.4e38).sum() >= 5 and (s.want_t[:n] > 3.4e38).sum() >= 5   # t on both sides of the float range
    return s


def triangle_worlds():
    """name -> maker of the triangle worlds"""
    return {"S1-4@2^20": lambda: offset_lattice(-4, 20), "S1+0@2^24": lambda: offset_lattice(0, 24), "S2": mixed_scale, "S3": direction_extremes}
