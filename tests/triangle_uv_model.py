"""NumPy (FP64) restatement of a triangle hit's texture coordinates and tangent frame, and the small helpers its tests share.

Input: triangles in WORLD space (the wrapper chain applied to the vertices here, in NumPy), their per-vertex coordinates, and a hit's point p and final normal n.
    w0, ub, wb = the barycentric weights of V0, V1, V2 at p, from the expressions triangle::hit interpolates the normal with
    u = w0 u0 + ub u1 + wb u2,  v likewise
    d1 = uv1 - uv0, d2 = uv2 - uv0, det = d1.u d2.v - d2.u d1.v
    T  = (d2.v E1 - d1.v E2) * (det < 0 ? -1 : 1),  E1 = V1 - V0, E2 = V2 - V0: the direction of increasing u
    Tp = T - dot(T, n) n,  tangent = unit(Tp),  bitangent = cross(n, tangent);  both zero when det == 0 or len2(Tp) is not > 0
bitangent = cross(n, tangent) is the convention of spheres and cubes, so a mirrored chart (det < 0) flips the frame's handedness relative to the chart's.
All-zero coordinates give u = v = 0 and a zero frame: "no coordinates" and "zero coordinates" are the same record."""
import numpy as np

T, RX, RY, RZ, S, M = 0, 1, 2, 3, 4, 5   # ZR_OP_*


def chain_points(points, chain):
    """object space -> world space: the forward maps of the wrappers (translate.hpp:27-29, rotate_*.hpp, scale.hpp:29-33), innermost first.
    chain = [(kind, (a0, a1, a2), ...)] outermost first, rotations as (sin, cos, 0)"""
    p = np.array(points, dtype=np.float64)
    for kind, a, *_ in reversed(list(chain)):
        x, y, z = p[..., 0].copy(), p[..., 1].copy(), p[..., 2].copy()
        s, c = a[0], a[1]
        if kind == T:
            p = p + np.asarray(a, dtype=np.float64)
        elif kind == RY:
            p[..., 0] = c * x - s * z; p[..., 2] = s * x + c * z
        elif kind == RX:
            p[..., 1] = c * y - s * z; p[..., 2] = s * y + c * z
        elif kind == RZ:
            p[..., 0] = c * x - s * y; p[..., 1] = s * x + c * y
        elif kind == S:
            p = p * np.asarray(a, dtype=np.float64)
    return p


def barycentrics(tri, p):
    """(w0, ub, wb) of the points p (N, 3) in the triangles tri (N, 3, 3): triangle.hpp:52-62"""
    v0, v1, v2 = tri[:, 0], tri[:, 1], tri[:, 2]
    normal = np.cross(v1 - v0, v2 - v0)
    area2 = (normal * normal).sum(1)
    ub = (normal * np.cross(v0 - v2, p - v2)).sum(1) / area2
    wb = (normal * np.cross(v1 - v0, p - v0)).sum(1) / area2
    return 1.0 - ub - wb, ub, wb


def triangle_uv(tri, uv, p, n):
    """tri (N, 3, 3) world-space vertices, uv (N, 3, 2), p (N, 3) hit points, n (N, 3) final normals -> u (N), v (N), tangent (N, 3), bitangent (N, 3)"""
    tri = np.asarray(tri, dtype=np.float64); uv = np.asarray(uv, dtype=np.float64)
    p = np.asarray(p, dtype=np.float64); n = np.asarray(n, dtype=np.float64)
    w0, ub, wb = barycentrics(tri, p)
    u = w0 * uv[:, 0, 0] + ub * uv[:, 1, 0] + wb * uv[:, 2, 0]
    v = w0 * uv[:, 0, 1] + ub * uv[:, 1, 1] + wb * uv[:, 2, 1]
    d1, d2 = uv[:, 1] - uv[:, 0], uv[:, 2] - uv[:, 0]
    det = d1[:, 0] * d2[:, 1] - d2[:, 0] * d1[:, 1]
    e1, e2 = tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0]
    t = (d2[:, 1, None] * e1 - d1[:, 1, None] * e2) * np.where(det < 0, -1.0, 1.0)[:, None]
    tp = t - (t * n).sum(1)[:, None] * n
    l2 = (tp * tp).sum(1)
    ok = (det != 0) & (l2 > 0)
    tangent = np.where(ok[:, None], tp / np.sqrt(np.where(ok, l2, 1.0))[:, None], 0.0)
    bitangent = np.where(ok[:, None], np.cross(n, tangent), 0.0)
    return u, v, tangent, bitangent


def closest_triangles(tris, rays, tmin=0.001, eps=1e-9):
    """Brute-force closest hit of rays (N, 6) on world-space triangles (K, 3, 3).  Returns (t (N), cand (N, K) bool): the distance of the closest triangle whose
    plane point lies inside it (barycentrics >= -eps) and every triangle that shares that distance within eps — the two sides of an edge, the fan of a vertex.
    t = inf where nothing is hit."""
    tris = np.asarray(tris, dtype=np.float64); rays = np.asarray(rays, dtype=np.float64)
    o, d = rays[:, None, :3], rays[:, None, 3:]
    v0, v1, v2 = tris[None, :, 0], tris[None, :, 1], tris[None, :, 2]
    nrm = np.cross(v1 - v0, v2 - v0)
    with np.errstate(divide="ignore", invalid="ignore"):
        t = ((v0 - o) * nrm).sum(2) / (d * nrm).sum(2)
        p = o + t[..., None] * d
        area2 = (nrm * nrm).sum(2)
        ub = (nrm * np.cross(v0 - v2, p - v2)).sum(2) / area2
        wb = (nrm * np.cross(v1 - v0, p - v0)).sum(2) / area2
    w0 = 1.0 - ub - wb
    inside = np.isfinite(t) & (t > tmin) & (w0 >= -eps) & (ub >= -eps) & (wb >= -eps)
    tt = np.where(inside, t, np.inf)
    best = tt.min(1)
    cand = inside & (tt <= best[:, None] + eps * np.maximum(1.0, np.abs(best[:, None])))
    margin = np.where(inside, np.minimum(np.minimum(w0, ub), wb), np.inf)   # how far inside: ~0 on an edge
    return best, cand, margin


def image_value_u8(texels, u, v):
    """texture::value of an 8-bit image (texture.hpp:50-78 as the device restates it): texels (h, w, 3) uint8; u wraps, v clamps; nearest texel, (1 / 255) * byte"""
    h, w = texels.shape[:2]
    u = u - np.floor(u)
    i = np.clip((u * w).astype(np.int64), 0, w - 1)
    j = np.clip((v * h).astype(np.int64), 0, h - 1)
    return (1.0 / 255.0) * texels[j, i].astype(np.float64)
