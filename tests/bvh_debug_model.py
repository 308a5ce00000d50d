"""NumPy restatement of the BVH debug view (include/zr_capi.h): the reference's rule of bvh_node::hit in debug mode
(bvh.hpp:46-110, aabb.hpp:44-84) applied to the device's own trees as zr_scene_tree_boxes exports them.

The walk is written as the reference writes it — recursively, a node's box test, the edge test of a current-level node, the left subtree,
the right subtree on the interval the left one narrowed, the volume colour on the way back — so that it checks the kernel's explicit-stack
walk rather than copying it.  Every operation on a box, an edge and the thickness is the kernel's, in the same order (the kernel is built
without contraction); Python floats are IEEE doubles, np.float32 rounds like the C++ casts.
"""
import math

import numpy as np

MISS, EDGE, VOLUME, SURFACE = 0, 1, 2, 3
ROOT_BOX, NO_BOX = 0x80000000, 0xFFFFFFFF
KIND_SPHERE, KIND_TRIANGLE, KIND_CUBE, KIND_GROUP = 0, 1, 2, 6
DEFAULT_LEVEL, DEFAULT_THICKNESS = -1, 0.01   # global_settings, common.hpp:120-124

F_0_0001 = float(np.float32(0.0001))   # the f literals of bvh.hpp:58-61, promoted to double
F_0_05 = float(np.float32(0.05))
F_0_1 = float(np.float32(0.1))


def thickness(bvh_thickness, t_in):
    """perspective_thickness = bvh_thickness * (0.05f + t_in * 0.1f), evaluated in double and stored as float (bvh.hpp:66)"""
    return float(np.float32(float(np.float32(bvh_thickness)) * (F_0_05 + t_in * F_0_1)))


def debug_color(cls, depth):
    """diffuse_light colour of a frame (x 4.0f) or a volume (x 0.1f) at `depth` (bvh.hpp:77-84, 97-100)"""
    g = min(np.float32(depth) * np.float32(0.15), np.float32(1.0))
    base = (float(np.float32(0.4)), float(g), float(np.float32(1.0) - g))
    m = 4.0 if cls == EDGE else F_0_1
    return tuple(c * m for c in base)


def _inv(x):
    """1.0 / x with IEEE semantics for a zero (Python raises)"""
    if x == 0.0:
        return math.copysign(math.inf, x)
    return 1.0 / x


def at(o, d, t):
    return (o[0] + t * d[0], o[1] + t * d[1], o[2] + t * d[2])


def box_hit(lo, hi, o, d, mn, mx):
    """aabb::hit (aabb.hpp:44-66) on [mn, mx]: (hit, mn, mx)"""
    for a in range(3):
        inv = _inv(d[a])
        t0 = (lo[a] - o[a]) * inv
        t1 = (hi[a] - o[a]) * inv
        if inv < 0.0:
            t0, t1 = t1, t0
        if t0 > mn:
            mn = t0
        if t1 < mx:
            mx = t1
        if mx <= mn:
            return False, mn, mx
    return True, mn, mx


def on_edge(lo, hi, p, th):
    """aabb::is_on_edge (aabb.hpp:68-84): (near two planes, smallest | |x - plane| - th | over the six comparisons)"""
    n, margin = 0, math.inf
    for a in range(3):
        dl, dh = abs(p[a] - lo[a]), abs(p[a] - hi[a])
        margin = min(margin, abs(dl - th), abs(dh - th))
        if dl < th or dh < th:
            n += 1
    return n >= 2, margin


# ---- primitives: the distance tests of raytracer_project_amd/csrc/zr_device.h ----
def sphere_t(s, o, d, tmin, tmax):
    oc = (s[0] - o[0], s[1] - o[1], s[2] - o[2])
    a = d[0] * d[0] + d[1] * d[1] + d[2] * d[2]
    h = d[0] * oc[0] + d[1] * oc[1] + d[2] * oc[2]
    c = (oc[0] * oc[0] + oc[1] * oc[1] + oc[2] * oc[2]) - s[3] * s[3]
    disc = h * h - a * c
    if disc < 0:
        return None
    sq = math.sqrt(disc)
    root = (h - sq) / a
    if not (tmin < root and tmax > root):
        root = (h + sq) / a
        if not (tmin < root and tmax > root):
            return None
    return root


def _cross(a, b):
    return (a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0])


def _dot(a, b):
    return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]


def _sub(a, b):
    return (a[0] - b[0], a[1] - b[1], a[2] - b[2])


def triangle_t(v, o, d, tmin, tmax):
    v0, v1, v2 = tuple(v[0:3]), tuple(v[3:6]), tuple(v[6:9])
    e1, e2 = _sub(v1, v0), _sub(v2, v0)
    n = _cross(e1, e2)
    nn = _dot(n, n)
    if nn < 1e-16:
        return None
    q = _cross(d, e2)
    det = _dot(e1, q)
    if det * det < 1e-16 * nn:
        return None
    s = _sub(o, v0)
    un = _dot(s, q)
    rr = _cross(s, e1)
    vn = _dot(d, rr)
    sg = -1.0 if det < 0 else 1.0
    ad = det * sg
    un *= sg
    vn *= sg
    if un < 0 or vn < 0 or un + vn > ad:
        return None
    tt = _dot(e2, rr) / det
    if not (tmin <= tt and tt <= tmax):
        return None
    return tt


def cube_t(he, o, d, tmin, tmax):
    """cube::hit's slabs about the origin (cube.hpp:44-73)"""
    for i in range(3):
        inv = _inv(d[i])
        t0 = (-he[i] - o[i]) * inv
        t1 = (he[i] - o[i]) * inv
        if inv < 0.0:
            t0, t1 = t1, t0
        tmin = max(t0, tmin) if not math.isnan(t0) else tmin
        tmax = min(t1, tmax) if not math.isnan(t1) else tmax
        if tmax < tmin:
            return None
    return tmin


class World:
    """What the model needs of a scene: the caller's arrays (as given to zr_scene_set_*) and the exported tree boxes."""

    def __init__(self, boxes, spheres=None, tri_v=None, cubes=None, objects=None, ops=None):
        self.boxes = {int(b["id"]): b for b in boxes}
        self.spheres = spheres if spheres is not None else np.zeros((0, 4))
        self.tri_v = tri_v if tri_v is not None else np.zeros((0, 9))
        self.cubes = cubes if cubes is not None else np.zeros((0, 12))
        self.objects = objects   # (type, index, chain_first, chain_count) rows of the world list
        self.ops = ops           # (kind, a0, a1, a2) rows; only translate is supported here
        self.margin = math.inf   # smallest edge margin met by the last trace (ties of the thickness comparison)
        self.tie = False         # the last trace met a box whose interval closed exactly (mx == mn)

    def children(self, b):
        first = int(b["first"])
        return [self.boxes[i] for i in (2 * first, 2 * first + 1) if i in self.boxes]

    def _leaf(self, b, o, d, tmin, tmax, level, thick):
        rec = None
        for k in range(int(b["count"])):
            src, kind = int(b["src"][k]), int(b["kind"])
            bound = rec["t"] if rec is not None else tmax
            if kind == KIND_GROUP:
                ob = self.objects[src]
                lo_ = list(o)
                for c in range(int(ob[3])):
                    op = self.ops[int(ob[2]) + c]
                    assert int(op[0]) == 0, "the model places runs under translate only"
                    lo_ = [lo_[0] - op[1], lo_[1] - op[2], lo_[2] - op[3]]
                inner = self.tree_hit(int(b["subtree"]), tuple(lo_), d, tmin, bound, level, thick)
                if inner is not None:
                    rec = inner
                continue
            if kind == KIND_SPHERE:
                t = sphere_t(self.spheres[src], o, d, tmin, bound)
            elif kind == KIND_TRIANGLE:
                t = triangle_t(self.tri_v[src], o, d, tmin, bound)
            elif kind == KIND_CUBE:
                t = cube_t(self.cubes[src][:3], o, d, tmin, bound)
            else:
                raise NotImplementedError(f"leaf kind {kind}")
            if t is not None:
                rec = dict(t=t, cls=SURFACE, box=int(b["id"]), depth=int(b["depth"]), tree=int(b["tree"]), prim=(kind, src))
        return rec

    def node_hit(self, b, o, d, tmin, tmax, level, thick):
        """bvh_node::hit in debug mode for box `b` on (tmin, tmax]: a record dict or None"""
        lo, hi = [float(x) for x in b["lo"]], [float(x) for x in b["hi"]]
        ok, mn, mx = box_hit(lo, hi, o, d, tmin, tmax)
        if mx == mn:
            self.tie = True
        if not ok:
            return None
        depth = int(b["depth"])
        cur = bool(b["leaf"]) if level == -1 else depth == level
        if cur:
            th = thickness(thick, mn)
            e_in, m_in = on_edge(lo, hi, at(o, d, mn + F_0_0001), th)
            e_out, m_out = on_edge(lo, hi, at(o, d, mx - F_0_0001), th)
            self.margin = min(self.margin, m_in, m_out)
            if e_in or e_out:
                return dict(t=mn if e_in else mx, cls=EDGE, box=int(b["id"]), depth=depth, tree=int(b["tree"]), prim=None)
        if b["leaf"]:
            rec = self._leaf(b, o, d, tmin, tmax, level, thick)
        else:
            rec = None
            for c in self.children(b):   # left, then right on the interval the left subtree narrowed
                r = self.node_hit(c, o, d, tmin, rec["t"] if rec is not None else tmax, level, thick)
                if r is not None:
                    rec = r
        if rec is not None and cur:
            rec = dict(rec, cls=VOLUME, box=int(b["id"]), depth=depth, tree=int(b["tree"]))
        return rec

    def tree_hit(self, tree, o, d, tmin, tmax, level, thick):
        root = self.boxes.get(ROOT_BOX | tree)
        if root is None:
            return None
        return self.node_hit(root, o, d, tmin, tmax, level, thick)

    def trace(self, o, d, tmin=0.001, level=DEFAULT_LEVEL, thick=DEFAULT_THICKNESS):
        """the debug answer for one world ray: a record dict (t, cls, box, depth, tree, prim) or None on a miss"""
        self.margin, self.tie = math.inf, False
        return self.tree_hit(0, tuple(float(x) for x in o), tuple(float(x) for x in d), tmin, math.inf, level, thick)


def secondary_color(rec, surface_emission=(0.0, 0.0, 0.0)):
    """ray_color's debug branch (camera.hpp:937-953) for the one secondary ray: 0 on a miss, the emission if longer than 0.1, else 0.01"""
    if rec is None:
        return (0.0, 0.0, 0.0)
    e = surface_emission if rec["cls"] == SURFACE else debug_color(rec["cls"], rec["depth"])
    return e if math.sqrt(e[0] * e[0] + e[1] * e[1] + e[2] * e[2]) > 0.1 else (0.01, 0.01, 0.01)


def single_box_world(lo, hi):
    """a tree of one leaf (no primitives) as zr_scene_tree_boxes would export it: the root box and its left child, the same box"""
    from numpy import zeros
    dt = np.dtype([("lo", "<f4", 3), ("hi", "<f4", 3), ("id", "<u4"), ("tree", "<u4"), ("parent", "<u4"), ("depth", "<i4"), ("slot", "<u4"),
                   ("leaf", "<u4"), ("kind", "<u4"), ("count", "<u4"), ("first", "<u4"), ("subtree", "<u4"), ("src", "<u4", 4)])
    b = zeros(2, dtype=dt)
    for k in range(2):
        b[k]["lo"], b[k]["hi"] = lo, hi
    b[0]["id"], b[0]["parent"], b[0]["depth"], b[0]["first"] = ROOT_BOX, NO_BOX, 0, 0
    b[1]["id"], b[1]["parent"], b[1]["depth"], b[1]["leaf"], b[1]["count"] = 0, ROOT_BOX, 1, 1, 0
    return World(b)
