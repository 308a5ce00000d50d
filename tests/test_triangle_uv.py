"""Per-vertex texture coordinates of triangles, the CPU part: known answers of the NumPy model (tests/triangle_uv_model.py) worked by hand, and
the drop-in's flatten (tests/native/texcoord_flatten_check.cpp compiled against include/zenith/zenith.hpp): the OBJ reader's `vt` handling and the bulk path."""
import json
import os
import subprocess

import numpy as np
import pytest

import triangle_uv_model as tm
from conftest import ROOT

CLANGXX = "/opt/rocm/lib/llvm/bin/clang++"
UNIT = np.array([[[0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [0.0, 1.0, 0.0]]])
Z = np.array([[0.0, 0.0, 1.0]])


def _at(ub, wb):
    return (1 - ub - wb) * UNIT[:, 0] + ub * UNIT[:, 1] + wb * UNIT[:, 2]


def test_unit_right_triangle():
    """UVs (0,0), (1,0), (0,1) on the unit right triangle: u, v are the barycentrics of V1, V2; T = E1 = +x, bitangent = cross(z, x) = +y"""
    uv = np.array([[[0.0, 0.0], [1.0, 0.0], [0.0, 1.0]]])
    u, v, tan, bit = tm.triangle_uv(UNIT, uv, _at(0.25, 0.5), Z)
    assert (u[0], v[0]) == (0.25, 0.5)
    assert np.array_equal(tan, [[1.0, 0.0, 0.0]]) and np.array_equal(bit, [[0.0, 1.0, 0.0]])
    # seen from the other side the normal is -z: same tangent, opposite bitangent
    _, _, tan, bit = tm.triangle_uv(UNIT, uv, _at(0.25, 0.5), -Z)
    assert np.array_equal(tan, [[1.0, 0.0, 0.0]]) and np.array_equal(bit, [[0.0, -1.0, 0.0]])
    # a bent normal: the tangent is T made orthogonal to it
    n = np.array([[0.6, 0.0, 0.8]])
    _, _, tan, bit = tm.triangle_uv(UNIT, uv, _at(0.25, 0.5), n)
    assert np.allclose(tan, [[0.8, 0.0, -0.6]], atol=1e-15) and np.allclose(bit, np.cross(n, tan), atol=1e-15) and abs((tan * n).sum()) < 1e-15


def test_mirrored_chart():
    """u runs against x (det < 0): u = 1 - ub, and the direction of increasing u is -x.  bitangent = cross(n, tangent) = -y while v still increases along +y:
    the frame's handedness is flipped relative to the chart's"""
    uv = np.array([[[1.0, 0.0], [0.0, 0.0], [1.0, 1.0]]])
    u, v, tan, bit = tm.triangle_uv(UNIT, uv, _at(0.25, 0.5), Z)
    assert (u[0], v[0]) == (0.75, 0.5)
    assert np.array_equal(tan, [[-1.0, 0.0, 0.0]]) and np.array_equal(bit, [[0.0, -1.0, 0.0]])


def test_constant_and_degenerate_charts():
    for uv in ([[0.3, 0.7]] * 3, [[0.0, 0.0]] * 3, [[0.1, 0.2], [0.1, 0.2], [0.9, 0.4]], [[0.0, 0.0], [0.5, 0.5], [1.0, 1.0]]):
        uv = np.array([uv])
        u, v, tan, bit = tm.triangle_uv(UNIT, uv, _at(0.25, 0.5), Z)
        assert not tan.any() and not bit.any()
        assert np.isclose(u[0], 0.25 * uv[0, 0, 0] + 0.25 * uv[0, 1, 0] + 0.5 * uv[0, 2, 0])
    u, v, _, _ = tm.triangle_uv(UNIT, np.zeros((1, 3, 2)), _at(0.25, 0.5), Z)
    assert u[0] == 0 and v[0] == 0   # "no coordinates" and "zero coordinates" are the same record


def test_coordinates_outside_the_unit_square():
    uv = np.array([[[-2.0, 3.0], [2.0, 3.0], [-2.0, 7.0]]])
    u, v, tan, bit = tm.triangle_uv(UNIT, uv, _at(0.25, 0.5), Z)
    assert (u[0], v[0]) == (-1.0, 5.0)
    assert np.array_equal(tan, [[1.0, 0.0, 0.0]]) and np.array_equal(bit, [[0.0, 1.0, 0.0]])
    # the chain's scale stretches T, not the unit tangent
    tri = tm.chain_points(UNIT, [(tm.T, (1.0, 2.0, 3.0)), (tm.S, (3.0, 0.5, 2.0))])
    assert np.array_equal(tri[0], [[1.0, 2.0, 3.0], [4.0, 2.0, 3.0], [1.0, 2.5, 3.0]])
    _, _, tan, _ = tm.triangle_uv(tri, uv, tri.mean(1), Z)
    assert np.array_equal(tan, [[1.0, 0.0, 0.0]])


def test_image_lookup_rows():
    tex = np.arange(2 * 3 * 3, dtype=np.uint8).reshape(2, 3, 3)
    got = tm.image_value_u8(tex, np.array([0.0, 0.99, 1.2, -0.1]), np.array([0.0, 0.6, 2.0, -1.0]))
    assert np.array_equal(got, (1.0 / 255.0) * tex[[0, 1, 1, 0], [0, 2, 0, 2]].astype(np.float64))   # v = 0 is row 0; u wraps, v clamps


OBJ = """# corners are v/vt, v/vt/vn, negative, and one face without vt
v 0 0 0
v 2 0 0
v 2 1 0
v 0 1 0
v 0 0 1
v 2 0 1
vn 0 0 1
vt 0.125 0.25
vt 0.875 0.25
vt 0.875 0.75
vt 0.125 0.75
vt 1.5 -0.5
f 1/1 2/2 3/3
f 1/1/1 3/3/1 4/4/1
f -6/-5 -5/-4 -1/-1
f 1/1 2/2 3/3 4/4
f 1 2 6
f 1/1 2 3/3
f 5//1 6//1 3//1
"""


@pytest.fixture(scope="module")
def flatten_report(built, tmp_path_factory):
    d = tmp_path_factory.mktemp("texcoord")
    csrc = os.path.join(ROOT, "raytracer_project_amd", "csrc")
    exe, obj = str(d / "texcoord_flatten_check"), str(d / "mesh.obj")
    with open(obj, "w") as f:
        f.write(OBJ)
    cxx = CLANGXX if os.path.exists(CLANGXX) else "g++"
    subprocess.run([cxx, "-std=c++20", "-O2", "-pthread", "-ffp-contract=off", "-I", os.path.join(ROOT, "include"), "-o", exe,
                    os.path.join(ROOT, "tests", "native", "texcoord_flatten_check.cpp"), "-L", csrc, "-lzr_hip", f"-Wl,-rpath,{csrc}"], check=True)
    p = subprocess.run([exe, obj], capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stdout + p.stderr
    return json.loads(p.stdout.strip().splitlines()[-1])


def test_obj_texcoords(flatten_report):
    vt = [(np.float32(a), np.float32(b)) for a, b in ((0.125, 0.25), (0.875, 0.25), (0.875, 0.75), (0.125, 0.75), (1.5, -0.5))]
    c = lambda k: [float(vt[k][0]), 1.0 - float(vt[k][1])]   # (vt.u, 1 - vt.v): OBJ's v = 0 is the bottom of the image
    zero = [0.0, 0.0]
    want = [c(0) + c(1) + c(2),            # v/vt
            c(0) + c(2) + c(3),            # v/vt/vn
            c(0) + c(1) + c(4),            # negative indices: -5, -4, -1 of five vt lines
            c(0) + c(1) + c(3), c(1) + c(2) + c(3),   # the quad 1 2 3 4, a 2 x 1 rectangle: its diagonals are equal, s02 < s13 is false: [0, 1, 3] [1, 2, 3]
            zero * 3,                      # no vt at all
            zero * 3,                      # one corner without vt: the whole face gets zeros
            zero * 3]                      # v//vn
    assert flatten_report["tris"] == len(want)
    assert np.array_equal(np.array(flatten_report["uv"]).reshape(-1, 6), np.array(want))
    assert flatten_report["obj_sized"]


def test_flag_off_and_untextured_worlds_flatten_as_before(flatten_report):
    assert flatten_report["obj_absent_without_flag"] and flatten_report["obj_same_but_uv"]
    assert flatten_report["plain_absent"] and flatten_report["bulk_equal_plain"]


def test_bulk_path_carries_coordinates(flatten_report):
    assert flatten_report["bulk_equal_textured"] and flatten_report["bulk_uv_textured"]
