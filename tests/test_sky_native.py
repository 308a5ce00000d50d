"""The sky pre-pass's predicates on the host (raytracer_project_amd/csrc/zr_device.h: sphere_passed_certain, camera_ray_escapes — __host__ __device__, the very
functions the pre-pass kernel calls).  tests/native/sky_check.cpp is compiled for the host only, once with multiply-adds contracted and once without (the proof
of the predicate must not depend on how either site is contracted), and run on a million rays per set: random rays, the horizon of cfg3's ground sphere seen
from its camera's region (impact parameters r (1 +- eps), eps from 1e-16 to 1e-3: where the discriminant changes sign), direction lengths 1e-3 ... 1e3, a
sphere of radius 1e5, origins inside a sphere.  No GPU is involved."""
import json
import os
import subprocess

import pytest

from conftest import ROOT

CSRC = os.path.join(ROOT, "raytracer_project_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")

SETS = ("random", "horizon", "lengths", "radius_1e5", "inside", "clear")


@pytest.fixture(scope="module", params=["off", "fast"])
def result(request, tmp_path_factory):
    out = str(tmp_path_factory.mktemp("sky") / ("sky_check_" + request.param))
    subprocess.run([HIPCC, "-x", "hip", "--offload-host-only", "-std=c++20", "-O2", "-ffp-contract=" + request.param, "-I", CSRC, "-o", out,
                    os.path.join(ROOT, "tests", "native", "sky_check.cpp")], check=True)
    p = subprocess.run([out, "1000000"], capture_output=True, text=True)
    r = json.loads(p.stdout.strip().splitlines()[-1])
    print({k: r[k] for k in SETS})
    return p.returncode, r, p.stderr


def test_a_sphere_passed_by_is_never_hit(result):
    """ruled out => sphere_t is false for every tmax (and its discriminant negative), with zero exceptions, over every set ([rays, culled, hits, violations]); the
    grazing sets hold rays on both sides of the horizon, and each set but the inside one does contain rays the predicate rules out"""
    _, r, _ = result
    for name in SETS:
        rays, culled, hits, violations = r[name]
        assert rays >= 990000 and violations == 0, (name, r[name])
    for name in ("random", "horizon", "lengths", "radius_1e5"):
        assert r[name][1] > 0, (name, r[name])
    for name in ("horizon", "lengths", "radius_1e5"):
        assert r[name][2] > 0, (name, r[name])


def test_an_origin_inside_the_sphere_is_never_ruled_out(result):
    """from 1e-13 of the radius below the surface to the centre, spheres of radius 0.05 ... 1e5"""
    _, r, _ = result
    rays, culled, hits, _ = r["inside"]
    assert culled == 0, r["inside"]


def test_rays_that_clear_the_horizon_are_ruled_out(result):
    """not vacuous: a ray from the camera's region that clears the horizon by a relative 1e-6 or more is ruled out every time"""
    _, r, _ = result
    rays, culled, hits, _ = r["clear"]
    assert culled == rays and hits == 0 and r["clear_kept"] == 0, r["clear"]


def test_root_cases(result):
    """camera_ray_escapes on hand-made roots: escape_check.cpp's cases (a one-sphere leaf, a two-sphere leaf, an inner node, a triangle leaf, an empty world, zero
    and NaN directions) and, from cfg3's camera, a one-sphere leaf passed overhead, met lower down, and missed altogether"""
    rc, r, err = result
    assert r["root_checks"] >= 24 and r["root_failed"] == 0, err
    assert rc == 0 and r["failed"] == 0, (r, err)
