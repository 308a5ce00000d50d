"""SHADE's escape predicate on the host (raytracer_project_amd/csrc/zr_device.h: sphere_miss_certain, ray_escapes — __host__ __device__, the very functions the
lean SHADE kernel calls).  tests/native/escape_check.cpp is compiled for the host only, once with multiply-adds contracted and once without (the proof of the
predicate must not depend on how either site is contracted), and run on a million random rays per set plus the adversarial sets: origins on cfg3's ground
sphere to within a few ulps, origins in the knot's region, grazing rays from up to 1e-3 inside, direction lengths 1e-3 ... 1e3.  No GPU is involved."""
import json
import os
import subprocess

import pytest

from conftest import ROOT

CSRC = os.path.join(ROOT, "raytracer_project_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


@pytest.fixture(scope="module", params=["off", "fast"])
def result(request, tmp_path_factory):
    out = str(tmp_path_factory.mktemp("escape") / ("escape_check_" + request.param))
    subprocess.run([HIPCC, "-x", "hip", "--offload-host-only", "-std=c++20", "-O2", "-ffp-contract=" + request.param, "-I", CSRC, "-o", out,
                    os.path.join(ROOT, "tests", "native", "escape_check.cpp")], check=True)
    p = subprocess.run([out, "1000000"], capture_output=True, text=True)
    return p.returncode, json.loads(p.stdout.strip().splitlines()[-1]), p.stderr


def test_a_ruled_out_sphere_is_never_hit(result):
    """culled => sphere_t is false, with zero exceptions, over every set ([rays, culled, hits, violations])"""
    _, r, _ = result
    for name in ("random", "on_surface", "knot_region", "inside_grazing"):
        rays, culled, hits, violations = r[name]
        assert rays >= 999000 and violations == 0, (name, r[name])
    assert r["random"][1] > 0 and r["knot_region"][1] > 0   # ... and the sets do contain rays the predicate rules out


def test_outward_rays_from_the_ground_are_ruled_out_and_rays_from_inside_are_not(result):
    """not vacuous: every outward ray from the surface of cfg3's ground sphere is ruled out; a grazing ray from just inside, which leaves through the
    surface beyond 0.001, never is"""
    _, r, _ = result
    rays, culled, hits, _ = r["on_surface"]
    assert culled == rays and hits == 0 and r["outward_kept"] == 0, r["on_surface"]
    rays, culled, hits, _ = r["inside_grazing"]
    assert culled == 0 and hits == rays, r["inside_grazing"]


def test_root_cases(result):
    """ray_escapes on hand-made roots: a one-sphere leaf, a two-sphere leaf, an inner node, a triangle leaf, an empty world, zero and NaN directions"""
    rc, r, err = result
    assert r["root_checks"] >= 12 and r["root_failed"] == 0, err
    assert rc == 0 and r["failed"] == 0, (r, err)
