"""The motion of a refit on the host (raytracer_project_amd/csrc/zr_motion.h) on its own: tests/native/motion_check.cpp is compiled against the
headers and zr_bvh.cpp with g++ exactly as tests/test_scene_update_native.py builds update_check.cpp — no HIP library — and checks: dyadic chains in every
stored form give A = M_prev M_now^-1 and Nm = (A_lin)^-T BIT-equal to hand-written matrices; random chains of up to ZR_MAX_CHAIN ops on both sides map the
new place of a point to its old one within a bound counted from the number of ops, against the same composition in long double; the cut cases are cut;
a medium reached through its inner chain, two entries over one sphere and a placed group are followed, and entries no update reaches stay STATIC.
The same program is built once more with -fsanitize=address,undefined (host code only, a stand-alone program) and must run clean."""
import json
import os
import subprocess

import pytest

from conftest import ROOT

CSRC = os.path.join(ROOT, "raytracer_project_amd", "csrc")
FLAGS = ["updates", "dyadic", "sharing", "cut", "random"]


def _build(tmp, name, extra):
    out = str(tmp / name)
    subprocess.run(["g++", "-std=c++20", "-O2", "-pthread", "-ffp-contract=off", *extra, "-I", CSRC, "-o", out, os.path.join(ROOT, "tests", "native", "motion_check.cpp"),
                    os.path.join(CSRC, "zr_bvh.cpp")], check=True)
    return out


@pytest.fixture(scope="module")
def checkers(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("motion")
    return {"plain": _build(tmp, "motion_check", []),
            "sanitized": _build(tmp, "motion_check_san", ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"])}


def _run(exe, seed):
    p = subprocess.run([exe, str(seed)], capture_output=True, text=True)
    assert p.returncode == 0, p.stdout + p.stderr
    assert "runtime error" not in p.stderr and "AddressSanitizer" not in p.stderr, p.stderr
    return json.loads(p.stdout.strip().splitlines()[-1])


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_motion_records_against_hand_written_matrices_and_long_double(checkers, seed):
    got = _run(checkers["plain"], seed)
    assert got["entries"] == 16 and got["movable"] == 14 and got["random_cases"] == 400 * 8 * 3, got
    for k in FLAGS:
        assert got[k] is True, (k, got)
    assert got["worst_over_bound"] <= 1.0, got


def test_motion_records_run_clean_under_the_sanitizers(checkers):
    got = _run(checkers["sanitized"], 1)
    assert got == _run(checkers["plain"], 1)
