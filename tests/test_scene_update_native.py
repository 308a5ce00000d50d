"""The CPU half of a moving world (raytracer_project_amd/csrc/zr_update.h: reverse indices, entry -> leaf primitive, the classification guard, the dirty
sets, an entry's box and record as patches) on its own: tests/native/update_check.cpp is compiled against the headers and zr_bvh.cpp with g++ — no HIP
library — and run on a seeded world that holds every stored form, chains that two entries share, chains that overlap, a sphere baked under two chains
and media with inner chains.  What must hold: the indices equal brute force; every refusal leaves the arrays untouched; and the committed arrays with the
patches applied equal, entry by entry, a fresh host commit of the moved world, with boxes that are chain_box of the fresh plan rounded outwards.
The same program is built once more with -fsanitize=address,undefined (host code only) and must run clean."""
import json
import os
import subprocess

import pytest

from conftest import ROOT

CSRC = os.path.join(ROOT, "raytracer_project_amd", "csrc")
FLAGS = ["all", "reverse", "slots", "refusals", "dirty_sets", "boxes", "records", "code", "cleared"]


def _build(tmp, name, extra):
    out = str(tmp / name)
    subprocess.run(["g++", "-std=c++20", "-O2", "-pthread", "-ffp-contract=off", *extra, "-I", CSRC, "-o", out, os.path.join(ROOT, "tests", "native", "update_check.cpp"),
                    os.path.join(CSRC, "zr_bvh.cpp")], check=True)
    return out


@pytest.fixture(scope="module")
def checkers(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("update")
    return {"plain": _build(tmp, "update_check", []),
            "sanitized": _build(tmp, "update_check_san", ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"])}


def _run(exe, seed):
    p = subprocess.run([exe, str(seed)], capture_output=True, text=True)
    assert p.returncode == 0, p.stdout + p.stderr
    assert "runtime error" not in p.stderr and "AddressSanitizer" not in p.stderr, p.stderr
    return json.loads(p.stdout.strip().splitlines()[-1])


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_update_rules_against_brute_force_and_a_fresh_commit(checkers, seed):
    got = _run(checkers["plain"], seed)
    assert got["n"] == 12 * 12 + 9 and got["dirty"] >= got["n"] // 4 and got["dirty"] <= got["movable"] < got["n"], got
    for k in FLAGS[1:]:
        assert got[k] is True, (k, got)


def test_update_rules_run_clean_under_the_sanitizers(checkers):
    got = _run(checkers["sanitized"], 1)
    assert got == _run(checkers["plain"], 1)
