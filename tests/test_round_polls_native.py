"""The pipeline's round loop (raytracer_project_amd/csrc/zr_round_polls.h: run_round_loop, the driver stream_render runs, in both poll modes: ring indexing, which
round emptied the pools, which launches of the log belong to the rounds a caller sees, the drain switch and why a stale count may size the drain pool, the cadenced
mode's runs, cancellation) and the host's count of started work units (zr_units.h) on their own: tests/native/round_polls_check.cpp is compiled for the host with
the address and undefined-behaviour sanitizers and runs the driver against scripted devices.  No HIP, no GPU."""
import os
import subprocess

from conftest import ROOT

CSRC = os.path.join(ROOT, "raytracer_project_amd", "csrc")


def test_round_polls_against_scripted_devices(tmp_path):
    exe = str(tmp_path / "round_polls_check")
    subprocess.run(["g++", "-std=c++20", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-Wall", "-I", CSRC, "-o", exe,
                    os.path.join(ROOT, "tests", "native", "round_polls_check.cpp")], check=True)
    p = subprocess.run([exe], capture_output=True, text=True)
    assert p.returncode == 0, p.stdout + p.stderr
    assert p.stdout.strip().endswith("round polls: ok"), p.stdout
