"""The reference's OWN demo scene code — load_materials(), sceneAssetsLoader and build_geometry() of
the reference's scene_management.hpp:28-236 — compiled twice from its own text (oracle/Makefile): against the reference headers
(oracle/_ref/zenith_ref, scene "refdemo") and, UNCHANGED, against the drop-in headers (oracle/_ref/refscene_dropin, through the
forwarding headers include/zenith/compat/ and the optional stb decode of image_texture).  The drop-in side flattens the world and
renders it with the CPU restatement; the tiles must equal the genuine reference's bit for bit.

The scene reads assets/ relative to its working directory at run time: tests/golden/refdemo_assets.py writes its images out of the committed
fixture tests/golden/refdemo_assets.npz and generates its models (the teapot, a blob missing from the reference's checkout, as a small synthetic
body; the five models that are loaded but never placed as strips with the reference files' triangle counts, which keeps the scene's RNG stream).
Runs wherever build() has made the two oracle/_ref binaries (they are compiled from the reference's text, and travel with the tree).  The mesh sits under
rotate_y, whose bounding box the reference builds with the inverse rotation (rotate_y.hpp:26-27): pixels
that see it are not reproducible even between two reference builds, so the compared tiles look elsewhere."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

BIN_REF = os.path.join(ROOT, "oracle", "_ref", "zenith_ref")
BIN_DROPIN = os.path.join(ROOT, "oracle", "_ref", "refscene_dropin")


sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
from refdemo_assets import asset_dir as _asset_dir   # (shared with tests/golden/make_golden.py, which makes the fixtures of tests/test_refdemo_gpu.py)


@pytest.mark.skipif(not (os.path.exists(BIN_REF) and os.path.exists(BIN_DROPIN)),
                    reason="needs the oracle/_ref binaries (build() makes them where the reference's text is available)")
def test_reference_scene_code_compiles_and_renders_unchanged(built, tmp_path):
    cwd = _asset_dir(str(tmp_path))
    st = json.loads(subprocess.run([BIN_DROPIN, "stats"], cwd=cwd, capture_output=True, text=True, check=True).stdout.strip().splitlines()[-1])
    # scene_management.hpp:103-236: ground + 5 prefabs + the mesh's triangles + <= 900 instances + fog
    assert st["media"] == 1 and st["warnings"] == 0 and 850 < st["spheres"] + st["cubes"] < 910 and st["triangles"] == 24 * 5 * 2
    assert st["textures"] >= 10 and st["texel_bytes"] > 1000000      # the reference's JPEG textures and bump maps, decoded through stb
    for (x0, y0, w, h) in ((40, 250, 24, 16), (500, 300, 24, 16)):   # the instance grid through the fog, left and right of the centre
        pre = os.path.join(cwd, f"ref_{x0}")
        r = subprocess.run([BIN_REF, "tile", "refdemo", str(x0), str(y0), str(w), str(h), "8", "4", pre, "0"], cwd=cwd, capture_output=True, text=True, check=True)
        ref_meta = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
        d = subprocess.run([BIN_DROPIN, "tile", str(x0), str(y0), str(w), str(h), "8", pre + "_dropin.npy"], cwd=cwd, capture_output=True, text=True, check=True)
        got_meta = json.loads([ln for ln in d.stdout.splitlines() if ln.startswith("{")][-1])
        assert (got_meta["segments"], got_meta["draws"]) == (ref_meta["segments"], ref_meta["draws"])
        ref_tile, got_tile = np.load(pre + "_mean.npy"), np.load(pre + "_dropin.npy")
        assert np.array_equal(ref_tile, got_tile), f"tile at ({x0}, {y0}): max abs diff {np.abs(ref_tile - got_tile).max()}"
        assert ref_tile.max() > 0
