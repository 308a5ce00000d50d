"""A working directory for the reference's own scene code (scene_management.hpp reads `assets/...` relative to the cwd).

Images: the four bump maps and the wood texture load_materials opens (scene_management.hpp:51-68), written out of tests/golden/refdemo_assets.npz,
which holds the reference's images at half their size re-encoded as baseline JPEG (182 KB in all instead of 900 KB).  Both binaries decode them
with the same stb code; they still decode to more than 1 MB of texels.
Models (scene_management.hpp:38-43), all generated: the teapot — the one model build_geometry places; the real teapot.obj is a blob missing from the
reference checkout (.MISSING_LARGE_BLOBS), without which the reference itself dereferences a null mesh — is a small lathe body (quads, no normals).
The other five are never placed, but loading each builds its BVH, which draws from the scene's RNG; a triangle strip with the triangle count of the
reference's file draws the same numbers, so the instance grid that follows is the reference's (with the full-size images, the world the drop-in
flattens is tests/golden/refdemo_scene.npz bit for bit).
`store()` makes the fixture from the reference's assets/ tree (build container only, like tests/golden/make_golden.py)."""
import io
import os

import numpy as np

REF = "/root/reference"
FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "refdemo_assets.npz")
IMAGES = ["bump_maps/wood_bump_map.jpg", "bump_maps/scratches_bump_map.jpg", "bump_maps/concrete_bump_map.jpg", "bump_maps/water_bump_map.jpg",
          "textures/fine-wood.jpg"]
# the models sceneAssetsLoader opens besides the teapot, with the number of triangles each of the reference's OBJ files loads as
MODEL_TRIANGLES = {"torus.obj": 1200, "bowl.obj": 20430, "cylinder.obj": 550, "pyramid.obj": 8, "torus_knot.obj": 4860}


def store(ref=REF):
    """tests/golden/refdemo_assets.npz: IMAGES at half size as baseline JPEG, quality 75, one uint8 array per file (key: path with '/' -> '__')"""
    from PIL import Image
    arrays = {}
    for rel in IMAGES:
        im = Image.open(os.path.join(ref, "assets", rel)).convert("RGB")
        im = im.resize((im.width // 2, im.height // 2), Image.LANCZOS)
        buf = io.BytesIO()
        im.save(buf, "JPEG", quality=75)
        arrays[rel.replace("/", "__")] = np.frombuffer(buf.getvalue(), dtype=np.uint8)
    np.savez_compressed(FIXTURE, **arrays)


def asset_dir(tmp, ref=None):
    """a working directory with assets/: the images written from the fixture — or, given `ref`, the reference's own full-size images, from which
    tests/golden/make_golden.py makes the refdemo fixtures of tests/test_refdemo_gpu.py — and a generated body for every model"""
    if ref:
        images = {rel: open(os.path.join(ref, "assets", rel), "rb").read() for rel in IMAGES}
    else:
        z = np.load(FIXTURE)
        images = {key.replace("__", "/"): z[key].tobytes() for key in z.files}
    for rel, data in images.items():
        path = os.path.join(tmp, "assets", rel)
        os.makedirs(os.path.dirname(path), exist_ok=True)
        with open(path, "wb") as f:
            f.write(data)
    os.makedirs(os.path.join(tmp, "assets", "models"), exist_ok=True)
    with open(os.path.join(tmp, "assets", "models", "teapot.obj"), "w") as f:   # a small lathe body: quads, no normals
        n, rings = 24, [(0.0, 0.0), (1.2, 0.0), (1.6, 0.8), (1.3, 1.6), (0.5, 2.0), (0.0, 2.1)]
        for r, y in rings:
            for k in range(n):
                a = 2 * np.pi * k / n
                f.write("v %.6f %.6f %.6f\n" % (r * np.cos(a), y, r * np.sin(a)))
        for j in range(len(rings) - 1):
            for k in range(n):
                a, b = j * n + k + 1, j * n + (k + 1) % n + 1
                f.write("f %d %d %d %d\n" % (a, b, b + n, a + n))
    for name, tris in MODEL_TRIANGLES.items():   # never placed, but loading one builds its BVH, which draws random_int once per node (bvh.hpp:17):
        with open(os.path.join(tmp, "assets", "models", name), "w") as f:   # a strip of as many triangles keeps the RNG stream, hence the world
            for k in range(tris + 2):
                f.write("v %.6f %.6f %.6f\n" % (0.1 * k, 0.1 * (k % 2), 0.01 * (k % 3)))
            for k in range(1, tris + 1):
                f.write("f %d %d %d\n" % (k, k + 1, k + 2))
    return tmp
