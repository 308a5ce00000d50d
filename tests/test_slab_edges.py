"""EXTEND's box tests at their edges through the real builders and the real kernel, with answers known without a tracer (tests/slab_edge_worlds.py).

The FP32 box tests (zr_device.h: ZR_RAY_CONSTANTS / ZR_FBOX / ZR_SLAB / ZR_QNODE) decide which primitives stream_extend asks at all; tests/test_slab_native.py
judges that arithmetic on the host.  Here the trees are the builders' own and the kernel is the compiled one: a hit the box tests drop shows as a decided ray
that misses.

  CPU  test_triangle_worlds_are_decided      undecided share <= 1/3 per triangle world (class B's cap); S1's rays from inside their cells are all decided
       test_oracle_answers_the_sphere_census  S4's answers are right before any GPU is asked: the oracle names every sphere, t to 1e-9, and misses every miss ray
  GPU  test_worlds_target_what_they_claim    from the committed trees: every world has grid nodes below the root; S2 has a node whose children differ by >= 2^20
       test_decided_rays                     S1 - S3 (S2 also as placed runs), both builders, ZR_EXTEND_LEVEL 0 - 3, EXTEND and the pair walk: test_triangle_edges'
                                             check_decided on every decided ray, none excluded; EXTEND and the pair walk name the same triangle where the winner is unique
       test_sphere_census                    S4, both builders, every level, both engines and zr_kat_shade_lean: the material equal, rel_err(t) < 1e-9
Before the limit on |1 / d| followed the world's size S4's hits were the ones at stake: every plane product of its rays leaves the float range.  Seen on the
MI355X with the kernels of that time: the rays from 1e13 away lost nothing (|o / d| itself passed 2^120 and the axes were dropped for that), and of the 40 rays
from beside the world's origin stream_extend lost all 40 hits, at every level and under both builders; the pair walk (FP64 boxes) none.  Lean SHADE's escape stage is reached only through a render's scattered rays; its predicate, ray_escapes, is the function
the host check calls."""
import numpy as np
import pytest

import slab_edge_worlds as sw
import triangle_edge_worlds as tw
from conftest import rel_err
from test_triangle_edges import check_decided, commit

CASES = [(n, False) for n in sw.triangle_worlds()] + [("S2", True)]
CASE_IDS = [n + ("-placed" if p else "") for n, p in CASES]

_worlds, _answers, _census = {}, {}, []


def world(name, is_placed=False):
    key = (name, is_placed)
    if key not in _worlds:
        _worlds[key] = tw.placed(world(name), sw.S2_TRANSLATE) if is_placed else sw.triangle_worlds()[name]()
    return _worlds[key]


def answers(name, is_placed=False):
    """the exact classifier's Answers: made once per world, shared by every test, never changed"""
    key = (name, is_placed)
    if key not in _answers:
        _answers[key] = tw.answers(world(name, is_placed))
    return _answers[key]


def census():
    if not _census:
        _census.append(sw.overflow_spheres())
    return _census[0]


# ---- CPU ------------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name,is_placed", CASES, ids=CASE_IDS)
def test_triangle_worlds_are_decided(name, is_placed):
    w, A = world(name, is_placed), answers(name, is_placed)
    share = 1.0 - A.decided.mean()
    print(f"{w.name}: {len(w.tri_v)} triangles, {len(w.all)} rays, {int(A.hit.sum())} exact hits, {share:.1%} undecided")
    assert share <= 1 / 3
    assert A.hit.any() and not A.hit.all() or name == "S2"       # S2: what misses the fan meets the ground
    if "near" in w.labels:
        assert A.decided[w.labels["near"]].all()
    if name == "S2":
        on_fan = np.array([bool(x) and min(x) < 196 for x in A.winners])
        assert on_fan.sum() >= 1000 and (~on_fan).sum() >= 300   # aimed lattice points inside and on the edges; one step outside goes on to the ground


def test_oracle_answers_the_sphere_census(built):
    from oracle import zr_oracle_py as zo
    s = census()
    h = zo.OracleScene(s.world.desc).trace(s.rays, tw.TMIN, tw.INF)
    hit = s.want_mat != tw.MISS
    assert np.array_equal(h["mat"], s.want_mat)
    assert rel_err(h["t"][hit], s.want_t[hit], 1e-300).max() < 1e-9


# ---- GPU ------------------------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def ctx(built):
    from raytracer_project_amd import capi
    c = capi.Context(0)
    yield c
    c.close()


def _grid_nodes(sc):
    """the committed trees' boxes grouped by parent: (boxes below the root's children, largest ratio of two siblings' extents under one grid node)"""
    b = sc.tree_boxes()
    deep = b[b["depth"] >= 2]
    worst = 1.0
    for tree in np.unique(deep["tree"]):
        t = deep[deep["tree"] == tree]
        for p in np.unique(t["parent"]):
            ext = (t[t["parent"] == p]["hi"].astype(np.float64) - t[t["parent"] == p]["lo"]).max(axis=1)
            if ext.min() > 0:
                worst = max(worst, ext.max() / ext.min())
    return len(deep), worst


@pytest.mark.gpu
@pytest.mark.parametrize("builder", ["host", "device"])
def test_worlds_target_what_they_claim(builder, ctx, monkeypatch):
    for name, is_placed in CASES:
        sc = commit(ctx, world(name, is_placed), builder, monkeypatch)
        n, ratio = _grid_nodes(sc)
        print(f"{name}{'-placed' if is_placed else ''} / {builder}: {sc.stats()['bvh_pairs']} pairs, {n} boxes on grids below the root, sibling extents differ by up to {ratio:.3g}")
        sc.close()
        assert n >= 8, (name, builder)
        if name == "S2" and not is_placed:
            assert ratio >= 2.0 ** 20, (builder, ratio)
    s = census()
    sc = commit(ctx, s.world, builder, monkeypatch)
    n, _ = _grid_nodes(sc)
    sc.close()
    assert n >= 8, ("S4", builder)


@pytest.mark.gpu
@pytest.mark.parametrize("builder", ["host", "device"])
@pytest.mark.parametrize("name,is_placed", CASES, ids=CASE_IDS)
def test_decided_rays(name, is_placed, builder, ctx, monkeypatch):
    w, A = world(name, is_placed), answers(name, is_placed)
    got, failed = {}, []
    for level in (None,) if is_placed else (None, "1", "2", "3"):
        sc = commit(ctx, w, builder, monkeypatch, level)
        want_level = 3 if is_placed else int(level or 0)
        assert sc.kernels()["extend_level"] == want_level, (w.name, level, sc.kernels())
        for engine in ("extend", "pairs") if level is None else ("extend",):
            monkeypatch.setenv("ZR_TRACE_ENGINE", engine)
            who = f"{builder} / {engine}" + (f" / level {want_level}" if engine == "extend" else "")
            h = got[who] = sc.trace(w.all)
            try:   # every compiled copy is asked before the test fails
                loose, n_ff, worst_t = check_decided(w, A, h, who)
                print(f"{w.name} / {who}: {len(w.all)} rays, {int(A.decided.sum())} decided, worst |t - exact| / bound {worst_t:.2f}; undecided rays differing: {loose}")
            except AssertionError as e:
                failed.append(str(e))
        if level is None and not is_placed and sc.kernels()["shade_lean"] == 1:
            h, _ = sc.kat_shade_lean(w.all, np.arange(len(w.all), dtype=np.uint64))
            try:
                check_decided(w, A, h, "lean pair")
            except AssertionError as e:
                failed.append(str(e))
        sc.close()
    assert not failed, f"{len(failed)} of {len(got)} engines:\n" + "\n".join(failed)
    ext, prs = got[f"{builder} / extend / level {3 if is_placed else 0}"], got[f"{builder} / pairs"]
    assert not ((ext["mat"] != prs["mat"]) & A.decided & np.array([len(x) == 1 for x in A.winners])).any()


@pytest.mark.gpu
@pytest.mark.parametrize("builder", ["host", "device"])
def test_sphere_census(builder, ctx, monkeypatch):
    s = census()
    hit = s.want_mat != tw.MISS
    failed = []

    def check(h, who):
        lost = int((hit & (h["mat"] == tw.MISS)).sum())
        lost_o = int((hit & s.from_origin & (h["mat"] == tw.MISS)).sum())
        wrong = int((h["mat"] != s.want_mat).sum())
        t_err = rel_err(h["t"][hit & (h["mat"] == s.want_mat)], s.want_t[hit & (h["mat"] == s.want_mat)], 1e-300)
        print(f"S4 / {who}: {len(s.rays)} rays ({int(s.from_origin.sum())} from beside the origin), {lost} hits lost ({lost_o} of them from beside the origin), {wrong - lost} other wrong answers, t off by {t_err.max() if t_err.size else 0:.2e}")
        if wrong or (t_err.size and t_err.max() >= 1e-9):
            failed.append(f"S4 / {who}: {lost} of {int(hit.sum())} hits lost, {wrong - lost} other wrong answers, rel_err(t) {t_err.max() if t_err.size else 0:.2e}")

    for level in (None, "1", "2", "3"):
        sc = commit(ctx, s.world, builder, monkeypatch, level)
        assert sc.kernels()["extend_level"] == int(level or 0)
        for engine in ("extend", "pairs") if level is None else ("extend",):
            monkeypatch.setenv("ZR_TRACE_ENGINE", engine)
            check(sc.trace(s.rays), f"{builder} / {engine} / level {int(level or 0)}")
        if level is None:
            assert sc.kernels()["shade_lean"] == 1
            h, _ = sc.kat_shade_lean(s.rays, np.arange(len(s.rays), dtype=np.uint64))
            check(h, f"{builder} / lean pair")
        sc.close()
    assert not failed, "\n".join(failed)
