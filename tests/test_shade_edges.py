"""scatter() and the lean pair lean_rec / lean_shade (zr_device.h) at their decision edges, against the genuine reference's answers on the hand-placed rays of
tests/golden/kat_kat2.npz (scene "kat2", a world that commits with SHADE's lean build; tests/golden/make_golden.py kat2_inputs() places the rays,
tests/shade_edge_worlds.py holds the layout and the float64 models): face-normal ties of both classes on every stored form, the dielectric threshold to the
last place, normal / clamped / grazing incidence, fuzzy metal at grazing incidence, vertex normals that oppose the face or cancel, lambertian's degenerate
direction reached on purpose.  What the tests found and the errors they print: DESIGN.md, parity section."""
import importlib.util
import os

import numpy as np
import pytest

import shade_edge_worlds as sw
from conftest import ROOT, demo_scene, load_golden, rel_err

REL_TOL, ABS_FLOOR = 1e-4, 1e-7            # test_gpu_parity.py: the north-star bound on radiance
TOL_CHAIN = 1e-12                          # of max(1, |value|): objects evaluated in the reference's own frame (kat0's bound)
TOL_WORLD_P, TOL_WORLD_N = 1e-9, 1e-7      # baked forms, evaluated in world space (test_wrapper_chains_at_their_edges): t, p and origins | normals and directions

# Documented deviations (parity section), by name: (class of rows in the fixture, how many, what is accepted there).  Nothing else is excused.
#   "tangent discriminant": the class (b) ties on spheres are tangent rays whose discriminant h h - a c is exactly 0 in the reference's order although its
#   products round.  closest_hit and EXTEND evaluate it with fused multiply-adds: -1 ulp is a miss, +1 ulp a hit whose t, p and normal are sqrt(1 ulp) ~ 1e-8
#   away, no tie any more.  On these 48 rows the device's answer is reported (hit or miss, finite) and not compared.  The class (a) tangent rays, whose
#   products are exact, are compared like any other row; the intersection kernels are not this file's subject.
#   "refraction at the threshold": FIVE rows, by number (index 2.4 met from behind at delta = -1e-12, the keys that refract).  refract() ends with
#   -sqrt(|1 - |perp|^2|) n; there the radicand is 2e-12 and the normal component 1.4e-6, so a difference d in |perp|^2 moves that component by d / 2.8e-6.
#   Each side's |perp|^2 ~ 1 is within 4 x 2^-53 of the exact value (unit_vector's half unit in the last place of ud.x = 0.417 carried through ri = 2.4 and the
#   square: 1.2 x 2^-53; the product ri x: 1; the square and the two sums of the squared length: 1.5; rounded up), and the device fuses where the reference
#   rounds: the two radicands may differ by 8 x 2^-53 = 8.9e-16 (seen: 4.4e-16, which is the 1.6e-10 in the component).  On these five rows, instead of the
#   component itself: the direction's part along the surface to the 1e-12 of every row, the component's sign exact, and its SQUARE (= the radicand) to
#   8 x 2^-53 — a conditioned bound; an error of refract() beyond the last places of |perp|^2 still fails it.  Every other row of the threshold, the other 51
#   refractions at delta = -1e-12 and -1e-9 among them, is held to 1e-12 on the raw direction.
DEVIATIONS = {"tangent discriminant": ("tie_b_sphere", 48), "refraction at the threshold": ((948, 949, 950, 951, 953), 8 * 2.0 ** -53)}


def kat2_inputs():
    spec = importlib.util.spec_from_file_location("make_golden", os.path.join(ROOT, "tests", "golden", "make_golden.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.kat2_inputs()


_fx = {}


def fixture():
    """the fixture, the classes of its rows, and per row: knife-edge?, stream key"""
    if not _fx:
        fx = load_golden("kat_kat2")
        rays, cls, delta, found = kat2_inputs()
        assert np.array_equal(fx["rays"], rays), "the fixture was not made from kat2_inputs()"
        knife = np.zeros(len(rays), bool)
        knife[[r for r, label in delta.items() if label in sw.KNIFE]] = True
        m = fx["meta"]["hits"]
        assert (m["seed"], m["stream_pixel"]) == (sw.KAT_SEED, sw.KAT_PIXEL)
        keys = np.array([sw.kat_key(k) for k in range(len(rays))], dtype=np.uint64)
        _fx.update(fx=fx, cls=cls, delta=delta, found=found, knife=knife, keys=keys)
    return _fx


def dielectric_rows(f):
    """rows whose hit is on a dielectric, with the glass index of each: by the cell the hit point lies in"""
    recs = f["fx"]["recs"]
    hit = recs[:, 0] > 0
    cell = np.where(hit, sw.cell_of(recs[:, 2:5]), -1)
    index = np.zeros(len(recs))
    tris, sphs = sw.triangles(), sw.spheres()
    for c in set(cell.tolist()) - {-1}:
        if c in tris and tris[c][2] == "dielectric":
            g = (c // 3) % 4 if c < 18 else (c - 18) // 2 if c < 26 else 0     # zr_build_kat2: GLASS + f % 4 | cells 18-25 | cells 33, 35
        elif c in sphs and sphs[c][0] == "dielectric":
            g = (c - 48) // 2
        else:
            continue
        index[cell == c] = sw.GLASS_INDEX[g]
    return np.flatnonzero(index > 0), index


def test_rng_mirror_is_the_contract(built):
    """the Python mirror of include/zr_rng.h that places the lambertian rays and reads the reflect / refract draw is the oracle's own key function"""
    from oracle import zr_oracle_py as zo
    for k in (0, 1, 77, 3004):
        assert sw.kat_key(k) == zo.stream_key(sw.KAT_SEED, sw.KAT_PIXEL, k)


def test_oracle_matches_reference_on_kat2(built):
    """zr_oracle's trace + kat_scatter on the fixture's rays against the genuine reference's records, as test_oracle_golden.py holds kat0 and kat1: decisions and
    draw counts exact, every value bit-equal."""
    from oracle import zr_oracle_py as zo
    f = fixture()
    fx = f["fx"]
    ds = demo_scene("kat2")
    assert not ds.warnings, ds.warnings
    osc = zo.OracleScene(ds.desc)
    rays, recs, scat = fx["rays"], fx["recs"], fx["scat"]
    assert np.all(rays[:, 6] == 0.001) and np.all(np.isinf(rays[:, 7]))
    hits = osc.trace(rays[:, :6], 0.001, float("inf"), seed=sw.KAT_SEED, pixel=sw.KAT_PIXEL, bounce=0)
    h = recs[:, 0] > 0
    assert np.array_equal(h, hits["t"] > 0)   # (an object without a material reports mat 0xFFFFFFFF on a hit too: t decides)
    assert fx["meta"]["hits"]["rays_hit"] == h.sum() and (~h).sum() >= 20
    assert np.array_equal(hits["t"][h], recs[h, 1]) and np.array_equal(hits["p"][h], recs[h, 2:5])
    assert np.array_equal(hits["normal"][h], recs[h, 5:8])
    assert np.array_equal(hits["front_face"][h], recs[h, 8].astype(np.uint32))
    assert np.array_equal(hits["u"][h], recs[h, 9]) and np.array_equal(hits["v"][h], recs[h, 10]) and np.array_equal(hits["tangent"][h], recs[h, 11:14])
    pairs = set(zip(recs[h, 14].astype(int).tolist(), hits["mat"][h].tolist()))
    assert len(pairs) == len({a for a, _ in pairs}) == len({b for _, b in pairs}) == 10 and 0xFFFFFFFF in {b for _, b in pairs}
    so = osc.kat_scatter(rays[h, :6], hits[h], f["keys"][h])
    assert np.array_equal(so["scattered"], scat[h, 0].astype(np.uint32))
    assert np.array_equal(so["draws"], scat[h, 13].astype(np.uint32))
    assert np.array_equal(so["attenuation"], scat[h, 1:4]) and np.array_equal(so["origin"], scat[h, 4:7])
    assert np.array_equal(so["direction"], scat[h, 7:10]) and np.array_equal(so["emitted"], scat[h, 10:13])


def test_edge_inputs_meet_their_conditions():
    """The fixture holds what it was built to hold — asserted on the reference's records alone, so that a regenerated fixture cannot quietly lose an edge."""
    f = fixture()
    fx, cls, delta = f["fx"], f["cls"], f["delta"]
    rays, recs, scat = fx["rays"], fx["recs"], fx["scat"]
    hit = recs[:, 0] > 0
    # face-normal ties: every one a hit with front_face = 0 and dot(d, normal) exactly 0 in the reference's order; class (b) has a product that rounds
    ties = cls["tie"]
    assert hit[ties].all() and not recs[ties, 8].any()
    assert all(sw.dot(rays[r, 3:6], recs[r, 5:8]) == 0.0 for r in ties)
    assert all(sw.inexact_products(rays[r, 3:6], recs[r, 5:8]) for r in cls["tie_b"])
    assert not any(sw.inexact_products(rays[r, 3:6], recs[r, 5:8]) for r in cls["tie_a"])
    for kind in ("lambertian", "metal", "dielectric"):
        assert len(cls["tie_a_" + kind]) >= 32 and len(cls["tie_b_" + kind]) >= 32, kind
    assert len(cls["tie_a_sphere"]) >= 16
    assert len(cls.get("tie_b_sphere", ())) == fx["meta"]["hits"]["sphere_ties_b"] >= 16
    # every stored form and both parities of reface(): the tie rows lie in all 18 cells of the bent triangles and on bare and translated spheres
    tie_cells = set(sw.cell_of(recs[ties, 2:5]).tolist())
    assert set(range(18)) <= tie_cells and {40, 41} <= tie_cells
    # fuzzy metal at grazing incidence answers both ways
    g = cls["fuzzy_grazing"]
    assert len(g) >= 200 and 0.1 * len(g) < scat[g, 0].sum() < 0.9 * len(g)
    # the dielectric threshold: all offsets present; away from the knife edge the model is on the side it was built on, by more than 1e-13
    rows, index = dielectric_rows(f)
    thr = np.array(sorted(delta))
    assert set(thr.tolist()) <= set(rows.tolist()) and {delta[r] for r in thr} == set(sw.KNIFE) | {s + e for s in "+-" for e in ("1e-12", "1e-09", "1e-06")}
    above = below = 0
    for r in thr:
        m = sw.dielectric(rays[r, 3:6], recs[r, 5:8], recs[r, 8] > 0, index[r], sw.draw(int(f["keys"][r]), 0))
        if f["knife"][r]:
            assert abs(m["ri_st"] - 1.0) < 1e-14, (r, delta[r], m["ri_st"])
            continue
        assert abs(m["ri_st"] - 1.0) > 1e-13 and (m["ri_st"] > 1.0) == delta[r].startswith("+"), (r, delta[r], m["ri_st"])
        assert scat[r, 13] == m["draws"]
        above += m["cannot"]; below += not m["cannot"]
    assert above >= 90 and below >= 90   # five (index, face, form) combinations x three offsets a side x six keys
    # ... and on the side that can refract, the draw sends some records each way
    sent = [np.abs(scat[r, 7:10] - sw.dielectric(rays[r, 3:6], recs[r, 5:8], recs[r, 8] > 0, index[r], 0.0)["reflect"]).max() < 1e-9 for r in thr if scat[r, 13] == 1]
    assert 4 <= sum(sent) <= len(sent) - 50, (sum(sent), len(sent))
    # the reflect / refract draw: no dielectric record that draws sits within 1e-12 of its Schlick weight (a pow5 that is 2 ulp off cannot excuse a flipped decision)
    margin = []
    for r in rows:
        if scat[r, 13] == 1:
            u = sw.draw(int(f["keys"][r]), 0)
            margin.append(abs(sw.dielectric(rays[r, 3:6], recs[r, 5:8], recs[r, 8] > 0, index[r], u)["rf"] - u))
    assert len(margin) > 500 and min(margin) > 1e-12, min(margin)
    # normal incidence is exact, the clamp is reached, grazing incidence is grazing; directions of length 1e-3 ... 1e3
    ct = lambda r: sw.dot(-sw.unit(rays[r, 3:6]), recs[r, 5:8])   # noqa: E731
    assert all(ct(r) == 1.0 for r in cls["normal_incidence"])
    assert sum(ct(r) > 1.0 for r in cls["central"]) >= 16
    assert all(0 < ct(r) < 1e-9 for r in cls["grazing"]) and len(cls["grazing"]) >= 16
    lens = np.linalg.norm(rays[cls["unnormalised"], 3:6], axis=1)
    assert lens.min() <= 1e-3 and lens.max() >= 1e3
    # lambertian: the fallback rays fall back (the direction IS the normal), their neighbours 1e-7 away do not
    fb, near = cls["lambert_fallback"], cls["lambert_near"]
    assert len(fb) >= 16 and len(near) >= 16 and hit[fb].all() and hit[near].all()
    assert np.array_equal(scat[fb, 7:10], recs[fb, 5:8])
    assert np.all(np.abs(scat[near, 7:10]).max(axis=1) > 1e-8) and np.all(np.abs(scat[near, 7:10]).max(axis=1) < 1e-6)
    # cancelling vertex normals reach unit_vector's zero branch; opposing ones put the normal below the face; the light, both faces, and no material
    assert sum(not recs[r, 5:8].any() for r in cls["cancel"]) >= 12
    assert (recs[cls["opposed"], 8] == 0).sum() >= 8
    lit = scat[:, 10:13].max(axis=1) > 0
    assert (lit & (recs[:, 8] > 0)).sum() >= 3 and (lit & hit & (recs[:, 8] == 0)).sum() >= 3
    bare = hit & np.isin(np.where(hit, sw.cell_of(recs[:, 2:5]), -1), (57, 59))   # the sphere and the triangle without a material
    assert bare.sum() >= 8 and not scat[bare].any()
    assert hit[cls["tri_positions"]].sum() >= 400 and hit[cls["sphere_inside"]].sum() >= 100 and not hit[cls["between"]].any()


# ---- on the device ----------------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def ctx(built):
    from raytracer_project_amd import capi
    c = capi.Context(0)
    yield c
    c.close()


def _close(got, want, tol, what, report, rows=None):
    err = np.abs(got - want) / np.maximum(1.0, np.abs(want))
    worst = float(err.max()) if err.size else 0.0
    report.append(f"{what} max error {worst:.3e} (bound {tol:g})")
    if worst > tol:
        over = np.flatnonzero(err.reshape(len(err), -1).max(axis=1) > tol)
        return [f"{what}: max error {worst:.3e} over {tol:g} on {over.size} records" + (f", rows {rows[over].tolist()[:40]}" if rows is not None else "")]
    return []


def _classes_of(f, rows):
    return {name for name, members in f["cls"].items() if np.isin(rows, members).any()}


def _check_against_fixture(f, hits, so, tag):
    """records and scatter outputs of the device (rows = the fixture's) against the reference's, by the bounds of this file's head"""
    fx, knife = f["fx"], f["knife"]
    rays, recs, scat = fx["rays"], fx["recs"], fx["scat"]
    h = recs[:, 0] > 0
    report, bad = [], []
    may_miss = np.zeros(len(rays), bool)
    name, count = DEVIATIONS["tangent discriminant"]
    assert len(f["cls"][name]) == count
    may_miss[f["cls"][name]] = True
    got = hits["t"] > 0
    wrong = np.flatnonzero((h != got) & ~may_miss)
    assert wrong.size == 0, f"{tag}: hit / miss differs on rays {wrong.tolist()[:20]}"
    report.append(f"tangent discriminant: {int((may_miss & ~got).sum())} of {count} class (b) sphere ties miss on the device, {int((may_miss & got & (hits['front_face'] == 0)).sum())} still tie")
    assert np.isfinite(hits["p"][may_miss]).all() and np.isfinite(so["direction"][may_miss]).all() and np.isfinite(so["origin"][may_miss]).all()
    k = h & got & ~may_miss
    wrong = np.flatnonzero(k & (hits["front_face"] != recs[:, 8].astype(np.uint32)))
    if wrong.size:
        bad.append(f"front_face differs on {wrong.size} rays {sorted(_classes_of(f, wrong))}, first {wrong.tolist()[:12]}")
    pairs = set(zip(recs[k, 14].astype(int).tolist(), hits["mat"][k].tolist()))
    assert len(pairs) == len({a for a, _ in pairs}) == len({b for _, b in pairs}), f"{tag}: materials {sorted(pairs)}"
    firm = k & ~knife
    for what, col in (("scattered", 0), ("draws", 13)):
        wrong = np.flatnonzero(firm & (so[what] != scat[:, col].astype(np.uint32)))
        if wrong.size:
            bad.append(f"{what} differs on {wrong.size} rays {sorted(_classes_of(f, wrong))}, first {wrong.tolist()[:12]}")
    firm &= (so["scattered"] == scat[:, 0].astype(np.uint32))
    world = np.zeros(len(rays), bool)
    world[h] = [sw.baked(c) for c in sw.cell_of(recs[h, 2:5])]
    _, index = dielectric_rows(f)
    five, radicand_tol = DEVIATIONS["refraction at the threshold"]
    near = np.zeros(len(rays), bool)
    near[list(five)] = True
    for r in five:   # what the five are: index 2.4 from behind the bare triangle, built at -1e-12, refracting in the reference
        assert f["delta"][r] == "-1e-12" and index[r] == 2.4 and recs[r, 8] == 0 and scat[r, 13] == 1
        assert not sw.dielectric(rays[r, 3:6], recs[r, 5:8], False, 2.4, sw.draw(int(f["keys"][r]), 0))["reflects"]
    s = near & firm
    assert s.sum() == len(five), f"{tag}: a decision differs on rows {np.flatnonzero(near & ~firm).tolist()}"
    along = np.einsum("ij,ij->i", so["direction"][s], recs[s, 5:8]), np.einsum("ij,ij->i", scat[s, 7:10], recs[s, 5:8])
    bad += _close(so["direction"][s] - along[0][:, None] * recs[s, 5:8], scat[s, 7:10] - along[1][:, None] * recs[s, 5:8], TOL_CHAIN,
                  "refraction at the threshold (5 rows), along the surface", report, np.flatnonzero(s))
    if not np.array_equal(np.sign(along[0]), np.sign(along[1])):
        bad.append("refraction at the threshold: the normal component's sign differs")
    gap = float(np.abs(along[0] ** 2 - along[1] ** 2).max())
    report.append(f"refraction at the threshold (5 rows), radicand max error {gap:.3e} (bound {radicand_tol:.3e}); raw normal component {np.abs(along[0] - along[1]).max():.3e}")
    if gap > radicand_tol:
        bad.append(f"refraction at the threshold: radicand {gap:.3e} over {radicand_tol:.3e}")
    firm_dir = firm & ~near
    for sel, tp, tn, form in ((k & ~world, TOL_CHAIN, TOL_CHAIN, "chain order"), (k & world, TOL_WORLD_P, TOL_WORLD_N, "world space")):
        assert sel.sum() > 500
        bad += _close(hits["t"][sel], recs[sel, 1], tp, f"t ({form})", report) + _close(hits["p"][sel], recs[sel, 2:5], tp, f"p ({form})", report)
        bad += _close(hits["normal"][sel], recs[sel, 5:8], tn, f"normal ({form})", report)
        s = sel & firm & (scat[:, 0] > 0)
        bad += _close(so["attenuation"][s], scat[s, 1:4], TOL_CHAIN, f"attenuation ({form})", report)
        bad += _close(so["origin"][s], scat[s, 4:7], tp, f"scattered origin ({form})", report)
        s = s & firm_dir
        bad += _close(so["direction"][s], scat[s, 7:10], tn, f"scattered direction ({form})", report, np.flatnonzero(s))
        bad += _close(so["emitted"][sel], scat[sel, 10:13], TOL_CHAIN, f"emitted ({form})", report)
    # knife-edge records: either decision; then no more than the one draw, finite outputs, and the direction of whichever branch the device took, by the
    # float64 restatement of material.hpp's dielectric branch on the REFERENCE's record
    worst = 0.0
    for r in np.flatnonzero(knife & k):
        assert so["scattered"][r] == 1 and so["draws"][r] in (0, 1), (tag, r, so[r])
        assert np.isfinite(so["origin"][r]).all() and np.isfinite(so["direction"][r]).all()
        m = sw.dielectric(rays[r, 3:6], recs[r, 5:8], recs[r, 8] > 0, index[r], 0.0)
        e = [np.abs(so["direction"][r] - m["reflect"]).max()] + ([np.abs(so["direction"][r] - m["refract"]).max()] if so["draws"][r] == 1 else [])
        worst = max(worst, min(e))
    report.append(f"knife-edge direction against the branch taken: max error {worst:.3e} (bound {TOL_CHAIN:g})")
    if worst > TOL_CHAIN:
        bad.append(f"knife-edge direction: {worst:.3e}")
    for line in report:
        print(f"kat2 {tag}: {line}")
    assert not bad, f"{tag}: " + "; ".join(bad)


_general = {}


def _general_pair(ctx, f, engine, builder, monkeypatch):
    """zr_trace + zr_kat_scatter on the fixture's rays in a scene of this cell's own: (hits, scatter outputs), rows = the fixture's"""
    from raytracer_project_amd import capi
    if (engine, builder) not in _general:
        monkeypatch.setenv("ZR_TRACE_ENGINE", engine)
        monkeypatch.setenv("ZR_BVH_BUILD", builder)
        monkeypatch.setenv("ZR_BUILD_CHECK", "1")
        rays = f["fx"]["rays"]
        sc = capi.Scene(ctx, demo_scene("kat2").desc)
        try:
            assert sc.stats()["builder"].startswith(builder) and sc.kernels()["shade_lean"] == 1
            hits = sc.trace(rays[:, :6], 0.001, float("inf"), seed=sw.KAT_SEED, pixel=sw.KAT_PIXEL, bounce=0)
            h = hits["t"] > 0
            so = np.zeros(len(rays), dtype=capi.SCATTER_DTYPE)
            so[h] = sc.kat_scatter(rays[h, :6], hits[h], f["keys"][h])
        finally:
            sc.close()
        _general[(engine, builder)] = (hits, so)
    return _general[(engine, builder)]


@pytest.mark.gpu
@pytest.mark.parametrize("builder", ["host", "device"])
@pytest.mark.parametrize("engine", ["extend", "pairs"])
def test_general_scatter_at_its_edges(engine, builder, ctx, monkeypatch):
    """zr_trace + zr_kat_scatter (object_rec, scatter) on kat2 against the fixture: hit / miss, front_face, material, the scatter decision and the draw count exact;
    t, p, normal, attenuation, the scattered origin and direction and the emission as values, to 1e-12 of max(1, |v|) for objects the device evaluates in the
    reference's own frame and to kat1's world-space bounds (1e-9 on t, p and origins, 1e-7 on normals and directions) for baked ones; at the dielectric
    threshold's knife edge either decision, then the direction of the branch taken."""
    f = fixture()
    hits, so = _general_pair(ctx, f, engine, builder, monkeypatch)
    _check_against_fixture(f, hits, so, f"general {engine} {builder}")
    _scatter_on_reference_records(ctx, f, hits, f"general {engine} {builder}")


def _scatter_on_reference_records(ctx, f, hits, tag):
    """The class (b) sphere ties never reach scatter() as ties through closest_hit (DEVIATIONS, "tangent discriminant"); zr_kat_scatter takes records, so here it
    gets the REFERENCE's records of those 48 rows: lambertian, fuzz-0 metal and glass of index 1.5 on a normal exactly perpendicular to the ray although the
    products round.  Decision and draws exact, attenuation, origin and direction to 1e-12 of max(1, |v|).  (What this cannot reach: the dot_sign() of sphere_rec's
    reface() call and of lean_rec's sphere branch, which only a record made on the device exercises.)"""
    from raytracer_project_amd import capi
    fx = f["fx"]
    rays, recs, scat = fx["rays"], fx["recs"], fx["scat"]
    rows = f["cls"][DEVIATIONS["tangent discriminant"][0]]
    seen = (recs[:, 0] > 0) & (hits["t"] > 0)
    to_mat = dict(zip(recs[seen, 14].astype(int).tolist(), hits["mat"][seen].tolist()))   # the reference's material numbers -> the scene's
    rec = np.zeros(len(rows), dtype=capi.HIT_DTYPE)
    rec["p"], rec["normal"], rec["tangent"] = recs[rows, 2:5], recs[rows, 5:8], recs[rows, 11:14]
    rec["bitangent"] = np.cross(recs[rows, 5:8], recs[rows, 11:14])
    rec["t"], rec["u"], rec["v"], rec["front_face"] = recs[rows, 1], recs[rows, 9], recs[rows, 10], recs[rows, 8].astype(np.uint32)
    rec["mat"] = [to_mat[int(m)] for m in recs[rows, 14]]
    assert not rec["front_face"].any() and len(set(rec["mat"].tolist())) == 3
    sc = capi.Scene(ctx, demo_scene("kat2").desc)
    try:
        so = sc.kat_scatter(rays[rows, :6], rec, f["keys"][rows])
    finally:
        sc.close()
    assert np.array_equal(so["scattered"], scat[rows, 0].astype(np.uint32)), (tag, rows[so["scattered"] != scat[rows, 0]])
    assert np.array_equal(so["draws"], scat[rows, 13].astype(np.uint32)), (tag, rows[so["draws"] != scat[rows, 13]])
    report, bad, ok = [], [], scat[rows, 0] > 0
    bad += _close(so["attenuation"][ok], scat[rows, 1:4][ok], TOL_CHAIN, "attenuation", report) + _close(so["origin"][ok], scat[rows, 4:7][ok], TOL_CHAIN, "scattered origin", report, rows[ok])
    bad += _close(so["direction"][ok], scat[rows, 7:10][ok], TOL_CHAIN, "scattered direction", report, rows[ok])
    for line in report:
        print(f"kat2 {tag}, scatter on the reference's records of the class (b) sphere ties: {line}")
    assert not bad, f"{tag}: " + "; ".join(bad)


@pytest.mark.gpu
@pytest.mark.parametrize("builder", ["host", "device"])
def test_lean_pair_at_its_edges(builder, ctx, monkeypatch):
    """The same through zr_kat_shade_lean (closest_hit, lean_rec, lean_shade: the hand-copied statement SHADE's lean build runs), with the same bounds; and
    against the general pair's answers: decisions and draws identical off the knife edge, values within 1e-12.  How many values are not bit-equal is printed,
    not asserted: under contraction that depends on the inlining context."""
    from raytracer_project_amd import capi
    f = fixture()
    rays = f["fx"]["rays"]
    ghits, gso = _general_pair(ctx, f, "pairs", builder, monkeypatch)
    monkeypatch.setenv("ZR_BVH_BUILD", builder)
    sc = capi.Scene(ctx, demo_scene("kat2").desc)
    try:
        assert sc.stats()["builder"].startswith(builder) and sc.kernels()["shade_lean"] == 1
        hits, so = sc.kat_shade_lean(rays[:, :6], f["keys"])
    finally:
        sc.close()
    assert not hits["tangent"].any() and not hits["bitangent"].any() and not hits["u"].any() and not hits["v"].any()
    miss = hits["t"] == 0
    assert np.all(hits["mat"][miss] == 0xFFFFFFFF) and not so["scattered"][miss].any() and not so["draws"][miss].any()
    _check_against_fixture(f, hits, so, f"lean {builder}")
    firm = ~f["knife"]
    both = (hits["t"] > 0) & (ghits["t"] > 0)
    assert np.array_equal(hits["t"] > 0, ghits["t"] > 0), np.flatnonzero((hits["t"] > 0) != (ghits["t"] > 0))   # (the same closest_hit: the same tangent rays)
    firm &= both
    firm[f["cls"][DEVIATIONS["tangent discriminant"][0]]] = False
    for what, a, b in (("front_face", hits["front_face"], ghits["front_face"]), ("material", hits["mat"], ghits["mat"]),
                       ("scattered", so["scattered"], gso["scattered"]), ("draws", so["draws"], gso["draws"])):
        wrong = np.flatnonzero(firm & (a != b))
        assert wrong.size == 0, f"lean against general, {what}: {wrong.size} rays differ, first {wrong.tolist()[:20]}"
    same = firm & (so["scattered"] == gso["scattered"])
    unequal = 0
    for what, a, b in (("t", hits["t"], ghits["t"]), ("p", hits["p"], ghits["p"]), ("normal", hits["normal"], ghits["normal"]),
                       ("attenuation", so["attenuation"], gso["attenuation"]), ("origin", so["origin"], gso["origin"]),
                       ("direction", so["direction"], gso["direction"]), ("emitted", so["emitted"], gso["emitted"])):
        a, b = a[same], b[same]
        err = np.abs(a - b) / np.maximum(1.0, np.abs(b))
        unequal += int((a != b).sum())
        print(f"kat2 lean against general {builder}: {what} max error {err.max():.3e}, {int((a != b).sum())} of {a.size} values not bit-equal")
        assert err.max() <= 1e-12, f"lean against general, {what}: {err.max():.3e}"
    print(f"kat2 lean against general {builder}: {unequal} values not bit-equal in all")


@pytest.mark.gpu
def test_lean_entry_refusals(ctx):
    """zr_kat_shade_lean refuses an uncommitted scene (ZR_E_STATE), a null argument (ZR_E_INVALID) and a scene that did not commit with the lean build, mix0
    (ZR_E_STATE), each with its text; n = 0 succeeds"""
    import ctypes as C
    from raytracer_project_amd import capi
    lib = ctx.lib
    rays = np.zeros((1, 6)); rays[0, 5] = -1.0
    keys = np.ones(1, dtype=np.uint64)
    hits = np.zeros(1, dtype=capi.HIT_DTYPE); out = np.zeros(1, dtype=capi.SCATTER_DTYPE)
    args = (rays.ctypes.data, keys.ctypes.data, None, 1, hits.ctypes.data, out.ctypes.data)
    INVALID, STATE = capi.ZR_E_INVALID, capi.ZR_E_STATE
    raw = lib.zr_scene_create(ctx._c)
    try:
        assert lib.zr_kat_shade_lean(ctx._c, raw, *args) == STATE and b"zr_scene_commit must precede zr_kat_shade_lean" in lib.zr_last_error()
    finally:
        lib.zr_scene_destroy(raw)
    lean = capi.Scene(ctx, demo_scene("kat2").desc)
    general = capi.Scene(ctx, demo_scene("mix0").desc)
    try:
        assert general.kernels()["shade_lean"] == 0
        assert lib.zr_kat_shade_lean(ctx._c, general._s, *args) == STATE and b"lean build" in lib.zr_last_error()
        assert lib.zr_kat_shade_lean(None, lean._s, *args) == INVALID and b"null argument" in lib.zr_last_error()
        assert lib.zr_kat_shade_lean(ctx._c, None, *args) == INVALID
        for k in (0, 1, 4, 5):   # rays, keys, the records, the scatter outputs
            a = list(args); a[k] = None
            assert lib.zr_kat_shade_lean(ctx._c, lean._s, *a) == INVALID and b"null argument" in lib.zr_last_error(), k
        assert lib.zr_kat_shade_lean(ctx._c, lean._s, None, None, None, 0, None, None) == 0
        assert lib.zr_kat_shade_lean(ctx._c, lean._s, *args) == 0
        h, s = lean.kat_shade_lean(np.zeros((0, 6)), np.zeros(0, dtype=np.uint64))
        assert len(h) == 0 and len(s) == 0
    finally:
        lean.close(); general.close()


# the world-list entries of kat2 (zr_build_kat2 adds cells 0-37, then 40-59) the fused kernel renders, at most ZR_FUSED_OBJECTS of them: bent triangles of four
# forms, flat glass, opposing and cancelling normals, spheres bare and translated, the light, no material
KAT2_FUSED_ENTRIES = [0, 4, 8, 11, 13, 17, 18, 25, 30, 35, 38, 41, 46, 53, 54, 57]


@pytest.mark.gpu
@pytest.mark.parametrize("count", [False, True], ids=["timed", "counting"])
@pytest.mark.parametrize("route", ["pipeline", "fused"])
def test_kat2_frames_on_both_shade_builds(route, count, built, monkeypatch):
    """kat2 from its own camera (64 x 48, 8 spp, its max_depth) with ZR_SHADE_LEAN=1 and =0: the two builds' frames are bit-equal, each within REL_TOL of the
    live oracle render, and (primary samples, segments, RNG draws, hits) exactly the oracle's — through the streaming pipeline on the whole world, and through
    the fused kernel on sixteen of its entries.  This binds the copy of the lean pair that is inlined into the render kernels, not only the kat kernel's."""
    import ctypes as C
    from oracle import zr_oracle_py as zo
    from raytracer_project_amd import capi
    ds = demo_scene("kat2")
    cam = ds.camera.copy()
    assert (cam.image_width, cam.image_height, cam.samples_per_pixel) == (64, 48, 8)
    desc, keep = ds.desc, None
    if route == "fused":
        desc = capi.SceneDesc()
        C.memmove(C.byref(desc), C.byref(ds.desc), C.sizeof(desc))
        all_objs = C.cast(ds.desc.objects, C.POINTER(capi.Object))
        keep = (capi.Object * len(KAT2_FUSED_ENTRIES))()
        for k, e in enumerate(KAT2_FUSED_ENTRIES):
            assert e < ds.desc.n_objects
            C.memmove(C.byref(keep, k * C.sizeof(capi.Object)), C.byref(all_objs[e]), C.sizeof(capi.Object))
        desc.objects, desc.n_objects = C.cast(keep, C.c_void_p), len(KAT2_FUSED_ENTRIES)
    else:
        monkeypatch.setenv("ZR_FUSED", "0")
    ref, rctr, _, _ = zo.OracleScene(desc).render(cam, ds.env, ds.seed, None)
    frames = {}
    for lean in ("1", "0"):
        monkeypatch.setenv("ZR_SHADE_LEAN", lean)
        c = capi.Context(0)
        try:
            sc = capi.Scene(c, desc)
            try:
                frames[lean] = sc.render(cam, ds.env, ds.seed, None, count=count)
                ctr = c.counters()
                assert (sc.kernels()["shade_lean"], ctr.path) == (int(lean), 3 if route == "fused" else 2), (route, lean, sc.kernels(), ctr.path)
            finally:
                sc.close()
        finally:
            c.close()
        err = rel_err(frames[lean], ref, ABS_FLOOR)
        assert err.max() <= REL_TOL, f"{route} lean={lean}: max rel err {err.max():.3e}"
        if count:
            got = (ctr.primary_samples, ctr.segments, ctr.rng_draws, ctr.hits)
            assert got == (64 * 48 * 8, rctr.segments, rctr.rng_draws, rctr.hits), (route, lean, got, (rctr.segments, rctr.rng_draws, rctr.hits))
    assert np.array_equal(frames["1"], frames["0"]), f"{route}: {int((frames['1'] != frames['0']).sum())} channels differ between the two SHADE builds"
    assert rctr.hits > (20 if route == "fused" else 100), "the frame barely sees the scene"
