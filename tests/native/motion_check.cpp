// Host-side check of the motion of a refit (raytracer_project_amd/csrc/zr_motion.h over zr_update.h and zr_flatten.h) — no HIP.  Compiled and run by
// tests/test_scene_motion_native.py, once plain and once with -fsanitize=address,undefined.
//   motion_check <seed>
// dyadic   chains whose numbers are dyadic (offsets k / 8, sin / cos in {0, +-1}, scales 2 and 1/2) in every stored form record_doubles and classify_object tell
//          apart: every operation is exact, so A and Nm must be BIT-equal to matrices written by hand.
// random   chains of 1 .. ZR_MAX_CHAIN random ops on both sides: A (M_now q) against M_prev q in long double, within a bound derived from the number of ops.
// cut      radius 0 before, radius 0 after, a scale factor 0, a value that is not finite.
// sharing  a medium reached through its inner chain, two entries over one sphere, a placed group; entries no update reaches stay STATIC.
// Prints one JSON line of flags; exit status 0 when all hold.
#include "zr_motion.h"

namespace zr_host {
static thread_local std::string g_err;
int fail(int code, const char* fmt, ...) { char buf[1024]; va_list ap; va_start(ap, fmt); vsnprintf(buf, sizeof buf, fmt, ap); va_end(ap); g_err = buf; return code; }
const char* last_error() { return g_err.c_str(); }
double env_double(const char* name, double dflt) { const char* v = std::getenv(name); return v && *v ? std::atof(v) : dflt; }
}

static uint64_t rng_state = 1;
static double u01() {   // splitmix64
    uint64_t z = (rng_state += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull; z = (z ^ (z >> 27)) * 0x94D049BB133111EBull; z ^= z >> 31;
    return (double)(z >> 11) * (1.0 / 9007199254740992.0);
}

static zr_xform_op op(uint32_t kind, double a0 = 0, double a1 = 0, double a2 = 0, uint32_t mat = 0) { zr_xform_op o{}; o.kind = kind; o.mat = mat; o.a[0] = a0; o.a[1] = a1; o.a[2] = a2; return o; }

// a small world described directly: the plan (world list + classification) is all the motion needs — no tree
struct World {
    std::vector<double> sph, tv, tn, cubes;
    std::vector<uint32_t> sph_mat, tmat, cmat;
    std::vector<zr_medium> media; std::vector<zr_xform_op> ops; std::vector<zr_object> objs; std::vector<zr_group> groups;
    uint32_t sphere(double x, double y, double z, double r) { sph.insert(sph.end(), {x, y, z, r}); sph_mat.push_back(0); return (uint32_t)sph_mat.size() - 1; }
    uint32_t triangle() { for (int k = 0; k < 9; k++) { tv.push_back(k == 0 || k == 4 || k == 8 ? 1.0 : 0.0); tn.push_back(k % 3 == 2 ? 1.0 : 0.0); } tmat.push_back(0); return (uint32_t)tmat.size() - 1; }
    uint32_t cube() { cubes.insert(cubes.end(), {1, 1, 1, 0, 0, 0, -1, -1, -1, 1, 1, 1}); cmat.push_back(0); return (uint32_t)cmat.size() - 1; }
    uint32_t chain(std::initializer_list<zr_xform_op> c) { const uint32_t at = (uint32_t)ops.size(); ops.insert(ops.end(), c.begin(), c.end()); return at; }
    uint32_t add(uint32_t type, uint32_t index, std::initializer_list<zr_xform_op> c = {}) { const uint32_t at = chain(c); objs.push_back({type, index, at, (uint32_t)c.size()}); return (uint32_t)objs.size() - 1; }
    uint32_t medium(uint32_t btype, uint32_t bindex, std::initializer_list<zr_xform_op> c = {}) {
        zr_medium m{}; m.boundary_type = btype; m.boundary_index = bindex; m.chain_first = chain(c); m.chain_count = (uint32_t)c.size(); m.mat = 1; m.neg_inv_density = -1.0;
        media.push_back(m); return (uint32_t)media.size() - 1;
    }
    uint32_t group() { const uint32_t first = (uint32_t)tmat.size(); triangle(); triangle(); groups.push_back({first, 2}); return (uint32_t)groups.size() - 1; }
};

struct Committed {
    SceneInput in;
    std::shared_ptr<const CommitPlan> plan;
    std::vector<zr::BuildBox> group_box;
    UpdateIndex ix;
    MotionTable mt;
    explicit Committed(const World& w) {
        in.spheres.copy(w.sph.data(), w.sph.size()); in.sphere_mat.copy(w.sph_mat.data(), w.sph_mat.size());
        in.tri_v.copy(w.tv.data(), w.tv.size()); in.tri_n.copy(w.tn.data(), w.tn.size()); in.tri_mat.copy(w.tmat.data(), w.tmat.size());
        in.cubes.copy(w.cubes.data(), w.cubes.size()); in.cube_mat.copy(w.cmat.data(), w.cmat.size());
        in.media.copy(w.media.data(), w.media.size()); in.ops.copy(w.ops.data(), w.ops.size());
        in.objects.copy(w.objs.data(), w.objs.size()); in.objects_set = true;
        in.groups = w.groups;
        zr_texture tex{}; tex.kind = ZR_TEX_SOLID; in.textures.push_back(tex);
        for (int k = 0; k < 2; k++) { zr_material m{}; m.kind = k == 1 ? ZR_MAT_ISOTROPIC : ZR_MAT_LAMBERTIAN; m.bump_tex = ZR_NO_TEXTURE; in.materials.push_back(m); }
        plan = make_plan(in, world_list(in));
        group_box.assign(w.groups.size(), zr::BuildBox{});
        UpdateWorld uw = world();
        ix.build_reverse(uw);
        mt.build(uw);
    }
    UpdateWorld world() { return UpdateWorld{in, plan->objs, plan->code, plan->kn.bake, group_box}; }
    bool set_op(uint32_t k, const zr_xform_op& o) { UpdateWorld uw = world(); return ix.update_ops(uw, k, &o, 1) == ZR_OK; }
    bool set_sphere(uint32_t k, double x, double y, double z, double r) { const double q[4] = {x, y, z, r}; UpdateWorld uw = world(); return ix.update_spheres(uw, k, q, 1) == ZR_OK; }
    void refit() { UpdateWorld uw = world(); mt.step(uw, ix.dirty_list); ix.clear_dirty(); }
    uint32_t word(uint32_t oi) const { for (size_t k = 0; k < mt.entries.size(); k++) if (mt.entries[k] == oi) return mt.slot[k]; return kMotionStatic; }
    const double* rec(uint32_t oi) const { const uint32_t w = word(oi); return w < kMotionCut ? &mt.records[(size_t)w * kMotionDoubles] : nullptr; }
};

// bit-equal to the hand-written A (rows of linear 3 + translation) and Nm
static bool equals(const double* rec, std::initializer_list<double> a12, std::initializer_list<double> nm9) {
    if (!rec) return false;
    std::vector<double> want(a12); want.insert(want.end(), nm9.begin(), nm9.end());
    return want.size() == (size_t)kMotionDoubles && std::memcmp(rec, want.data(), sizeof(double) * kMotionDoubles) == 0;
}

// the same composition in long double: the chain applied to a point, innermost first
static void apply_ld(const std::vector<zr_xform_op>& c, long double p[3]) {
    for (int k = (int)c.size() - 1; k >= 0; k--) {
        const zr_xform_op& o = c[k];
        if (o.kind == ZR_OP_TRANSLATE) for (int a = 0; a < 3; a++) p[a] += (long double)o.a[a];
        else if (o.kind == ZR_OP_SCALE) for (int a = 0; a < 3; a++) p[a] *= (long double)o.a[a];
        else if (o.kind != ZR_OP_MATERIAL) {
            const int ra = o.kind == ZR_OP_ROTATE_X ? 1 : 0, rb = o.kind == ZR_OP_ROTATE_Z ? 1 : 2;
            const long double sn = o.a[0], co = o.a[1], a = p[ra], b = p[rb];
            p[ra] = co * a - sn * b; p[rb] = sn * a + co * b;
        }
    }
}
// ... and in double, as a caller places a point, with the largest magnitude any intermediate of the composition can have (absolute values throughout)
static void apply_d(const std::vector<zr_xform_op>& c, double p[3], double& mag) {
    double m[3] = {std::fabs(p[0]), std::fabs(p[1]), std::fabs(p[2])};
    for (int k = (int)c.size() - 1; k >= 0; k--) {
        const zr_xform_op& o = c[k];
        if (o.kind == ZR_OP_TRANSLATE) for (int a = 0; a < 3; a++) { p[a] += o.a[a]; m[a] += std::fabs(o.a[a]); }
        else if (o.kind == ZR_OP_SCALE) for (int a = 0; a < 3; a++) { p[a] *= o.a[a]; m[a] *= std::fabs(o.a[a]); }
        else if (o.kind != ZR_OP_MATERIAL) {
            const int ra = o.kind == ZR_OP_ROTATE_X ? 1 : 0, rb = o.kind == ZR_OP_ROTATE_Z ? 1 : 2;
            const double sn = o.a[0], co = o.a[1], a = p[ra], b = p[rb], ma = m[ra], mb = m[rb];
            p[ra] = co * a - sn * b; p[rb] = sn * a + co * b;
            m[ra] = std::fabs(co) * ma + std::fabs(sn) * mb; m[rb] = std::fabs(sn) * ma + std::fabs(co) * mb;
        }
    }
    mag = std::max(m[0], std::max(m[1], m[2]));
}
static std::vector<zr_xform_op> random_chain(int n) {
    std::vector<zr_xform_op> c;
    for (int k = 0; k < n; k++) {
        const int what = (int)(u01() * 5);
        if (what == 0) c.push_back(op(ZR_OP_TRANSLATE, u01() * 20 - 10, u01() * 20 - 10, u01() * 20 - 10));
        else if (what <= 3) { const double a = u01() * 6.283; c.push_back(op(what == 1 ? ZR_OP_ROTATE_X : what == 2 ? ZR_OP_ROTATE_Y : ZR_OP_ROTATE_Z, std::sin(a), std::cos(a))); }
        else c.push_back(op(ZR_OP_SCALE, 0.5 + u01() * 1.5, 0.5 + u01() * 1.5, 0.5 + u01() * 1.5));
    }
    return c;
}
static double norm_inf3(const double* l, int st) { double n = 0; for (int k = 0; k < 3; k++) n = std::max(n, std::fabs(l[st * k]) + std::fabs(l[st * k + 1]) + std::fabs(l[st * k + 2])); return n; }

int main(int argc, char** argv) {
    rng_state = argc > 1 ? (uint64_t)std::atoll(argv[1]) : 1;
    const uint32_t T = ZR_OP_TRANSLATE, RY = ZR_OP_ROTATE_Y, RX = ZR_OP_ROTATE_X, S = ZR_OP_SCALE, MAT = ZR_OP_MATERIAL;

    // ---- 1. dyadic chains, one entry per stored form -------------------------------------------------------------------------------------------------------
    World w;
    const uint32_t s_bare = w.sphere(0.5, -1.25, 2, 0.5), s_mat = w.sphere(1, 1, 1, 2), s_baked = w.sphere(0, 0, 0, 1), s_bscaled = w.sphere(1, 0, 0, 1),
                   s_wrapped = w.sphere(0, 0, 0, 1), s_med = w.sphere(0, 0, 0, 1), s_shared = w.sphere(2, 0, 0, 1), s_still = w.sphere(9, 9, 9, 1);
    const uint32_t e_bare = w.add(ZR_PRIM_SPHERE, s_bare);                                                        // bare sphere: moved by update_spheres
    const uint32_t e_mat = w.add(ZR_PRIM_SPHERE, s_mat, {op(MAT, 0, 0, 0, 0)});                                   // material-only chain
    const uint32_t e_baked = w.add(ZR_PRIM_SPHERE, s_baked, {op(T, 1, 2, 3)});                                    // baked sphere
    const uint32_t e_bscaled = w.add(ZR_PRIM_SPHERE, s_bscaled, {op(T, 1, 2, 3), op(S, 2, 2, 2)});                // ... under a uniform scale
    const uint32_t e_tri = w.add(ZR_PRIM_TRIANGLE, w.triangle(), {op(T, 0.5, 0, -0.5), op(RY, 0, 1)});            // baked triangle
    const uint32_t e_pcube = w.add(ZR_PRIM_CUBE, w.cube(), {op(T, 4, 0, 0)});                                     // placed cube
    const uint32_t e_pturn = w.add(ZR_PRIM_CUBE, w.cube(), {op(T, 0, 4, 0), op(RY, 0, 1)});                       // ... turned
    const uint32_t e_pscale = w.add(ZR_PRIM_CUBE, w.cube(), {op(T, 0, 0, 4), op(RY, 0, 1), op(S, 2, 0.5, 2)});    // ... turned and scaled
    const uint32_t e_wrapped = w.add(ZR_PRIM_SPHERE, s_wrapped, {op(T, 1, 0, 0), op(RX, 0, 1)});                  // generic wrapped object
    const uint32_t e_medium = w.add(ZR_PRIM_MEDIUM, w.medium(ZR_PRIM_SPHERE, s_med));                             // plain medium: nothing reaches it
    const uint32_t e_minner = w.add(ZR_PRIM_MEDIUM, w.medium(ZR_PRIM_CUBE, w.cube(), {op(T, 1, -1, 2)}), {op(T, 3, 0, 0)});   // medium with an inner chain under an outer one
    const uint32_t e_group = w.add(ZR_PRIM_GROUP, w.group(), {op(T, -2, 0, 0), op(RY, 0, 1)});                    // placed group
    const uint32_t e_sh0 = w.add(ZR_PRIM_SPHERE, s_shared), e_sh1 = w.add(ZR_PRIM_SPHERE, s_shared, {op(MAT, 0, 0, 0, 1)});   // two entries over one sphere
    const uint32_t e_still = w.add(ZR_PRIM_SPHERE, s_still), e_tstill = w.add(ZR_PRIM_TRIANGLE, w.triangle());    // never touched
    Committed c(w);
    auto first_op = [&](uint32_t e) { return c.plan->objs[e].chain_first; };
    const uint32_t inner_op = c.in.media[c.plan->objs[e_minner].index].chain_first;
    bool moved_ok = true;
    moved_ok &= c.set_sphere(s_bare, 1.5, -1.25, 2, 1);                      // radius 1/2 -> 1, centre +1 in x
    moved_ok &= c.set_sphere(s_mat, 1, 3, 1, 2);
    moved_ok &= c.set_op(first_op(e_baked), op(T, 1, 2, 3.5));
    moved_ok &= c.set_op(first_op(e_bscaled) + 1, op(S, 4, 4, 4));           // uniform scale 2 -> 4
    moved_ok &= c.set_op(first_op(e_tri) + 1, op(RY, 1, 0));                 // a quarter turn
    moved_ok &= c.set_op(first_op(e_pcube), op(T, 4, 0.125, 0));
    moved_ok &= c.set_op(first_op(e_pturn) + 1, op(RY, -1, 0));
    moved_ok &= c.set_op(first_op(e_pscale) + 2, op(S, 1, 1, 1));            // scale (2, 1/2, 2) -> 1
    moved_ok &= c.set_op(first_op(e_wrapped) + 1, op(RX, 1, 0));
    moved_ok &= c.set_op(inner_op, op(T, 1, -1, 2.25));                      // through the medium's INNER chain
    moved_ok &= c.set_op(first_op(e_group), op(T, -2, 1, 0));
    moved_ok &= c.set_sphere(s_shared, 2, 0, -1, 1);
    c.refit();
    bool dyadic = moved_ok;
    const std::initializer_list<double> I9 = {1, 0, 0, 0, 1, 0, 0, 0, 1};
    // bare sphere: M = c + r x.  A = (r0 / r1) x + (c0 - (r0 / r1) c1) = x / 2 + (0.5 - 0.75, -1.25 + 0.625, 2 - 1); Nm = (r1 / r0) I
    dyadic &= equals(c.rec(e_bare), {0.5, 0, 0, -0.25, 0, 0.5, 0, -0.625, 0, 0, 0.5, 1}, {2, 0, 0, 0, 2, 0, 0, 0, 2});
    dyadic &= equals(c.rec(e_mat), {1, 0, 0, 0, 0, 1, 0, -2, 0, 0, 1, 0}, I9);
    dyadic &= equals(c.rec(e_baked), {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, -0.5}, I9);
    // baked sphere under a scale: M = T + s (c + r x): s 2 -> 4, c = (1, 0, 0), T = (1, 2, 3).  M_prev M_now^-1 y = T + (y - T) / 2 = y / 2 + T / 2
    dyadic &= equals(c.rec(e_bscaled), {0.5, 0, 0, 0.5, 0, 0.5, 0, 1, 0, 0, 0.5, 1.5}, {2, 0, 0, 0, 2, 0, 0, 0, 2});
    // rotate_y from (sn, co) = (0, 1) to (1, 0): M_now p = (-z, y, x) + T, so M_now^-1 y = (y_z - T_z, y_y - T_y, -(y_x - T_x)) and A = that + T, T = (0.5, 0, -0.5)
    dyadic &= equals(c.rec(e_tri), {0, 0, 1, 1, 0, 1, 0, 0, -1, 0, 0, 0}, {0, 0, 1, 0, 1, 0, -1, 0, 0});
    dyadic &= equals(c.rec(e_pcube), {1, 0, 0, 0, 0, 1, 0, -0.125, 0, 0, 1, 0}, I9);
    // rotate_y to (sn, co) = (-1, 0): M_now p = (z, y, -x) + T, M_now^-1 y = (-(y_z - T_z), y_y - T_y, y_x - T_x), T = (0, 4, 0)
    dyadic &= equals(c.rec(e_pturn), {0, 0, -1, 0, 0, 1, 0, 0, 1, 0, 0, 0}, {0, 0, -1, 0, 1, 0, 1, 0, 0});
    // scale (2, 1/2, 2) -> 1 under an unturned rotate_y and T = (0, 0, 4): A y = T + s0 (y - T) = (2 x, y / 2, 2 z - 4); Nm = diag(1 / s0)
    dyadic &= equals(c.rec(e_pscale), {2, 0, 0, 0, 0, 0.5, 0, 0, 0, 0, 2, -4}, {0.5, 0, 0, 0, 2, 0, 0, 0, 0.5});
    // rotate_x to (1, 0): M_now p = (x, -z, y) + T, M_now^-1 y = (y_x - T_x, y_z, -y_y), T = (1, 0, 0): A y = (y_x, y_z, -y_y)
    dyadic &= equals(c.rec(e_wrapped), {1, 0, 0, 0, 0, 0, 1, 0, 0, -1, 0, 0}, {1, 0, 0, 0, 0, 1, 0, -1, 0});
    dyadic &= equals(c.rec(e_minner), {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, -0.25}, I9);
    dyadic &= equals(c.rec(e_group), {1, 0, 0, 0, 0, 1, 0, -1, 0, 0, 1, 0}, I9);
    // ---- 4. sharing: both entries over the shared sphere follow it; what no update reached is STATIC
    bool sharing = equals(c.rec(e_sh0), {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 1}, I9) && equals(c.rec(e_sh1), {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 1}, I9);
    sharing &= c.word(e_minner) < kMotionCut && c.word(e_group) < kMotionCut;
    for (uint32_t e : {e_medium, e_still, e_tstill}) sharing &= c.word(e) == kMotionStatic;
    sharing &= c.mt.entries.size() == 13 && c.mt.records.size() == 13u * kMotionDoubles;
    sharing &= c.mt.map_of[e_medium] == kNoSlot && c.mt.map_of[e_tstill] == kNoSlot && c.mt.map_of[e_still] != kNoSlot;
    // the table is of ONE step: a second refit that moves one entry back holds that entry alone, and its record is the inverse step
    moved_ok &= c.set_op(first_op(e_baked), op(T, 1, 2, 3));
    c.refit();
    sharing &= c.mt.entries.size() == 1 && equals(c.rec(e_baked), {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0.5}, I9) && c.word(e_bare) == kMotionStatic;
    c.refit();                                                               // nothing dirty: an empty table
    sharing &= c.mt.entries.empty() && c.mt.records.empty() && c.word(e_baked) == kMotionStatic;

    // ---- 3. cut cases -----------------------------------------------------------------------------------------------------------------------------------------
    bool cut = true;
    cut &= c.set_sphere(s_bare, 1.5, -1.25, 2, 0); c.refit();                // radius 0 AFTER: M_now is singular
    cut &= c.word(e_bare) == kMotionCut && c.mt.records.empty();
    cut &= c.set_sphere(s_bare, 1.5, -1.25, 2, 1); c.refit();                // radius 0 BEFORE: A_lin = 0
    cut &= c.word(e_bare) == kMotionCut;
    cut &= c.set_sphere(s_bare, 1.5, -1.25, 2, -3); c.refit();               // a negative radius is stored as 0
    cut &= c.word(e_bare) == kMotionCut;
    cut &= c.set_sphere(s_bare, 0, 0, 0, 1); c.refit();
    cut &= c.word(e_bare) == kMotionCut;                                     // (0 before again)
    cut &= c.set_sphere(s_bare, 1, 0, 0, 1); c.refit();
    cut &= c.word(e_bare) < kMotionCut;                                      // and followed again once both sides are regular
    {
        Affine a, b; double rec[kMotionDoubles];
        b.apply(op(S, 2, 0, 2)); cut &= !motion_record(a, b, rec) && !motion_record(b, a, rec);          // a scale factor 0 on either side
        Affine inf; inf.apply(op(T, HUGE_VAL, 0, 0)); cut &= !motion_record(inf, a, rec) && !motion_record(a, inf, rec);   // not finite
        Affine nan; nan.apply(op(S, std::nan(""), 1, 1)); cut &= !motion_record(nan, a, rec) && !motion_record(a, nan, rec);
        Affine big; big.apply(op(S, 1e200, 1e200, 1e200)); cut &= !motion_record(a, big, rec);            // the determinant overflows
        cut &= motion_record(a, a, rec) && equals(rec, {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0}, I9);
    }

    // ---- 2. random chains -----------------------------------------------------------------------------------------------------------------------------------
    // A (M_now q) against M_prev q.  With u = 2^-53, chains of n_p and n_n ops and the magnitudes G (below), every rounding the result depends on:
    //   M_prev, M_now as matrices   3 per element and op (a rotation's two products and a sum; translate and scale 1)             3 n_p + 3 n_n
    //   M_now^-1                    cofactor 3, determinant 5, division 1; -(L^-1 t) 5 + 1                                         15
    //   A = M_prev M_now^-1         linear part 5, translation 6                                                                   11
    //   the caller's M_now q        3 per op                                                                                       3 n_n
    //   A applied                   6                                                                                              6
    // The errors of M_now and of its inverse reach the result through L_now^-1, i.e. times kappa = |L_now|_inf |L_now^-1|_inf (of the computed matrices), so
    // bound = (3 n_p + 6 n_n + 32) u kappa G,   G = mag(M_prev q) + |A_lin|_inf mag(M_now q) + |A_t|_inf: absolute values through both compositions.
    bool random_ok = true; double worst = 0; int cases = 0;
    for (int rep = 0; rep < 400; rep++) {
        const int np = 1 + (int)(u01() * ZR_MAX_CHAIN), nn = 1 + (int)(u01() * ZR_MAX_CHAIN);
        const std::vector<zr_xform_op> cp = random_chain(np), cn = random_chain(nn);
        Affine mp, mn; mp.apply_chain(cp.data(), 0, (uint32_t)np); mn.apply_chain(cn.data(), 0, (uint32_t)nn);
        double rec[kMotionDoubles], li[9];
        if (!motion_record(mp, mn, rec) || !inverse3(mn.m, 4, li)) { random_ok = false; continue; }
        const double kappa = norm_inf3(mn.m, 4) * norm_inf3(li, 3);
        const double a_lin = norm_inf3(rec, 4), a_t = std::max(std::fabs(rec[3]), std::max(std::fabs(rec[7]), std::fabs(rec[11])));
        for (int pt = 0; pt < 8; pt++) {
            const double q[3] = {u01() * 4 - 2, u01() * 4 - 2, u01() * 4 - 2};
            long double want[3] = {q[0], q[1], q[2]};
            apply_ld(cp, want);
            double y[3] = {q[0], q[1], q[2]}, mag_now = 0, mag_prev = 0, tmp[3] = {q[0], q[1], q[2]};
            apply_d(cn, y, mag_now); apply_d(cp, tmp, mag_prev);
            const double bound = (3.0 * np + 6.0 * nn + 32.0) * 0x1p-53 * kappa * (mag_prev + a_lin * mag_now + a_t);
            for (int k = 0; k < 3; k++) {
                const double got = ((rec[4 * k] * y[0] + rec[4 * k + 1] * y[1]) + rec[4 * k + 2] * y[2]) + rec[4 * k + 3];
                const double err = (double)fabsl((long double)got - want[k]);
                if (!(err <= bound)) random_ok = false;
                worst = std::max(worst, err / bound); cases++;
            }
        }
        // Nm is the inverse transpose of A's linear part: Nm^T A_lin = I within the same kind of bound
        for (int r = 0; r < 3; r++) for (int cc = 0; cc < 3; cc++) {
            double sacc = 0; for (int k = 0; k < 3; k++) sacc += rec[12 + 3 * k + r] * rec[4 * k + cc];
            if (!(std::fabs(sacc - (r == cc ? 1.0 : 0.0)) <= 32 * 0x1p-53 * norm_inf3(rec, 4) * norm_inf3(rec + 12, 3))) random_ok = false;
        }
    }
    const bool all = dyadic && moved_ok && sharing && cut && random_ok;
    auto b = [](bool x) { return x ? "true" : "false"; };
    std::printf("{\"entries\": %zu, \"movable\": %zu, \"updates\": %s, \"dyadic\": %s, \"sharing\": %s, \"cut\": %s, \"random\": %s, \"random_cases\": %d, \"worst_over_bound\": %.3g}\n",
                c.plan->objs.size(), c.mt.prev.size(), b(moved_ok), b(dyadic), b(sharing), b(cut), b(random_ok), cases, worst);
    return all ? 0 : 1;
}
