// texcoord_flatten_check.cpp — per-vertex texture coordinates through the drop-in's flatten (include/zenith/zenith.hpp).
//   texcoord_flatten_check <file.obj>
// 1. model(file, mat, 1.0, true): the flattened tri_uv is printed for the test to compare with what it wrote into the file; without the flag tri_uv is absent and
//    every other array is byte-identical to the flagged flatten's.
// 2. 20000 ten-argument triangles with a seven-argument one in the middle: the bulk path (all threads) flattens exactly what the one-by-one path flattens,
//    tri_uv included, and the seven-argument triangle's coordinates are zero.
// 3. the same list made of seven-argument triangles only: tri_uv stays absent on both paths.
// Prints one JSON line.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include "zenith/zenith.hpp"

static bool same_but_uv(const zenith::flat_scene& a, const zenith::flat_scene& b) {
    if (a.tri_mat.size() != b.tri_mat.size() || a.objects.size() != b.objects.size() || a.ops.size() != b.ops.size() || a.groups.size() != b.groups.size() ||
        a.materials.size() != b.materials.size() || a.textures.size() != b.textures.size() || a.spheres != b.spheres || a.cubes != b.cubes) return false;
    if (std::memcmp(a.tri_v.data(), b.tri_v.data(), a.tri_v.size() * sizeof(double)) || std::memcmp(a.tri_n.data(), b.tri_n.data(), a.tri_n.size() * sizeof(double)) ||
        std::memcmp(a.tri_mat.data(), b.tri_mat.data(), a.tri_mat.size() * sizeof(uint32_t))) return false;
    for (size_t k = 0; k < a.objects.size(); k++) if (std::memcmp(&a.objects[k], &b.objects[k], sizeof(zr_object))) return false;
    for (size_t k = 0; k < a.ops.size(); k++) if (std::memcmp(&a.ops[k], &b.ops[k], sizeof(zr_xform_op))) return false;
    return true;
}
static bool same_uv(const zenith::flat_scene& a, const zenith::flat_scene& b) {
    return a.tri_uv.size() == b.tri_uv.size() && (a.tri_uv.empty() || std::memcmp(a.tri_uv.data(), b.tri_uv.data(), a.tri_uv.size() * sizeof(double)) == 0);
}

int main(int argc, char** argv) {
    if (argc < 2) return 2;
    shared_ptr<material> m0 = make_shared<lambertian>(color(0.5, 0.5, 0.5));
    // 1. the OBJ reader
    zenith::flat_scene with, without;
    { hittable_list w; w.add(make_shared<model>(argv[1], m0, 1.0, true)); zenith::scene_builder b(with); w.flatten(b); b.finish(); }
    { hittable_list w; w.add(make_shared<model>(argv[1], m0)); zenith::scene_builder b(without); w.flatten(b); b.finish(); }
    const bool obj_same = same_but_uv(with, without), obj_absent = without.tri_uv.empty(), obj_sized = with.tri_uv.size() == with.tri_mat.size() * 6;
    // 2. / 3. the bulk path
    bool bulk_equal[2] = {false, false}, bulk_uv[2] = {false, false};
    for (int textured = 1; textured >= 0; textured--) {
        hittable_list bulk, plain;
        uint64_t st = 99;
        auto rnd = [&]() { st = st * 6364136223846793005ull + 1442695040888963407ull; return (double)(st >> 11) * (1.0 / 9007199254740992.0); };
        const size_t N = 20000, mid = 10000;
        for (size_t k = 0; k < N; k++) {
            point3 a(rnd(), rnd(), rnd()), b(rnd(), rnd(), rnd()), c(rnd(), rnd(), rnd());
            vec3 nn(rnd(), rnd(), rnd());
            shared_ptr<triangle> t;
            if (textured && k != mid) t = make_shared<triangle>(a, b, c, nn, nn, nn, zenith::texcoord{rnd() + 0.5, rnd()}, zenith::texcoord{rnd() + 0.5, rnd()}, zenith::texcoord{rnd() + 0.5, rnd()}, m0);
            else t = make_shared<triangle>(a, b, c, nn, nn, nn, m0);
            bulk.add(t);
            auto wrap = make_shared<hittable_list>(); wrap->add(t); plain.add(wrap);
        }
        zenith::flat_scene fa, fb;
        { zenith::scene_builder b(fa); bulk.flatten(b); b.finish(); }
        { zenith::scene_builder b(fb); plain.flatten(b); b.finish(); }
        bulk_equal[textured] = fa.tri_mat.size() == N && same_but_uv(fa, fb) && same_uv(fa, fb);
        if (!textured) bulk_uv[0] = fa.tri_uv.empty() && fb.tri_uv.empty();
        else {
            bool ok = fa.tri_uv.size() == N * 6;
            for (size_t k = 0; ok && k < N; k++) {
                const double* q = fa.tri_uv.data() + k * 6;
                for (int c = 0; c < 6; c += 2) ok = ok && (k == mid ? (q[c] == 0 && q[c + 1] == 0) : q[c] >= 0.5);
            }
            bulk_uv[1] = ok;
        }
    }
    std::printf("{\"obj_same_but_uv\": %s, \"obj_absent_without_flag\": %s, \"obj_sized\": %s, \"bulk_equal_textured\": %s, \"bulk_uv_textured\": %s, "
                "\"bulk_equal_plain\": %s, \"plain_absent\": %s, \"tris\": %zu, \"uv\": [",
                obj_same ? "true" : "false", obj_absent ? "true" : "false", obj_sized ? "true" : "false", bulk_equal[1] ? "true" : "false", bulk_uv[1] ? "true" : "false",
                bulk_equal[0] ? "true" : "false", bulk_uv[0] ? "true" : "false", (size_t)with.tri_mat.size());
    for (size_t k = 0; k < with.tri_uv.size(); k++) std::printf("%s%.17g", k ? ", " : "", with.tri_uv[k]);
    std::printf("]}\n");
    return 0;
}
