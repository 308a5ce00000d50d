// zr_scenes_mix.inc — small parity scenes that exercise every primitive, wrapper, material and texture on
// the path at least once (SURVEY.md §8a rows a-11 … a-22).  Same rules as zr_scenes.inc: reference public
// API only, one statement per random draw, no reference code.

static inline std::string zr_write_ppm(const std::string& path, int W, int H, int variant) {
    // binary P6: stb_image decodes PNM (texture.hpp:31), and the drop-in has its own P6 reader
    std::vector<unsigned char> px((size_t)W * H * 3);
    for (int j = 0; j < H; j++)
        for (int i = 0; i < W; i++) {
            unsigned char* p = &px[((size_t)j * W + i) * 3];
            if (variant == 0) {  // colourful albedo
                p[0] = (unsigned char)((i * 255) / (W - 1));
                p[1] = (unsigned char)((j * 255) / (H - 1));
                p[2] = (unsigned char)(((i ^ j) & 1) ? 220 : 40);
            } else {  // height field for bump mapping
                int v = (int)(127.5 + 127.5 * std::sin(i * 0.9) * std::cos(j * 1.3));
                p[0] = p[1] = p[2] = (unsigned char)v;
            }
        }
    FILE* f = std::fopen(path.c_str(), "wb");
    if (!f) { std::fprintf(stderr, "zr_scenes: cannot write %s\n", path.c_str()); return path; }
    std::fprintf(f, "P6\n%d %d\n255\n", W, H);
    std::fwrite(px.data(), 1, px.size(), f);
    std::fclose(f);
    return path;
}

static inline void zr_quad(hittable_list& w, point3 a, point3 b, point3 c, point3 d, vec3 na, vec3 nb, vec3 nc, vec3 nd,
                           shared_ptr<material> m) {
    w.add(make_shared<triangle>(a, b, c, na, nb, nc, m));
    w.add(make_shared<triangle>(a, c, d, na, nc, nd, m));
}

// variant 0: PHYSICAL_SUN (low sun: sunset branch + sun disc), pinhole camera
// variant 1: HDR_MAP 64x32 with yaw/tilt/roll, thin-lens camera
// variant 2: SOLID_COLOR grey background, deep paths (max_depth 40: exercises Russian roulette)
static inline void zr_build_mix(zr_demo_scene& s, int variant, const std::string& tmpdir = "/tmp") {
    s.name = "mix" + std::to_string(variant); s.seed = 0x5EED1000ull + (uint64_t)variant;
    std::string tag = std::to_string((long)getpid());
    std::string ppm_a = zr_write_ppm(tmpdir + "/zr_mix_albedo_" + tag + ".ppm", 16, 8, 0);
    std::string ppm_b = zr_write_ppm(tmpdir + "/zr_mix_bump_" + tag + ".ppm", 32, 32, 1);
    s.temp_files.push_back(ppm_a); s.temp_files.push_back(ppm_b);
    auto tex_img = make_shared<image_texture>(ppm_a.c_str());
    auto tex_bump = make_shared<image_texture>(ppm_b.c_str());
    auto tex_chk = make_shared<checker_texture>(0.32, color(.2, .3, .1), color(.9, .9, .9));
    auto tex_chk2 = make_shared<checker_texture>(0.7, make_shared<solid_color>(0.9, 0.2, 0.2), tex_chk);

    auto m_ground = make_shared<lambertian>(tex_chk);
    auto m_metal_fuzzy = make_shared<metal>(color(0.8, 0.7, 0.6), 0.3);
    auto m_mirror_chk = make_shared<metal>(tex_chk2, 0.0);
    auto m_glass = make_shared<dielectric>(1.5, color(0.9, 1.0, 0.9));
    auto m_light = make_shared<diffuse_light>(color(4, 4, 4));
    auto m_red = make_shared<lambertian>(color(0.7, 0.1, 0.1));
    auto m_img = make_shared<lambertian>(tex_img);
    auto m_bumpy = make_shared<lambertian>(color(0.6, 0.6, 0.8), tex_bump, 2.0);
    auto m_bumpy_metal = make_shared<metal>(color(0.9, 0.8, 0.5), 0.05, tex_bump, 1.5);
    auto m_bumpy_glass = make_shared<dielectric>(1.3, tex_bump, 0.7);
    auto m_blue = make_shared<lambertian>(color(0.1, 0.2, 0.7));

    s.world.add(make_shared<sphere>(point3(0, -1000, 0), 1000.0, m_ground));
    s.world.add(make_shared<sphere>(point3(-2.2, 1, 0), 1.0, m_metal_fuzzy));
    s.world.add(make_shared<sphere>(point3(0, 1, 0), 1.0, m_glass));
    s.world.add(make_shared<sphere>(point3(2.2, 1, 0), 1.0, m_mirror_chk));
    s.world.add(make_shared<sphere>(point3(0, 4.5, 2), 0.6, m_light));
    s.world.add(make_shared<sphere>(point3(-1, 0.5, 2.2), 0.5, m_img));
    s.world.add(make_shared<sphere>(point3(0.3, 0.5, 2.5), 0.5, m_bumpy));
    s.world.add(make_shared<sphere>(point3(1.6, 0.5, 2.3), 0.5, m_bumpy_metal));
    s.world.add(make_shared<sphere>(point3(-2.3, 0.45, 2.4), 0.45, m_bumpy_glass));

    // flat quad and a "smooth" quad with tilted vertex normals
    zr_quad(s.world, point3(3.5, 0, -1.5), point3(5.5, 0, -1.5), point3(5.5, 2, -1.5), point3(3.5, 2, -1.5),
            vec3(0, 0, 1), vec3(0, 0, 1), vec3(0, 0, 1), vec3(0, 0, 1), m_red);
    zr_quad(s.world, point3(-5.5, 0, -1.0), point3(-3.5, 0, -1.8), point3(-3.5, 2, -1.8), point3(-5.5, 2, -1.0),
            unit_vector(vec3(-0.3, 0, 1)), unit_vector(vec3(0.6, 0.1, 1)), unit_vector(vec3(0.6, -0.1, 1)),
            unit_vector(vec3(-0.3, 0.2, 1)), m_metal_fuzzy);
    // a degenerate triangle (zero area) must never be hit (triangle.hpp:24-26)
    s.world.add(make_shared<triangle>(point3(0, 3, 0), point3(1, 3, 0), point3(2, 3, 0), vec3(0, 1, 0), vec3(0, 1, 0),
                                      vec3(0, 1, 0), m_red));

    // wrapper chains in the order scene_management.hpp:178-188 uses: scale -> rotate_y -> material_instance -> translate
    {
        auto master = make_shared<cube>(point3(-0.4, -0.4, -0.4), point3(0.4, 0.4, 0.4), nullptr);
        auto sc = make_shared<scale>(master, vec3(1.0, 2.0, 1.0));
        auto ry = make_shared<rotate_y>(sc, 0.5);
        auto mi = make_shared<material_instance>(ry, m_blue);
        s.world.add(make_shared<translate>(mi, vec3(3.6, 0.8, 2.0)));
    }
    {
        auto c = make_shared<cube>(point3(0, 0, 0), m_metal_fuzzy);  // 2-arg ctor: half extents 1
        auto sc = make_shared<scale>(c, vec3(0.35, 0.35, 0.35));
        auto rx = make_shared<rotate_x>(sc, 30.0);   // degrees (rotate_x.hpp:10)
        auto rz = make_shared<rotate_z>(rx, -20.0);  // degrees
        s.world.add(make_shared<translate>(rz, vec3(-3.8, 0.9, 2.2)));
    }
    {
        // glass sphere inside translate: front_face is forced true on exit (translate.hpp:29)
        auto g = make_shared<sphere>(point3(0, 0, 0), 0.6, make_shared<dielectric>(1.5));
        s.world.add(make_shared<translate>(g, vec3(1.0, 0.6, -2.2)));
        // material_instance with a null material falls back to magenta lambertian (material_instance.hpp:22-26)
        auto g2 = make_shared<sphere>(point3(0, 0, 0), 0.4, nullptr);
        auto mi = make_shared<material_instance>(g2, nullptr);
        s.world.add(make_shared<translate>(mi, vec3(-1.0, 0.4, -2.0)));
    }
    // two media: a dense coloured ball and a thin global fog
    {
        auto b1 = make_shared<sphere>(point3(-4, 1.2, 2), 1.2, nullptr);
        s.world.add(zr_hook_medium(make_shared<constant_medium>(b1, 0.8, color(0.2, 0.4, 0.9))));
        auto b2 = make_shared<sphere>(point3(0, 0, 0), 30.0, nullptr);
        s.world.add(zr_hook_medium(make_shared<constant_medium>(b2, 0.01, make_shared<solid_color>(1.0, 1.0, 1.0))));
    }

    zr_cam_defaults(s.cam);
    s.cam.image_width = 96; s.cam.image_height = 64; s.cam.samples_per_pixel = 32; s.cam.max_depth = 12;
    s.cam.vfov = 35; zr_set3(s.cam.lookfrom, 1.5, 3.0, 11); zr_set3(s.cam.lookat, 0, 1, 0);
    s.cam.defocus_angle = 0; s.cam.focus_dist = 10;
    if (variant == 0) {
        s.env.sun_direction = vec3(1.0, 0.06, -0.45);  // not normalised on purpose (camera.hpp:874 normalises)
        s.env.sun_size = 8.0; s.env.sun_intensity = 3.0; s.env.intensity = 0.8;
    } else if (variant == 1) {
        std::string hdr = zr_write_synthetic_hdr(tmpdir + "/zr_mix_env_" + tag + ".hdr", 64, 32);
        s.temp_files.push_back(hdr);
        s.env.load_hdr(hdr);
        s.env.hdri_rotation = 0.7; s.env.hdri_tilt = -0.2; s.env.hdri_roll = 0.15; s.env.intensity = 0.6;
        s.cam.defocus_angle = 1.2; s.cam.focus_dist = 11.0;
    } else {
        s.env.set_mode(EnvironmentSettings::SOLID_COLOR);
        s.env.background_color = color(0.25, 0.25, 0.3);
        s.env.intensity = 1.2;
        s.cam.max_depth = 40; s.cam.samples_per_pixel = 24;
    }
}


// ---- mesh0: OBJ ingest through `model` (model.hpp:12-103) ------------------------------------------------------
// Two generated Wavefront files: a (2,3) torus-knot tube made of QUADS with per-vertex normals (exercises the
// loader's quad split and the smooth-normal path) and a unit cube of quads plus one triangle WITHOUT normals
// (flat-normal fallback).  Numbers are printed as %.9g of a float, so every OBJ parser recovers the same floats.
static inline std::string zr_write_knot_obj(const std::string& path, int NU, int NV) {
    FILE* f = std::fopen(path.c_str(), "w");
    if (!f) { std::fprintf(stderr, "zr_scenes: cannot write %s\n", path.c_str()); return path; }
    const double PI = 3.14159265358979323846, R = 1.0, r = 0.4, a = 0.17;
    std::fprintf(f, "# generated torus knot, quads, smooth normals\no knot\n");
    for (int iu = 0; iu < NU; iu++) {
        double t = 2 * PI * iu / NU;
        double c2 = std::cos(2 * t), s2 = std::sin(2 * t), c3 = std::cos(3 * t), s3 = std::sin(3 * t);
        double rho = R + r * c3, drho = -3 * r * s3;
        vec3 C(rho * c2, r * s3, rho * s2);
        vec3 T = unit_vector(vec3(drho * c2 - 2 * rho * s2, 3 * r * c3, drho * s2 + 2 * rho * c2));
        vec3 B = unit_vector(cross(T, vec3(c3 * c2, s3, c3 * s2)));
        vec3 N = cross(B, T);
        for (int iv = 0; iv < NV; iv++) {
            double ph = 2 * PI * iv / NV;
            vec3 d = std::cos(ph) * N + std::sin(ph) * B;
            vec3 P = C + a * d;
            std::fprintf(f, "v %.9g %.9g %.9g\n", (double)(float)P.x(), (double)(float)P.y(), (double)(float)P.z());
            std::fprintf(f, "vn %.9g %.9g %.9g\n", (double)(float)d.x(), (double)(float)d.y(), (double)(float)d.z());
        }
    }
    for (int iu = 0; iu < NU; iu++)
        for (int iv = 0; iv < NV; iv++) {
            int i00 = iu * NV + iv + 1, i10 = ((iu + 1) % NU) * NV + iv + 1, i11 = ((iu + 1) % NU) * NV + (iv + 1) % NV + 1, i01 = iu * NV + (iv + 1) % NV + 1;
            std::fprintf(f, "f %d//%d %d//%d %d//%d %d//%d\n", i00, i00, i10, i10, i11, i11, i01, i01);
        }
    std::fclose(f);
    return path;
}

static inline std::string zr_write_box_obj(const std::string& path) {
    FILE* f = std::fopen(path.c_str(), "w");
    if (!f) { std::fprintf(stderr, "zr_scenes: cannot write %s\n", path.c_str()); return path; }
    std::fprintf(f, "# skewed box: quads with unequal diagonals, no normals, relative indices, one extra triangle\n");
    const double v[8][3] = {{0, 0, 0}, {1.25, 0, 0}, {1.25, 0.5, 0.125}, {0, 0.75, 0}, {0, 0, 1}, {1.25, 0, 1.5}, {1.5, 0.75, 1.25}, {0, 0.5, 1}};
    for (auto& q : v) std::fprintf(f, "v %.9g %.9g %.9g\n", q[0], q[1], q[2]);
    std::fprintf(f, "f 1 4 3 2\nf 5 6 7 8\nf 1 2 6 5\nf 2 3 7 6\nf 3 4 8 7\nf -8 -4 -1 -5\n");
    std::fprintf(f, "v 0.5 1.5 0.5\nf 4 9 3\n");
    std::fclose(f);
    return path;
}

static inline void zr_build_mesh0(zr_demo_scene& s, const std::string& tmpdir = "/tmp") {
    s.name = "mesh0"; s.seed = 0x5EED2000ull;
    std::string tag = std::to_string((long)getpid());
    std::string knot = zr_write_knot_obj(tmpdir + "/zr_mesh_knot_" + tag + ".obj", 60, 12);
    std::string box = zr_write_box_obj(tmpdir + "/zr_mesh_box_" + tag + ".obj");
    s.temp_files.push_back(knot); s.temp_files.push_back(box);
    auto m_ground = make_shared<lambertian>(make_shared<checker_texture>(0.5, color(.15, .2, .3), color(.85, .85, .8)));
    auto m_gold = make_shared<metal>(color(0.9, 0.75, 0.4), 0.15);
    auto m_clay = make_shared<lambertian>(color(0.7, 0.3, 0.25));
    auto m_light = make_shared<diffuse_light>(color(5, 5, 5));
    s.world.add(make_shared<sphere>(point3(0, -1000, 0), 1000.0, m_ground));
    {   // like the reference's teapot chain (scene_management.hpp:112-117) but with rotate_z instead of rotate_y: rotate_y
        // builds its bounding box with the inverse rotation (rotate_y.hpp:26-27), so around a mesh that is not symmetric
        // about y the reference culls real geometry depending on its random BVH — not a reproducible behaviour
        auto mesh = make_shared<model>(knot, nullptr, 1.3);
        auto inst = make_shared<material_instance>(mesh, m_gold);
        auto rx = make_shared<rotate_x>(inst, -90.0);
        auto rz = make_shared<rotate_z>(rx, 25.0);
        s.world.add(make_shared<translate>(rz, point3(0.0, 1.4, 0.0)));
    }
    s.world.add(make_shared<translate>(make_shared<model>(box, m_clay, 0.9), vec3(2.4, 0.0, 0.6)));
    s.world.add(make_shared<model>(box, m_clay, 0.5));   // bare mesh at the origin
    s.world.add(make_shared<sphere>(point3(-2.5, 3.5, 2.0), 0.7, m_light));
    zr_cam_defaults(s.cam);
    s.cam.image_width = 96; s.cam.image_height = 64; s.cam.samples_per_pixel = 16; s.cam.max_depth = 8;
    s.cam.vfov = 38; zr_set3(s.cam.lookfrom, 3.5, 3.2, 7.5); zr_set3(s.cam.lookat, 0.6, 1.0, 0);
    s.cam.defocus_angle = 0; s.cam.focus_dist = 10;
}

// "inst0": ONE mesh placed many times — what translate / rotate_* / scale / material_instance around a shared model are for in
// the reference (the same shared_ptr<hittable> in every wrapper) and what the drop-in stores as a two-level BVH: a knot placed
// 36 times (scale -> material_instance -> rotate_x -> rotate_z -> translate, every parameter a function of the index) and a
// box placed 8 times under a bare translate, over a checker ground, lit by the sky and one light.  rotate_y is kept away from
// the meshes for the reason given in mesh0.
static inline void zr_build_inst0(zr_demo_scene& s, const std::string& tmpdir = "/tmp") {
    s.name = "inst0"; s.seed = 0x5EED2100ull;
    std::string tag = std::to_string((long)getpid());
    std::string knot = zr_write_knot_obj(tmpdir + "/zr_inst_knot_" + tag + ".obj", 48, 10);
    std::string box = zr_write_box_obj(tmpdir + "/zr_inst_box_" + tag + ".obj");
    s.temp_files.push_back(knot); s.temp_files.push_back(box);
    auto m_ground = make_shared<lambertian>(make_shared<checker_texture>(0.6, color(.2, .25, .3), color(.8, .8, .75)));
    shared_ptr<material> pal[4] = {make_shared<metal>(color(0.9, 0.75, 0.4), 0.1), make_shared<lambertian>(color(0.7, 0.3, 0.25)),
                                   make_shared<metal>(color(0.8, 0.85, 0.9), 0.0), make_shared<lambertian>(color(0.25, 0.55, 0.35))};
    auto m_light = make_shared<diffuse_light>(color(6, 6, 6));
    s.world.add(make_shared<sphere>(point3(0, -1000, 0), 1000.0, m_ground));
    auto mesh = make_shared<model>(knot, pal[1], 1.0);    // the shared child
    for (int i = 0; i < 6; i++)
        for (int j = 0; j < 6; j++) {
            const int k = 6 * i + j;
            const double f = 0.45 + 0.05 * ((k * 7) % 5);
            auto sc = make_shared<scale>(mesh, vec3(f, f, f));
            auto mi = make_shared<material_instance>(sc, pal[k % 4]);
            auto rx = make_shared<rotate_x>(mi, -90.0 + 11.0 * (k % 7));
            auto rz = make_shared<rotate_z>(rx, 9.0 * ((k * 5) % 8));
            s.world.add(make_shared<translate>(rz, vec3(-5.0 + 2.0 * i, 0.9 + 0.15 * ((k * 3) % 4), -5.0 + 2.0 * j)));
        }
    auto crate = make_shared<model>(box, pal[3], 0.6);
    for (int k = 0; k < 8; k++) s.world.add(make_shared<translate>(crate, vec3(-6.0 + 1.7 * k, 0.0, 6.6)));
    s.world.add(make_shared<sphere>(point3(-3.0, 6.0, 3.0), 1.0, m_light));
    zr_cam_defaults(s.cam);
    s.cam.image_width = 128; s.cam.image_height = 80; s.cam.samples_per_pixel = 16; s.cam.max_depth = 8;
    s.cam.vfov = 42; zr_set3(s.cam.lookfrom, 9.5, 6.5, 11.0); zr_set3(s.cam.lookat, 0.0, 0.6, 0.0);
    s.cam.defocus_angle = 0; s.cam.focus_dist = 10;
}

// "inst1": the corners of the grouping rule — a shared bvh_node that holds a sphere next to its triangles (not a run of bare
// triangles: every placement is flattened primitive by primitive), a shared model under nested translates (one chain of two ops per
// placement), the same model once more bare (a world-list entry of its own beside its group), and a model placed only once (no group).
static inline void zr_build_inst1(zr_demo_scene& s, const std::string& tmpdir = "/tmp") {
    s.name = "inst1"; s.seed = 0x5EED2200ull;
    std::string tag = std::to_string((long)getpid());
    std::string box = zr_write_box_obj(tmpdir + "/zr_inst1_box_" + tag + ".obj");
    std::string knot = zr_write_knot_obj(tmpdir + "/zr_inst1_knot_" + tag + ".obj", 24, 6);
    s.temp_files.push_back(box); s.temp_files.push_back(knot);
    auto m_ground = make_shared<lambertian>(color(0.55, 0.55, 0.5));
    auto m_red = make_shared<lambertian>(color(0.7, 0.25, 0.2));
    auto m_steel = make_shared<metal>(color(0.8, 0.85, 0.9), 0.05);
    auto m_glass = make_shared<dielectric>(1.5);
    s.world.add(make_shared<sphere>(point3(0, -1000, 0), 1000.0, m_ground));
    hittable_list mixed;
    mixed.add(make_shared<sphere>(point3(0.0, 0.5, 0.0), 0.5, m_glass));
    mixed.add(make_shared<triangle>(point3(-0.8, 0.0, -0.8), point3(0.8, 0.0, -0.8), point3(0.0, 1.6, -0.8), vec3(0, 0, 1), vec3(0, 0, 1), vec3(0, 0, 1), m_red));
    mixed.add(make_shared<triangle>(point3(-0.8, 0.0, -0.8), point3(0.0, 1.6, -0.8), point3(-0.8, 1.6, -0.8), vec3(0, 0, 1), vec3(0, 0, 1), vec3(0, 0, 1), m_steel));
    auto shared_mixed = make_shared<bvh_node>(mixed);
    for (int k = 0; k < 3; k++) s.world.add(make_shared<translate>(shared_mixed, vec3(-3.0 + 3.0 * k, 0.0, -2.0)));
    auto crate = make_shared<model>(box, m_red, 0.8);
    for (int k = 0; k < 4; k++) {
        auto inner = make_shared<translate>(crate, vec3(0.0, 0.0, 0.3 * k));
        s.world.add(make_shared<translate>(make_shared<rotate_z>(inner, 10.0 * k), vec3(-3.5 + 2.2 * k, 0.0, 1.5)));
    }
    s.world.add(crate);   // bare, at the origin
    s.world.add(make_shared<translate>(make_shared<material_instance>(make_shared<model>(knot, m_red, 0.9), m_steel), vec3(0.0, 1.2, 3.5)));
    zr_cam_defaults(s.cam);
    s.cam.image_width = 112; s.cam.image_height = 72; s.cam.samples_per_pixel = 16; s.cam.max_depth = 8;
    s.cam.vfov = 40; zr_set3(s.cam.lookfrom, 5.0, 4.0, 10.0); zr_set3(s.cam.lookat, 0.0, 0.7, 0.5);
    s.cam.defocus_angle = 0; s.cam.focus_dist = 10;
}

// "inst2": a COMPOSITE prefab and a group inside a group.  The prefab is a shared bvh_node over a list that holds a mesh (itself a
// shared `model`, under a translate of its own: a shared child inside a shared child), a glass sphere, a rotated cube under
// translate and a pedestal of six bare triangles; it is placed `copies` times under scale -> material_instance? -> rotate_z ->
// translate chains.  The inner mesh is also placed three times by itself, and a second prefab is placed once.  Through the drop-in
// the mesh's triangles and the pedestal are stored once (zr_groups), whatever `copies` is.
static inline void zr_build_inst2(zr_demo_scene& s, int copies = 6, const std::string& tmpdir = "/tmp") {
    s.name = "inst2"; s.seed = 0x5EED2300ull;
    std::string tag = std::to_string((long)getpid());
    std::string knot = zr_write_knot_obj(tmpdir + "/zr_inst2_knot_" + tag + ".obj", 30, 8);
    s.temp_files.push_back(knot);
    auto m_ground = make_shared<lambertian>(color(0.5, 0.52, 0.5));
    auto m_red = make_shared<lambertian>(color(0.7, 0.25, 0.2));
    auto m_blue = make_shared<lambertian>(color(0.2, 0.3, 0.7));
    auto m_steel = make_shared<metal>(color(0.8, 0.85, 0.9), 0.05);
    auto m_glass = make_shared<dielectric>(1.5);
    s.world.add(make_shared<sphere>(point3(0, -1000, 0), 1000.0, m_ground));
    auto mesh = make_shared<model>(knot, m_red, 0.9);   // shared: inside the prefab AND placed by itself
    hittable_list parts;
    parts.add(make_shared<translate>(mesh, vec3(0.0, 0.75, 0.0)));
    parts.add(make_shared<sphere>(point3(0.0, 0.45, 0.9), 0.3, m_glass));
    parts.add(make_shared<translate>(make_shared<rotate_y>(make_shared<cube>(point3(-0.25, -0.2, -0.25), point3(0.25, 0.2, 0.25), m_steel), 0.5), vec3(-0.8, 0.36, 0.3)));   // (its bottom face clear of the pedestal: coincident coplanar faces tie, and the winner of a tie is the traversal order)
    {   // pedestal: six triangles, flat normals
        const point3 a(-1.0, 0.0, -1.0), b(1.0, 0.0, -1.0), c(1.0, 0.0, 1.0), d(-1.0, 0.0, 1.0), e(0.0, 0.12, 0.0);
        const vec3 up(0, 1, 0);
        parts.add(make_shared<triangle>(a, b, e, up, up, up, m_blue)); parts.add(make_shared<triangle>(b, c, e, up, up, up, m_blue));
        parts.add(make_shared<triangle>(c, d, e, up, up, up, m_blue)); parts.add(make_shared<triangle>(d, a, e, up, up, up, m_blue));
        parts.add(make_shared<triangle>(a, c, b, -up, -up, -up, m_blue)); parts.add(make_shared<triangle>(a, d, c, -up, -up, -up, m_blue));
    }
    auto prefab = make_shared<bvh_node>(parts);
    for (int k = 0; k < copies; k++) {
        const double sc = 0.6 + 0.08 * (k % 4);
        shared_ptr<hittable> h = make_shared<scale>(prefab, vec3(sc, sc, sc));
        if (k % 3 == 1) h = make_shared<material_instance>(h, m_steel);
        h = make_shared<rotate_z>(h, 4.0 * (k % 5) - 8.0);
        s.world.add(make_shared<translate>(h, vec3(-5.0 + 2.1 * (k % 6), 0.0, -2.5 + 2.6 * (k / 6))));
    }
    for (int k = 0; k < 3; k++) s.world.add(make_shared<translate>(make_shared<rotate_x>(mesh, 25.0 * k), vec3(-3.0 + 3.0 * k, 1.0, 3.2)));
    {   // a prefab placed only once: nothing to share
        hittable_list once;
        once.add(make_shared<sphere>(point3(0, 0.3, 0), 0.3, m_red));
        once.add(make_shared<triangle>(point3(-0.5, 0, -0.5), point3(0.5, 0, -0.5), point3(0, 0.9, -0.5), vec3(0, 0, 1), vec3(0, 0, 1), vec3(0, 0, 1), m_steel));
        s.world.add(make_shared<translate>(make_shared<bvh_node>(once), vec3(4.5, 0.0, 3.0)));
    }
    zr_cam_defaults(s.cam);
    s.cam.image_width = 128; s.cam.image_height = 80; s.cam.samples_per_pixel = 16; s.cam.max_depth = 8;
    s.cam.vfov = 42; zr_set3(s.cam.lookfrom, 1.0, 5.5, 11.0); zr_set3(s.cam.lookat, 0.0, 0.6, 0.3);
    s.cam.defocus_angle = 0; s.cam.focus_dist = 10;
}

// "demo": the workload of the reference's own demo scene (scene_management.hpp:103-236) — a checker ground under a
// material_instance, a mesh and four prefabs in the middle, a 30 x 30 grid of randomly scaled / rotated / re-materialed
// instances of one master cube and one master sphere (scale -> rotate_y -> material_instance -> translate, rotate_y fed
// "degrees" as the reference does), and a fog volume.  The mesh chain uses rotate_z for the reason given in mesh0; the
// material library is this file's own (the reference's needs its asset textures).
static inline void zr_build_demo(zr_demo_scene& s, int grid = 15, const std::string& tmpdir = "/tmp") {
    s.name = "demo"; s.seed = 0x5EED3000ull;
    zr_hook_seed_scene(s.seed, 0);
    std::string tag = std::to_string((long)getpid());
    std::string knot = zr_write_knot_obj(tmpdir + "/zr_demo_knot_" + tag + ".obj", 120, 16);
    std::string bump = zr_write_ppm(tmpdir + "/zr_demo_bump_" + tag + ".ppm", 32, 32, 1);
    s.temp_files.push_back(knot); s.temp_files.push_back(bump);
    auto tex_bump = make_shared<image_texture>(bump.c_str());
    auto m_floor = make_shared<metal>(make_shared<checker_texture>(1.0, color(.05, .05, .05), color(.9, .9, .9)), 0.08);
    auto m_glass = make_shared<dielectric>(1.5);
    auto m_bubble = make_shared<dielectric>(1.0 / 1.5);
    auto m_steel = make_shared<metal>(color(0.85, 0.9, 0.95), 0.02);
    auto m_mirror = make_shared<metal>(color(0.95, 0.95, 0.95), 0.0, tex_bump, 0.4);
    auto m_gold = make_shared<metal>(color(0.9, 0.75, 0.4), 0.1, tex_bump, 0.8);
    auto m_wood = make_shared<lambertian>(color(0.55, 0.35, 0.2), tex_bump, 1.5);
    std::vector<shared_ptr<material>> glow = {make_shared<diffuse_light>(color(6, 1, 1)), make_shared<diffuse_light>(color(1, 6, 2)),
                                              make_shared<diffuse_light>(color(1, 2, 7)), make_shared<diffuse_light>(color(5, 4, 1))};
    std::vector<shared_ptr<material>> plain = {make_shared<lambertian>(color(0.7, 0.2, 0.2)), make_shared<lambertian>(color(0.2, 0.6, 0.3)),
                                                 make_shared<lambertian>(color(0.25, 0.3, 0.75)), make_shared<metal>(color(0.8, 0.8, 0.8), 0.3),
                                                 make_shared<metal>(color(0.9, 0.6, 0.3), 0.05), m_wood,
                                                 make_shared<lambertian>(make_shared<checker_texture>(0.11, color(.9, .1, .1), color(.9, .9, .9)))};
    // 1. floor
    s.world.add(make_shared<material_instance>(make_shared<sphere>(point3(0.0, -1000.0, 0.0), 1000.0, nullptr), m_floor));
    // 2. free-standing shape
    {
        auto mesh = make_shared<model>(knot, nullptr, 1.1);
        auto inst = make_shared<material_instance>(mesh, m_glass);
        auto rx = make_shared<rotate_x>(inst, -90.0);
        auto rz = make_shared<rotate_z>(rx, 30.0);
        s.world.add(make_shared<translate>(rz, point3(0.0, 1.0, -2.5)));
    }
    auto mirror_ball = make_shared<sphere>(point3(0.0, 0.0, 0.0), 1.0, nullptr);
    s.world.add(make_shared<translate>(make_shared<material_instance>(mirror_ball, m_mirror), point3(0.0, 1.0, 0.0)));
    auto half_ball = make_shared<sphere>(point3(0.0, 0.0, 0.0), 0.5, nullptr);
    s.world.add(make_shared<translate>(make_shared<material_instance>(half_ball, m_gold), point3(3.0, 0.5, -1.0)));
    s.world.add(make_shared<translate>(make_shared<material_instance>(half_ball, m_wood), point3(3.0, 0.5, 1.0)));
    // the reference gives this cube a glass material.  cube::hit returns t = ray_t.min for a ray that starts inside
    // (cube.hpp:44-73), so a ray refracted into a glass cube advances in steps of exactly 0.001 and meets the faces at
    // parametric distances that TIE with ray_t.min by construction; which side of the tie it lands on depends on the
    // last bit of the ray origin, i.e. on the compiler's rounding of everything upstream (measured: 17 of 1536 pixels of
    // this tile flipped between the CPU and the GPU arithmetic).  Not a reproducible behaviour: the parity scene uses a
    // metal here, glass stays on the spheres and on the mesh.
    auto steel_block = make_shared<cube>(point3(0.0, 0.0, 0.0), nullptr);
    s.world.add(make_shared<translate>(make_shared<material_instance>(steel_block, m_steel), point3(0.0, 1.0, 2.5)));
    // 3. the random grid.  The reference's `model` builds its own bvh_node, whose constructor draws from the global
    // generator (bvh.hpp:17); the drop-in's does not, so the grid gets a stream of its own
    zr_hook_seed_scene(s.seed, 1);
    auto cube_prefab = make_shared<cube>(point3(-0.2, -0.2, -0.2), point3(0.2, 0.2, 0.2), nullptr);
    auto ball_prefab = make_shared<sphere>(point3(0.0, 0.0, 0.0), 0.2, nullptr);
    for (int a = -grid; a < grid; a++) {
        for (int b = -grid; b < grid; b++) {
            double ox = random_double();
            double oz = random_double();
            point3 where(a + 0.9 * ox, 0.2, b + 0.9 * oz);
            if ((where - point3(4.0, 0.2, 0.0)).length() > 0.9) {
                shared_ptr<material> mat;
                shared_ptr<hittable> shape;
                vec3 factors(1.0, 1.0, 1.0);
                double roll = random_double();
                if (roll < 0.25) {
                    int k = random_int(0, (int)glow.size() - 1);
                    mat = glow[(size_t)k];
                    shape = cube_prefab;
                    double sy = random_double(1.5, 4.5);
                    factors = vec3(0.4, sy, 0.4);
                } else if (roll < 0.55) {
                    double g = random_double();
                    mat = g < 0.7 ? m_glass : m_bubble;
                    shape = ball_prefab;
                    double sc = random_double(0.5, 1.0);
                    factors = vec3(sc, sc, sc);
                } else {
                    int k = random_int(0, (int)plain.size() - 1);
                    mat = plain[(size_t)k];
                    double pick = random_double();
                    if (pick < 0.5) shape = ball_prefab; else shape = cube_prefab;
                    double sc = random_double(0.8, 1.2);
                    factors = vec3(sc, sc, sc);
                }
                shared_ptr<hittable> obj = make_shared<scale>(shape, factors);
                if (shape == cube_prefab) {
                    double ang = random_double(0.0, 90.0);
                    obj = make_shared<rotate_y>(obj, ang);
                }
                s.world.add(make_shared<translate>(make_shared<material_instance>(obj, mat), where));
            }
        }
    }
    // 4. fog
    s.world.add(zr_hook_medium(make_shared<constant_medium>(make_shared<sphere>(point3(0.0, 0.0, 0.0), 50.0, nullptr), 0.012, color(0.8, 0.85, 0.9))));
    zr_cam_defaults(s.cam);
    s.cam.image_width = 1280; s.cam.image_height = 720; s.cam.samples_per_pixel = 128; s.cam.max_depth = 10;
    s.cam.vfov = 30; zr_set3(s.cam.lookfrom, 10, 3.0, 4.0); zr_set3(s.cam.lookat, 0, 0.8, 0);
    s.cam.defocus_angle = 0.5; s.cam.focus_dist = 10;
}

// "kat0": a few isolated objects for the per-function known-answer tests (SURVEY.md 8c (1)): hand-placed rays meet them at
// triangle edges / vertices / exactly at ray_t.max, at sphere poles, from inside the cube, at grazing angles inside glass, ...
// and `kat_textures` lists the textures whose value(u, v, p) is evaluated at and beyond the edges of [0, 1].
static inline void zr_build_kat0(zr_demo_scene& s, const std::string& tmpdir = "/tmp") {
    s.name = "kat0"; s.seed = 0x5EED3000ull;
    std::string tag = std::to_string((long)getpid());
    std::string ppm = zr_write_ppm(tmpdir + "/zr_kat_albedo_" + tag + ".ppm", 16, 8, 0);
    std::string ppm_b = zr_write_ppm(tmpdir + "/zr_kat_bump_" + tag + ".ppm", 32, 32, 1);
    std::string hdr = zr_write_synthetic_hdr(tmpdir + "/zr_kat_env_" + tag + ".hdr", 64, 32);
    s.temp_files.push_back(ppm); s.temp_files.push_back(ppm_b); s.temp_files.push_back(hdr);
    auto tex_img = make_shared<image_texture>(ppm.c_str());
    auto tex_bump = make_shared<image_texture>(ppm_b.c_str());
    auto tex_chk = make_shared<checker_texture>(0.5, color(.1, .2, .3), color(.9, .8, .7));
    auto tex_chk2 = make_shared<checker_texture>(1.5, make_shared<solid_color>(0.9, 0.1, 0.2), tex_chk);
    auto tex_missing = make_shared<image_texture>((tmpdir + "/zr_kat_no_such_file_" + tag + ".ppm").c_str());   // failed load: cyan (texture.hpp:52-54)
    s.env.load_hdr(hdr);
    s.env.hdri_rotation = 1.1; s.env.hdri_tilt = 0.35; s.env.hdri_roll = -0.4; s.env.intensity = 0.75;
    s.kat_textures = {tex_img, tex_bump, tex_chk, tex_chk2, tex_missing, s.env.hdr_texture};

    auto m_img = make_shared<lambertian>(tex_img);
    auto m_mirror = make_shared<metal>(color(0.9, 0.8, 0.7), 0.0);          // draws a unit vector although fuzz == 0
    auto m_fuzzy = make_shared<metal>(tex_chk2, 0.4, tex_bump, 1.2);
    auto m_glass = make_shared<dielectric>(1.5);
    auto m_glass_tint = make_shared<dielectric>(1.33, color(0.8, 0.9, 1.0), tex_bump, 0.5);
    auto m_light = make_shared<diffuse_light>(tex_chk);
    auto m_missing = make_shared<lambertian>(tex_missing);
    auto m_bumpy = make_shared<lambertian>(color(0.5, 0.6, 0.7), tex_bump, 2.5);

    s.world.add(make_shared<sphere>(point3(0, 4, 0), 1.0, m_img));                              // poles, u / v of the image texture
    s.world.add(make_shared<cube>(point3(-1.0, -0.5, -0.75), point3(1.0, 0.5, 0.75), m_glass_tint));   // origin-centred, bare
    s.world.add(make_shared<sphere>(point3(6, 0, 0), 1.0, m_glass));                            // both faces, total internal reflection
    s.world.add(make_shared<sphere>(point3(0, -4, 0), 1.0, m_mirror));
    s.world.add(make_shared<sphere>(point3(-6, 0, 0), 0.5, m_light));
    s.world.add(make_shared<sphere>(point3(-6, 3, 0), 0.5, m_missing));
    s.world.add(make_shared<sphere>(point3(-6, -3, 0), -0.75, m_bumpy));                        // negative radius: hit uses max(0, r) = 0 (sphere.hpp:9)
    s.world.add(make_shared<sphere>(point3(6, 4, 0), 1.0, m_fuzzy));
    s.world.add(make_shared<sphere>(point3(6, -4, 0), 1.0, m_bumpy));
    // one triangle in the plane z = -2 (exact arithmetic for axis-parallel rays), one tilted with smooth normals, one degenerate
    s.world.add(make_shared<triangle>(point3(3, 0, -2), point3(5, 0, -2), point3(3, 2, -2), vec3(0, 0, 1), vec3(0, 0, 1), vec3(0, 0, 1), m_mirror));
    s.world.add(make_shared<triangle>(point3(-5, 0, -2), point3(-3, 0.5, -2.5), point3(-4, 2, -1.5), unit_vector(vec3(0.2, 0.1, 1)),
                                      unit_vector(vec3(-0.3, 0, 1)), unit_vector(vec3(0, 0.4, 1)), m_fuzzy));
    s.world.add(make_shared<triangle>(point3(0, 8, 0), point3(1, 8, 0), point3(3, 8, 0), vec3(0, 1, 0), vec3(0, 1, 0), vec3(0, 1, 0), m_img));
    // a cube under translate (front_face forced true) and a medium in a sphere
    s.world.add(make_shared<translate>(make_shared<cube>(point3(-0.5, -0.5, -0.5), point3(0.5, 0.5, 0.5), m_glass), vec3(0, 0, 6)));
    s.world.add(zr_hook_medium(make_shared<constant_medium>(make_shared<sphere>(point3(0, 0, -8), 2.0, nullptr), 0.6, color(0.3, 0.5, 0.8))));

    zr_cam_defaults(s.cam);
    s.cam.image_width = 64; s.cam.image_height = 48; s.cam.samples_per_pixel = 8; s.cam.max_depth = 12;
    s.cam.vfov = 50; zr_set3(s.cam.lookfrom, 4, 6, 18); zr_set3(s.cam.lookat, 0, 0, 0); zr_set3(s.cam.vup, 0.1, 1, 0);
    s.cam.defocus_angle = 2.0; s.cam.focus_dist = 17.0;
}

// "kat1": wrapper chains at their edges (translate, rotate_x / rotate_y / rotate_z, scale, material_instance, and constant_medium under them) for the
// known-answer fixture tests/golden/kat_kat1.npz; tests/golden/make_golden.py kat1_inputs() places the rays and mirrors this layout.  Isolated objects,
// one per cell of a grid with pitch 8 (cell k is centred at (8 (k % 10) - 36, 8 (k / 10) - 28, 8 ((k % 10 + k / 10) % 11) - 40): no two cells of a row or
// of a column share their z, so an axis-parallel ray through one cell meets no other), every number a small integer or a dyadic fraction, opaque materials on cubes (glass on a cube is chaotic in the reference itself, DESIGN §1), glass and metal on wrapped spheres and
// triangles so that front_face and the normal reach scatter.  Cubes are origin-centred under their wrappers (cube.hpp:45-58).
// rotate_y builds its box with the inverse rotation (rotate_y.hpp:26-27) while this project bounds the true geometry: here rotate_y only ever holds a
// child whose box is symmetric about the y axis, or turns by an angle of 0, where both boxes are the same.
static inline void zr_build_kat1(zr_demo_scene& s) {
    s.name = "kat1"; s.seed = 0x5EED3100ull;
    zr_hook_seed_scene(s.seed, 0);   // the shared mesh's bvh_node draws its split axes (bvh.hpp:17)
    typedef shared_ptr<hittable> H;
    typedef shared_ptr<material> M;
    M m_glass = make_shared<dielectric>(1.5);
    M m_water = make_shared<dielectric>(1.33);
    M m_mirror = make_shared<metal>(color(0.9, 0.8, 0.7), 0.0);
    M m_fuzzy = make_shared<metal>(color(0.7, 0.8, 0.9), 0.25);
    M m_red = make_shared<lambertian>(color(0.7, 0.2, 0.2));
    M m_green = make_shared<lambertian>(color(0.2, 0.7, 0.3));
    M m_blue = make_shared<lambertian>(color(0.2, 0.3, 0.7));
    M none = nullptr;
    auto at = [](int k) { return vec3(8.0 * (k % 10) - 36.0, 8.0 * (k / 10) - 28.0, 8.0 * ((k % 10 + k / 10) % 11) - 40.0); };
    const vec3 O(0, 0, 0);
    auto ball = [](vec3 c, M m) -> H { return make_shared<sphere>(c, 1.0, m); };
    auto box = [](M m) -> H { return make_shared<cube>(point3(-1.0, -0.5, -0.75), point3(1.0, 0.5, 0.75), m); };
    // "bent": axis-aligned vertex normals that disagree, so the interpolated normal at the hit ( = (1, 0, 1) / sqrt 2 where vertex B weighs 1/2)
    // is exactly perpendicular to the direction (1, 0, -1) although the geometric normal (0, 0, 1) is not
    auto bent = [](vec3 c, M m) -> H { return make_shared<triangle>(c + vec3(-1, -1, 0), c + vec3(1, -1, 0), c + vec3(-1, 1, 0), vec3(0, 0, 1), vec3(1, 0, 0), vec3(0, 0, 1), m); };
    auto flat = [](vec3 c, M m) -> H { return make_shared<triangle>(c + vec3(-1, -1, 0), c + vec3(1, -1, 0), c + vec3(0, 1, 0), vec3(0, 0, 1), vec3(0, 0, 1), vec3(0, 0, 1), m); };
    auto T = [](H h, vec3 v) -> H { return make_shared<translate>(h, v); };
    auto S = [](H h, vec3 f) -> H { return make_shared<scale>(h, f); };
    auto RX = [](H h, double degrees) -> H { return make_shared<rotate_x>(h, degrees); };
    auto RY = [](H h, double radians) -> H { return make_shared<rotate_y>(h, radians); };
    auto RZ = [](H h, double degrees) -> H { return make_shared<rotate_z>(h, degrees); };
    auto MI = [](H h, M m) -> H { return make_shared<material_instance>(h, m); };
    const double half_pi = 1.57079632679489661923;   // pi / 2 as a double: rotate_y takes radians, sin(k half_pi) is ~1e-16 where it "should" be 0

    // cells 0-9: spheres whose tangent rays tie dot(d, outward) at exactly 0
    s.world.add(T(ball(O, m_glass), at(0)));                                          // translate: refreshes front_face with the normal already turned
    s.world.add(RY(ball(at(1), m_glass), 0.0));                                       // rotate_y(0): does the same, sin = 0 and cos = 1 exactly
    s.world.add(S(T(ball(O, m_glass), 0.5 * at(2)), vec3(2, 2, 2)));                  // translate inside a positive uniform scale
    s.world.add(T(ball(O, m_mirror), at(3)));
    s.world.add(T(ball(at(4), m_red), vec3(0, 0, 0)));                                // identity wrappers
    s.world.add(S(ball(at(5), m_fuzzy), vec3(1, 1, 1)));
    s.world.add(RX(ball(at(6), m_glass), 0.0));                                       // rotate_x / rotate_z do not refresh front_face
    s.world.add(RZ(ball(at(7), m_fuzzy), 0.0));
    s.world.add(T(T(ball(O, m_glass), vec3(1, 0, 0)), at(8) - vec3(1, 0, 0)));        // refreshed twice
    s.world.add(T(MI(RX(ball(O, m_red), 0.0), m_water), at(9)));
    // cells 10-16: the same ties on triangles with bent vertex normals
    s.world.add(T(bent(O, m_mirror), at(10)));
    s.world.add(RY(bent(at(11), m_glass), 0.0));
    s.world.add(RX(bent(at(12), m_glass), 0.0));
    s.world.add(RZ(bent(at(13), m_mirror), 0.0));
    s.world.add(T(S(bent(O, m_glass), vec3(2, 2, 2)), at(14)));                       // under a scale: never stored in world space
    s.world.add(T(RY(bent(O, m_water), 0.0), at(15)));                                // refreshed twice
    s.world.add(T(MI(bent(O, m_red), m_fuzzy), at(16)));
    // cells 20-64: rotate_x / rotate_y / rotate_z by 0, 90, -90, 180, 360 in the constructors' own units around a sphere, a cube and a triangle
    const double turns[5] = {0.0, 1.0, -1.0, 2.0, 4.0};
    for (int axis = 0; axis < 3; axis++)
        for (int j = 0; j < 5; j++)
            for (int shape = 0; shape < 3; shape++) {
                const vec3 off = axis == 1 ? vec3(0, 0, 0) : vec3(1, 1, 0);   // (rotate_y: children symmetric about the y axis)
                H h = shape == 0 ? ball(off, j % 2 ? m_mirror : m_glass) : shape == 1 ? (axis == 1 ? box(j % 2 ? m_fuzzy : m_green) : T(box(j % 2 ? m_fuzzy : m_green), off)) : flat(off, j % 2 ? m_water : m_fuzzy);
                h = axis == 0 ? RX(h, 90.0 * turns[j]) : axis == 1 ? RY(h, turns[j] * half_pi) : RZ(h, 90.0 * turns[j]);
                s.world.add(T(h, at(20 + (axis * 5 + j) * 3 + shape)));
            }
    // cells 65-82: mirrors and extreme scales around an off-centre sphere, a triangle and a cube, each sized so that the scaled object is about one unit
    const double tiny = std::ldexp(1.0, -20), huge = std::ldexp(1.0, 20);
    const vec3 factors[6] = {vec3(-1, 1, 1), vec3(1, -2, 1), vec3(-1, -1, -1), vec3(tiny, tiny, tiny), vec3(huge, huge, huge), vec3(1024.0, 1.0 / 1024.0, 1.0)};
    for (int i = 0; i < 6; i++)
        for (int shape = 0; shape < 3; shape++) {
            const vec3 f = factors[i];
            const vec3 inv(1.0 / std::fabs(f.x()), 1.0 / std::fabs(f.y()), 1.0 / std::fabs(f.z()));
            const double r = std::fmin(inv.x(), std::fmin(inv.y(), inv.z()));
            H h;
            if (shape == 0) h = make_shared<sphere>(point3(0.5 * r, 0.25 * r, 0.0), r, i % 2 ? m_mirror : m_glass);
            else if (shape == 1) h = make_shared<triangle>(point3(-inv.x(), -inv.y(), 0), point3(inv.x(), -inv.y(), 0), point3(0, inv.y(), 0), vec3(0, 0, 1), vec3(0, 0, 1), vec3(0, 0, 1), i % 2 ? m_glass : m_mirror);
            else h = make_shared<cube>(point3(-inv.x(), -0.5 * inv.y(), -0.75 * inv.z()), point3(inv.x(), 0.5 * inv.y(), 0.75 * inv.z()), i % 2 ? m_blue : m_fuzzy);
            s.world.add(T(S(h, f), at(65 + 3 * i + shape)));   // (a cube here is the placed-cube pattern translate -> scale)
        }
    s.world.add(T(RY(S(box(m_fuzzy), vec3(-1, 1, 1)), 0.5), at(83)));                 // translate -> rotate_y -> scale with a negative factor
    s.world.add(T(RY(S(box(m_red), vec3(-1, 2, -0.5)), -0.75), at(84)));              // ... and with a mixed-sign triple
    // cells 85-92 and the origin: order and depth
    s.world.add(T(RX(box(m_green), 90.0), at(85)));
    s.world.add(RX(T(box(m_green), vec3(at(86).x(), at(86).z(), -at(86).y())), 90.0));   // the same cube, wrappers swapped: rotate_x(90) takes (x, z, -y) to (x, y, z)
    s.world.add(T(RZ(S(box(m_blue), vec3(2, 1, 1)), 90.0), at(87)));                  // scale inside / outside a rotation
    s.world.add(T(S(RZ(box(m_blue), 90.0), vec3(2, 1, 1)), at(88)));
    s.world.add(T(RZ(S(MI(RX(T(RY(S(ball(O, m_red), vec3(0.5, 0.5, 0.5)), 0.0), vec3(0.5, 0, 0)), 180.0), m_glass), vec3(2, 2, 2)), 90.0), at(89)));   // ZR_MAX_CHAIN = 8 wrappers
    s.world.add(T(MI(MI(ball(O, m_red), m_green), m_mirror), at(90)));                // nested material_instance: the outer one wins
    s.world.add(MI(MI(T(ball(O, m_red), at(91)), m_blue), m_water));
    s.world.add(MI(ball(at(92), m_red), m_fuzzy));
    s.world.add(MI(MI(box(m_red), m_green), m_blue));                                 // at the origin, which is no cell's centre
    // cells 93-99: constant_medium in a sphere and in a cube, under translate, a non-uniform scale and rotate_z; the last one has the wrapper on its boundary
    auto fog = [](H boundary) -> H { return zr_hook_medium(make_shared<constant_medium>(boundary, 0.6, color(0.3, 0.5, 0.8))); };
    s.world.add(T(fog(ball(O, none)), at(93)));
    s.world.add(T(fog(box(none)), at(94)));
    s.world.add(T(S(fog(ball(O, none)), vec3(2, 0.5, 1)), at(95)));
    s.world.add(T(S(fog(box(none)), vec3(2, 0.5, 1)), at(96)));
    s.world.add(T(RZ(fog(ball(vec3(1, 1, 0), none)), 90.0), at(97)));
    s.world.add(T(RZ(fog(box(none)), 90.0), at(98)));
    s.world.add(fog(T(ball(O, none), at(99))));
    // cells 100-102: one shared mesh of six triangles (a fan of four around the origin in the plane y = 0 and a fin of two in the plane x = 0) placed three times
    {
        const point3 a(-1, 0, -1), b(1, 0, -1), c(1, 0, 1), d(-1, 0, 1), e(0, 0.25, -1), f(0, 1.25, -1), g(0, 1.25, 1), h(0, 0.25, 1);
        const vec3 up(0, 1, 0), side(1, 0, 0);
        hittable_list parts;
        parts.add(make_shared<triangle>(a, b, O, up, up, up, m_fuzzy)); parts.add(make_shared<triangle>(b, c, O, up, up, up, m_fuzzy));
        parts.add(make_shared<triangle>(c, d, O, up, up, up, m_fuzzy)); parts.add(make_shared<triangle>(d, a, O, up, up, up, m_fuzzy));
        parts.add(make_shared<triangle>(e, f, g, side, side, side, m_water)); parts.add(make_shared<triangle>(e, g, h, side, side, side, m_water));
        H mesh = make_shared<bvh_node>(parts);
        s.world.add(T(S(mesh, vec3(-1, 1, 1)), at(100)));
        s.world.add(T(RX(mesh, 90.0), at(101)));
        s.world.add(T(RY(S(mesh, vec3(2, 2, 2)), 2.0 * half_pi), at(102)));   // (the mesh's box is symmetric about the y axis)
    }
    zr_cam_defaults(s.cam);
    s.cam.image_width = 64; s.cam.image_height = 48; s.cam.samples_per_pixel = 4; s.cam.max_depth = 8;
    s.cam.vfov = 40; zr_set3(s.cam.lookfrom, 10, 20, 120); zr_set3(s.cam.lookat, 0, 12, 0);
    s.cam.defocus_angle = 0; s.cam.focus_dist = 10;
}

// "kat2": a LEAN world (DScene::shade_lean: bare spheres and triangles, and spheres / triangles under translate and rotate_y chains that the flattener bakes;
// lambertian / metal / dielectric / light over solid colours) for the known-answer fixture tests/golden/kat_kat2.npz, which pins scatter() and the lean
// pair lean_rec / lean_shade at their decision edges.  kat1's cells (pitch 8, one object per cell); tests/golden/make_golden.py kat2_inputs() places the
// rays and mirrors this layout.  Triangle forms 0-5: bare, translate, rotate_y(0), translate(translate), translate(rotate_y(0)), rotate_y(0)(translate) — chains
// of one and of two wrappers, so that both parities of reface() occur; a sphere is baked from under one translate only (classify_object).
static inline void zr_build_kat2(zr_demo_scene& s) {
    s.name = "kat2"; s.seed = 0x5EED3200ull;
    typedef shared_ptr<hittable> H;
    typedef shared_ptr<material> M;
    const M mats[10] = {make_shared<lambertian>(color(0.7, 0.2, 0.2)),
                        make_shared<metal>(color(0.9, 0.8, 0.7), 0.0), make_shared<metal>(color(0.7, 0.8, 0.9), 0.4), make_shared<metal>(color(0.6, 0.9, 0.6), 1.0),
                        make_shared<dielectric>(1.5, color(0.9, 0.8, 0.7)), make_shared<dielectric>(1.0, color(0.7, 0.9, 0.8)),
                        make_shared<dielectric>(1.0 / 1.5, color(0.8, 0.7, 0.9)), make_shared<dielectric>(2.4, color(0.95, 0.9, 0.6)),
                        make_shared<diffuse_light>(color(4.0, 3.0, 2.0)), nullptr};
    enum { LAMB = 0, MIRROR = 1, FUZZY = 2, ROUGH = 3, GLASS = 4, LIGHT = 8, NONE = 9 };
    auto at = [](int k) { return vec3(8.0 * (k % 10) - 36.0, 8.0 * (k / 10) - 28.0, 8.0 * ((k % 10 + k / 10) % 11) - 40.0); };
    const vec3 O(0, 0, 0), Z(0, 0, 1);
    // shapes 0-3: "bent" (kat1's: the interpolated normal is (1, 0, 1) / sqrt 2 on the line x = 0), "flat", "opposed" (vertex B's normal points below the
    // face: the interpolated normal opposes the geometric one for u > 5/9), "cancel" (n0 = -n1: the interpolated normal vanishes on x = 0 and unit_vector answers 0)
    auto tri = [&](int shape, vec3 c, M m) -> H {
        if (shape == 1) return make_shared<triangle>(c + vec3(-1, -1, 0), c + vec3(1, -1, 0), c + vec3(0, 1, 0), Z, Z, Z, m);
        const vec3 nb = shape == 0 ? vec3(1, 0, 0) : shape == 2 ? vec3(0.6, 0, -0.8) : vec3(0, 0, -1);
        return make_shared<triangle>(c + vec3(-1, -1, 0), c + vec3(1, -1, 0), c + vec3(-1, 1, 0), Z, nb, Z, m);
    };
    auto T = [](H h, vec3 v) -> H { return make_shared<translate>(h, v); };
    auto RY = [](H h, double radians) -> H { return make_shared<rotate_y>(h, radians); };
    auto placed = [&](int form, int shape, int cell, M m) -> H {
        const vec3 c = at(cell), e(1, 0, 0);
        switch (form) {
            case 0: return tri(shape, c, m);
            case 1: return T(tri(shape, O, m), c);
            case 2: return RY(tri(shape, c, m), 0.0);
            case 3: return T(T(tri(shape, O, m), e), c - e);
            case 4: return T(RY(tri(shape, O, m), 0.0), c);
            default: return RY(T(tri(shape, O, m), c), 0.0);
        }
    };
    // cells 0-17: the face-normal ties, every form x (lambertian, the three metals in turn, the four glasses in turn)
    for (int f = 0; f < 6; f++)
        for (int j = 0; j < 3; j++) s.world.add(placed(f, 0, 3 * f + j, mats[j == 0 ? LAMB : j == 1 ? MIRROR + f % 3 : GLASS + f % 4]));
    // cells 18-25: a flat triangle of each glass, bare and under a translate (the dielectric threshold, the hit positions)
    for (int g = 0; g < 4; g++) { s.world.add(placed(0, 1, 18 + 2 * g, mats[GLASS + g])); s.world.add(placed(1, 1, 19 + 2 * g, mats[GLASS + g])); }
    s.world.add(placed(0, 1, 26, mats[MIRROR]));
    s.world.add(T(RY(tri(1, O, mats[FUZZY]), 0.5), at(27)));   // an angle that is nothing special (the box is symmetric about the y axis: see kat1)
    s.world.add(placed(3, 1, 28, mats[LAMB]));
    s.world.add(placed(0, 1, 29, mats[LIGHT]));
    // cells 30-37: vertex normals that oppose the face, and that cancel
    s.world.add(placed(0, 2, 30, mats[MIRROR])); s.world.add(placed(1, 2, 31, mats[FUZZY])); s.world.add(placed(2, 2, 32, mats[ROUGH]));
    s.world.add(placed(0, 2, 33, mats[GLASS])); s.world.add(placed(1, 2, 34, mats[LAMB]));
    s.world.add(placed(0, 3, 35, mats[GLASS])); s.world.add(placed(1, 3, 36, mats[MIRROR])); s.world.add(placed(2, 3, 37, mats[LAMB]));
    // cells 40-55: a unit sphere of every scattering material, bare and under a translate; 56-59: the light, the null material, a negative radius
    for (int m = 0; m < 8; m++) { s.world.add(make_shared<sphere>(at(40 + 2 * m), 1.0, mats[m])); s.world.add(T(make_shared<sphere>(O, 1.0, mats[m]), at(41 + 2 * m))); }
    s.world.add(make_shared<sphere>(at(56), 1.0, mats[LIGHT]));
    s.world.add(make_shared<sphere>(at(57), 1.0, mats[NONE]));   // (bare: a sphere without a material is not baked from under a wrapper)
    s.world.add(make_shared<sphere>(at(58), -0.75, mats[LAMB]));   // hit radius max(0, r) = 0 (sphere.hpp:9)
    s.world.add(placed(0, 1, 59, mats[NONE]));
    zr_cam_defaults(s.cam);
    s.cam.image_width = 64; s.cam.image_height = 48; s.cam.samples_per_pixel = 8; s.cam.max_depth = 12;
    s.cam.vfov = 40; zr_set3(s.cam.lookfrom, 10, 20, 120); zr_set3(s.cam.lookat, 0, -4, 0);
    s.cam.defocus_angle = 0; s.cam.focus_dist = 10;
}

static inline bool zr_build_scene_mix(const std::string& name, zr_demo_scene& s, int arg0 = 0) {
    if (name == "kat0") { zr_build_kat0(s); return true; }
    if (name == "kat1") { zr_build_kat1(s); return true; }
    if (name == "kat2") { zr_build_kat2(s); return true; }
    if (name == "demo") { zr_build_demo(s); return true; }
    if (name == "mesh0") { zr_build_mesh0(s); return true; }
    if (name == "inst0") { zr_build_inst0(s); return true; }
    if (name == "inst1") { zr_build_inst1(s); return true; }
    if (name == "inst2") { zr_build_inst2(s, arg0 > 0 ? arg0 : 6); return true; }
    if (name == "mix0") { zr_build_mix(s, 0); return true; }
    if (name == "mix1") { zr_build_mix(s, 1); return true; }
    if (name == "mix2") { zr_build_mix(s, 2); return true; }
    return false;
}
