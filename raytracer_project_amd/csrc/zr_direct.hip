// zr_direct.hip — direct light sampling for gfx950 (the rules: include/zr_capi.h): the kernel that renders a batch of samples with next-event
// estimation and multiple importance sampling, the kernels that collect the scene's emitters into the light table, and the known-answer kernels.
//
// Kernel `render_direct_samples`: render_pixel_samples' layout (zr_kernels.hip) — one thread per sample, the samples of a pixel consecutive, so the 64 primary
// rays of a wave share a pixel — writing per-sample radiance for launch_accumulate.  A sample walks exactly the vertices of sample_radiance / path_radiance:
// the same camera draws, closest-hit queries, scatter() draws and Russian roulette on the main stream; light draws come from the vertex's own light stream
// (zr_light_key) and the shadow query's medium draws are keyed with bounce | 0x80000000.  Path and shadow queries share the lane's LDS stack column: a
// query leaves nothing on it.
#include "zr_device.h"
#include "zr_launch.h"
#include "zr_light.h"
#include "zr_envlight.h"

// Compiled twice like zr_kernels.hip: as itself for scenes whose triangles carry no texture coordinates, and from zr_direct_uv.hip (ZR_UV 1, namespace
// zr::uvbuild) for those that do.  The table and known-answer kernels read no coordinates and exist once.
#ifndef ZR_UV
#define ZR_UV 0
#endif
#if ZR_UV
namespace zr { namespace uvbuild {
#else
namespace zr {
namespace uvbuild {   // zr_direct_uv.hip
hipError_t launch_direct_samples(const DScene& sc, const DCamera& cam, const DEnv& env, const LightTable& lt, const EnvLight& el, uint64_t seed, const uint32_t* pixels,
                                 uint32_t n_pix, uint32_t sample0, uint32_t n, double* samples, unsigned long long* gctr, bool count, hipStream_t stream);
}
#endif

struct DirectCtr { uint32_t shadow, visible, sun, env, env_visible; };

// the sun term of background() (zr_device.h) alone: what the cone sample gathers and what a scattered ray's miss is weighted on
__device__ inline V3 sun_term(const DEnv& env, V3 rd) {
    const V3 ud = unit(rd);
    const double focus = dot(ud, mk(env.sun[0], env.sun[1], env.sun[2]));
    if (!(env.sun_on && focus > env.sun_thr)) return mk(0, 0, 0);
    const double x = clampd((focus - env.sun_thr) / ((env.sun_thr + 0.0002) - env.sun_thr), 0.0, 1.0);
    const double alpha = x * x * (3 - 2 * x);
    return mk(env.sun_add[0], env.sun_add[1], env.sun_add[2]) * alpha;
}

// D of one vertex, without the path's throughput: albedo-free f cos Le / (pdf_w + p_b) of one light sample seen from the scattered ray's origin.
// p_next: the density with which scatter() drew the direction it did, for the weight of whatever that ray finds.
// ENV: the environment table el may be sampled too; without it the function is what it was.
template <bool ENV>
__device__ inline V3 direct_term(const DScene& sc, const DEnv& env, const LightTable& lt, const EnvLight& el, const Rec& rec, const Ray& out, const Rng& g, uint32_t* stack,
                                 int stride, DirectCtr& dc, double& p_next) {
    const zr_material& m = sc.mats[rec.mat];
    const bool iso = m.kind == ZR_MAT_ISOTROPIC;
    const double INV_PI = 0.31830988618379067154, INV_4PI = 0.079577471545947667884;
    V3 wn = rec.n;   // the shading normal scatter() used
    if (!iso && m.bump_tex != ZR_NO_TEXTURE) wn = bumped_normal(sc, rec, m.bump_tex, m.bump_strength);
    p_next = iso ? INV_4PI : fmax(0.0, dot(wn, unit(out.d))) * INV_PI;
    LightRng lg; lg.key = zr_light_key(g.key, g.bounce); lg.j = 0; lg.forced = nullptr;
    LightSample s;
    V3 le_env = mk(0, 0, 0);
    if (ENV) direct_light_sample(sc, env, lt, el, out.o, lg, s, le_env); else light_sample(lt, out.o, lg, s);
    if (!(s.pdf > 0)) return mk(0, 0, 0);
    const double p_b = iso ? INV_4PI : fmax(0.0, dot(wn, s.w)) * INV_PI;   // = f cos / albedo
    if (!(p_b > 0)) return mk(0, 0, 0);
    Ray sr; sr.o = out.o; sr.d = s.w;
    Rng gs; gs.key = g.key; gs.k = 0; gs.bounce = g.bounce | 0x80000000u;
    const bool sun = s.choice == 2, sky = ENV && s.choice == 3;   // sky: a direction of the environment map, seen iff the query misses, like the sun's
    const double tol = ZR_DIRECT_T_TOL * fmax(1.0, s.dist);
    Counters none = {0, 0, 0, 0, 0};
    double t; uint32_t kind, idx;
    dc.shadow++;
    if (sun) dc.sun++;
    if (sky) dc.env++;
    const bool h = closest_hit<false>(sc, sr, 0.001, gs, stack, stride, t, kind, idx, none, sun || sky ? __builtin_huge_val() : s.dist + tol);
    V3 le;
    if (sun) {
        if (h) return mk(0, 0, 0);
        le = sun_term(env, s.w);
    } else if (sky) {
        if (h) return mk(0, 0, 0);
        le = le_env;   // the chosen texel's colour, not a second lookup of the direction
        dc.env_visible++;
    } else {
        if (!h || kind != s.kind || idx != s.index || !(fabs(t - s.dist) <= tol)) return mk(0, 0, 0);
        Rec lr;
        object_rec<true, ZR_UV != 0>(sc, kind, idx, sr, t, lr);
        le = emitted(sc, lr);
    }
    dc.visible++;
    return le * (p_b / (s.pdf + p_b));
}

// radiance of one primary sample: sample_radiance + path_radiance (zr_kernels.hip) as one loop, b = path_radiance's loop index (-1: the peeled camera vertex)
template <bool COUNT, bool ENV>
__device__ inline V3 direct_radiance(const DScene& sc, const DCamera& cam, const DEnv& env, const LightTable& lt, const EnvLight& el, int i, int j, Rng& g, uint32_t* stack,
                                     int stride, Counters& ctr, uint32_t& segments, uint32_t& hits, DirectCtr& dc) {
    Ray cur = camera_ray(cam, i, j, g);
    V3 L0 = mk(0, 0, 0), att0 = mk(1, 1, 1);   // the camera vertex: ray_color_from_hit's emitted + attenuation * ray_color
    V3 L = mk(0, 0, 0), beta = mk(1, 1, 1);
    const int depth = cam.max_depth - 1;
    const bool sampling = lt.n != 0 || lt.sun != 0 || (ENV && el.on != 0);
    bool took = false, missed = false;   // took: the vertex before took a D, with p_b the density of the direction it scattered into
    double p_b = 0;
    for (int b = -1;;) {
        double t; uint32_t kind, idx;
        segments++;
        const bool h = closest_hit<COUNT>(sc, cur, 0.001, g, stack, stride, t, kind, idx, ctr);
        g.bounce++;
        if (!h) { missed = true; break; }
        hits++;
        Rec rec;
        object_rec<true, ZR_UV != 0>(sc, kind, idx, cur, t, rec);
        V3 em = emitted(sc, rec);
        if (took && lt.n != 0 && (em.x != 0 || em.y != 0 || em.z != 0)) {
            const double p_l = light_pdf_hit(lt, sc, kind, idx, cur, t, rec);
            if (p_l > 0) em = em * (p_b / (p_b + p_l));
        }
        L = L + beta * em;
        V3 att; Ray out;
        if (!scatter(sc, cur, rec, att, out, g)) break;
        beta = beta * att;
        took = false;
        const uint32_t mk_ = sc.mats[rec.mat].kind;
        if (sampling && (mk_ == ZR_MAT_LAMBERTIAN || mk_ == ZR_MAT_ISOTROPIC) && b + 1 < depth) {   // a next segment exists: the plain path could still see light there
            L = L + beta * direct_term<ENV>(sc, env, lt, el, rec, out, g, stack, stride, dc, p_b);
            took = true;
        }
        cur = out;
        if (b > 10) {
            if (len(beta) < 0.0001) break;
            double p = fmax(fmax(beta.x, beta.y), beta.z);
            p = clampd(p, 0.05, 0.95);
            if (g.next() > p) break;
            beta = beta * (1 / p);
        }
        if (b < 0) { L0 = L; att0 = beta; L = mk(0, 0, 0); beta = mk(1, 1, 1); }   // ray_color starts its own L and beta after the peeled bounce
        b++;
        if (b >= depth) break;
    }
    if (missed) {
        V3 bg = background(sc, env, cur.d);
        if (took && lt.sun) {
            const double p_l = light_pdf_sun(lt, cur.d);
            if (p_l > 0) bg = bg - (p_l / (p_b + p_l)) * sun_term(env, cur.d);   // sky + w sun
        }
        if (ENV && took && el.on) {
            const double p_l = env_light_pdf(el, bg);   // read from the colour the lookup returned: no reverse lookup
            if (p_l > 0) bg = bg * (p_b / (p_b + p_l));
        }
        L = L + beta * bg;
    }
    return L0 + att0 * L;
}

template <bool COUNT, bool ENV>
__global__ __launch_bounds__(ZR_BLOCK) void render_direct_samples(DScene sc, DCamera cam, DEnv env, LightTable lt, EnvLight el, uint64_t seed,
                                                                   const uint32_t* __restrict__ pixels, uint32_t n_pix, uint32_t sample0, uint32_t n,
                                                                   double* __restrict__ samples, unsigned long long* __restrict__ gctr) {
    __shared__ uint32_t lds_stack[ZR_STACK_DEPTH * ZR_BLOCK];
    uint32_t* stack = lds_stack + threadIdx.x;
    const unsigned long long k = (unsigned long long)blockIdx.x * ZR_BLOCK + threadIdx.x;
    if (k >= (unsigned long long)n_pix * n) return;
    const uint32_t i = (uint32_t)(k / n), sidx = (uint32_t)(k - (unsigned long long)i * n);
    const uint32_t pk = pixels[i];
    const int px = (int)(pk & 0xFFFFu), py = (int)(pk >> 16);
    Counters ctr = {0, 0, 0, 0, 0};
    DirectCtr dc = {0, 0, 0, 0, 0};
    uint32_t segments = 0, hits = 0;
    Rng g; g.key = zr_stream_key(seed, (uint64_t)py * (uint64_t)cam.W + (uint64_t)px, (uint64_t)sample0 + sidx); g.k = 0; g.bounce = 0;
    const V3 c = direct_radiance<COUNT, ENV>(sc, cam, env, lt, el, px, py, g, stack, ZR_BLOCK, ctr, segments, hits, dc);
    double* o = samples + k * 3;
    o[0] = c.x; o[1] = c.y; o[2] = c.z;
    if (COUNT) {
        atomicAdd(&gctr[CTR_SAMPLES], 1ull);
        atomicAdd(&gctr[CTR_SEGMENTS], (unsigned long long)segments);
        atomicAdd(&gctr[CTR_NODES], (unsigned long long)ctr.nodes);
        atomicAdd(&gctr[CTR_SPHERES], (unsigned long long)ctr.sph);
        atomicAdd(&gctr[CTR_TRIANGLES], (unsigned long long)ctr.tri);
        atomicAdd(&gctr[CTR_CUBES], (unsigned long long)ctr.cube);
        atomicAdd(&gctr[CTR_MEDIA], (unsigned long long)ctr.med);
        atomicAdd(&gctr[CTR_HITS], (unsigned long long)hits);
        atomicAdd(&gctr[CTR_DRAWS], (unsigned long long)g.k);
        atomicAdd(&gctr[CTR_DIRECT_SHADOW], (unsigned long long)dc.shadow);
        atomicAdd(&gctr[CTR_DIRECT_VISIBLE], (unsigned long long)dc.visible);
        atomicAdd(&gctr[CTR_DIRECT_SUN], (unsigned long long)dc.sun);
        if (ENV) {
            atomicAdd(&gctr[CTR_DIRECT_ENV], (unsigned long long)dc.env);
            atomicAdd(&gctr[CTR_DIRECT_ENV_VISIBLE], (unsigned long long)dc.env_visible);
        }
    }
}

hipError_t launch_direct_samples(const DScene& sc, const DCamera& cam, const DEnv& env, const LightTable& lt, const EnvLight& el, uint64_t seed, const uint32_t* pixels,
                                 uint32_t n_pix, uint32_t sample0, uint32_t n, double* samples, unsigned long long* gctr, bool count, hipStream_t stream) {
#if !ZR_UV
    if (sc.tri_uv_at) return uvbuild::launch_direct_samples(sc, cam, env, lt, el, seed, pixels, n_pix, sample0, n, samples, gctr, count, stream);
#endif
    const unsigned long long blocks = ((unsigned long long)n_pix * n + ZR_BLOCK - 1) / ZR_BLOCK;
    if (blocks == 0) return hipSuccess;
    if (blocks > 0x7FFFFFFFull) return hipErrorInvalidValue;
    dim3 grid((unsigned)blocks), block(ZR_BLOCK);
    // the environment build runs only when a table is sampled: every other render goes through the kernel without it, whose frames are §20's bit for bit
    if (el.on) {
        if (count) hipLaunchKernelGGL((render_direct_samples<true, true>), grid, block, 0, stream, sc, cam, env, lt, el, seed, pixels, n_pix, sample0, n, samples, gctr);
        else hipLaunchKernelGGL((render_direct_samples<false, true>), grid, block, 0, stream, sc, cam, env, lt, el, seed, pixels, n_pix, sample0, n, samples, gctr);
    } else if (count) hipLaunchKernelGGL((render_direct_samples<true, false>), grid, block, 0, stream, sc, cam, env, lt, el, seed, pixels, n_pix, sample0, n, samples, gctr);
    else hipLaunchKernelGGL((render_direct_samples<false, false>), grid, block, 0, stream, sc, cam, env, lt, el, seed, pixels, n_pix, sample0, n, samples, gctr);
    return hipGetLastError();
}

#if !ZR_UV
// ---- the light table: mark and compact the emissive records of the final primitive arrays ------------------------------------------------------------------
// Candidates are the world-level leaf primitives in table order: the first leaf_cnt[k] records of the spheres, triangles, cubes and placed cubes.  An
// emissive sphere or triangle makes one slot, a cube six.  Three launches: slots per block of 256 candidates, an exclusive scan of the block counts by one
// block, then every block writes its slots at its offset, in candidate order — no atomics, so the order is the table's.  The host drops the slots that are
// not sampled (weight zero, negative or not finite) and makes the running sum.
__device__ __forceinline__ bool light_candidate(const DScene& sc, uint32_t c, uint32_t& kind, uint32_t& idx, uint32_t& mat) {
    const uint32_t nS = sc.leaf_cnt[ZR_PRIM_SPHERE], nT = sc.leaf_cnt[ZR_PRIM_TRIANGLE], nC = sc.leaf_cnt[ZR_PRIM_CUBE], nP = sc.leaf_cnt[ZR_KIND_PCUBE];
    if (c < nS) { kind = ZR_PRIM_SPHERE; idx = c; mat = sc.sphere_mat[idx]; if (mat != 0xFFFFFFFFu) mat &= 0x7FFFFFFFu; }
    else if (c - nS < nT) { kind = ZR_PRIM_TRIANGLE; idx = c - nS; mat = (uint32_t)__double_as_longlong(sc.tri_s[(size_t)idx * ZR_TRI_SHADE_DOUBLES + 18]); }
    else if (c - nS - nT < nC) { kind = ZR_PRIM_CUBE; idx = c - nS - nT; mat = sc.cube_mat[idx]; }
    else if (c - nS - nT - nC < nP) { kind = ZR_KIND_PCUBE; idx = c - nS - nT - nC; mat = sc.pcube_mat[idx]; }
    else return false;
    return mat < sc.n_mats && sc.mats[mat].kind == ZR_MAT_LIGHT;
}
__device__ __forceinline__ uint32_t light_slots_of(const DScene& sc, uint32_t c) {
    uint32_t kind, idx, mat;
    if (!light_candidate(sc, c, kind, idx, mat)) return 0;
    return kind == ZR_PRIM_CUBE || kind == ZR_KIND_PCUBE ? 6u : 1u;
}
// a point (or, lin: a direction) of a placed cube's own space in the world: scale, rotate_y, translate, as zr_entry.h put_pcube stores them
__device__ __forceinline__ V3 pcube_to_world(const double* q, V3 p, bool lin) {
    if (q[15] != 0.0) p = mk(p.x * q[12], p.y * q[13], p.z * q[14]);
    if (q[11] != 0.0) { const double sn = q[9], co = q[10], x = p.x, z = p.z; p.x = co * x - sn * z; p.z = sn * x + co * z; }
    if (!lin) p = p + mk(q[6], q[7], q[8]);
    return p;
}
__device__ inline void light_fill_slot(const DScene& sc, uint32_t kind, uint32_t idx, uint32_t mat, uint32_t face, zr_light_slot& s) {
    s.kind = kind; s.index = idx; s.face = face; s.cdf = 0;
    for (int k = 0; k < 3; k++) { s.o[k] = 0; s.e1[k] = 0; s.e2[k] = 0; }
    const zr_texture& tx = sc.texs[sc.mats[mat].tex];
    s.lum = tx.kind == ZR_TEX_SOLID ? 0.2126 * tx.color[0] + 0.7152 * tx.color[1] + 0.0722 * tx.color[2] : 1.0;
    if (kind == ZR_PRIM_SPHERE) {
        const double* q = sc.spheres + (size_t)idx * ZR_SPHERE_DOUBLES;
        s.type = ZR_LIGHT_SPHERE;
        s.o[0] = q[0]; s.o[1] = q[1]; s.o[2] = q[2]; s.e1[0] = q[3];
        s.area = 4.0 * 3.14159265358979323846 * q[3] * q[3];
    } else if (kind == ZR_PRIM_TRIANGLE) {
        const double* v = sc.tri_v + (size_t)idx * ZR_TRI_STRIDE;
        const V3 v0 = ld3(v), e1 = ld3(v + 3) - v0, e2 = ld3(v + 6) - v0;
        s.type = ZR_LIGHT_TRIANGLE;
        s.o[0] = v0.x; s.o[1] = v0.y; s.o[2] = v0.z; s.e1[0] = e1.x; s.e1[1] = e1.y; s.e1[2] = e1.z; s.e2[0] = e2.x; s.e2[1] = e2.y; s.e2[2] = e2.z;
        s.area = 0.5 * len(cross(e1, e2));
    } else {
        const bool placed = kind == ZR_KIND_PCUBE;
        const double* q = placed ? sc.pcubes + (size_t)idx * ZR_PCUBE_STRIDE : sc.cubes + (size_t)idx * ZR_CUBE_DOUBLES;
        const double hx = q[0], hy = q[1], hz = q[2];   // cube::hit's slabs lie about the origin (cube.hpp:57-58)
        const int axis = (int)(face >> 1);
        const double side = (face & 1u) ? 1.0 : -1.0;
        V3 o = mk(axis == 0 ? side * hx : -hx, axis == 1 ? side * hy : -hy, axis == 2 ? side * hz : -hz);
        V3 e1 = axis == 0 ? mk(0, 2 * hy, 0) : mk(2 * hx, 0, 0);
        V3 e2 = axis == 2 ? mk(0, 2 * hy, 0) : mk(0, 0, 2 * hz);
        if (placed) { o = pcube_to_world(q, o, false); e1 = pcube_to_world(q, e1, true); e2 = pcube_to_world(q, e2, true); }
        s.type = ZR_LIGHT_PARALLELOGRAM;
        s.o[0] = o.x; s.o[1] = o.y; s.o[2] = o.z; s.e1[0] = e1.x; s.e1[1] = e1.y; s.e1[2] = e1.z; s.e2[0] = e2.x; s.e2[1] = e2.y; s.e2[2] = e2.z;
        s.area = len(cross(e1, e2));
    }
    s.weight = s.area * s.lum;
}

// exclusive scan of one value per thread across the block (256 threads); returns the thread's offset, *total = the block's sum
__device__ inline uint32_t block_exclusive_scan(uint32_t v, uint32_t* sh, uint32_t* total) {
    const uint32_t tid = threadIdx.x;
    sh[tid] = v;
    __syncthreads();
    for (uint32_t d = 1; d < ZR_BLOCK; d <<= 1) {
        const uint32_t add = tid >= d ? sh[tid - d] : 0u;
        __syncthreads();
        sh[tid] += add;
        __syncthreads();
    }
    const uint32_t incl = sh[tid];
    *total = sh[ZR_BLOCK - 1];
    __syncthreads();
    return incl - v;
}

__global__ __launch_bounds__(ZR_BLOCK) void light_count(DScene sc, uint32_t n_cand, uint32_t* __restrict__ block_count) {
    __shared__ uint32_t sh[ZR_BLOCK];
    const uint32_t c = blockIdx.x * ZR_BLOCK + threadIdx.x;
    uint32_t total;
    (void)block_exclusive_scan(c < n_cand ? light_slots_of(sc, c) : 0u, sh, &total);
    if (threadIdx.x == 0) block_count[blockIdx.x] = total;
}
// one block: block_count[0 .. n_blocks) -> their exclusive prefix sums in place, *total = the sum (saturating at 0xFFFFFFFF)
__global__ __launch_bounds__(ZR_BLOCK) void light_scan(uint32_t* __restrict__ block_count, uint32_t n_blocks, uint32_t* __restrict__ total_out) {
    __shared__ uint32_t sh[ZR_BLOCK];
    unsigned long long base = 0;
    for (uint32_t first = 0; first < n_blocks; first += ZR_BLOCK) {
        const uint32_t k = first + threadIdx.x;
        const uint32_t v = k < n_blocks ? block_count[k] : 0u;
        uint32_t total;
        const uint32_t off = block_exclusive_scan(v, sh, &total);
        if (k < n_blocks) block_count[k] = (uint32_t)(base + off > 0xFFFFFFFFull ? 0xFFFFFFFFull : base + off);
        base += total;
    }
    if (threadIdx.x == 0) *total_out = (uint32_t)(base > 0xFFFFFFFFull ? 0xFFFFFFFFull : base);
}
__global__ __launch_bounds__(ZR_BLOCK) void light_emit(DScene sc, uint32_t n_cand, const uint32_t* __restrict__ block_offset, uint32_t cap, zr_light_slot* __restrict__ out) {
    __shared__ uint32_t sh[ZR_BLOCK];
    const uint32_t c = blockIdx.x * ZR_BLOCK + threadIdx.x;
    uint32_t kind = 0, idx = 0, mat = 0;
    const bool lit = c < n_cand && light_candidate(sc, c, kind, idx, mat);
    const uint32_t cnt = lit ? (kind == ZR_PRIM_CUBE || kind == ZR_KIND_PCUBE ? 6u : 1u) : 0u;
    uint32_t total;
    const uint32_t at = block_offset[blockIdx.x] + block_exclusive_scan(cnt, sh, &total);
    for (uint32_t f = 0; f < cnt; f++)
        if ((unsigned long long)at + f < cap) light_fill_slot(sc, kind, idx, mat, f, out[at + f]);
}

hipError_t launch_light_count(const DScene& sc, uint32_t n_cand, uint32_t* block_count, uint32_t* total, hipStream_t stream) {
    const uint32_t n_blocks = (n_cand + ZR_BLOCK - 1) / ZR_BLOCK;
    if (n_blocks) hipLaunchKernelGGL(light_count, dim3(n_blocks), dim3(ZR_BLOCK), 0, stream, sc, n_cand, block_count);
    hipLaunchKernelGGL(light_scan, dim3(1), dim3(ZR_BLOCK), 0, stream, block_count, n_blocks, total);
    return hipGetLastError();
}
hipError_t launch_light_emit(const DScene& sc, uint32_t n_cand, const uint32_t* block_offset, uint32_t cap, zr_light_slot* out, hipStream_t stream) {
    const uint32_t n_blocks = (n_cand + ZR_BLOCK - 1) / ZR_BLOCK;
    if (n_blocks == 0 || cap == 0) return hipSuccess;
    hipLaunchKernelGGL(light_emit, dim3(n_blocks), dim3(ZR_BLOCK), 0, stream, sc, n_cand, block_offset, cap, out);
    return hipGetLastError();
}

// ---- known-answer kernels ----------------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(ZR_BLOCK) void kat_light_sample(LightTable lt, const double* __restrict__ origins, const uint64_t* __restrict__ keys,
                                                              const uint32_t* __restrict__ bounces, const double* __restrict__ draws8, size_t n,
                                                              zr_light_sample* __restrict__ out) {
    const size_t k = (size_t)blockIdx.x * ZR_BLOCK + threadIdx.x;
    if (k >= n) return;
    LightRng lg; lg.key = zr_light_key(keys[k], bounces[k]); lg.j = 0; lg.forced = draws8 ? draws8 + k * 8 : nullptr;
    LightSample s;
    light_sample(lt, ld3(origins + k * 3), lg, s);
    zr_light_sample o;
    o.choice = s.choice; o.slot = s.slot; o.kind = s.kind; o.index = s.index; o.draws = lg.j; o.pad_ = 0;
    o.y[0] = s.y.x; o.y[1] = s.y.y; o.y[2] = s.y.z; o.normal[0] = s.n.x; o.normal[1] = s.n.y; o.normal[2] = s.n.z; o.w[0] = s.w.x; o.w[1] = s.w.y; o.w[2] = s.w.z;
    o.dist = s.dist; o.pdf = s.pdf;
    out[k] = o;
}
__global__ __launch_bounds__(ZR_BLOCK) void kat_light_pdf(DScene sc, LightTable lt, const double* __restrict__ origins, const double* __restrict__ dirs, size_t n,
                                                           double* __restrict__ out_pdf, uint64_t* __restrict__ out_key) {
    __shared__ uint32_t lds_stack[ZR_STACK_DEPTH * ZR_BLOCK];
    const size_t k = (size_t)blockIdx.x * ZR_BLOCK + threadIdx.x;
    if (k >= n) return;
    Ray r; r.o = ld3(origins + k * 3); r.d = ld3(dirs + k * 3);
    Rng g; g.key = 0; g.k = 0; g.bounce = 0;
    Counters ctr = {0, 0, 0, 0, 0};
    double t; uint32_t kind, idx;
    if (closest_hit<false>(sc, r, 0.001, g, lds_stack + threadIdx.x, ZR_BLOCK, t, kind, idx, ctr)) {
        Rec rec;
        object_rec<true, false>(sc, kind, idx, r, t, rec);   // (no coordinates wanted: the geometric normal does not read them)
        out_pdf[k] = light_pdf_hit(lt, sc, kind, idx, r, t, rec);
        out_key[k] = ((uint64_t)kind << 32) | idx;
    } else {
        out_pdf[k] = light_pdf_sun(lt, r.d);
        out_key[k] = 0xFFFFFFFFFFFFFFFFull;
    }
}
hipError_t launch_kat_light_sample(const LightTable& lt, const double* origins, const uint64_t* keys, const uint32_t* bounces, const double* draws8, size_t n,
                                   zr_light_sample* out, hipStream_t stream) {
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(kat_light_sample, dim3((unsigned)((n + ZR_BLOCK - 1) / ZR_BLOCK)), dim3(ZR_BLOCK), 0, stream, lt, origins, keys, bounces, draws8, n, out);
    return hipGetLastError();
}
hipError_t launch_kat_light_pdf(const DScene& sc, const LightTable& lt, const double* origins, const double* dirs, size_t n, double* out_pdf, uint64_t* out_key,
                                hipStream_t stream) {
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(kat_light_pdf, dim3((unsigned)((n + ZR_BLOCK - 1) / ZR_BLOCK)), dim3(ZR_BLOCK), 0, stream, sc, lt, origins, dirs, n, out_pdf, out_key);
    return hipGetLastError();
}
#endif

#if ZR_UV
}  // namespace uvbuild
#endif
}  // namespace zr

#if !ZR_UV
extern "C" uint64_t zr_kat_light_key(uint64_t key, uint32_t bounce) { return zr_light_key(key, bounce); }   // (here: the host units do not include zr_rng.h)
#endif
