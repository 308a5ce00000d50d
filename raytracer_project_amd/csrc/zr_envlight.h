// zr_envlight.h — importance sampling of the HDR environment map for direct light sampling: the environment table as the kernels get it, how a
// direction is drawn from it and the density the MIS weight of a miss reads back.  The rules are stated in include/zr_capi.h; tests/envlight_model.py
// restates this file in NumPy.  The host (g++) sees the table type and the launchers only; the device functions need zr_device.h before this header.
#pragma once
#include <stdint.h>
#include "../../include/zr_capi.h"
#include "zr_launch.h"
#include "zr_light.h"

namespace zr {

// The table travels as a kernel argument of its own, like LightTable.  cdf: H rows of W running sums of the texel weights lum x solid angle, each row from
// zero; row_cdf: the running sum of the rows' totals, total = row_cdf[H - 1]; omega: the solid angle of a texel of each row.  on = 0: nothing of the
// environment is sampled and nothing else of the struct is read.
struct EnvLight {
    const double* cdf; const double* row_cdf; const double* omega;
    uint32_t W, H;
    uint32_t on;           // 1: the map is sampled
    uint32_t tex;          // the map's texture
    double total;          // T
    double p_choice;       // 1/2 when emitters are sampled too, else 1
    double intensity;      // the environment's: radiance = texel colour x intensity
};

// zr_envlight.hip.  launch_env_row_cdf: one block per row of the map `tex`: cdf[j][0 .. W), row_total[j] = cdf[j][W - 1], row_count[j] = texels with weight.
hipError_t launch_env_row_cdf(const DScene& sc, uint32_t tex, uint32_t W, uint32_t H, const double* omega, double* cdf, double* row_total, uint32_t* row_count,
                              hipStream_t stream);
hipError_t launch_kat_env_light_sample(const DScene& sc, const DEnv& env, const LightTable& lt, const EnvLight& el, const double* origins, const uint64_t* keys,
                                       const uint32_t* bounces, const double* draws8, size_t n, zr_light_sample* out, hipStream_t stream);
hipError_t launch_kat_env_light_pdf(const DScene& sc, const DEnv& env, const EnvLight& el, const double* dirs, size_t n, double* out_pdf, hipStream_t stream);

#ifdef __HIPCC__
// texel (i, j) of an image texture at intensity 1, decoded as tex_value (zr_device.h) decodes it
__device__ __forceinline__ V3 env_texel(const DScene& sc, const zr_texture& t, uint32_t i, uint32_t j) {
    const unsigned char* base = sc.texels + t.texel_offset;
    const size_t o = ((size_t)j * t.width + i) * 3;
    if (t.kind == ZR_TEX_IMAGE_F32) {
        const float* px = (const float*)base + o;
        return mk((double)px[0], (double)px[1], (double)px[2]);
    }
    const double s = 1.0 / 255.0;
    const unsigned char* px = base + o;
    return mk(s * px[0], s * px[1], s * px[2]);
}
// luminance, summed left to right without contraction: the table must not depend on the flags of the unit that includes this
__device__ __forceinline__ double env_lum(V3 c) {
#pragma clang fp contract(off)
    return (0.2126 * c.x + 0.7152 * c.y) + 0.0722 * c.z;
}
// the weight of a texel: zero, negative or not finite counts as 0
__device__ __forceinline__ double env_weight(double lum, double omega) {
    const double w = lum * omega;
    return w > 0 && w < __builtin_huge_val() ? w : 0.0;
}

// the first entry of cdf[0 .. n) that exceeds target (the last one when none does: u * total can round up to total)
__device__ inline uint32_t env_pick(const double* __restrict__ cdf, uint32_t n, double target) {
    uint32_t lo = 0, hi = n - 1;
    while (lo < hi) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if (cdf[mid] > target) hi = mid; else lo = mid + 1;
    }
    return lo;
}

// one direction of the map: four draws (row, column, cos theta inside the row, phi inside the column).  le = the chosen texel's colour x intensity
__device__ inline void env_light_sample(const DScene& sc, const DEnv& env, const EnvLight& el, LightRng& g, LightSample& s, V3& le) {
    const double PI = 3.14159265358979323846;
    s.choice = 3; s.kind = 0xFFFFFFFFu; s.index = 0xFFFFFFFFu;
    s.y = mk(0, 0, 0); s.n = mk(0, 0, 0); s.dist = __builtin_huge_val(); s.pdf = 0;
    const double u_r = g.next(), u_c = g.next(), u_a = g.next(), u_b = g.next();
    const uint32_t j = env_pick(el.row_cdf, el.H, u_r * el.total);
    const double* row = el.cdf + (size_t)j * el.W;
    const uint32_t i = env_pick(row, el.W, u_c * row[el.W - 1]);
    s.slot = j * el.W + i;
    const double c0 = cos((double)j * PI / (double)el.H), c1 = cos((double)(j + 1) * PI / (double)el.H);
    const double ct = c0 - u_a * (c0 - c1);
    const double st = sqrt(fmax(0.0, 1.0 - ct * ct));
    const double phi = -PI + 2 * PI * ((double)i + u_b) / (double)el.W;
    const double x3 = st * cos(phi), y3 = ct, z2 = st * sin(phi);   // map space: background()'s direction after yaw, tilt and roll
    const double x1 = env.cr * x3 + env.sr * y3, y2 = -env.sr * x3 + env.cr * y3;
    const double y = env.cp * y2 + env.sp * z2, z1 = -env.sp * y2 + env.cp * z2;
    s.w = mk(env.cy * x1 - env.sy * z1, y, env.sy * x1 + env.cy * z1);
    const V3 c = env_texel(sc, sc.texs[el.tex], i, j);
    le = c * el.intensity;
    const double lum = env_lum(c);
    if (env_weight(lum, el.omega[j]) > 0) s.pdf = el.p_choice * lum / el.total;
}

// the light sample of a vertex when the environment may be sampled: emitter-or-environment first (only when both are sampled: u < 0.5 takes an emitter)
__device__ inline void direct_light_sample(const DScene& sc, const DEnv& env, const LightTable& lt, const EnvLight& el, V3 x, LightRng& g, LightSample& s, V3& le) {
    le = mk(0, 0, 0);
    if (el.on) {
        bool take_env = true;
        if (lt.n != 0) take_env = !(g.next() < 0.5);
        if (take_env) { env_light_sample(sc, env, el, g, s, le); return; }
    }
    light_sample(lt, x, g, s);
}

// the density with which environment sampling would have produced the direction whose lookup gave bg (= texel colour x intensity): 0 where that is not
// finite and positive
__device__ inline double env_light_pdf(const EnvLight& el, V3 bg) {
    if (!el.on) return 0.0;
    const double p = el.p_choice * env_lum(bg) / (el.intensity * el.total);
    return p > 0 && p < __builtin_huge_val() ? p : 0.0;
}
#endif

}  // namespace zr

namespace zr_host {
// zr_envlight.cpp: the kernels' view of the environment table of (s, de), built and cached on the scene at the first use; el.on = 0 where nothing is sampled.
// ZR_E_INVALID for a map beyond ZR_DIRECT_ENV_MAX_TEXELS.
int scene_env_light(zr_ctx* c, const zr_scene* s, const zr::DEnv& de, zr::EnvLight& el);
// zr_direct.cpp: both tables of one direct render (direct: FrameJob::direct), with the choice probability they share
int direct_tables(zr_ctx* c, const zr_scene* s, uint32_t direct, const zr::DEnv& de, zr::LightTable& lt, zr::EnvLight& el, uint64_t* slots, uint64_t* objects);
}  // namespace zr_host
