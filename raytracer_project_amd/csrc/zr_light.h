// zr_light.h — direct light sampling: the light table as the kernels get it, how a light sample is drawn from it and the density the
// MIS weight reads back for a hit.  The table's rules are stated in include/zr_capi.h; tests/direct_model.py restates this file in NumPy.
// The host (g++) sees the table type only; the device functions need zr_device.h before this header.
#pragma once
#include <stdint.h>
#include "../../include/zr_capi.h"
#include "zr_launch.h"

namespace zr {

// The table travels as a kernel argument of its own: DScene stays what it is.  slots / cdf: device arrays of n entries (zr_light_slot is the dump's record
// and the kernels'); total = cdf[n - 1].  The sun's cone and its fixed frame come ready from the host (make_light_table, zr_direct.cpp).
struct LightTable {
    const zr_light_slot* slots; const double* cdf;
    uint32_t n;            // slots that are sampled: 0 when the table is empty or ZR_DIRECT_EMITTERS is off
    uint32_t sun;          // 1: the sun is sampled
    double total;          // sum of the slots' weights
    double p_choice;       // 1/2 when emitters and the sun (or the environment map) are both sampled, else 1
    double sun_dir[3], sun_t[3], sun_b[3], sun_thr, sun_pdf;   // sun_pdf = 1 / (2 pi (1 - sun_thr))
};

// zr_direct.hip.  launch_direct_samples: launch_render_samples (zr_launch.h) with light sampling.  launch_light_count: per block of 256 candidates (the
// world-level spheres, triangles, cubes, placed cubes: n_cand of them) the slots its emitters make, scanned in place into block offsets, *total = their sum;
// launch_light_emit then writes those slots, in table order, into out[0 .. cap).
struct EnvLight;   // zr_envlight.h: the environment table; on = 0 renders without it
hipError_t launch_direct_samples(const DScene& sc, const DCamera& cam, const DEnv& env, const LightTable& lt, const EnvLight& el, uint64_t seed, const uint32_t* pixels,
                                 uint32_t n_pix, uint32_t sample0, uint32_t n, double* samples, unsigned long long* gctr, bool count, hipStream_t stream);
hipError_t launch_light_count(const DScene& sc, uint32_t n_cand, uint32_t* block_count, uint32_t* total, hipStream_t stream);
hipError_t launch_light_emit(const DScene& sc, uint32_t n_cand, const uint32_t* block_offset, uint32_t cap, zr_light_slot* out, hipStream_t stream);
hipError_t launch_kat_light_sample(const LightTable& lt, const double* origins, const uint64_t* keys, const uint32_t* bounces, const double* draws8, size_t n,
                                   zr_light_sample* out, hipStream_t stream);
hipError_t launch_kat_light_pdf(const DScene& sc, const LightTable& lt, const double* origins, const double* dirs, size_t n, double* out_pdf, uint64_t* out_key,
                                hipStream_t stream);

#ifdef __HIPCC__
// draw j of a light stream; forced (the known-answer entry only): up to 8 numbers that replace the draws 0..7 where they lie in [0, 1)
struct LightRng {
    uint64_t key; uint32_t j; const double* forced;
    __device__ __forceinline__ double next() {
        double u = zr_bits_to_unit(zr_stream_bits(key, j));
        if (forced && j < 8 && forced[j] >= 0.0 && forced[j] < 1.0) u = forced[j];
        j++;
        return u;
    }
    __device__ __forceinline__ double range(double a, double b) { return a + (b - a) * next(); }
};

struct LightSample {
    uint32_t choice, slot, kind, index;   // choice: 0 nothing, 1 emitter, 2 sun
    V3 y, n, w;
    double dist, pdf;
};

// the first slot whose cdf exceeds target (the last one when none does: u * total can round up to total)
__device__ inline uint32_t light_pick(const LightTable& lt, double target) {
    uint32_t lo = 0, hi = lt.n - 1;
    while (lo < hi) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if (lt.cdf[mid] > target) hi = mid; else lo = mid + 1;
    }
    return lo;
}

// one light sample seen from x
__device__ inline void light_sample(const LightTable& lt, V3 x, LightRng& g, LightSample& s) {
    s.choice = 0; s.slot = 0; s.kind = 0xFFFFFFFFu; s.index = 0xFFFFFFFFu;
    s.y = mk(0, 0, 0); s.n = mk(0, 0, 0); s.w = mk(0, 0, 0); s.dist = 0; s.pdf = 0;
    const bool em = lt.n != 0, sun = lt.sun != 0;
    if (!em && !sun) return;
    bool take_sun = sun;
    if (em && sun) take_sun = !(g.next() < 0.5);
    if (take_sun) {
        const double u1 = g.next(), u2 = g.next();
        const double ct = 1.0 - u1 * (1.0 - lt.sun_thr);
        const double st = sqrt(fmax(0.0, 1.0 - ct * ct));
        const double phi = 6.283185307179586476925 * u2;
        const double cp = cos(phi), sp = sin(phi);
        s.choice = 2;
        s.w = ((st * cp) * ld3(lt.sun_t) + (st * sp) * ld3(lt.sun_b)) + ct * ld3(lt.sun_dir);
        s.dist = __builtin_huge_val();
        s.pdf = lt.p_choice * lt.sun_pdf;
        return;
    }
    const uint32_t i = light_pick(lt, g.next() * lt.total);
    const zr_light_slot& q = lt.slots[i];
    s.choice = 1; s.slot = i; s.kind = q.kind; s.index = q.index;
    const V3 o = ld3(q.o);
    if (q.type == ZR_LIGHT_SPHERE) {
        V3 ruv;
        for (;;) {   // random_unit_vector (vec3.hpp:184-191) on the light stream
            const double a = g.range(-1, 1), b = g.range(-1, 1), c = g.range(-1, 1);
            const V3 p = mk(a, b, c);
            const double l2 = len2(p);
            if (1e-160 < l2 && l2 <= 1) { ruv = vdiv(p, sqrt(l2)); break; }
        }
        s.y = o + q.e1[0] * ruv;
        s.n = ruv;
    } else {
        double u1 = g.next(), u2 = g.next();
        if (q.type == ZR_LIGHT_TRIANGLE && u1 + u2 > 1.0) { u1 = 1.0 - u1; u2 = 1.0 - u2; }
        const V3 e1 = ld3(q.e1), e2 = ld3(q.e2);
        s.y = (o + u1 * e1) + u2 * e2;
        const V3 c = cross(e1, e2);
        s.n = vdiv(c, len(c));
    }
    const V3 v = s.y - x;
    s.dist = len(v);
    if (!(s.dist > 0)) return;
    s.w = vdiv(v, s.dist);
    const double cos_l = fabs(dot(s.n, s.w));
    if (!(cos_l > 1e-12)) return;
    s.pdf = lt.p_choice * (q.lum / lt.total) * (s.dist * s.dist) / cos_l;
}

// rho of the object closest hit names (kind, index): the slots are ordered by (kind, index), so any slot of the object is found by bisection; 0: not sampled
__device__ inline double light_rho(const LightTable& lt, uint32_t kind, uint32_t index) {
    if (lt.n == 0) return 0.0;
    const uint64_t want = ((uint64_t)kind << 32) | index;
    uint32_t lo = 0, hi = lt.n;
    while (lo < hi) {
        const uint32_t mid = lo + (hi - lo) / 2;
        const uint64_t have = ((uint64_t)lt.slots[mid].kind << 32) | lt.slots[mid].index;
        if (have == want) return lt.slots[mid].lum / lt.total;
        if (have < want) lo = mid + 1; else hi = mid;
    }
    return 0.0;
}

// the geometric normal of a sampled object at the hit (either sign): the sphere's and the cubes' is the record's, a triangle's comes from its vertices
__device__ inline V3 light_geo_normal(const DScene& sc, uint32_t kind, uint32_t index, const Rec& rec) {
    if (kind != ZR_PRIM_TRIANGLE) return rec.n;
    const double* v = sc.tri_v + (size_t)index * ZR_TRI_STRIDE;
    const V3 v0 = ld3(v), c = cross(ld3(v + 3) - v0, ld3(v + 6) - v0);
    return vdiv(c, len(c));
}

// the density by solid angle with which light sampling would have produced the hit (kind, index, rec) of the ray r at parameter t: what the MIS weight of
// a scattered ray that found a light reads.  0: the object is not sampled (or is seen edge-on: light sampling contributes nothing there either)
__device__ inline double light_pdf_hit(const LightTable& lt, const DScene& sc, uint32_t kind, uint32_t index, const Ray& r, double t, const Rec& rec) {
    const double rho = light_rho(lt, kind, index);
    if (!(rho > 0)) return 0.0;
    const double dl = len(r.d);
    const double dist = t * dl;
    const double cos_l = fabs(dot(light_geo_normal(sc, kind, index, rec), r.d)) / dl;
    if (!(cos_l > 1e-12)) return 0.0;
    return lt.p_choice * rho * (dist * dist) / cos_l;
}
// ... and for a ray that left the world in direction d: the sun's cone
__device__ inline double light_pdf_sun(const LightTable& lt, V3 d) {
    if (!lt.sun) return 0.0;
    return dot(unit(d), ld3(lt.sun_dir)) > lt.sun_thr ? lt.p_choice * lt.sun_pdf : 0.0;
}
#endif

}  // namespace zr
