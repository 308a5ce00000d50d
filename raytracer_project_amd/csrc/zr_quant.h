// zr_quant.h — the 8-bit grid of a 4-wide node (zr_device_types.h: NodeQ) as the device computes it: the exact plane comparisons and the choice of origin, scale
// and plane numbers per axis.  Device code only, written once: the builder (zr_build.hip, k_plan) puts a node's children on their grid with it, and a refit
// (zr_refit.hip, k_refit_quads) puts the moved children on a fresh one — a refitted node is then the node the builder would have written over the same boxes.
// The host builder's own statement is Flattener::quant_axis (zr_flatten.h).  Compile with -ffp-contract=off.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace zr {

// origin + q * scale against a plane x, as real numbers: a = origin and m = q * scale are exact doubles, TwoSum gives a + m = s + e
__device__ __forceinline__ void plane_sum(float origin, float scale, int q, double& s, double& e) {
    const double a = (double)origin, m = (double)q * (double)scale;
    s = a + m;
    const double bb = s - a;
    e = (a - (s - bb)) + (m - bb);
}
__device__ __forceinline__ bool plane_le(float origin, float scale, int q, double x) { double s, e; plane_sum(origin, scale, q, s, e); return s < x || (s == x && e <= 0.0); }
__device__ __forceinline__ bool plane_ge(float origin, float scale, int q, double x) { double s, e; plane_sum(origin, scale, q, s, e); return s > x || (s == x && e >= 0.0); }
__device__ __forceinline__ double plane_val(float origin, float scale, int q) { return (double)origin + (double)q * (double)scale; }

// the grid of one axis over n boxes: the planes origin + q * scale, q in 0 .. 255, with every lower plane at or below lo[k] and every upper plane at or above
// hi[k]; false when the boxes cannot be represented (not finite, beyond 1e30)
static __device__ bool quant_axis(const float* lo, const float* hi, int n, float& origin, float& scale, uint32_t* qlo, uint32_t* qhi) {
    float mn = lo[0], mx = hi[0];
    for (int k = 1; k < n; k++) { mn = fminf(mn, lo[k]); mx = fmaxf(mx, hi[k]); }
    if (!(fabsf(mn) <= 1e30f) || !(fabsf(mx) <= 1e30f)) return false;
    origin = nextafterf(mn, -__builtin_huge_valf());
    const double ext = (double)mx - (double)origin;
    int e = ext > 0 ? (int)ceil(log2(ext / 255.0)) : -100;
    const int emin = origin != 0.0f ? max(-100, ilogbf(origin) - 30) : -100;
    if (e < emin) e = emin;
    for (int tries = 0; tries < 64; tries++, e++) {
        scale = ldexpf(1.0f, e);
        bool ok = true;
        for (int k = 0; k < n && ok; k++) {
            long ql = (long)floor(((double)lo[k] - (double)origin) / (double)scale);
            ql = ql < 0 ? 0 : (ql > 255 ? 255 : ql);
            while (ql > 0 && !plane_le(origin, scale, (int)ql, (double)lo[k])) ql--;
            if (!plane_le(origin, scale, (int)ql, (double)lo[k])) ok = false;
            long qh = (long)ceil(((double)hi[k] - (double)origin) / (double)scale);
            qh = qh < 0 ? 0 : (qh > 255 ? 255 : qh);
            while (qh < 255 && !plane_ge(origin, scale, (int)qh, (double)hi[k])) qh++;
            if (!plane_ge(origin, scale, (int)qh, (double)hi[k])) ok = false;
            qlo[k] = (uint32_t)ql; qhi[k] = (uint32_t)qh;
        }
        if (ok) return true;
    }
    return false;
}

}  // namespace zr
