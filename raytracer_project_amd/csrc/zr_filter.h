// zr_filter.h — the per-pixel rules the image filters share (zr_denoise.hip, zr_nlm.hip), each stated once: how an input is cleaned, what an
// albedo divides by, how a normal is decoded and weighed, the 3 x 3 Gaussian, and the 16 x 16 pixel grid every filter kernel runs on.  FP32, no contraction
// (both files are compiled with -ffp-contract=off); tests/denoise_model.py restates the same rules once for the three NumPy models (clean, albedo_divisor,
// prepare, the normal weight of atrous_level) and tests/denoise_guided_model.py the stencil (smoothed_spread).  zr_temporal.hip and zr_post.hip have rules of
// their own and do not include this.
#pragma once
#include <hip/hip_runtime.h>

namespace zr {

// the grid of 16 x 16 blocks over a W x H frame, and how a kernel on it begins: its thread's pixel (i, j) and p = j W + i; a thread off the frame returns
// (a macro because it returns from the kernel)
inline dim3 grid16(int W, int H) { return dim3((unsigned)((W + 15) / 16), (unsigned)((H + 15) / 16)); }
#define ZR_PIXEL16(W, H, i, j, p)                                                        \
    const int i = blockIdx.x * 16 + threadIdx.x, j = blockIdx.y * 16 + threadIdx.y;      \
    if (i >= (W) || j >= (H)) return;                                                    \
    const size_t p = (size_t)j * (W) + i

__device__ __forceinline__ float clean(double v) {   // clean_val (camera.hpp:596-600) after the reference's cast to float: NaN / Inf -> 0
    const float f = (float)v;
    return isfinite(f) ? f : 0.0f;
}

__device__ __forceinline__ float lum709(float x, float y, float z) { return 0.2126f * x + 0.7152f * y + 0.0722f * z; }
// a colour with the reciprocal of its tone-compression divisor in .w
__device__ __forceinline__ float4 with_tone(float x, float y, float z) { return make_float4(x, y, z, 1.0f / (1.0f + fmaxf(lum709(x, y, z), 0.0f))); }

// a': what a colour is divided by going in and multiplied by coming out, per channel of the cleaned albedo a (1 for a black material, and without demodulation)
__device__ __forceinline__ float3 albedo_divisor(const float4& a, int demodulate) {
    return make_float3(demodulate && a.x > 1e-3f ? a.x : 1.0f, demodulate && a.y > 1e-3f ? a.y : 1.0f, demodulate && a.z > 1e-3f ? a.z : 1.0f);
}

// guide1 of a pixel from its cleaned encoded normal e: xyz = normalize(2e - 1), w = 1; all 0 when |2e - 1| < 1e-6 (no information)
__device__ __forceinline__ float4 decode_normal(float ex, float ey, float ez) {
    float mx = 2.0f * ex - 1.0f, my = 2.0f * ey - 1.0f, mz = 2.0f * ez - 1.0f;
    const float len = sqrtf(mx * mx + my * my + mz * mz);
    float valid = 1.0f;
    if (len < 1e-6f) { mx = my = mz = 0.0f; valid = 0.0f; }
    else { mx = mx / len; my = my / len; mz = mz / len; }
    return make_float4(mx, my, mz, valid);
}

// w_n = max(0, n_p . n_q)^sigma_n of two guide1 entries, 1 when either carries no information
__device__ __forceinline__ float normal_weight(const float4& np, const float4& nq, float sigma_n) {
    float wn = 1.0f;
    if (np.w != 0.0f && nq.w != 0.0f) wn = exp2f(sigma_n * log2f(fmaxf(0.0f, np.x * nq.x + np.y * nq.y + np.z * nq.z)));
    return wn;
}

// The 3 x 3 Gaussian [1 2 1] x [1 2 1] / 16 around (i, j) at unit spacing, ky outer / kx inner, taps off the frame skipped: tap(g, q) for every tap inside with
// its weight g = g1(kx) g1(ky) and its pixel q; returns gw = sum g, by which the caller renormalises its own sums.
template <class Tap>
__device__ __forceinline__ float gauss3x3(int i, int j, int W, int H, Tap&& tap) {
    const float g[3] = {1.0f / 4.0f, 1.0f / 2.0f, 1.0f / 4.0f};
    float gw = 0.0f;
#pragma unroll
    for (int ky = -1; ky <= 1; ky++) {
        const int qj = j + ky;
        if (qj < 0 || qj >= H) continue;
#pragma unroll
        for (int kx = -1; kx <= 1; kx++) {
            const int qi = i + kx;
            if (qi < 0 || qi >= W) continue;
            const float gk = g[kx + 1] * g[ky + 1];
            tap(gk, (size_t)qj * W + qi);
            gw = gw + gk;
        }
    }
    return gw;
}

}  // namespace zr
