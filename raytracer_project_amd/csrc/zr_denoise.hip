// zr_denoise.hip — the denoiser behind camera::use_denoiser (camera.hpp:268-291): an edge-avoiding a-trous wavelet filter
// (Dammertz, Sewtz, Hanika, Lensch, HPG 2010) guided by the first-hit albedo and normal passes and, optionally, the z-depth pass.
// The reference runs Intel OIDN there (apply_denoising, camera.hpp:581-699); its network weights are not part of the reference and
// this is NOT a reproduction of it.  The contract of this file is its own NumPy restatement (tests/denoise_model.py), DESIGN §9.
//
// The rules this file shares with zr_nlm.hip are written once, in zr_filter.h; the names in brackets below are its helpers.
//
//   pack     per pixel, FP32: clean (NaN / Inf -> 0, every input) [clean], n = normalize(2e - 1) (0 = no information when |2e - 1| < 1e-6)
//            [decode_normal], a' = a where a > 1e-3 else 1 (per channel, demodulation on; else a' = 1) [albedo_divisor], d = c / a'
//   atrous   one launch per level i = 0..L-1, step s = 2^i, taps (kx, ky) in {-2..2}^2 at (kx s, ky s), ky outer / kx inner,
//            taps outside the frame skipped; w = h(kx) h(ky) w_c w_n w_a w_z with
//              w_c = exp(-|t(d_p) - t(d_q)|^2 / (sigma_c^2 4^-i)),  t(x) = x / (1 + max(lum(x), 0)),  lum = Rec.709
//              w_n = max(0, n_p . n_q)^sigma_n  (1 when either normal is 0) [normal_weight]
//              w_a = exp(-|a_p - a_q|^2 / sigma_a^2)
//              w_z = exp(-|z_p - z_q| / sigma_z)  (1 without a depth frame or with sigma_z <= 0)
//            d'_p = sum w d_q / sum w  (the centre tap's weight is h(0)^2 w_n(p, p) > 0)
//   unpack   c_out = d' a', widened to double
//
// As evaluated (the same formula up to FP32 rounding; the taps are ALU-bound): whoever writes a colour also writes
// r = 1 / (1 + max(lum, 0)) into its .w, so t(x) = x r; the three exponentials are one, w_c w_a w_z = exp(-(|dt|^2 ic + |da|^2 ia
// + |dz| iz)) with the reciprocals ic, ia, iz taken once on the host; w_n = exp2(sigma_n log2(max(0, n_p . n_q))).  Then
// w = (h(kx) h(ky)) (w_c w_a w_z) w_n.
//
// Buffers: colour ping-pong float4 (xyz = d, w = r), guide0 float4 (xyz = cleaned albedo, w = depth), guide1 float4 (xyz = n,
// w = 1 when n carries information).  A plain gather: the 25 taps of a 16 x 16 block come from L2 / MALL.  Compiled with
// -ffp-contract=off, so that the NumPy model follows the arithmetic operation for operation; only expf / exp2f / log2f differ
// from NumPy's (an ulp or two).
//
// The variance-guided form (zr_denoise_guided; tests/denoise_guided_model.py) is the spatial stage of SVGF (Schied et al.,
// HPG 2017, §4.4) laid over the filter above.  It runs denoise_pack / denoise_unpack unchanged for colour and guides and adds
//   guided_pack    V = max(clean(variance), 0) / (a' a')  per channel (a' = 1 without demodulation)
//   guided_atrous  the level kernel with the colour term |t(d_p) - t(d_q)|^2 / (sigma_v^2 s^_p + eps) in place of |..|^2 / (sigma_c^2 4^-i):
//                  s_q = r_q^2 (V_q.x + V_q.y + V_q.z) is the expected squared length of the noise of t(d_q), s^_p its 3 x 3 Gaussian
//                  ([1 2 1] x [1 2 1] / 16, unit spacing at every level, taps off the frame skipped, renormalised by the weights used) [gauss3x3];
//                  d'_p = sum w d_q / sum w and V'_p = sum w^2 V_q / (sum w)^2, colour and variance ping-pong together
//   guided_unpack  out_variance = V' a' a', widened to double
// As evaluated: whoever writes a variance writes s = (r r) ((V.x + V.y) + V.z) into its .w, r being the .w of the colour written beside it.
// Per pixel: gs = sum g s_k, gw = sum g over the 3 x 3 taps inside the frame (ky outer, kx inner, g = g1(kx) g1(ky), g1 = 1/4, 1/2, 1/4),
// ic = 1 / (sv2 (gs / gw) + eps) with sv2 = sigma_v sigma_v taken on the host — one reciprocal per pixel.  Per tap arg and w exactly as
// above with ic for lv.inv_c (both level kernels call tap_weight); then sx += w d_q.x ..., w2 = w w, vx += w2 V_q.x ..., sw += w.  At the end d' = sx / sw ...,
// ss = sw sw, V' = vx / ss ....  A buffer more per tap (float4 variance) and nine float4 per pixel on top of the plain level kernel.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/zr_capi.h"
#include "zr_filter.h"

namespace zr {

namespace {

// what a level's taps weigh the guides by, the same for both forms of the filter
struct TapGuides {
    float inv_a;      // 1 / sigma_a^2
    float inv_z;      // 1 / sigma_z with the depth guide on, else 0
    float sigma_n;
    int step;         // 2^i
};
struct DenoiseLevel {
    float inv_c;      // 1 / (sigma_c^2 4^-i)
    TapGuides t;
};

template <class Params>   // zr_denoise_params or zr_denoise_guided_params
TapGuides tap_guides(const Params& dp, bool depth, int it) {
    return {1.0f / (dp.sigma_albedo * dp.sigma_albedo), depth && dp.sigma_depth > 0.0f ? 1.0f / dp.sigma_depth : 0.0f, dp.sigma_normal, 1 << it};
}

// w of the tap at q seen from p (the file header: "as evaluated"): hk = h(kx) h(ky), (tpx, tpy, tpz) = t(d_p), cq the tap's colour with r in .w, inv_c the
// colour term's reciprocal
__device__ __forceinline__ float tap_weight(float hk, float tpx, float tpy, float tpz, const float4& cq, const float4& ap, const float4& aq, const float4& np, const float4& nq, float inv_c,
                                            const TapGuides& t) {
    const float ex = tpx - cq.x * cq.w, ey = tpy - cq.y * cq.w, ez = tpz - cq.z * cq.w;
    const float bx = ap.x - aq.x, by = ap.y - aq.y, bz = ap.z - aq.z;
    const float arg = (ex * ex + ey * ey + ez * ez) * inv_c + (bx * bx + by * by + bz * bz) * t.inv_a + fabsf(ap.w - aq.w) * t.inv_z;
    return hk * expf(-arg) * normal_weight(np, nq, t.sigma_n);
}

__global__ __launch_bounds__(256) void denoise_pack(const double* __restrict__ color, const double* __restrict__ albedo,
                                                    const double* __restrict__ normal, const double* __restrict__ zdepth, int W, int H,
                                                    int demodulate, float4* __restrict__ col, float4* __restrict__ g0, float4* __restrict__ g1) {
    ZR_PIXEL16(W, H, i, j, p);
    const float4 a = make_float4(clean(albedo[3 * p]), clean(albedo[3 * p + 1]), clean(albedo[3 * p + 2]), zdepth ? clean(zdepth[3 * p]) : 0.0f);
    const float4 n = decode_normal(clean(normal[3 * p]), clean(normal[3 * p + 1]), clean(normal[3 * p + 2]));
    float dx = clean(color[3 * p]), dy = clean(color[3 * p + 1]), dz = clean(color[3 * p + 2]);
    if (demodulate) {
        const float3 m = albedo_divisor(a, demodulate);
        dx = dx / m.x; dy = dy / m.y; dz = dz / m.z;
    }
    col[p] = with_tone(dx, dy, dz);
    g0[p] = a;
    g1[p] = n;
}

__global__ __launch_bounds__(256) void denoise_atrous(const float4* __restrict__ in, const float4* __restrict__ g0, const float4* __restrict__ g1,
                                                      int W, int H, DenoiseLevel lv, float4* __restrict__ out) {
    ZR_PIXEL16(W, H, i, j, p);
    const float h[5] = {1.0f / 16.0f, 1.0f / 4.0f, 3.0f / 8.0f, 1.0f / 4.0f, 1.0f / 16.0f};
    const float4 cp = in[p], ap = g0[p], np = g1[p];
    const float tpx = cp.x * cp.w, tpy = cp.y * cp.w, tpz = cp.z * cp.w;
    float sx = 0.0f, sy = 0.0f, sz = 0.0f, sw = 0.0f;
#pragma unroll
    for (int ky = -2; ky <= 2; ky++) {
        const int qj = j + ky * lv.t.step;
        if (qj < 0 || qj >= H) continue;
#pragma unroll
        for (int kx = -2; kx <= 2; kx++) {
            const int qi = i + kx * lv.t.step;
            if (qi < 0 || qi >= W) continue;
            const size_t q = (size_t)qj * W + qi;
            const float4 cq = in[q];
            const float w = tap_weight(h[kx + 2] * h[ky + 2], tpx, tpy, tpz, cq, ap, g0[q], np, g1[q], lv.inv_c, lv.t);
            sx = sx + w * cq.x; sy = sy + w * cq.y; sz = sz + w * cq.z;
            sw = sw + w;
        }
    }
    out[p] = with_tone(sx / sw, sy / sw, sz / sw);
}

__global__ __launch_bounds__(256) void denoise_unpack(const float4* __restrict__ col, const float4* __restrict__ g0, int W, int H, int demodulate,
                                                      double* __restrict__ out) {
    ZR_PIXEL16(W, H, i, j, p);
    float4 d = col[p];
    if (demodulate) {
        const float3 m = albedo_divisor(g0[p], demodulate);
        d.x = d.x * m.x; d.y = d.y * m.y; d.z = d.z * m.z;
    }
    out[3 * p] = (double)d.x; out[3 * p + 1] = (double)d.y; out[3 * p + 2] = (double)d.z;
}

}  // namespace

// d_color / d_albedo / d_normal / d_zdepth (may be null): W*H*3 doubles on the device; d_col0 / d_col1 / d_g0 / d_g1: W*H float4
// scratch; d_out: W*H*3 doubles (may be d_color).  The caller has validated the parameters (zr_denoise).
hipError_t launch_denoise(const double* d_color, const double* d_albedo, const double* d_normal, const double* d_zdepth, int W, int H,
                          const zr_denoise_params& dp, float4* d_col0, float4* d_col1, float4* d_g0, float4* d_g1, double* d_out,
                          hipStream_t stream) {
    const dim3 block(16, 16), grid = grid16(W, H);
    const int demod = dp.demodulate_albedo ? 1 : 0;
    hipLaunchKernelGGL(denoise_pack, grid, block, 0, stream, d_color, d_albedo, d_normal, d_zdepth, W, H, demod, d_col0, d_g0, d_g1);
    float4* cur = d_col0;
    float4* nxt = d_col1;
    for (int it = 0; it < dp.iterations; it++) {
        const DenoiseLevel lv = {1.0f / (dp.sigma_color * dp.sigma_color * ldexpf(1.0f, -2 * it)), tap_guides(dp, d_zdepth != nullptr, it)};
        hipLaunchKernelGGL(denoise_atrous, grid, block, 0, stream, (const float4*)cur, (const float4*)d_g0, (const float4*)d_g1, W, H, lv, nxt);
        float4* t = cur; cur = nxt; nxt = t;
    }
    hipLaunchKernelGGL(denoise_unpack, grid, block, 0, stream, (const float4*)cur, (const float4*)d_g0, W, H, demod, d_out);
    return hipGetLastError();
}

// ---- the variance-guided form (the file header's second part) ---------------------------------------------------------

namespace {

struct GuidedLevel {
    float sv2;        // sigma_v^2
    float eps;
    TapGuides t;
};

// a variance with s = r^2 (V.x + V.y + V.z) in .w, r being the .w of the colour it belongs to
__device__ __forceinline__ float4 with_spread(float vx, float vy, float vz, float r) { return make_float4(vx, vy, vz, (r * r) * ((vx + vy) + vz)); }

// after denoise_pack: col holds the (demodulated) colour with r, g0 the cleaned albedo
__global__ __launch_bounds__(256) void guided_pack(const double* __restrict__ variance, const float4* __restrict__ col, const float4* __restrict__ g0, int W,
                                                   int H, int demodulate, float4* __restrict__ var) {
    ZR_PIXEL16(W, H, i, j, p);
    float vx = fmaxf(clean(variance[3 * p]), 0.0f), vy = fmaxf(clean(variance[3 * p + 1]), 0.0f), vz = fmaxf(clean(variance[3 * p + 2]), 0.0f);
    if (demodulate) {
        const float3 m = albedo_divisor(g0[p], demodulate);
        vx = vx / (m.x * m.x); vy = vy / (m.y * m.y); vz = vz / (m.z * m.z);
    }
    var[p] = with_spread(vx, vy, vz, col[p].w);
}

__global__ __launch_bounds__(256) void guided_atrous(const float4* __restrict__ in, const float4* __restrict__ vin, const float4* __restrict__ g0,
                                                     const float4* __restrict__ g1, int W, int H, GuidedLevel lv, float4* __restrict__ out,
                                                     float4* __restrict__ vout) {
    ZR_PIXEL16(W, H, i, j, p);
    const float h[5] = {1.0f / 16.0f, 1.0f / 4.0f, 3.0f / 8.0f, 1.0f / 4.0f, 1.0f / 16.0f};
    // the pixel's own noise in tone-compressed space, smoothed over 3 x 3 at unit spacing
    float gs = 0.0f;
    const float gw = gauss3x3(i, j, W, H, [&](float gk, size_t q) { gs = gs + gk * vin[q].w; });
    const float inv_c = 1.0f / (lv.sv2 * (gs / gw) + lv.eps);
    const float4 cp = in[p], ap = g0[p], np = g1[p];
    const float tpx = cp.x * cp.w, tpy = cp.y * cp.w, tpz = cp.z * cp.w;
    float sx = 0.0f, sy = 0.0f, sz = 0.0f, sw = 0.0f, vx = 0.0f, vy = 0.0f, vz = 0.0f;
#pragma unroll
    for (int ky = -2; ky <= 2; ky++) {
        const int qj = j + ky * lv.t.step;
        if (qj < 0 || qj >= H) continue;
#pragma unroll
        for (int kx = -2; kx <= 2; kx++) {
            const int qi = i + kx * lv.t.step;
            if (qi < 0 || qi >= W) continue;
            const size_t q = (size_t)qj * W + qi;
            const float4 cq = in[q], vq = vin[q];
            const float w = tap_weight(h[kx + 2] * h[ky + 2], tpx, tpy, tpz, cq, ap, g0[q], np, g1[q], inv_c, lv.t);
            const float w2 = w * w;
            sx = sx + w * cq.x; sy = sy + w * cq.y; sz = sz + w * cq.z;
            vx = vx + w2 * vq.x; vy = vy + w2 * vq.y; vz = vz + w2 * vq.z;
            sw = sw + w;
        }
    }
    const float4 d = with_tone(sx / sw, sy / sw, sz / sw);
    const float ss = sw * sw;
    out[p] = d;
    vout[p] = with_spread(vx / ss, vy / ss, vz / ss, d.w);
}

__global__ __launch_bounds__(256) void guided_unpack(const float4* __restrict__ var, const float4* __restrict__ g0, int W, int H, int demodulate,
                                                     double* __restrict__ out) {
    ZR_PIXEL16(W, H, i, j, p);
    float4 v = var[p];
    if (demodulate) {
        const float3 m = albedo_divisor(g0[p], demodulate);
        v.x = v.x * (m.x * m.x); v.y = v.y * (m.y * m.y); v.z = v.z * (m.z * m.z);
    }
    out[3 * p] = (double)v.x; out[3 * p + 1] = (double)v.y; out[3 * p + 2] = (double)v.z;
}

}  // namespace

// launch_denoise's buffers plus d_variance (W*H*3 doubles), the variance ping-pong d_var0 / d_var1 (W*H float4) and d_out_var (W*H*3
// doubles, may be null, may be d_variance).  The caller has validated the parameters (zr_denoise_guided).
hipError_t launch_denoise_guided(const double* d_color, const double* d_variance, const double* d_albedo, const double* d_normal, const double* d_zdepth, int W,
                                 int H, const zr_denoise_guided_params& dp, float4* d_col0, float4* d_col1, float4* d_var0, float4* d_var1, float4* d_g0,
                                 float4* d_g1, double* d_out, double* d_out_var, hipStream_t stream) {
    const dim3 block(16, 16), grid = grid16(W, H);
    const int demod = dp.demodulate_albedo ? 1 : 0;
    hipLaunchKernelGGL(denoise_pack, grid, block, 0, stream, d_color, d_albedo, d_normal, d_zdepth, W, H, demod, d_col0, d_g0, d_g1);
    hipLaunchKernelGGL(guided_pack, grid, block, 0, stream, d_variance, (const float4*)d_col0, (const float4*)d_g0, W, H, demod, d_var0);
    float4 *cur = d_col0, *nxt = d_col1, *vcur = d_var0, *vnxt = d_var1;
    for (int it = 0; it < dp.iterations; it++) {
        const GuidedLevel lv = {dp.sigma_variance * dp.sigma_variance, dp.epsilon, tap_guides(dp, d_zdepth != nullptr, it)};
        hipLaunchKernelGGL(guided_atrous, grid, block, 0, stream, (const float4*)cur, (const float4*)vcur, (const float4*)d_g0, (const float4*)d_g1, W, H, lv,
                           nxt, vnxt);
        float4* t = cur; cur = nxt; nxt = t;
        t = vcur; vcur = vnxt; vnxt = t;
    }
    hipLaunchKernelGGL(denoise_unpack, grid, block, 0, stream, (const float4*)cur, (const float4*)d_g0, W, H, demod, d_out);
    if (d_out_var) hipLaunchKernelGGL(guided_unpack, grid, block, 0, stream, (const float4*)vcur, (const float4*)d_g0, W, H, demod, d_out_var);
    return hipGetLastError();
}

}  // namespace zr
