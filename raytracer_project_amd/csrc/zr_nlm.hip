// zr_nlm.hip — the dual-buffer non-local-means denoiser (zr_denoise_nlm): Rousselle, Knaus, Zwicker, "Adaptive rendering with non-local means
// filtering" (SIGGRAPH Asia 2012) on the two half images of an accumulator (zr_accum_halves) and the variance of its pixel means (zr_accum_variance).
// Patch distances are normalised by the per-pixel variance, a variance-cancellation term is subtracted from every squared difference, and the weights
// computed from one half filter the other.  FP32, compiled with -ffp-contract=off, no atomics, a fixed evaluation order: tests/denoise_nlm_model.py restates
// it operation for operation; only expf / exp2f / log2f differ from NumPy's (an ulp or two).
//
//   nlm_pack     per pixel: cleaning, normal decoding and the albedo divisor a' are denoise_pack's, by the same helpers (zr_filter.h: clean, decode_normal,
//                albedo_divisor); uA = clean(A) / a', uB = clean(B) / a', Vh = 2 max(clean(variance), 0) / (a' a') (a half holds half the samples: twice the
//                variance of the full mean)
//   nlm_smooth   V^ = the 3 x 3 Gaussian of Vh per channel, guided_atrous's stencil (zr_filter.h: gauss3x3): g = g1(kx) g1(ky), g1 = 1/4, 1/2, 1/4, ky outer /
//                kx inner, taps off the frame skipped, gs = sum g Vh_k, gw = sum g, V^ = gs / gw
//   nlm_filter   with clamp() moving a coordinate to the nearest frame pixel, for every offset D = (dx, dy) in [-r, r]^2, dy outer / dx inner:
//                  e_D(s)  = e(s, clamp(s + D)), per buffer u in {uA, uB};  per channel c with vs = V^_s.c, vt = V^_t.c
//                            canc = alpha (vs + min(vt, vs)),  id = 1 / (eps + kk (vs + vt)),  kk = k k taken on the host,
//                            delta_c = ((u_s.c - u_t.c)^2 - canc) id;   e = ((delta_x + delta_y) + delta_z) (1/3)
//                  D_D(p)  = (sum of e_D(clamp(p + tau)) over tau in [-f, f]^2, tau_y outer / tau_x inner, from 0) inv_np,  inv_np = 1 / (2f + 1)^2 taken on the host
//                  w_u     = exp(-(max(D_D(p), 0) + |a_p - a_q|^2 inv_a)) w_n  for q = p + D inside the frame (no weight outside), inv_a = 1 / sigma_a^2 and
//                            w_n = exp2(sigma_n log2(max(0, n_p . n_q))) (1 when either normal is 0), denoise_atrous's (zr_filter.h: normal_weight); the centre tap's weight is 1
//                  fB = sum w_uA uB_q / sum w_uA,  fA = sum w_uB uA_q / sum w_uB
//                out = ((fA + fB) 0.5) a',  out_error = (((fA - fB) 0.5) a')^2, widened to double
// As evaluated (the formula of DESIGN §16 up to FP32 rounding): canc and id depend on the variances alone and serve both buffers, so a pair of pixels costs
// three reciprocals; the albedo weight shares the exponential of the patch distance.
//
// The filter kernel: a 16 x 16 output tile per workgroup.  uA, uB and V^ of the tile and its halo of r + f pixels sit in LDS as three float4 planes (48 KiB at
// r 7 f 1, 83 KiB at r 10 f 3; positions off the frame are never read).  Per offset the workgroup first writes the distance plane e_D(clamp(s)) of both buffers
// for the (16 + 2f)^2 positions s its patches reach (one float2 each, at most two positions a thread, whose own pixel stays in registers across the offsets),
// then every thread sums its patch out of that plane, so a pixel distance is computed once and shared by the (2f + 1)^2 patches it belongs to.  Two distance
// planes alternate, which leaves one barrier per offset.  A pixel's sums never depend on where the tiles lie.  The guides of q come from L2 as in
// guided_atrous.  f is a template parameter (the patch loops unroll), r a run-time one.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/zr_capi.h"
#include "zr_filter.h"

namespace zr {

namespace {

constexpr int NLM_TILE = 16;

struct NlmArgs {
    int r;            // search radius
    int demodulate;
    float kk;         // k k
    float alpha;
    float eps;
    float inv_a;      // 1 / sigma_a^2
    float sigma_n;
    float inv_np;     // 1 / (2f + 1)^2
};

__global__ __launch_bounds__(256) void nlm_pack(const double* __restrict__ half_a, const double* __restrict__ half_b, const double* __restrict__ variance,
                                                const double* __restrict__ albedo, const double* __restrict__ normal, int W, int H, int demodulate,
                                                float4* __restrict__ uA, float4* __restrict__ uB, float4* __restrict__ Vh, float4* __restrict__ g0,
                                                float4* __restrict__ g1) {
    ZR_PIXEL16(W, H, i, j, p);
    const float4 a = make_float4(clean(albedo[3 * p]), clean(albedo[3 * p + 1]), clean(albedo[3 * p + 2]), 0.0f);
    const float4 n = decode_normal(clean(normal[3 * p]), clean(normal[3 * p + 1]), clean(normal[3 * p + 2]));
    const float3 m = albedo_divisor(a, demodulate);
    uA[p] = make_float4(clean(half_a[3 * p]) / m.x, clean(half_a[3 * p + 1]) / m.y, clean(half_a[3 * p + 2]) / m.z, 0.0f);
    uB[p] = make_float4(clean(half_b[3 * p]) / m.x, clean(half_b[3 * p + 1]) / m.y, clean(half_b[3 * p + 2]) / m.z, 0.0f);
    const float vx = fmaxf(clean(variance[3 * p]), 0.0f), vy = fmaxf(clean(variance[3 * p + 1]), 0.0f), vz = fmaxf(clean(variance[3 * p + 2]), 0.0f);
    Vh[p] = make_float4(2.0f * vx / (m.x * m.x), 2.0f * vy / (m.y * m.y), 2.0f * vz / (m.z * m.z), 0.0f);
    g0[p] = a;
    g1[p] = n;
}

__global__ __launch_bounds__(256) void nlm_smooth(const float4* __restrict__ Vh, int W, int H, float4* __restrict__ Vs) {
    ZR_PIXEL16(W, H, i, j, p);
    float sx = 0.0f, sy = 0.0f, sz = 0.0f;
    const float gw = gauss3x3(i, j, W, H, [&](float gk, size_t q) {
        const float4 v = Vh[q];
        sx = sx + gk * v.x; sy = sy + gk * v.y; sz = sz + gk * v.z;
    });
    Vs[p] = make_float4(sx / gw, sy / gw, sz / gw, 0.0f);
}

// one channel of the pixel distance of both buffers: x = buffer A's delta, y = buffer B's
__device__ __forceinline__ float2 nlm_delta(float as, float at, float bs, float bt, float vs, float vt, float alpha, float eps, float kk) {
    const float canc = alpha * (vs + fminf(vt, vs));
    const float id = 1.0f / (eps + kk * (vs + vt));
    const float da = as - at, db = bs - bt;
    return make_float2((da * da - canc) * id, (db * db - canc) * id);
}

template <int F>
__global__ __launch_bounds__(256) void nlm_filter(const float4* __restrict__ uA, const float4* __restrict__ uB, const float4* __restrict__ Vs,
                                                  const float4* __restrict__ g0, const float4* __restrict__ g1, int W, int H, NlmArgs a,
                                                  double* __restrict__ out, double* __restrict__ out_error) {
    extern __shared__ float4 nlm_lds[];
    const int r = a.r, R = r + F, S = NLM_TILE + 2 * R;
    const float alpha = a.alpha, eps = a.eps, kk = a.kk, inv_a = a.inv_a, sigma_n = a.sigma_n, inv_np = a.inv_np;
    constexpr int E = NLM_TILE + 2 * F, NE = E * E;
    float4* sA = nlm_lds;
    float4* sB = sA + S * S;
    float4* sV = sB + S * S;
    float2* sE = (float2*)(sV + S * S);   // two planes of NE
    const int tx = threadIdx.x, ty = threadIdx.y, tid = ty * NLM_TILE + tx;
    const int x0 = blockIdx.x * NLM_TILE, y0 = blockIdx.y * NLM_TILE, ox = x0 - R, oy = y0 - R;

    for (int idx = tid; idx < S * S; idx += 256) {
        const int ly = idx / S, lx = idx - ly * S, gx = ox + lx, gy = oy + ly;
        float4 va = make_float4(0.0f, 0.0f, 0.0f, 0.0f), vb = va, vv = va;
        if (gx >= 0 && gx < W && gy >= 0 && gy < H) {
            const size_t g = (size_t)gy * W + gx;
            va = uA[g]; vb = uB[g]; vv = Vs[g];
        }
        sA[idx] = va; sB[idx] = vb; sV[idx] = vv;
    }
    __syncthreads();

    // this thread's (at most two) positions of the distance plane: plane position idx is the pixel clamp(x0 - F + ex, y0 - F + ey).  Clamping moves a
    // coordinate towards the tile, and by at most r further off it than the patches reach: every index below lies inside the S x S planes.
    int sgx[2], sgy[2];
    float4 pa[2], pb[2], pv[2];
#pragma unroll
    for (int k = 0; k < 2; k++) {
        const int idx = tid + 256 * k;
        const int ey = idx / E, ex = idx - ey * E;
        sgx[k] = min(max(x0 - F + ex, 0), W - 1); sgy[k] = min(max(y0 - F + ey, 0), H - 1);
        if (idx < NE) { const int ls = (sgy[k] - oy) * S + (sgx[k] - ox); pa[k] = sA[ls]; pb[k] = sB[ls]; pv[k] = sV[ls]; }
    }

    const int i = x0 + tx, j = y0 + ty;
    const bool live = i < W && j < H;
    const size_t p = live ? (size_t)j * W + i : 0;
    const float4 ap = g0[p], np = g1[p];
    float ax = 0.0f, ay = 0.0f, az = 0.0f, aw = 0.0f;   // sum w_uB uA_q, sum w_uB
    float bx = 0.0f, by = 0.0f, bz = 0.0f, bw = 0.0f;   // sum w_uA uB_q, sum w_uA
    int plane = 0;
    for (int dy = -r; dy <= r; dy++) {
        for (int dx = -r; dx <= r; dx++) {
            float2* e = sE + plane * NE;
#pragma unroll
            for (int k = 0; k < 2; k++) {
                const int idx = tid + 256 * k;
                if (idx < NE) {
                    const int tgx = min(max(sgx[k] + dx, 0), W - 1), tgy = min(max(sgy[k] + dy, 0), H - 1);
                    const int lt = (tgy - oy) * S + (tgx - ox);
                    const float4 qa = sA[lt], qb = sB[lt], qv = sV[lt];
                    const float2 d0 = nlm_delta(pa[k].x, qa.x, pb[k].x, qb.x, pv[k].x, qv.x, alpha, eps, kk);
                    const float2 d1 = nlm_delta(pa[k].y, qa.y, pb[k].y, qb.y, pv[k].y, qv.y, alpha, eps, kk);
                    const float2 d2 = nlm_delta(pa[k].z, qa.z, pb[k].z, qb.z, pv[k].z, qv.z, alpha, eps, kk);
                    e[idx] = make_float2(((d0.x + d1.x) + d2.x) * (1.0f / 3.0f), ((d0.y + d1.y) + d2.y) * (1.0f / 3.0f));
                }
            }
            __syncthreads();
            const int qi = i + dx, qj = j + dy;
            if (live && qi >= 0 && qi < W && qj >= 0 && qj < H) {
                float wa = 1.0f, wb = 1.0f;
                if (dx != 0 || dy != 0) {
                    float da = 0.0f, db = 0.0f;
#pragma unroll
                    for (int vy = 0; vy <= 2 * F; vy++) {
#pragma unroll
                        for (int vx = 0; vx <= 2 * F; vx++) {
                            const float2 t = e[(ty + vy) * E + tx + vx];
                            da = da + t.x; db = db + t.y;
                        }
                    }
                    da = da * inv_np; db = db * inv_np;
                    const size_t q = (size_t)qj * W + qi;
                    const float4 aq = g0[q], nq = g1[q];
                    const float cx = ap.x - aq.x, cy = ap.y - aq.y, cz = ap.z - aq.z;
                    const float arg_a = (cx * cx + cy * cy + cz * cz) * inv_a;
                    const float wn = normal_weight(np, nq, sigma_n);
                    wa = expf(-(fmaxf(da, 0.0f) + arg_a)) * wn;
                    wb = expf(-(fmaxf(db, 0.0f) + arg_a)) * wn;
                }
                const int lq = (ty + R + dy) * S + tx + R + dx;
                const float4 qa = sA[lq], qb = sB[lq];
                bx = bx + wa * qb.x; by = by + wa * qb.y; bz = bz + wa * qb.z; bw = bw + wa;
                ax = ax + wb * qa.x; ay = ay + wb * qa.y; az = az + wb * qa.z; aw = aw + wb;
            }
            plane ^= 1;
        }
    }
    if (!live) return;
    const float fax = ax / aw, fay = ay / aw, faz = az / aw, fbx = bx / bw, fby = by / bw, fbz = bz / bw;
    const float3 m = albedo_divisor(ap, a.demodulate);
    out[3 * p] = (double)(((fax + fbx) * 0.5f) * m.x); out[3 * p + 1] = (double)(((fay + fby) * 0.5f) * m.y); out[3 * p + 2] = (double)(((faz + fbz) * 0.5f) * m.z);
    if (out_error) {
        const float ex = ((fax - fbx) * 0.5f) * m.x, ey = ((fay - fby) * 0.5f) * m.y, ez = ((faz - fbz) * 0.5f) * m.z;
        out_error[3 * p] = (double)(ex * ex); out_error[3 * p + 1] = (double)(ey * ey); out_error[3 * p + 2] = (double)(ez * ez);
    }
}

template <int F>
hipError_t launch_filter(dim3 grid, size_t lds, hipStream_t stream, const float4* uA, const float4* uB, const float4* Vs, const float4* g0, const float4* g1, int W,
                         int H, const NlmArgs& a, double* out, double* out_error) {
    // more than the 64 KiB a kernel gets without asking
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(&nlm_filter<F>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(nlm_filter<F>, grid, dim3(NLM_TILE, NLM_TILE), lds, stream, uA, uB, Vs, g0, g1, W, H, a, out, out_error);
    return hipGetLastError();
}

}  // namespace

// the filter kernel's LDS in bytes at (search_radius, patch_radius)
size_t nlm_lds_bytes(int r, int f) {
    const size_t S = NLM_TILE + 2 * (r + f), E = NLM_TILE + 2 * f;
    return 3 * S * S * sizeof(float4) + 2 * E * E * sizeof(float2);
}

// d_half_a / d_half_b / d_variance / d_albedo / d_normal: W*H*3 doubles on the device; d_ua / d_ub / d_vh / d_vs / d_g0 / d_g1: W*H float4 scratch; d_out: W*H*3
// doubles (may be d_half_a: the halves have been packed before the filter writes); d_out_error likewise (may be null, may be d_half_b).  The caller has
// validated the parameters (zr_denoise_nlm).
hipError_t launch_denoise_nlm(const double* d_half_a, const double* d_half_b, const double* d_variance, const double* d_albedo, const double* d_normal, int W, int H,
                              const zr_denoise_nlm_params& dp, float4* d_ua, float4* d_ub, float4* d_vh, float4* d_vs, float4* d_g0, float4* d_g1, double* d_out,
                              double* d_out_error, hipStream_t stream) {
    static_assert(NLM_TILE == 16, "the filter's tiles are the blocks of grid16");
    const dim3 block(16, 16), grid = grid16(W, H);
    const int demod = dp.demodulate_albedo ? 1 : 0;
    hipLaunchKernelGGL(nlm_pack, grid, block, 0, stream, d_half_a, d_half_b, d_variance, d_albedo, d_normal, W, H, demod, d_ua, d_ub, d_vh, d_g0, d_g1);
    hipLaunchKernelGGL(nlm_smooth, grid, block, 0, stream, (const float4*)d_vh, W, H, d_vs);
    NlmArgs a;
    const int f = dp.patch_radius, np = (2 * f + 1) * (2 * f + 1);
    a.r = dp.search_radius; a.demodulate = demod;
    a.kk = dp.k * dp.k; a.alpha = dp.alpha; a.eps = dp.epsilon;
    a.inv_a = 1.0f / (dp.sigma_albedo * dp.sigma_albedo);
    a.sigma_n = dp.sigma_normal;
    a.inv_np = 1.0f / (float)np;
    const size_t lds = nlm_lds_bytes(a.r, f);
    switch (f) {
        case 0: return launch_filter<0>(grid, lds, stream, d_ua, d_ub, d_vs, d_g0, d_g1, W, H, a, d_out, d_out_error);
        case 1: return launch_filter<1>(grid, lds, stream, d_ua, d_ub, d_vs, d_g0, d_g1, W, H, a, d_out, d_out_error);
        case 2: return launch_filter<2>(grid, lds, stream, d_ua, d_ub, d_vs, d_g0, d_g1, W, H, a, d_out, d_out_error);
        default: return launch_filter<3>(grid, lds, stream, d_ua, d_ub, d_vs, d_g0, d_g1, W, H, a, d_out, d_out_error);
    }
}

}  // namespace zr
