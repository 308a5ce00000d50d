// zr_robust.hip — the firefly-robust resolve of a zr_accum: a symmetric trimmed mean over a pixel's 64 lane sums whose trim follows their Gini
// coefficient, after Buisine et al., "Firefly removal in Monte Carlo rendering with adaptive Median of meaNs" (EGSR 2021).  The rule is stated in
// include/zr_capi.h (zr_accum_resolve_robust) and restated operation for operation by tests/robust_model.py; compiled without contraction (csrc/Makefile).
// One wave per pixel, four pixels per block, the three coalesced 512-byte rows that accum_variance reads; lane 0 writes.  No atomics, no scratch, no LDS.
// The rank is a stable total order that the header defines by counting, and here it IS counted: every lane's key is broadcast through a scalar register
// pair (v_readlane with a constant lane) and compared with the lane's own — 64 steps of four instructions, no sorting network whose wiring the result could
// depend on (profiles/robust_resolve.txt has the listing and the comparison with a bitonic network).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "zr_launch.h"

namespace zr {
namespace {

__device__ __forceinline__ double xor_lane(double v, int m) { return __hiloint2double(__shfl_xor(__double2hiint(v), m, 64), __shfl_xor(__double2loint(v), m, 64)); }

// the xor butterfly 32, 16, ... 1 of stream_reduce: every lane ends with the total
__device__ __forceinline__ double wave_total(double v) {
    for (int m = 32; m >= 1; m >>= 1) v += xor_lane(v, m);
    return v;
}

// lane j's value in every lane (j uniform)
__device__ __forceinline__ double from_lane(double v, int j) {
    return __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(v), j), __builtin_amdgcn_readlane(__double2loint(v), j));
}

// r_l = #{ j : k_j < k_l, or k_j == k_l and j < l } for keys without NaN.  The first term is counted for every wave.  The 64 first terms sum to the number of
// pairs of lanes with unequal keys, 2016 when no two keys tie: only a wave with ties (a pixel of the background, whose lanes are all equal) counts the second.
__device__ __forceinline__ int stable_rank(double key, int lane) {
    int r = 0;
#pragma unroll
    for (int j = 0; j < 64; j++) r += from_lane(key, j) < key ? 1 : 0;
    int pairs = r;
    for (int m = 32; m >= 1; m >>= 1) pairs += __shfl_xor(pairs, m, 64);
    if (__builtin_amdgcn_readfirstlane(pairs) != 2016) {
#pragma unroll
        for (int j = 0; j < 63; j++) r += (from_lane(key, j) == key && j < lane) ? 1 : 0;
    }
    return r;
}

constexpr long long INF_BITS = 0x7FF0000000000000ll;

// pixels: the slots' packed pixels of a frame W wide, or null for slot i -> output i (zr_kat_resolve_robust); out_var / out_trim may be null
__global__ __launch_bounds__(256) void accum_resolve_robust(const double* __restrict__ partial, const uint32_t* __restrict__ pixels, const int32_t* __restrict__ count,
                                                             int uniform_count, uint32_t n_pix, int W, int mode, int trim, double strength,
                                                             double* __restrict__ out, double* __restrict__ out_var, int32_t* __restrict__ out_trim) {
    const uint32_t i = blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (i >= n_pix) return;   // (a whole wave: the broadcasts and butterflies below see all 64 lanes)
    const double* q = partial + (size_t)i * 192 + lane;
    const double S[3] = {q[0], q[64], q[128]};
    const int m = (count ? count[i] : uniform_count) / 64;
    const double inf = __longlong_as_double(INF_BITS);

    // key, rank
    const double v = (S[0] + S[1]) + S[2];
    const bool bad = !isfinite(v);
    const int n_bad = __popcll(__ballot(bad));
    const double key = bad ? inf : v;
    const int r = stable_rank(key, lane);

    // Gini: the good lanes hold the ranks 0 .. 63 - n_bad, so the largest finite key is that of rank 63 - n_bad
    const unsigned long long top = __ballot(r == 63 - n_bad);
    const double K = n_bad < 64 ? from_lane(key, (__ffsll((long long)top) - 1) & 63) : 0.0;
    const double kh = bad ? K : key;
    const double T = wave_total(kh);
    const double A = wave_total((double)(2 * r - 63) * kh);
    double g;
    if (!isfinite(T) || !isfinite(A)) g = 1.0;
    else if (T <= 0.0) g = 0.0;
    else {
        g = A / (64.0 * T);
        g = g < 0.0 ? 0.0 : g;
        g = g > 1.0 ? 1.0 : g;
    }

    // trim
    int t = trim;
    if (mode == 0) {
        double x = strength * g;
        x = x > 1.0 ? 1.0 : x;
        t = (int)floor(x * 32.0);
        t = t > 31 ? 31 : t;
    }
    const int floor_t = n_bad > 31 ? 31 : n_bad;
    t = t < floor_t ? floor_t : t;
    const bool kept = t <= r && r <= 63 - t;
    const int n_k = 64 - 2 * t;

    const double scale = 1.0 / (double)(m * n_k);
    const double inv_m = 1.0 / (double)m, inv_nk = 1.0 / (double)n_k, inv_nk1 = 1.0 / (double)(n_k - 1);
    double col[3], var[3];
#pragma unroll
    for (int c = 0; c < 3; c++) {
        const double Tk = wave_total(kept ? S[c] : 0.0);
        col[c] = Tk * scale;
        const double mu = Tk * inv_nk;
        const double d = kept ? S[c] - mu : 0.0;
        const double Q = wave_total(d * d);
        var[c] = isfinite(Tk) ? Q * inv_nk1 * inv_nk * inv_m * inv_m : inf;
        if (n_bad >= 32) { col[c] = inf; var[c] = inf; }
    }
    if (lane == 0) {
        size_t o = i;
        if (pixels) { const uint32_t pk = pixels[i]; o = (size_t)(pk >> 16) * W + (pk & 0xFFFFu); }
        out[o * 3] = col[0]; out[o * 3 + 1] = col[1]; out[o * 3 + 2] = col[2];
        if (out_var) { out_var[o * 3] = var[0]; out_var[o * 3 + 1] = var[1]; out_var[o * 3 + 2] = var[2]; }
        if (out_trim) out_trim[o] = t;
    }
}

}  // namespace

hipError_t launch_accum_resolve_robust(const double* partial, const uint32_t* pixels, const int32_t* count, int uniform_count, uint32_t n_pix, int W, int mode,
                                       int trim, double strength, double* out, double* out_var, int32_t* out_trim, hipStream_t stream) {
    if (n_pix == 0) return hipSuccess;
    hipLaunchKernelGGL(accum_resolve_robust, dim3((n_pix + 3) / 4), dim3(256), 0, stream, partial, pixels, count, uniform_count, n_pix, W, mode, trim, strength, out,
                       out_var, out_trim);
    return hipGetLastError();
}

}  // namespace zr
