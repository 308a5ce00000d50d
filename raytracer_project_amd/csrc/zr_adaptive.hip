// zr_adaptive.hip — adaptive sampling over a zr_accum: the noise estimate of a pixel from its 64 lane sums, the pass kernel that adds a pass's
// samples to the still-active pixels and decides which of them go on, the stable compaction of the active list, the resolve with a sample count per pixel, and
// the per-channel variance of a pixel's mean that the variance-guided denoiser reads (tests/denoise_guided_model.py restates it) and the two half
// images that the non-local-means denoiser cross-filters (tests/denoise_nlm_model.py).
// Compiled without contraction (csrc/Makefile): tests/adaptive_model.py restates the estimate operation for operation, and the decisions of an adaptive run
// are exactly `err > threshold` on those numbers.  No atomics: the next pass's pixel list depends on the flags alone, never on the order waves ran in.
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

// The relative standard error of a pixel's mean from its lane sums (this lane's sx, sy, sz), `count` = 64 m samples: the 64 lane sums of the channel sum are
// 64 equally weighted, independent estimates of m times the pixel.  Every lane returns the same number.  All lanes equal: exactly 0.  A non-finite total: +inf.
__device__ __forceinline__ double noise_estimate(double sx, double sy, double sz, int count, double dark_floor) {
    const double v = sx + sy + sz;
    const double T = wave_total(v);
    const double mu = T * (1.0 / 64);
    const double d = v - mu;
    const double Q = wave_total(d * d);
    const double inv_m = 1.0 / (double)(count / 64);
    const double se = sqrt(Q * (1.0 / 63) * (1.0 / 64)) * inv_m;
    const double I = mu * inv_m;
    if (!isfinite(T)) return __longlong_as_double(0x7FF0000000000000ll);
    if (Q == 0.0) return 0.0;
    return se / (I + dark_floor);
}

// One pass of an adaptive run, one wave per ACTIVE pixel: list position i holds the pass's samples ([n_list][n][3], sample sample0 + sidx at index sidx) of the
// accumulator slot slot[i].  Adds them to that slot's lane sums exactly as stream_accumulate does (sample s to lane s % 64, in increasing s), and with the
// updated sums still in registers evaluates the estimate: the new count per slot, and per list position flag = 1 (noisy, goes on), 2 (noisy, but at
// max_samples) or 0 (converged).  The estimate itself is not stored: zr_accum_error recomputes it from the sums with the caller's dark floor.
// n = 0: the estimate of the sums as they are.
__global__ __launch_bounds__(256) void adaptive_accumulate(const double* __restrict__ samples, const uint32_t* __restrict__ slot, uint32_t n_list, uint32_t n,
                                                            uint32_t sample0, double* __restrict__ partial, int32_t* __restrict__ count,
                                                            uint32_t* __restrict__ flag, int new_count, int max_samples, double threshold, double dark_floor) {
    const uint32_t i = blockIdx.x * 4 + (threadIdx.x >> 6);
    const uint32_t lane = threadIdx.x & 63u;
    if (i >= n_list) return;   // (a whole wave: the butterflies below see all 64 lanes)
    const uint32_t k = slot[i];
    double* q = partial + (size_t)k * 192 + lane;
    double sx = q[0], sy = q[64], sz = q[128];
    const uint32_t first = (lane - sample0) & 63u;   // the pass's first sample of this lane: (sample0 + first) % 64 == lane
    if (first < n) {
        const double* pp = samples + (size_t)i * n * 3;
        for (uint32_t sidx = first; sidx < n; sidx += 64) { sx += pp[(size_t)sidx * 3]; sy += pp[(size_t)sidx * 3 + 1]; sz += pp[(size_t)sidx * 3 + 2]; }
        q[0] = sx; q[64] = sy; q[128] = sz;
    }
    const double e = noise_estimate(sx, sy, sz, new_count, dark_floor);
    if (lane == 0) {
        count[k] = new_count;
        flag[i] = e > threshold ? (new_count < max_samples ? 1u : 2u) : 0u;
    }
}

// the estimate of every slot's sums as they are (zr_accum_error); count: per slot, or null for `uniform_count` everywhere
__global__ __launch_bounds__(256) void accum_error(const double* __restrict__ partial, const int32_t* __restrict__ count, int uniform_count, uint32_t n_pix,
                                                    double dark_floor, double* __restrict__ err) {
    const uint32_t i = blockIdx.x * 4 + (threadIdx.x >> 6);
    const uint32_t lane = threadIdx.x & 63u;
    if (i >= n_pix) return;
    const double* q = partial + (size_t)i * 192 + lane;
    const double e = noise_estimate(q[0], q[64], q[128], count ? count[i] : uniform_count, dark_floor);
    if (lane == 0) err[i] = e;
}

// The variance of every slot's mean, per channel (zr_accum_variance), into the slot's pixel of a frame W wide: with `count` = 64 m samples the 64
// lane sums of a channel are 64 equally weighted, independent estimates of m times the pixel, so
//   T = sum S_l;  mu = T * (1.0 / 64);  d_l = S_l - mu;  Q = sum d_l * d_l;  var = Q * (1.0 / 63) * (1.0 / 64) * (1.0 / m) * (1.0 / m)
// (both sums by wave_total).  All lanes equal: exactly 0.  A non-finite total: +inf.  count: per slot, or null for `uniform_count` everywhere.
__global__ __launch_bounds__(256) void accum_variance(const double* __restrict__ partial, const uint32_t* __restrict__ pixels, const int32_t* __restrict__ count,
                                                       int uniform_count, uint32_t n_pix, int W, double* __restrict__ out) {
    const uint32_t i = blockIdx.x * 4 + (threadIdx.x >> 6);
    const uint32_t lane = threadIdx.x & 63u;
    if (i >= n_pix) return;   // (a whole wave: the butterflies below see all 64 lanes)
    const double* q = partial + (size_t)i * 192 + lane;
    const double inv_m = 1.0 / (double)((count ? count[i] : uniform_count) / 64);
    double var[3];
#pragma unroll
    for (int c = 0; c < 3; c++) {
        const double S = q[64 * c];
        const double T = wave_total(S);
        const double mu = T * (1.0 / 64);
        const double d = S - mu;
        const double Q = wave_total(d * d);
        var[c] = isfinite(T) ? Q * (1.0 / 63) * (1.0 / 64) * inv_m * inv_m : __longlong_as_double(0x7FF0000000000000ll);
    }
    if (lane == 0) {
        const uint32_t pk = pixels[i];
        double* o = out + ((size_t)(pk >> 16) * W + (pk & 0xFFFFu)) * 3;
        o[0] = var[0]; o[1] = var[1]; o[2] = var[2];
    }
}

// The two half images of every slot (zr_accum_halves), into the slot's pixel of two frames W wide: the resolve butterfly stopped one step early.
// After the steps 32, 16, 8, 4, 2 lane 0 holds T_A, the sum of the even lanes, and lane 1 T_B, the sum of the odd lanes; with `count` = 64 m samples each half
// holds count / 2 of them: A = T_A * (1.0 / (count / 2)), B = T_B * (1.0 / (count / 2)).  The step the resolve goes on with is T_A + T_B.  count: as above.
__global__ __launch_bounds__(256) void accum_halves(const double* __restrict__ partial, const uint32_t* __restrict__ pixels, const int32_t* __restrict__ count,
                                                     int uniform_count, uint32_t n_pix, int W, double* __restrict__ out_a, double* __restrict__ out_b) {
    const uint32_t i = blockIdx.x * 4 + (threadIdx.x >> 6);
    const uint32_t lane = threadIdx.x & 63u;
    if (i >= n_pix) return;   // (a whole wave: the butterflies below see all 64 lanes)
    const double* q = partial + (size_t)i * 192 + lane;
    double sx = q[0], sy = q[64], sz = q[128];
    for (int m = 32; m >= 2; m >>= 1) { sx += xor_lane(sx, m); sy += xor_lane(sy, m); sz += xor_lane(sz, m); }
    if (lane < 2) {
        const uint32_t pk = pixels[i];
        const double scale = 1.0 / (double)((count ? count[i] : uniform_count) / 2);
        double* o = (lane == 0 ? out_a : out_b) + ((size_t)(pk >> 16) * W + (pk & 0xFFFFu)) * 3;
        o[0] = sx * scale; o[1] = sy * scale; o[2] = sz * scale;
    }
}

// accum_resolve (zr_stream.hip) with 1.0 / count[pixel]: same butterflies, same asc_lanes rule
__global__ __launch_bounds__(256) void accum_resolve_counts(const double* __restrict__ partial, const uint32_t* __restrict__ pixels, const int32_t* __restrict__ count,
                                                             uint32_t n_pix, int W, int asc_lanes, double* __restrict__ out) {
    const uint32_t i = blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (i >= n_pix) return;
    const double* q = partial + (size_t)i * 192 + lane;
    double sx = q[0], sy = q[64], sz = q[128];
    for (int m = 32; m >= asc_lanes; m >>= 1) { sx += xor_lane(sx, m); sy += xor_lane(sy, m); sz += xor_lane(sz, m); }
    for (int m = 1; m < asc_lanes; m <<= 1) { sx += xor_lane(sx, m); sy += xor_lane(sy, m); sz += xor_lane(sz, m); }
    if (lane == 0) {
        const uint32_t pk = pixels[i];
        const int px = (int)(pk & 0xFFFFu), py = (int)(pk >> 16);
        const double scale = 1.0 / count[i];
        double* o = out + ((size_t)py * W + px) * 3;
        o[0] = sx * scale; o[1] = sy * scale; o[2] = sz * scale;
    }
}

// ---- stable compaction of the list positions whose flag is 1: block counts, a scan of them, a scatter ------------------------------------------------
// A block covers 256 consecutive list positions.  The order of the list survives (it is the tile order that carries the pipeline's coherence).

// this thread's position among the flagged threads of its block, and (in *block_total) how many there are; s_wave: 4 words of LDS
__device__ __forceinline__ uint32_t block_rank(bool on, uint32_t* s_wave, uint32_t* block_total) {
    const unsigned long long bm = __ballot(on);
    const int wl = threadIdx.x & 63, w = threadIdx.x >> 6;
    if (wl == 0) s_wave[w] = (uint32_t)__popcll(bm);
    __syncthreads();
    uint32_t before = 0, total = 0;
    for (int k = 0; k < 4; k++) { const uint32_t c = s_wave[k]; total += c; if (k < w) before += c; }
    *block_total = total;
    return before + (uint32_t)__popcll(bm & ((1ull << wl) - 1ull));
}

__global__ __launch_bounds__(256) void compact_count(const uint32_t* __restrict__ flag, uint32_t n_list, uint32_t* __restrict__ block_active,
                                                      uint32_t* __restrict__ block_at_max) {
    __shared__ uint32_t s_a[4], s_m[4];
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    const uint32_t f = i < n_list ? flag[i] : 0u;
    uint32_t n_active, n_at_max;
    (void)block_rank(f == 1u, s_a, &n_active);
    (void)block_rank(f == 2u, s_m, &n_at_max);
    if (threadIdx.x == 0) { block_active[blockIdx.x] = n_active; block_at_max[blockIdx.x] = n_at_max; }
}

// one block: block_active[] becomes its exclusive prefix sum, totals = {active, at max} positions of the whole list.  Thread t owns a contiguous chunk.
__global__ __launch_bounds__(256) void compact_scan(uint32_t* __restrict__ block_active, const uint32_t* __restrict__ block_at_max, uint32_t n_blocks,
                                                     uint32_t* __restrict__ totals) {
    __shared__ uint32_t s_a[256], s_m[256];
    const uint32_t chunk = (n_blocks + 255u) / 256u;
    const uint32_t b0 = min(threadIdx.x * chunk, n_blocks), b1 = min(b0 + chunk, n_blocks);
    uint32_t a = 0, m = 0;
    for (uint32_t b = b0; b < b1; b++) { a += block_active[b]; m += block_at_max[b]; }
    s_a[threadIdx.x] = a; s_m[threadIdx.x] = m;
    __syncthreads();
    uint32_t base = 0;
    for (uint32_t t = 0; t < threadIdx.x; t++) base += s_a[t];
    for (uint32_t b = b0; b < b1; b++) { const uint32_t c = block_active[b]; block_active[b] = base; base += c; }
    if (threadIdx.x == 255) {
        uint32_t tm = 0;
        for (int t = 0; t < 256; t++) tm += s_m[t];
        totals[0] = base; totals[1] = tm;
    }
}

__global__ __launch_bounds__(256) void compact_scatter(const uint32_t* __restrict__ flag, uint32_t n_list, const uint32_t* __restrict__ block_offset,
                                                        const uint32_t* __restrict__ pixels_in, const uint32_t* __restrict__ slot_in,
                                                        uint32_t* __restrict__ pixels_out, uint32_t* __restrict__ slot_out) {
    __shared__ uint32_t s_a[4];
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    const bool on = i < n_list && flag[i] == 1u;
    uint32_t total;
    const uint32_t r = block_rank(on, s_a, &total);
    if (!on) return;
    const uint32_t d = block_offset[blockIdx.x] + r;   // < the list's active count <= n_list: the outputs are as long as the inputs
    pixels_out[d] = pixels_in[i]; slot_out[d] = slot_in[i];
}

}  // namespace

hipError_t launch_adaptive_accumulate(const double* samples, const uint32_t* slot, uint32_t n_list, uint32_t n, uint32_t sample0, double* partial, int32_t* count,
                                      uint32_t* flag, int new_count, int max_samples, double threshold, double dark_floor, hipStream_t stream) {
    if (n_list == 0) return hipSuccess;
    hipLaunchKernelGGL(adaptive_accumulate, dim3((n_list + 3) / 4), dim3(256), 0, stream, samples, slot, n_list, n, sample0, partial, count, flag, new_count,
                       max_samples, threshold, dark_floor);
    return hipGetLastError();
}

hipError_t launch_adaptive_compact(const uint32_t* flag, uint32_t n_list, const uint32_t* pixels_in, const uint32_t* slot_in, uint32_t* pixels_out,
                                   uint32_t* slot_out, uint32_t* block_active, uint32_t* block_at_max, uint32_t* totals, hipStream_t stream) {
    if (n_list == 0) return hipMemsetAsync(totals, 0, 2 * sizeof(uint32_t), stream);
    const uint32_t n_blocks = (uint32_t)(((uint64_t)n_list + 255u) / 256u);
    hipLaunchKernelGGL(compact_count, dim3(n_blocks), dim3(256), 0, stream, flag, n_list, block_active, block_at_max);
    hipLaunchKernelGGL(compact_scan, dim3(1), dim3(256), 0, stream, block_active, block_at_max, n_blocks, totals);
    hipLaunchKernelGGL(compact_scatter, dim3(n_blocks), dim3(256), 0, stream, flag, n_list, block_active, pixels_in, slot_in, pixels_out, slot_out);
    return hipGetLastError();
}

hipError_t launch_accum_error(const double* partial, const int32_t* count, int uniform_count, uint32_t n_pix, double dark_floor, double* err, hipStream_t stream) {
    if (n_pix == 0) return hipSuccess;
    hipLaunchKernelGGL(accum_error, dim3((n_pix + 3) / 4), dim3(256), 0, stream, partial, count, uniform_count, n_pix, dark_floor, err);
    return hipGetLastError();
}

hipError_t launch_accum_variance(const double* partial, const uint32_t* pixels, const int32_t* count, int uniform_count, uint32_t n_pix, int W, double* out,
                                 hipStream_t stream) {
    if (n_pix == 0) return hipSuccess;
    hipLaunchKernelGGL(accum_variance, dim3((n_pix + 3) / 4), dim3(256), 0, stream, partial, pixels, count, uniform_count, n_pix, W, out);
    return hipGetLastError();
}

hipError_t launch_accum_halves(const double* partial, const uint32_t* pixels, const int32_t* count, int uniform_count, uint32_t n_pix, int W, double* out_a,
                               double* out_b, hipStream_t stream) {
    if (n_pix == 0) return hipSuccess;
    hipLaunchKernelGGL(accum_halves, dim3((n_pix + 3) / 4), dim3(256), 0, stream, partial, pixels, count, uniform_count, n_pix, W, out_a, out_b);
    return hipGetLastError();
}

hipError_t launch_accum_resolve_counts(const double* partial, const uint32_t* pixels, const int32_t* count, uint32_t n_pix, int W, int asc_lanes, double* out,
                                       hipStream_t stream) {
    if (n_pix == 0) return hipSuccess;
    hipLaunchKernelGGL(accum_resolve_counts, dim3((n_pix + 3) / 4), dim3(256), 0, stream, partial, pixels, count, n_pix, W, asc_lanes, out);
    return hipGetLastError();
}

}  // namespace zr
