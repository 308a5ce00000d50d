// zr_envlight.hip — the environment table of direct light sampling for gfx950 (the rules: include/zr_capi.h): the kernel that turns the HDR map's
// texels into per-row running sums of lum x solid angle, and the known-answer kernels of the sampling functions in zr_envlight.h.  The direct kernel that
// uses the table is render_direct_samples<., true> (zr_direct.hip).
#include "zr_device.h"
#include "zr_launch.h"
#include "zr_envlight.h"

namespace zr {

// Kernel `env_row_cdf`: one block of 256 threads (four wave64) per row.  Thread k owns the contiguous columns [k c, (k + 1) c), c = ceil(W / 256).  The row
// passes through LDS in tiles of ZR_ENV_TILE texels: the block reads a tile's texels with consecutive threads on consecutive texels and leaves their weights
// in LDS, then every thread sums the part of its columns that lies in the tile, left to right.  Thread 0 turns the 256 chunk sums into offsets with a
// sequential running sum in index order; a second pass over the tiles forms the weights again, replaces them by offset + running in LDS and writes the tile
// out with consecutive threads on consecutive entries.  No atomics and no dependence on scheduling: NumPy restates the order (envlight_model.chunked_cdf).
#define ZR_ENV_TILE 2048u

__global__ __launch_bounds__(ZR_BLOCK) void env_row_cdf(DScene sc, uint32_t tex, uint32_t W, const double* __restrict__ omega, double* __restrict__ cdf,
                                                         double* __restrict__ row_total, uint32_t* __restrict__ row_count) {
    __shared__ double w[ZR_ENV_TILE];
    __shared__ double chunk[ZR_BLOCK];
    __shared__ uint32_t cnt[ZR_BLOCK];
    const zr_texture& t = sc.texs[tex];
    const uint32_t tid = threadIdx.x, j = blockIdx.x;
    const uint32_t c = (W + ZR_BLOCK - 1) / ZR_BLOCK;
    const uint32_t my0 = (uint32_t)(((uint64_t)tid * c) < W ? (uint64_t)tid * c : W), my1 = W - my0 < c ? W : my0 + c;
    const double om = omega[j];
    double* out = cdf + (size_t)j * W;
    double run = 0;
    uint32_t n = 0;
    for (uint32_t tile0 = 0; tile0 < W; tile0 += ZR_ENV_TILE) {
        const uint32_t tw = W - tile0 < ZR_ENV_TILE ? W - tile0 : ZR_ENV_TILE;
        for (uint32_t x = tid; x < tw; x += ZR_BLOCK) w[x] = env_weight(env_lum(env_texel(sc, t, tile0 + x, j)), om);
        __syncthreads();
        const uint32_t lo = my0 > tile0 ? my0 : tile0, hi = my1 < tile0 + tw ? my1 : tile0 + tw;
        for (uint32_t x = lo; x < hi; x++) { const double v = w[x - tile0]; run += v; n += v > 0 ? 1u : 0u; }
        __syncthreads();
    }
    chunk[tid] = run; cnt[tid] = n;
    __syncthreads();
    if (tid == 0) {
        double acc = 0;
        uint32_t m = 0;
        for (uint32_t k = 0; k < ZR_BLOCK; k++) { const double s = chunk[k]; chunk[k] = acc; acc += s; m += cnt[k]; }
        row_total[j] = acc;   // = offset + running at column W - 1: the chunks behind its owner are empty and add 0
        row_count[j] = m;
    }
    __syncthreads();
    const double offset = chunk[tid];
    run = 0;
    for (uint32_t tile0 = 0; tile0 < W; tile0 += ZR_ENV_TILE) {
        const uint32_t tw = W - tile0 < ZR_ENV_TILE ? W - tile0 : ZR_ENV_TILE;
        for (uint32_t x = tid; x < tw; x += ZR_BLOCK) w[x] = env_weight(env_lum(env_texel(sc, t, tile0 + x, j)), om);
        __syncthreads();
        const uint32_t lo = my0 > tile0 ? my0 : tile0, hi = my1 < tile0 + tw ? my1 : tile0 + tw;
        for (uint32_t x = lo; x < hi; x++) { run += w[x - tile0]; w[x - tile0] = offset + run; }
        __syncthreads();
        for (uint32_t x = tid; x < tw; x += ZR_BLOCK) out[tile0 + x] = w[x];
        __syncthreads();
    }
}

hipError_t launch_env_row_cdf(const DScene& sc, uint32_t tex, uint32_t W, uint32_t H, const double* omega, double* cdf, double* row_total, uint32_t* row_count,
                              hipStream_t stream) {
    if (W == 0 || H == 0) return hipSuccess;
    hipLaunchKernelGGL(env_row_cdf, dim3(H), dim3(ZR_BLOCK), 0, stream, sc, tex, W, omega, cdf, row_total, row_count);
    return hipGetLastError();
}

// ---- known-answer kernels ----------------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(ZR_BLOCK) void kat_env_light_sample(DScene sc, DEnv env, LightTable lt, EnvLight el, const double* __restrict__ origins,
                                                                  const uint64_t* __restrict__ keys, const uint32_t* __restrict__ bounces,
                                                                  const double* __restrict__ draws8, size_t n, zr_light_sample* __restrict__ out) {
    const size_t k = (size_t)blockIdx.x * ZR_BLOCK + threadIdx.x;
    if (k >= n) return;
    LightRng lg; lg.key = zr_light_key(keys[k], bounces[k]); lg.j = 0; lg.forced = draws8 ? draws8 + k * 8 : nullptr;
    LightSample s;
    V3 le;
    direct_light_sample(sc, env, lt, el, ld3(origins + k * 3), lg, s, le);
    zr_light_sample o;
    o.choice = s.choice; o.slot = s.slot; o.kind = s.kind; o.index = s.index; o.draws = lg.j; o.pad_ = 0;
    o.y[0] = s.y.x; o.y[1] = s.y.y; o.y[2] = s.y.z; o.normal[0] = s.n.x; o.normal[1] = s.n.y; o.normal[2] = s.n.z; o.w[0] = s.w.x; o.w[1] = s.w.y; o.w[2] = s.w.z;
    o.dist = s.dist; o.pdf = s.pdf;
    out[k] = o;
}
__global__ __launch_bounds__(ZR_BLOCK) void kat_env_light_pdf(DScene sc, DEnv env, EnvLight el, const double* __restrict__ dirs, size_t n, double* __restrict__ out_pdf) {
    const size_t k = (size_t)blockIdx.x * ZR_BLOCK + threadIdx.x;
    if (k >= n) return;
    out_pdf[k] = env_light_pdf(el, background(sc, env, ld3(dirs + k * 3)));
}

hipError_t launch_kat_env_light_sample(const DScene& sc, const DEnv& env, const LightTable& lt, const EnvLight& el, const double* origins, const uint64_t* keys,
                                       const uint32_t* bounces, const double* draws8, size_t n, zr_light_sample* out, hipStream_t stream) {
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(kat_env_light_sample, dim3((unsigned)((n + ZR_BLOCK - 1) / ZR_BLOCK)), dim3(ZR_BLOCK), 0, stream, sc, env, lt, el, origins, keys, bounces, draws8, n, out);
    return hipGetLastError();
}
hipError_t launch_kat_env_light_pdf(const DScene& sc, const DEnv& env, const EnvLight& el, const double* dirs, size_t n, double* out_pdf, hipStream_t stream) {
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(kat_env_light_pdf, dim3((unsigned)((n + ZR_BLOCK - 1) / ZR_BLOCK)), dim3(ZR_BLOCK), 0, stream, sc, env, el, dirs, n, out_pdf);
    return hipGetLastError();
}

}  // namespace zr
