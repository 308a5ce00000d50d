// zr_sky.hip — the sky pre-pass of the streaming pipeline: before a frame's round loop starts, the pixels whose every camera ray provably sees only
// the environment are finished here, one wave per pixel, and the rest are compacted, in order, into the list the pipeline walks.  A sky sample needs camera_ray
// and background and nothing else; through the pipeline it cost a slot-round and ~250 bytes of traffic.  Only certain misses are decided (zr_device.h:
// camera_ray_escapes — EXTEND's own box arithmetic and the two sphere predicates), no hit is ever resolved outside EXTEND, and a sky pixel's value is formed by
// the arithmetic that forms it in the pipeline: begin_sample's ray, SHADE's MISS stage for a first miss (the sample is background(ray.d)), stream_reduce's sum
// (wave_pixel_mean).  Compiled with the flags of zr_stream.hip: the ray and the background contract their multiply-adds as they do there.
#include "zr_device.h"
#include "zr_launch.h"
#include <algorithm>
#include <cstdlib>

namespace zr {
namespace {

// One wave per listed pixel.  Classify: lane l makes the camera rays of samples l, l + 64, ... of [sample0, sample0 + spp) exactly as begin_sample does and asks
// camera_ray_escapes; the ballot after a batch of 64 lets a pixel with a ray that does not escape leave at once (nearly every non-sky pixel, after one ray per
// lane).  Fill: a pixel whose every ray escapes gets its mean written to `out`; nothing goes to samples[].  flag[i] = 1: the pixel stays with the pipeline.
__device__ __forceinline__ void sky_pixel(const DScene& sc, const DCamera& cam, const DEnv& env, uint64_t seed, const uint32_t* __restrict__ pixels, uint32_t i, int lane,
                                          uint32_t spp, uint32_t sample0, uint32_t* __restrict__ flag, double* __restrict__ out) {
    const uint32_t pk = pixels[i];
    const int px = (int)(pk & 0xFFFFu), py = (int)(pk >> 16);
    const uint64_t pixel = (uint64_t)py * (uint64_t)cam.W + (uint64_t)px;
    auto ray_of = [&](uint32_t sidx) {
        Rng g; g.key = zr_stream_key(seed, pixel, (uint64_t)(sample0 + sidx)); g.k = 0; g.bounce = 0;
        return camera_ray(cam, px, py, g);
    };
    for (uint32_t base = 0; base < spp; base += 64) {   // (wave-uniform)
        const uint32_t sidx = base + (uint32_t)lane;
        const bool stays = sidx < spp && !camera_ray_escapes(ray_of(sidx), sc.root, sc.spheres);
        if (__ballot(stays) != 0ull) {
            if (lane == 0) flag[i] = 1u;
            return;
        }
    }
    const V3 mean = wave_pixel_mean(lane, spp, cam.spp, [&](uint32_t sidx) {
        V3 bg = background(sc, env, ray_of(sidx).d);
        // the pipeline's sample is a value in memory (samples[unit]) before stream_reduce adds it: keep the background's last multiply from contracting into the sum
        asm volatile("" : "+v"(bg.x), "+v"(bg.y), "+v"(bg.z));
        return bg;
    });
    if (lane == 0) {
        flag[i] = 0u;
        double* o = out + ((size_t)py * cam.W + px) * 3;
        o[0] = mean.x; o[1] = mean.y; o[2] = mean.z;
    }
}

__global__ __launch_bounds__(256) void sky_prepass(DScene sc, DCamera cam, DEnv env, uint64_t seed, const uint32_t* __restrict__ pixels, uint32_t n_pix, uint32_t spp,
                                                   uint32_t sample0, uint32_t* __restrict__ flag, double* __restrict__ out) {
    const uint32_t i = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (i >= n_pix) return;   // (a whole wave: the ballots and butterflies of sky_pixel see all 64 lanes)
    sky_pixel(sc, cam, env, seed, pixels, i, (int)(threadIdx.x & 63), spp, sample0, flag, out);
}

// THE SIEVE (ZR_SKY_SIEVE=1; off by default).  sky_prepass spends a wave (64 camera rays) on every pixel to find, for five pixels in six of a cfg3 frame, that the
// first batch holds a ray that stays.  One thread per pixel asks that of ONE ray first, the ray of the pixel's first sample, made as sky_pixel makes it: a pixel is
// sky only if EVERY ray escapes, so a pixel whose first ray stays stays (flag 1, the value sky_pixel would have written), and only the others, the candidates
// (flag SKY_CANDIDATE), get their wave.  Flags, `out` and the walk list come out as without the sieve by construction.
// Measured (profiles/r25_round_loop_ab.txt): the pass's kernels take 4.90 ms of a cfg3 frame instead of 5.53 - the sky pixels' 512 rays and backgrounds are the
// pass, not the 1.7 M waves that leave after one batch - and the frame 296.5 against 296.7 ms, inside the run-to-run spread: not a gain one can show, so it is off.
enum : uint32_t { SKY_CANDIDATE = 2u };
__global__ __launch_bounds__(256) void sky_sieve(DScene sc, DCamera cam, uint64_t seed, const uint32_t* __restrict__ pixels, uint32_t n_pix, uint32_t sample0,
                                                 uint32_t* __restrict__ flag) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n_pix) return;
    const uint32_t pk = pixels[i];
    const int px = (int)(pk & 0xFFFFu), py = (int)(pk >> 16);
    const uint64_t pixel = (uint64_t)py * (uint64_t)cam.W + (uint64_t)px;
    Rng g; g.key = zr_stream_key(seed, pixel, (uint64_t)sample0); g.k = 0; g.bounce = 0;
    flag[i] = camera_ray_escapes(camera_ray(cam, px, py, g), sc.root, sc.spheres) ? (uint32_t)SKY_CANDIDATE : 1u;
}
// sky_pixel for the candidates cand[0 .. *n_cand) (list positions, in list order).  How many there are only the device knows: a fixed grid of waves strides over them.
__global__ __launch_bounds__(256) void sky_prepass_candidates(DScene sc, DCamera cam, DEnv env, uint64_t seed, const uint32_t* __restrict__ pixels,
                                                              const uint32_t* __restrict__ cand, const uint32_t* __restrict__ n_cand, uint32_t spp, uint32_t sample0,
                                                              uint32_t* __restrict__ flag, double* __restrict__ out) {
    const uint32_t n = *n_cand, waves = gridDim.x * 4u;
    for (uint32_t j = blockIdx.x * 4u + (threadIdx.x >> 6); j < n; j += waves)   // (wave-uniform)
        sky_pixel(sc, cam, env, seed, pixels, cand[j], (int)(threadIdx.x & 63), spp, sample0, flag, out);
}

// ---- stable compaction of the list positions whose flag is `want`: block counts, a scan of them, a scatter (the scheme of zr_adaptive.hip) -------------
// A block covers 256 consecutive list positions; the order of the list survives (bottom-up tile order: zr_render.cpp, upload_pixel_list).  want = 1: the pixels
// the pipeline walks; want = SKY_CANDIDATE: the sieve's candidates, as list positions (pixels == nullptr).

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

__global__ __launch_bounds__(256) void sky_count(const uint32_t* __restrict__ flag, uint32_t n_pix, uint32_t want, uint32_t* __restrict__ block_count) {
    __shared__ uint32_t s_w[4];
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    uint32_t total;
    (void)block_rank(i < n_pix && flag[i] == want, s_w, &total);
    if (threadIdx.x == 0) block_count[blockIdx.x] = total;
}

// one block: block_count[] becomes its exclusive prefix sum, *n_walk the flagged positions of the whole list.  Thread t owns a contiguous chunk.
__global__ __launch_bounds__(256) void sky_scan(uint32_t* __restrict__ block_count, uint32_t n_blocks, uint32_t* __restrict__ n_walk) {
    __shared__ uint32_t s_a[256];
    const uint32_t chunk = (n_blocks + 255u) / 256u;
    const uint32_t b0 = min(threadIdx.x * chunk, n_blocks), b1 = min(b0 + chunk, n_blocks);
    uint32_t a = 0;
    for (uint32_t b = b0; b < b1; b++) a += block_count[b];
    s_a[threadIdx.x] = a;
    __syncthreads();
    uint32_t base = 0;
    for (uint32_t t = 0; t < threadIdx.x; t++) base += s_a[t];
    for (uint32_t b = b0; b < b1; b++) { const uint32_t c = block_count[b]; block_count[b] = base; base += c; }
    if (threadIdx.x == 255) *n_walk = base;
}

__global__ __launch_bounds__(256) void sky_scatter(const uint32_t* __restrict__ flag, uint32_t n_pix, uint32_t want, const uint32_t* __restrict__ block_offset,
                                                   const uint32_t* __restrict__ pixels, uint32_t* __restrict__ walk) {
    __shared__ uint32_t s_w[4];
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    const bool on = i < n_pix && flag[i] == want;
    uint32_t total;
    const uint32_t r = block_rank(on, s_w, &total);
    if (!on) return;
    walk[block_offset[blockIdx.x] + r] = pixels ? pixels[i] : i;   // < the flagged count <= n_pix: `walk` is as long as the list
}

}  // namespace

hipError_t launch_sky_prepass(const DScene& sc, const DCamera& cam, const DEnv& env, uint64_t seed, const uint32_t* pixels, uint32_t n_pix, uint32_t spp,
                              uint32_t sample0, double* out, uint32_t* flag, uint32_t* block_count, uint32_t* walk, uint32_t* n_walk, hipStream_t stream) {
    if (n_pix == 0) return hipMemsetAsync(n_walk, 0, sizeof(uint32_t), stream);
    const uint32_t n_blocks = (uint32_t)(((uint64_t)n_pix + 255u) / 256u);
    auto compact = [&](uint32_t want, const uint32_t* src) {
        hipLaunchKernelGGL(sky_count, dim3(n_blocks), dim3(256), 0, stream, flag, n_pix, want, block_count);
        hipLaunchKernelGGL(sky_scan, dim3(1), dim3(256), 0, stream, block_count, n_blocks, n_walk);
        hipLaunchKernelGGL(sky_scatter, dim3(n_blocks), dim3(256), 0, stream, flag, n_pix, want, block_count, src, walk);
    };
    const char* sieve_env = std::getenv("ZR_SKY_SIEVE");   // (1: the sieve; otherwise every pixel gets its wave)
    if (!sieve_env || std::atoi(sieve_env) == 0)
        hipLaunchKernelGGL(sky_prepass, dim3((n_pix + 3) / 4), dim3(256), 0, stream, sc, cam, env, seed, pixels, n_pix, spp, sample0, flag, out);
    else {
        // `walk` and `n_walk` hold the candidates and their number until the last compaction below overwrites them (one stream: the kernels run in this order)
        hipLaunchKernelGGL(sky_sieve, n_blocks, dim3(256), 0, stream, sc, cam, seed, pixels, n_pix, sample0, flag);
        compact(SKY_CANDIDATE, nullptr);
        const uint32_t grid = std::min<uint32_t>((n_pix + 3) / 4, 256u * 32u);   // 32 blocks for each of 256 CUs: enough to even out sky pixels (spp rays) and early leavers
        hipLaunchKernelGGL(sky_prepass_candidates, dim3(grid), dim3(256), 0, stream, sc, cam, env, seed, pixels, walk, n_walk, spp, sample0, flag, out);
    }
    compact(1u, pixels);
    return hipGetLastError();
}

}  // namespace zr
