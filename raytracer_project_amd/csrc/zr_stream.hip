// zr_stream.hip — render variant 2: streaming wavefront pipeline for gfx950.
//
// The megakernels (variants 0/1) keep a whole path — ray, throughput, radiance, RNG, hit record, traversal — in
// registers: ~256 VGPRs, 2 waves per SIMD, and measured throughput is proportional to the number of resident
// waves (dependent BVH fetches: latency bound).  This variant splits the sample loop into stages so that the
// stage that chases pointers is register-lean and runs at several times the occupancy:
//
//   pool of P path SLOTS resident in HBM (SoA, FP64): ray, throughput, radiance, RNG position, pixel/sample ids
//   round:  EXTEND  persistent waves pull ray indices from a global head (ballot + one atomic per refill), walk the
//                   BVH with the NODE/LEAF wave scheduler (per-lane LDS stack, cull-on-pop) and write (t, object)
//           SHADE   one thread per slot: hit record, emission, scatter, Russian roulette, background; a finished
//                   path adds its radiance to the SLOT's running sum and the slot starts its next sample in place
//                   (regeneration), so every slot carries exactly one segment per round until the frame drains
//   end:    REDUCE  every finished sample wrote its radiance to samples[pixel][s]; one fixed-order sum per pixel
//                   gives the mean — no atomics on radiance anywhere, the image is bit-reproducible
//
// Work units: unit u = one primary sample = (pixel u / spp of the frame's pixel list, sample u % spp).  Slot k starts on
// unit k (64 consecutive slots = one pixel: coherent primary rays); a slot whose path ends writes the sample's
// radiance to samples[u] and takes the next unit from one of ST_SHARDS interleaved counters (one atomic per wave per
// round, spread over ST_SHARDS cache lines).  Every sample is written exactly once, by whichever slot computed it, and
// REDUCE sums a pixel's samples in an order that depends only on spp — so the image is bit-reproducible and does not
// depend on the pool size, on scheduling, or on how the frame is sharded over GPUs.
#include "zr_device.h"
#include "zr_launch.h"
#include "zr_units.h"
#ifdef ZR_SHADE_ASSERT   /* a debug build (ZR_DEFS=-DZR_SHADE_ASSERT): lean SHADE checks its early unit reservation against the lanes that end */
#include <cassert>
#endif

namespace zr {

#ifndef ST_EXT_WAVES
#define ST_EXT_WAVES 4  /* waves per SIMD the EXTEND kernel's register budget must allow */
#endif
#ifndef ST_CHUNK
#define ST_CHUNK 256    /* rays a wave reserves per global atomic */
#endif
#ifndef ST_SHADE_WAVES
#define ST_SHADE_WAVES 4 /* waves per SIMD the SHADE kernel must fit (128 VGPRs): its natural allocation sits at 126-129 */
#endif
#ifndef ST_EXT_WAVES_LEAN
#define ST_EXT_WAVES_LEAN 6  /* same for the triangles-and-spheres-only build of EXTEND */
#endif
#ifndef ST_EXT_WAVES_MID
#define ST_EXT_WAVES_MID 4   /* ... and for the build that adds bare / placed cubes and unwrapped media (cfg5): at 5 waves (96 VGPRs) it spills 18 registers and is 1.5 % slower, at 6 waves 14 % slower */
#endif
#ifndef ST_FETCH_MIN
#define ST_FETCH_MIN 16  /* idle lanes that trigger a refill even when another phase has more ready lanes */
#endif
#ifndef ST_LDS_STACK
#define ST_LDS_STACK 12
#endif

enum { F_FIRST = 1u << 16, F_ACTIVE = 1u << 17, F_L0 = 1u << 18,
       F_LZERO = 1u << 19 /* SF_L not written yet: it is (0,0,0) */, F_BONE = 1u << 20 /* SF_BETA not written yet: it is (1,1,1) */ };  // meta.y: bounce | b_inner << 8 | flags (F_L0: SF_SUM holds the primary hit's emission)

struct SEntry { uint32_t node; float tn; };

// Slot pool layout: array of 64-slot blocks, each block = SF_N rows of 64 x 8 bytes ([block][field][lane]).  A wave
// that works on 64 consecutive slots touches one contiguous 12 KB block, every field access is one coalesced
// 512-B row, and all of a slot's state shares a page (a plain [field][P] layout put each of the 23 fields 128 MB
// apart and ran the SHADE stage at 1.7 TB/s).
enum { SF_RAY = 0, SF_HIT_T = 6, SF_HIT_KI = 7, SF_BETA = 8, SF_L = 11, SF_ATT0 = 14, SF_SUM = 17, SF_KEY = 20,
       SF_MA = 21 /* RNG draw index, bounce | b_inner << 8 | flags */, SF_MB = 22 /* work unit */, SF_N = 24 };

// Control block of one (sub-)pool, 32-bit words: a header, then CTL_STRIDE words per shard s from CTL_SHARD0 on, so that the ST_SHARDS copies of
// a counter lie on separate cache lines; word w of shard s is ctl[CTL_SHARD0 + CTL_STRIDE * s + w].  The host keeps ST_MAX_POOLS such blocks and one
// more behind them for the work-unit counters, which the sub-pools share: that one has no header, shard s counts in uctl[CTL_STRIDE * s + CTL_SH_UNITS].
// (CTL_CAPPED, the header word the host reads after a trace: zr_launch.h.)
enum { CTL_COMPACT = 4,      // header: the drain's compaction counter (stream_compact); zero since the frame began
       CTL_INACTIVE = 5,     // header: WHILE IT IS 0, EVERY SLOT OF THE POOL HAS F_ACTIVE.  Zeroed with the block; whoever leaves a slot without the bit stores 1
                             // (stream_init, stream_shade, stream_compact_pad, stream_load_rays).  The lean EXTEND reads it once per wave: see its FETCH
       CTL_SHARD0 = 16, CTL_STRIDE = 32,
       CTL_SH_UNITS = 0,     // work units the shard has handed out dynamically (in the unit-counter block only)
       CTL_SH_CHUNK = 8,     // EXTEND's chunk cursor: chunks of ST_CHUNK slots reserved this round
       CTL_SH_ACTIVE = 16 }; // slots left active by the last SHADE

struct StreamBuf {
    double* pool;             // [P / 64][SF_N][64] 8-byte cells
    const uint32_t* pixels;   // [n_pix] px | py << 16
    double* samples;          // [n_pix][spp][3] radiance of every primary sample
    unsigned int* ctl;        // this pool's control block
    unsigned int* uctl;       // the unit-counter block, shared by the sub-pools
    uint32_t P, spp, n_units, n_pix;
    uint32_t unit0;           // slot k of this pool starts on unit unit0 + k
    uint32_t unit_base;       // first dynamically assigned unit (= slots of both pools)
    uint32_t unit_chunk;      // 0: units are striped over the shards (unit_base + k * ST_SHARDS + shard); G > 0: XCD-affine hand-out, see st_unit_of
    uint32_t shard_k0;        // affine hand-out: index in its shard's sequence of the first unit a shard deals dynamically (= slots per shard)
    uint32_t sample0;         // the run renders samples [sample0, sample0 + spp) of every pixel: unit u is sample sample0 + u % spp (0: a whole frame)
    uint2* kend;              // reflection / refraction split: per unit (draws, segments) the beauty path consumed
    unsigned char* cls;       // reflection / refraction split: per unit 1 = reflection, 2 = refraction, 0 = no contribution
    unsigned long long* cpart; // reflection / refraction split: per SHADE block (samples, segments, hits, draws), owned by that block
    __device__ __forceinline__ double* cell(int f, uint32_t slot) const { return pool + ((size_t)(slot >> 6) * SF_N + f) * 64 + (slot & 63u); }
    __device__ __forceinline__ double ld(int f, uint32_t slot) const { return *cell(f, slot); }
    __device__ __forceinline__ void st(int f, uint32_t slot, double v) const { *cell(f, slot) = v; }
    __device__ __forceinline__ uint2 ld2(int f, uint32_t slot) const { return *reinterpret_cast<const uint2*>(cell(f, slot)); }
    __device__ __forceinline__ void st2(int f, uint32_t slot, uint2 v) const { *reinterpret_cast<uint2*>(cell(f, slot)) = v; }
    __device__ __forceinline__ V3 ld3(int f, uint32_t slot) const { return mk(ld(f, slot), ld(f + 1, slot), ld(f + 2, slot)); }
    __device__ __forceinline__ void st3(int f, uint32_t slot, V3 v) const { st(f, slot, v.x); st(f + 1, slot, v.y); st(f + 2, slot, v.z); }
};

// A slot addressed RELATIVE TO ITS 256-SLOT BLOCK (round 4).  SHADE and INIT work on the slots of one block per workgroup, so `base` is the same in every
// thread (a scalar register pair), `off` a 32-bit byte offset below 48 KB and the field a constant: every row access becomes
// `global_load/store v, v_off, s[base] offset:imm` with ONE vector register of address for all 23 rows.  Through StreamBuf::cell() every row had a 64-bit
// address of its own, and the rows a segment reads and writes back kept theirs alive across the whole kernel (12+ registers, part of them spilled in the
// lean build): SHADE's speed follows its occupancy (profiles/r4_experiments_ab.txt), so registers are time.
struct SlotAt {
    const char* base; uint32_t off;
    __device__ __forceinline__ const char* at(int f) const { return base + (off + (uint32_t)f * 512u); }
    __device__ __forceinline__ double ld(int f) const { return *reinterpret_cast<const double*>(at(f)); }
    __device__ __forceinline__ void st(int f, double v) const { *reinterpret_cast<double*>(const_cast<char*>(at(f))) = v; }
    __device__ __forceinline__ uint2 ld2(int f) const { return *reinterpret_cast<const uint2*>(at(f)); }
    __device__ __forceinline__ void st2(int f, uint2 v) const { *reinterpret_cast<uint2*>(const_cast<char*>(at(f))) = v; }
    __device__ __forceinline__ V3 ld3(int f) const { return mk(ld(f), ld(f + 1), ld(f + 2)); }
    __device__ __forceinline__ void st3(int f, V3 v) const { st(f, v.x); st(f + 1, v.y); st(f + 2, v.z); }
};
// slot `block * 256 + src` (src < 256); `block` must be wave-uniform
__device__ __forceinline__ SlotAt slot_at(const StreamBuf& B, uint32_t block, uint32_t src) {
    SlotAt a;
    a.base = reinterpret_cast<const char*>(B.pool) + (size_t)block * (size_t)(4 * SF_N * 512);
    a.off = (src >> 6) * (uint32_t)(SF_N * 512) + (src & 63u) * 8u;
    return a;
}


// (which unit a slot starts on, and which a shard hands out next: st_first_unit and st_unit_of, zr_units.h)

// ---- begin a sample in a slot: camera ray + fresh path state --------------------------------------------
// sample `sample` of the pixel whose word (B.pixels) is `pk`
__device__ __forceinline__ void begin_sample_at(const DCamera& cam, uint64_t seed, const SlotAt& S, uint32_t unit, uint32_t sample, uint32_t pk, uint32_t& c_samp) {
    const int px = (int)(pk & 0xFFFFu), py = (int)(pk >> 16);
    Rng g; g.key = zr_stream_key(seed, (uint64_t)py * (uint64_t)cam.W + (uint64_t)px, (uint64_t)sample); g.k = 0; g.bounce = 0;
    Ray r = camera_ray(cam, px, py, g);
    S.st3(SF_RAY, r.o); S.st3(SF_RAY + 3, r.d);
    S.st(SF_KEY, __longlong_as_double((long long)g.key));
    uint2 ma; ma.x = (uint32_t)g.k; ma.y = F_FIRST | F_ACTIVE;
    uint2 mb; mb.x = unit; mb.y = 0;
    S.st2(SF_MA, ma); S.st2(SF_MB, mb);
    c_samp++;
}
__device__ inline void begin_sample(const StreamBuf& B, const DCamera& cam, uint64_t seed, const SlotAt& S, uint32_t unit, uint32_t& c_samp) {
    const uint32_t pix_i = unit / B.spp, sample = unit - pix_i * B.spp + B.sample0;
    const uint32_t pk = B.pixels[pix_i];
    begin_sample_at(cam, seed, S, unit, sample, pk, c_samp);
}
// ... with the unit's pixel word, B.pixels[unit / B.spp], loaded by the caller already (the lean SHADE requests it before its MISS stage)
__device__ inline void begin_sample(const StreamBuf& B, const DCamera& cam, uint64_t seed, const SlotAt& S, uint32_t unit, uint32_t pk, uint32_t& c_samp) {
    const uint32_t pix_i = unit / B.spp, sample = unit - pix_i * B.spp + B.sample0;
    begin_sample_at(cam, seed, S, unit, sample, pk, c_samp);
}

template <bool COUNT>
__global__ __launch_bounds__(256) void stream_init(StreamBuf B, DCamera cam, uint64_t seed, unsigned long long* __restrict__ gctr) {
    const uint32_t slot = blockIdx.x * 256 + threadIdx.x;
    if (slot >= B.P) return;
    uint32_t c_samp = 0;
    const unsigned long long u0 = st_first_unit(B.unit_chunk, B.unit0 + slot);
    const SlotAt S = slot_at(B, blockIdx.x, threadIdx.x);
    if (u0 < (unsigned long long)B.n_units) begin_sample(B, cam, seed, S, (uint32_t)u0, c_samp);
    else { uint2 z; z.x = 0; z.y = 0; S.st2(SF_MA, z); B.ctl[CTL_INACTIVE] = 1u; }
    if (COUNT && c_samp) atomicAdd(&gctr[CTR_SAMPLES], (unsigned long long)c_samp);
}

// ---- EXTEND: closest hit for every active slot ------------------------------------------------------------
// Walks the 4-wide tree (zr_device_types.h: FP32 root in the kernel arguments, 64-byte nodes with boxes on an 8-bit
// grid below it).  The kernel sits where VALU issue and the node / primitive fetches are in balance (rocprofv3:
// SQ_INSTS_VALU x 4 clocks / 1024 SIMDs ~ its duration — and yet 6.8 % fewer vector instructions per launch, round 3's
// node step, left the duration where it was, while 4 / 9 / 17 % MORE cost 2 / 10 / 15 %: profiles/r3_experiments_ab.txt;
// 128-byte FP32 nodes with fewer operations per visit were 15 % slower), so the slab test is arranged for few operations
// AND few bytes, and it is CONSERVATIVE: a superset of box hits cannot change the closest
// primitive, and every primitive test stays FP64.
//   per ray:   id = 1 / (float)d (float, taken as exact: it perturbs t by a relative 2^-23),  c = (float)(-o * id)
//   per plane: t = fmaf(P, id, c)                          (root: P is an FP32 plane)
//              t = fmaf(q, a, b), a = scale * id (exact, scale is a power of two), b = fmaf(origin, id, c)
//   error:     |t - (P - o) id| <= 2^-24 (|t| + |b| + |c|), and |b| <= |t| + 255 |a|
// The absolute part of that bound is folded, per axis, into the constants: the plane a ray ENTERS an axis' slab through
// (the lower one when id > 0) uses c_n = c - 2^-22 |c|, the one it leaves through c_f = c + 2^-22 |c| (and b_n, b_f move by a
// further 2^-15 |a|); a slack shared by the three axes would let an axis with a tiny d inflate the other two.  The
// relative part lowers the entry distance and raises the exit distance by |t| 2^-20.
// DOMAIN: every finite o, every d, a tree whose planes lie within M (the device builder accepts M <= 1e18, the host builder
// 1e30).  The bound above assumes every float intermediate is finite, and that is a property of the WORLD, not of the ray
// alone: a product P id, origin id or 255 a leaves the range once M |id| reaches 2^128, and then a plane that should be
// moderate is -inf (b = fmaf(origin, id, c) overflows, fmaf(q, a, -inf) stays there: the child is culled) or the entry
// distance is +inf and its slack makes it NaN (inf - inf: n <= f is false).  RULE: an axis is kept only while
//   |id| < 2^(115 - ilogb M), at most 2^100   (slab_id_limit, zr_device.h: from the root's planes; a placed run's own tree
//                                               from its root's grid),   id != 0   ((float)d = +-inf: every plane would be c = 0),
//   |c| < 2^120
// so that |P id| < 2^116, |origin id| < 2^116, 255 |a| < 2^119 (a grid's 255 steps span less than four times its children's
// extent of at most 2 M), |b| and |t| < 2^121: nothing leaves the float range, and no distance is infinite but tbest_f, for
// which inf <= inf is a hit.  Any other axis gets id = 0, c = NaN: its planes evaluate to NaN, which fminf / fmaxf ignore,
// i.e. the slab is dropped (conservative).  A world within 2^16 has the limit 2^100 it always had.
// Checked against exact rational arithmetic over the whole domain on the host, the very macros expanded there
// (tests/test_slab_native.py), and through both builders and this kernel (tests/test_slab_edges.py).
enum { X_IDLE = 0, X_NODE = 1, X_LEAF = 2 };
#define X_LEAF_BIT ZR_REF_LEAF

__device__ __forceinline__ void cswap(float& ta, uint32_t& ra, float& tb, uint32_t& rb) {
    const bool sw = tb < ta;
    const float t0 = sw ? tb : ta, t1 = sw ? ta : tb;
    const uint32_t r0 = sw ? rb : ra, r1 = sw ? ra : rb;
    ta = t0; tb = t1; ra = r0; rb = r1;
}

// LEVEL: which leaf kinds the build knows, chosen per scene at commit (zr_scene::leaf_level) so that a world pays only for
// the code — and the registers — of what it contains:
//   0  bare triangles and spheres (cfg2, cfg3)
//   1  + bare cubes, placed cubes (cube -> [rotate_y] -> translate) and media in an unwrapped sphere or cube (cfg5)
//   2  + objects under arbitrary wrapper chains and wrapped media (the op-list interpreter)
//   3  + placed runs of triangles (two-level BVH: zr_device.h instance_t; its private stack costs this build registers)
// Stack: ST_LDS_STACK entries per lane in LDS, deeper ones in this wave's slab of `overflow` (ovf_levels x 64 entries); the
// host sizes the slab from the exact worst-case demand of the committed tree (Flattener::stack_demand), so no push can
// leave it.
// ST_EXT_GROUP waves form a workgroup; they share nothing (own stack slice, ray chunks and state machine).  1 is the measured
// best: groups of 8 sharing an LDS copy of the tree's first three levels (84 nodes) were tried in round 2 — the copy's reads
// and the extra branch in the node step cost more than the requests they saved (cfg3 3.31 -> 3.60 ms per launch, cfg5 -3 %
// against +1 % for the grouping alone): profiles/r2_experiments_ab.txt.
#ifndef ST_EXT_GROUP
#define ST_EXT_GROUP 1
#endif
template <bool COUNT, int LEVEL>
__global__ __launch_bounds__(64 * ST_EXT_GROUP, LEVEL >= 2 ? ST_EXT_WAVES : (LEVEL == 1 ? ST_EXT_WAVES_MID : ST_EXT_WAVES_LEAN)) void stream_extend(DScene sc, StreamBuf B, SEntry* __restrict__ overflow,
                                                                  uint32_t ovf_levels, unsigned long long* __restrict__ gctr, float id_lim /* slab_id_limit(sc.root), zr_device.h */) {
    __shared__ SEntry lstack[ST_EXT_GROUP * ST_LDS_STACK * 64];
    const int lane = threadIdx.x & 63;
    const uint32_t wave_id = blockIdx.x * ST_EXT_GROUP + (threadIdx.x >> 6);
    const int lbase = (int)(threadIdx.x >> 6) * ST_LDS_STACK * 64 + lane;   // this lane's column of this wave's stack slice
    const unsigned long long lt_mask = (1ull << lane) - 1ull;
    SEntry* gstack = overflow + (size_t)wave_id * ovf_levels * 64 + lane;
    const double INF = __builtin_huge_val();
    const float INFf = __builtin_huge_valf();
    const uint32_t NONE = 0xFFFFFFFFu;

    int st = X_IDLE;
    uint32_t slot = 0;
    Ray ray; ray.o = mk(0, 0, 0); ray.d = mk(0, 0, 1);
    float idx_ = 0, idy_ = 0, idz_ = 0;
    float cnx = 0, cny = 0, cnz = 0, cfx = 0, cfy = 0, cfz = 0;  // per axis: c for the plane the ray ENTERS through and for the one it LEAVES through (slack folded in)
    double tbest = INF;
    float tbest_f = INFf;
    uint32_t kbest = NONE, ibest = 0;
    uint32_t inst_cur = 0;  // level 3: 0 = the lane walks the world's tree with the world ray; p + 1 = it is inside placement p, with the ray mapped into the run's space
    uint32_t cur = 0;       // X_NODE: quad index; X_LEAF: leaf reference (kind << 28 | (count - 1) << 24 | first)
    uint32_t pend_i = 0;
    int sp = 0;
    Rng g; g.key = 0; g.k = 0; g.bounce = 0;  // only the medium test reads it
    int work_left = 1;      // wave-uniform: some shard may still have chunks
    uint32_t chunk_next = 0, chunk_end = 0;  // wave-uniform: the private range of ray indices being handed out
    uint32_t head_shard = wave_id % ST_SHARDS, shards_tried = 0;
    if (wave_id == 0 && lane < ST_SHARDS) B.ctl[CTL_SHARD0 + CTL_STRIDE * lane + CTL_SH_ACTIVE] = 0;  // SHADE of this round recounts the active slots
    // LEVEL 0: is every slot of the pool active (CTL_INACTIVE)?  The value cannot change under this launch: what stores the word runs before it on the pool's stream.
    const bool all_active = LEVEL == 0 && __builtin_amdgcn_readfirstlane(B.ctl[CTL_INACTIVE]) == 0u;
    uint32_t c_nodes = 0, c_sph = 0, c_tri = 0, c_cube = 0, c_med = 0, c_seg = 0, c_hits = 0, c_fetch[2] = {0, 0};
    unsigned long long s_exec[2] = {0, 0}, s_lanes[2] = {0, 0};

    auto finish = [&]() {  // traversal of this lane's ray is complete: publish the result
        B.st(SF_HIT_T, slot, tbest);
        uint2 ki; ki.x = kbest; ki.y = ibest;
        B.st2(SF_HIT_KI, slot, ki);
        if (COUNT && kbest != NONE) c_hits++;
        st = X_IDLE;
    };
// stack helpers are macros, not lambdas: a lambda capturing the __shared__ array by reference turns its accesses into
// flat-pointer accesses (and trips an LLVM verifier error on gfx950)
#define ZR_LDS_LEVELS ST_LDS_STACK
#define ZR_PUSH(REF, TN)                                                                                        \
    {                                                                                                           \
        SEntry e_; e_.node = (REF); e_.tn = (TN);                                                               \
        if (sp < ZR_LDS_LEVELS) lstack[sp * 64 + lbase] = e_; else gstack[(size_t)(sp - ZR_LDS_LEVELS) * 64] = e_; \
        sp++;                                                                                                   \
    }
// nearest deferred entry that can still matter, else the ray is done
#define ZR_POP_NEXT()                                                                                           \
    for (;;) {                                                                                                  \
        if (sp == 0) { finish(); break; }                                                                       \
        sp--;                                                                                                   \
        SEntry e_;                                                                                              \
        if (sp < ZR_LDS_LEVELS) e_ = lstack[sp * 64 + lbase]; else e_ = gstack[(size_t)(sp - ZR_LDS_LEVELS) * 64]; \
        if (e_.tn <= tbest_f) { cur = e_.node; pend_i = 0; st = (e_.node & X_LEAF_BIT) ? X_LEAF : X_NODE; break; } \
    }

// (ZR_SLAB, ZR_RAY_CONSTANTS, ZR_FBOX, ZR_QNODE — the slab test itself: zr_device.h, shared with SHADE's escape stage and with the host check tests/native/slab_check.cpp)
// the four children by entry distance (5-comparator network): push far -> near, continue with the nearest
#define ZR_DESCEND()                                                                                        \
    {                                                                                                       \
        cswap(tn0, r0, tn1, r1); cswap(tn2, r2, tn3, r3); cswap(tn0, r0, tn2, r2); cswap(tn1, r1, tn3, r3); cswap(tn1, r1, tn2, r2); \
        if (tn3 < INFf) ZR_PUSH(r3, tn3)                                                                    \
        if (tn2 < INFf) ZR_PUSH(r2, tn2)                                                                    \
        if (tn1 < INFf) ZR_PUSH(r1, tn1)                                                                    \
        if (tn0 < INFf) { cur = r0; pend_i = 0; st = (r0 & X_LEAF_BIT) ? X_LEAF : X_NODE; }                 \
        else { ZR_POP_NEXT() }                                                                              \
    }

    const unsigned long long iter_cap = (unsigned long long)B.P * 64ull + (1ull << 24);
    unsigned long long iter = 0;
#ifdef ZR_WAVE_PROFILE
    const unsigned long long t_begin = wall_clock64();
    unsigned long long p_exec[3] = {0, 0, 0}, p_lanes[3] = {0, 0, 0};
    // per-phase lane histogram: iterations of NODE / LEAF / FETCH by the number of lanes the phase ran with, in eight buckets of eight lanes
    __shared__ unsigned int p_hist[ST_EXT_GROUP][24];
    if (lane < 24) p_hist[threadIdx.x >> 6][lane] = 0;
#endif
    for (; iter < iter_cap; iter++) {
        work_left = __builtin_amdgcn_readfirstlane(work_left);
        const uint32_t lkind = (cur >> 28) & 7u;
        // the lane counts and work_left are wave-uniform, and said to be (readfirstlane): the phase below is chosen by scalar compares and branches and the loop
        // is left by a scalar branch, where the popcounts used to go back into a VGPR and the loop ran under an exec mask (cfg3 frame -3.3 %)
        const int n1 = __builtin_amdgcn_readfirstlane(__popcll(__ballot(st == X_NODE)));
        const int n2t = __builtin_amdgcn_readfirstlane(__popcll(__ballot(st == X_LEAF && lkind == ZR_PRIM_TRIANGLE)));
        const int n2s = __builtin_amdgcn_readfirstlane(__popcll(__ballot(st == X_LEAF && lkind == ZR_PRIM_SPHERE)));
        const int n2g = LEVEL > 0 ? __builtin_amdgcn_readfirstlane(__popcll(__ballot(st == X_LEAF))) - n2t - n2s : 0;
        const int n0 = work_left ? __builtin_amdgcn_readfirstlane(__popcll(__ballot(st == X_IDLE))) : 0;
        const int n2 = n2t + n2s + n2g;
        if (n1 + n2 + n0 == 0) break;

        // one phase per iteration, as three separate wave-uniform ifs and not an if / else-if chain: at each join a state variable is (changed | as it was), never
        // undefined, so the loop-carried state (st, cur, pend_i, sp, tbest, tbest_f, kbest, ibest, slot) keeps its registers around the back-edge instead of being
        // copied to a second set and back.  A NODE iteration: 198 -> 167 vector instructions, 36 -> 7 of them v_mov; the lean build spills 4 registers instead
        // of 6.  The launch is 0.5 ms of 193 shorter for it, no more: profiles/r30_extend_loop_ab.txt
        const int phase = (n0 >= ST_FETCH_MIN || (n0 > 0 && n0 >= n1 && n0 >= n2)) ? X_IDLE : (n1 >= n2 ? X_NODE : X_LEAF);
        if (phase == X_IDLE) {
            // ================= FETCH: idle lanes take the next ray indices =================
            // rays are handed out from a wave-private chunk; one global atomic per ST_CHUNK rays
            const unsigned long long idle = __ballot(st == X_IDLE);
            uint32_t n = (uint32_t)__popcll(idle);
#ifdef ZR_WAVE_PROFILE
            p_exec[2]++; p_lanes[2] += n;
            if (lane == 0 && n > 0) p_hist[threadIdx.x >> 6][16 + ((n - 1) >> 3)]++;
#endif
            while (chunk_next >= chunk_end && work_left) {
                // reserve the next chunk of this wave's shard; an exhausted shard sends the wave to the next one
                uint32_t nb = 0;
                if (lane == 0) nb = atomicAdd(&B.ctl[CTL_SHARD0 + CTL_STRIDE * head_shard + CTL_SH_CHUNK], 1u);
                nb = __builtin_amdgcn_readfirstlane(nb);
                const unsigned long long first = ((unsigned long long)nb * ST_SHARDS + head_shard) * ST_CHUNK;
                if (first < (unsigned long long)B.P) {
                    chunk_next = (uint32_t)first;
                    chunk_end = first + ST_CHUNK < (unsigned long long)B.P ? (uint32_t)first + ST_CHUNK : B.P;
                } else {
                    head_shard = (head_shard + 1) % ST_SHARDS;
                    if (++shards_tried >= ST_SHARDS) work_left = 0;
                }
            }
            if (!work_left) n = 0;
            if (n > chunk_end - chunk_next) n = chunk_end - chunk_next;
            const uint32_t base = chunk_next;
            chunk_next += n;
            const uint32_t lim = base + n;
            if (st == X_IDLE) {
                const uint32_t my = base + (uint32_t)__popcll(idle & lt_mask);
                if (my < lim) {
                    // LEVEL > 0: meta word and ray requested together, one memory round trip per refill instead of two (an inactive
                    // slot's ray row is addressable like any other): cfg5 -1 %.  The lean build has no registers to hold the ray
                    // while the meta word is tested (2 more spilled, cfg3 +3 %): it asks for the ray once the slot is known active — and reads nothing else from the
                    // word, so while every slot of the pool is active (all_active: the rounds in which finished paths regenerate in place) it skips the word, its
                    // 8 bytes and its round trip, and asks for the ray at once.  A wave-uniform branch around the load, one copy of the body.
                    uint2 m; m.x = 0; m.y = F_ACTIVE;
                    if (LEVEL > 0 || !all_active) m = B.ld2(SF_MA, my);
                    if (COUNT && LEVEL == 0) c_fetch[all_active ? 1 : 0]++;
                    V3 ro_ = mk(0, 0, 0), rd_ = mk(0, 0, 0);
                    double key_ = 0;
                    if (LEVEL > 0) {
                        ro_ = B.ld3(SF_RAY, my); rd_ = B.ld3(SF_RAY + 3, my); key_ = B.ld(SF_KEY, my);
                        asm volatile("" ::"v"(ro_.x), "v"(rd_.z), "v"(key_));   // keeps the requests above the branch
                    }
                    if (m.y & F_ACTIVE) {
                        slot = my;
                        if (LEVEL > 0) { ray.o = ro_; ray.d = rd_; } else { ray.o = B.ld3(SF_RAY, my); ray.d = B.ld3(SF_RAY + 3, my); }
                        if (LEVEL > 0) { g.key = (uint64_t)__double_as_longlong(key_); g.bounce = m.y & 0xFFu; }
                        ZR_RAY_CONSTANTS(id_lim)
                        tbest = INF; tbest_f = INFf; kbest = NONE; cur = 0; sp = 0; pend_i = 0; inst_cur = 0;
                        if (COUNT) c_seg++;
                        // the root's FP32 boxes come with the kernel arguments: no memory access for the first step, and a
                        // ray that misses the whole world is finished right here
                        float tn0, tn1, tn2, tn3;
                        uint32_t r0, r1, r2, r3;
                        ZR_FBOX(sc.root, 0, tn0, r0)
                        ZR_FBOX(sc.root, 1, tn1, r1)
                        ZR_FBOX(sc.root, 2, tn2, r2)
                        ZR_FBOX(sc.root, 3, tn3, r3)
                        ZR_DESCEND()
                    }
                }
            }
        }
        if (phase == X_NODE) {
            // ================= NODE: one 4-wide node per lane =================
            if (COUNT) { s_exec[0]++; s_lanes[0] += n1; }
#ifdef ZR_WAVE_PROFILE
            p_exec[0]++; p_lanes[0] += n1;
            if (lane == 0 && n1 > 0) p_hist[threadIdx.x >> 6][(n1 - 1) >> 3]++;
#endif
            if (st == X_NODE) {
                float tn0, tn1, tn2, tn3;
                uint32_t r0, r1, r2, r3;
                const uint4* nq = reinterpret_cast<const uint4*>(sc.quads + cur);
                const uint4 w0 = nq[0], w1 = nq[1], w2 = nq[2], ref = nq[3];
                ZR_QNODE(w0, w1, w2, ref)   // zr_device.h: the planes on the node's grid, then the four children
                ZR_DESCEND()
            }
        }
        if (phase == X_LEAF) {
            // ================= LEAF: one primitive per lane, every kind that has waiting lanes =================
            // kind by kind, each under a wave-uniform guard: the few lanes at a minority kind (cfg3: the ground sphere every ray meets) do not
            // sit out NODE iterations waiting for company.  Against serving only the kind with most lanes, and with NODE and LEAF lanes
            // weighed 1:1 above: cfg3 EXTEND 213.1 -> 204.6 ms per frame, image bit-identical (profiles/r3_experiments_ab.txt)
            if (COUNT) { s_exec[1]++; s_lanes[1] += n2; }
#ifdef ZR_WAVE_PROFILE
            p_exec[1]++; p_lanes[1] += n2;
            if (lane == 0 && n2 > 0) p_hist[threadIdx.x >> 6][8 + ((n2 - 1) >> 3)]++;
#endif
            const bool is_leaf = st == X_LEAF;
            const bool do_tri = n2t > 0;
            const bool do_sph = n2s > 0;
            const uint32_t prim = (cur & 0xFFFFFFu) + pend_i;
            bool tested = false;
            if (do_tri) {
                if (is_leaf && lkind == ZR_PRIM_TRIANGLE) {
                    double t;
                    if (COUNT) c_tri++;
                    if (triangle_t(sc.tri_v + (size_t)prim * ZR_TRI_STRIDE, ray, 0.001, tbest, t)) {
                        tbest = t; tbest_f = __double2float_ru(t); ibest = prim;
                        kbest = (LEVEL == 3 && inst_cur) ? (ZR_KIND_INSTANCE | ((inst_cur - 1u) << 8)) : lkind;   // a triangle of a placed run: kind word = placement
                    }
                    tested = true;
                }
            }
            if (do_sph) {
                if (is_leaf && lkind == ZR_PRIM_SPHERE) {
                    double t;
                    if (COUNT) c_sph++;
                    if (sphere_t(sc.spheres + (size_t)prim * 4, ray, 0.001, tbest, t)) { tbest = t; tbest_f = __double2float_ru(t); kbest = lkind; ibest = prim; }
                    tested = true;
                }
            }
            if (LEVEL > 0 && is_leaf && lkind != ZR_PRIM_TRIANGLE && lkind != ZR_PRIM_SPHERE) {
                double t;
                if (COUNT && lkind < ZR_KIND_INSTANCE) {
                    uint32_t kk = lkind;
                    if (kk == ZR_KIND_WRAPPED) kk = sc.wrapped[prim].type;
                    if (kk == ZR_PRIM_SPHERE) c_sph++; else if (kk == ZR_PRIM_TRIANGLE) c_tri++; else if (kk == ZR_PRIM_CUBE || kk == ZR_KIND_PCUBE) c_cube++; else c_med++;
                }
                bool h;
                if (LEVEL == 3 && lkind == ZR_KIND_INSTANCE) {
                    // ENTER a placed run of triangles (two-level BVH): a sentinel stays on the stack where the world's walk goes on, the
                    // ray is mapped through the placement's wrappers (t is the same in both spaces: the reference's wrappers do not
                    // renormalise the direction) and the lane continues in the run's own 4-wide tree — same loop, same stack
                    const DInstance in = sc.insts[prim];
                    ZR_PUSH(ZR_REF_LEAF | (7u << 28), -INFf)
                    ray = chain_ray(sc, in.chain_first, in.chain_count, ray);
                    ZR_RAY_CONSTANTS(slab_id_limit(sc.quads[in.pad_]))   // the run's own tree, in the run's space: the limit of its root's grid
                    inst_cur = prim + 1u;
                    cur = in.pad_; pend_i = 0; st = X_NODE;
                } else if (LEVEL == 3 && lkind == 7u) {
                    // LEAVE: the run's tree is exhausted (its entries were above the sentinel); the world ray again, from the slot
                    ray.o = B.ld3(SF_RAY, slot); ray.d = B.ld3(SF_RAY + 3, slot);
                    ZR_RAY_CONSTANTS(id_lim)
                    inst_cur = 0;
                    ZR_POP_NEXT()
                } else {
                if (LEVEL == 1) {   // cubes, placed cubes, plain media: no op-list interpreter in this build
                    if (lkind == ZR_KIND_PCUBE) h = pcube_t(sc.pcubes + (size_t)prim * ZR_PCUBE_STRIDE, ray, 0.001, tbest, t);
                    else if (lkind == ZR_PRIM_CUBE) h = cube_t(sc.cubes + (size_t)prim * 6, ray, 0.001, tbest, t);
                    else h = medium_plain_t(sc, prim, ray, 0.001, tbest, g, t);
                } else h = object_t(sc, lkind, prim, ray, 0.001, tbest, g, t);
                if (h) { tbest = t; tbest_f = __double2float_ru(t); kbest = lkind; ibest = prim; }
                tested = true;
                }
            }
            if (tested) {
                pend_i++;
                if (pend_i > ((cur >> 24) & 0xFu)) { ZR_POP_NEXT() }
            }
        }
    }
    if (iter >= iter_cap && lane == 0) atomicAdd(&B.ctl[CTL_CAPPED], 1u);
#ifdef ZR_WAVE_PROFILE
    if (!COUNT && lane == 0) {  // development build: wave lifetime (10 ns ticks) and phase statistics into the raw counter words
        atomicAdd(&gctr[CTR_PROF_WAVE_TICKS], wall_clock64() - t_begin); atomicAdd(&gctr[CTR_PROF_WAVES], 1ull);
        for (int k = 0; k < 3; k++) { atomicAdd(&gctr[CTR_PROF_EXECS + 2 * k], p_exec[k]); atomicAdd(&gctr[CTR_PROF_LANES + 2 * k], p_lanes[k]); }
        for (int k = 0; k < CTR_HIST_WORDS; k++) if (p_hist[threadIdx.x >> 6][k]) atomicAdd(&gctr[CTR_HIST + k], (unsigned long long)p_hist[threadIdx.x >> 6][k]);
    }
#endif
    if (COUNT) {
        atomicAdd(&gctr[CTR_SEGMENTS], (unsigned long long)c_seg);
        atomicAdd(&gctr[CTR_NODES], (unsigned long long)c_nodes);
        atomicAdd(&gctr[CTR_SPHERES], (unsigned long long)c_sph);
        atomicAdd(&gctr[CTR_TRIANGLES], (unsigned long long)c_tri);
        atomicAdd(&gctr[CTR_CUBES], (unsigned long long)c_cube);
        atomicAdd(&gctr[CTR_MEDIA], (unsigned long long)c_med);
        atomicAdd(&gctr[CTR_HITS], (unsigned long long)c_hits);
        if (LEVEL == 0) { atomicAdd(&gctr[CTR_FETCH_CHECKED], (unsigned long long)c_fetch[0]); atomicAdd(&gctr[CTR_FETCH_SKIPPED], (unsigned long long)c_fetch[1]); }
        if (lane == 0) for (int k = 0; k < 2; k++) { atomicAdd(&gctr[CTR_NODE_EXECS + 2 * k], s_exec[k]); atomicAdd(&gctr[CTR_NODE_LANES + 2 * k], s_lanes[k]); }   // k = 1: CTR_LEAF_*
    }
}

// ---- SHADE: one segment of every active slot ------------------------------------------------------------------
// MODE 0: the render.  MODE 1 / 2: the two passes of the reflection / refraction split (camera.hpp:490-517) on the same pipeline:
// 1 = the beauty pass, which also records per unit how many draws and segments its path consumed; 2 = the replay: the camera
// ray is traced again, at its first hit the sample's stream is positioned after the beauty path (so the SECOND scatter of that
// hit gets the draws the reference gives it), the scattered path runs as ray_color(scattered, max_depth - 1), and its
// luma-clamped radiance times the attenuation is written with its class.
#ifndef ST_SHADE_WAVES_LEAN
#define ST_SHADE_WAVES_LEAN 6
#endif
// UV: the general build for scenes whose triangles carry texture coordinates (zr_device.h: triangle_rec_uv); the lean build reads none
// SORT = false: the IN-PLACE build of the lean render (round 28).  A thread shades the slot it indexes: no partition, no LDS, no barrier, and the segment's
// first batch of rows is requested together with the meta word instead of one round trip behind it.  For a world with ONE material kind the sort only
// separates hits from misses, and since the escape stage and the sky pre-pass most hit waves run the MISS stage anyway while the misses EXTEND finds are too
// few to fill a wave of their own: what is left of the sort is its cost, which sits on the kernel's chain of dependent round trips.
// Its next work units are reserved, and their pixel words requested, before the MISS stage (RESERVE_EARLY below).  The host takes this build while work units
// are left (stream_render); once the pool thins out the sorted build packs the survivors into full waves.
template <bool COUNT, int MODE, bool LEAN = false, bool UV = false, bool SORT = true>
__global__ __launch_bounds__(SORT ? 256 : 64, LEAN ? ST_SHADE_WAVES_LEAN : ST_SHADE_WAVES) void stream_shade(DScene sc, DCamera cam, DEnv env, uint64_t seed, StreamBuf B,
                                                    unsigned long long* __restrict__ gctr) {
    // the block of 256 slots this workgroup works on, and its thread's place in it.  The in-place build's waves share nothing, so its workgroup is ONE wave, a
    // quarter of a slot block: a finished wave's registers free without waiting for three siblings (cfg3: 1.5-2 ms of a frame against 256-thread groups, in
    // ten of ten A/B cycles: profiles/r28_shade_in_place_ab.txt).  The slot block, its shard and the control-word reset are what they are in the sorted build.
    constexpr bool QUARTER = !SORT;
    const uint32_t sblock = QUARTER ? blockIdx.x >> 2 : blockIdx.x, sthread = QUARTER ? (blockIdx.x & 3u) * 64u + threadIdx.x : threadIdx.x;
    const uint32_t slot0 = sblock * 256 + sthread;
    if (slot0 < ST_SHARDS) B.ctl[CTL_SHARD0 + CTL_STRIDE * slot0 + CTL_SH_CHUNK] = 0;  // EXTEND of the next round starts from chunk 0 of every shard
    // the split passes count through LDS into a per-block record (a global atomic per thread costs ~1.5 ms per round and word)
    __shared__ unsigned long long s_cnt[4];
    if (MODE != 0 && threadIdx.x < 4) s_cnt[threadIdx.x] = 0;   // ordered before its use by the partition's barriers
    // In-block MATERIAL SORT: the 256 slots of this block are re-dealt to its threads by what their segment will execute —
    // class 0..4 = the hit's material kind (lambertian, metal, dielectric, light, isotropic: material.hpp:58-279,
    // constant_medium.hpp:14-18), 5 = a hit without a valid material, 6 = miss (background), 7 = inactive slot — so that a
    // wave runs one scatter routine (and one rejection sampler) under a full exec mask instead of five under sparse ones;
    // unsorted, almost every wave of a mixed scene runs every branch.  A counting sort through LDS: per-wave ballots per class,
    // a 4 x 8 table of counts, ranks by prefix popcount.  The material lookup it needs (primitive -> material id -> kind) is
    // the first access of the lines the hit record reads anyway; a scene with a single material kind skips it (hit / miss only).
    // The whole kernel is a chain of dependent memory round trips (73 % of its wave cycles sit in s_waitcnt, SQ counters of
    // round 2), so the rows a segment needs are requested as early and as much at once as their addresses are known:
    // the slot's meta word and its hit together; the sort hands both through LDS to the thread that will shade the slot (no
    // second read); that thread requests every state row of the segment in one go.
    __shared__ unsigned int wave_cls[4][8];
    __shared__ uint4 x_mk[256];          // (meta.x, meta.y, hit kind, hit index) of the slot a thread will shade
    __shared__ unsigned char x_src[256]; // ... and which slot of the block that is
    uint32_t src;   // which slot of the block this thread shades
    uint2 m, ki;
    // the in-place build's first batch: every row a segment reads whose address does not depend on the meta word
    Ray ray_in; double key_in, t_in; uint2 mb_in;
    if constexpr (!SORT) {
        static_assert(LEAN && MODE == 0, "the in-place build exists for the lean render only");
        src = sthread;
        m.x = 0; m.y = 0; ki.x = 0xFFFFFFFFu; ki.y = 0;
        if (slot0 < B.P) {   // (a slot is addressable whether or not it is active; a thread beyond the pool keeps meta = 0)
            const SlotAt S0 = slot_at(B, sblock, sthread);
            m = S0.ld2(SF_MA); ki = S0.ld2(SF_HIT_KI); t_in = S0.ld(SF_HIT_T);
            ray_in.o = S0.ld3(SF_RAY); ray_in.d = S0.ld3(SF_RAY + 3);
            key_in = S0.ld(SF_KEY); mb_in = S0.ld2(SF_MB);
        }
    } else {
        uint2 m0; m0.x = 0; m0.y = 0;
        uint2 k0; k0.x = 0xFFFFFFFFu; k0.y = 0;
        if (slot0 < B.P) { const SlotAt S0 = slot_at(B, blockIdx.x, threadIdx.x); m0 = S0.ld2(SF_MA); k0 = S0.ld2(SF_HIT_KI); }
        uint32_t cls = 7;
        if (m0.y & F_ACTIVE) {
            if (k0.x == 0xFFFFFFFFu) cls = 6;
            else {
                cls = 0;
                if (sc.mat_kinds & (sc.mat_kinds - 1u)) {   // more than one material kind in the scene (wave-uniform)
                    const uint32_t mat = object_material(sc, k0.x, k0.y);
                    cls = mat < sc.n_mats ? sc.mats[mat].kind : 5u;
                    if (cls > 5u) cls = 5u;
                }
            }
        }
        const int w = threadIdx.x >> 6, wl = threadIdx.x & 63;
        const unsigned long long below = (1ull << wl) - 1ull;
        unsigned int my_rank = 0;
#pragma unroll
        for (uint32_t c = 0; c < 8; c++) {
            const unsigned long long bm = __ballot(cls == c);
            if (wl == 0) wave_cls[w][c] = (unsigned int)__popcll(bm);
            if (cls == c) my_rank = (unsigned int)__popcll(bm & below);
        }
        __syncthreads();
        unsigned int base = 0;   // slots of lower classes in any wave + slots of this class in earlier waves
        for (uint32_t c = 0; c < 8; c++)
            for (int k = 0; k < 4; k++)
                if (c < cls || (c == cls && k < w)) base += wave_cls[k][c];
        uint4 mk4; mk4.x = m0.x; mk4.y = m0.y; mk4.z = k0.x; mk4.w = k0.y;
        x_mk[base + my_rank] = mk4;
        x_src[base + my_rank] = (unsigned char)threadIdx.x;
        __syncthreads();
        mk4 = x_mk[threadIdx.x];
        src = x_src[threadIdx.x];
        m.x = mk4.x; m.y = mk4.y; ki.x = mk4.z; ki.y = mk4.w;
    }
    const SlotAt S = slot_at(B, sblock, src);
    bool active_after = false, want_unit = false;
    uint32_t c_samp = 0, c_seg2 = 0, c_hit2 = 0, c_esc = 0, c_esc_nodes = 0, c_seen = 0; unsigned long long c_draws = 0;
    // The in-place build reserves a lane's next work unit BEFORE its MISS stage (below): the unit (ST_NO_UNIT: none was reserved, or it lies beyond the frame) and its
    // pixel word.  Not the sorted lean build: with the two values held across the stages (or the unit alone) it went from 6 scratch operations outside the stages to 32
    // inside them (scripts/dev/kernel_regs.sh, profiles/r28_shade_in_place_ab.txt), so it hands out units behind MISS as it always has.
    constexpr uint32_t ST_NO_UNIT = 0xFFFFFFFFu;   // no unit has this number: ST_MAX_UNITS (zr_launch.h)
    constexpr bool RESERVE_EARLY = LEAN && MODE == 0 && !SORT;
    uint32_t next_unit = ST_NO_UNIT, next_pk = 0;
#ifdef ZR_SHADE_ASSERT
    bool reserved = false;
#endif
    {
        if (m.y & F_ACTIVE) {   // (a thread beyond the pool got meta = 0 from the prologue)
            const uint32_t NONE = 0xFFFFFFFFu;
            const bool first = (m.y & F_FIRST) != 0;
            if (COUNT && LEAN && MODE == 0) c_seen++;   // a segment EXTEND traced: CTR_SEGMENTS - CTR_ESCAPED, counted from this side
            // every row this segment reads, requested in one go (a row of a slot is always addressable; what a path does not
            // need is not requested: beta before the second hit, the unit id is 8 bytes)
            Ray ray;
            if constexpr (SORT) { ray.o = S.ld3(SF_RAY); ray.d = S.ld3(SF_RAY + 3); } else ray = ray_in;
            Rng g; g.key = (uint64_t)__double_as_longlong(SORT ? S.ld(SF_KEY) : key_in); g.k = m.x; g.bounce = (m.y & 0xFFu) + 1u;  // this query is complete
            const uint2 mb_now = SORT ? S.ld2(SF_MB) : mb_in;
            const double t_hit = SORT ? S.ld(SF_HIT_T) : t_in;
            // after the first hit L = 0 and beta = 1 (camera.hpp:930): both stay implicit (two flag bits) until something else is
            // stored, which saves their 48 bytes written and read back per path; the values used are the same (0 + x, 1 * x)
            V3 beta_now = mk(1, 1, 1);
            if (!first && !(m.y & F_BONE)) beta_now = S.ld3(SF_BETA);
            V3 att0_now = mk(0, 0, 0);
            if (!first && ki.x == NONE) att0_now = S.ld3(SF_ATT0);   // a miss ends the path: its sample is att0 * (L + beta * background)
            int b_inner = (int)((m.y >> 8) & 0xFFu);
            const int depth_inner = cam.max_depth - 1;
            V3 L_now = mk(0, 0, 0);
            bool have_L_now = false;    // L_now holds L (an escaped path whose L is in registers); otherwise L is what the slot says
            auto load_L = [&]() { return have_L_now ? L_now : ((m.y & F_LZERO) ? mk(0, 0, 0) : S.ld3(SF_L)); };
            auto load_beta = [&]() { return beta_now; };
            uint32_t keep_lzero = m.y & F_LZERO;
            // the split passes count segments and hits here (SHADE sees every segment exactly once), so that their EXTEND can be
            // the uninstrumented build; the replay's first segment is the beauty pass's, found again: not counted
            if (COUNT && MODE != 0 && !(MODE == 2 && first)) { c_seg2++; if (ki.x != 0xFFFFFFFFu) c_hit2++; }
            // L, att0 and the slot's running sum are read only on the paths that need them
            bool ended = false;
            V3 contrib = mk(0, 0, 0);   // added to the slot sum when the path ends
            V3 add_now = mk(0, 0, 0);   // emission of a primary hit: added to the slot sum immediately
            bool has_add = false;
            bool no_output = false;     // MODE 2: the sample contributes nothing to the split frames
            // Two stages.  HIT: emission, scatter, depth and roulette; the path ends here or goes on with the ray `nr`.  MISS: the environment seen along
            // `ray` ends the path.  A slot whose ray found nothing enters MISS directly.  In the lean render a path that goes on enters it in the SAME
            // round when its new ray provably leaves the world (ray_escapes, zr_device.h: only certain misses, by EXTEND's own box arithmetic): the
            // ray and the state rows are not stored, MISS gets from registers exactly the values the slot would have handed it one round later —
            // att0, beta, L, the draw count, the primary hit's emission — and the slot starts its next sample a round earlier.  No hit is ever
            // resolved here, and a regenerated camera ray always goes to EXTEND.
            bool miss_first = first;    // MISS: `ray` is the camera ray (its sample is the background itself)
            bool escaped = false;
// MISS as a macro, not a lambda: through a lambda the general builds came out with other registers and, in two of them, with spills
#define ZR_MISS_STAGE()                                                                                                                    \
            {                                                                                                                              \
                if (MODE == 2 && first) { ended = true; no_output = true; }   /* the primary ray saw the background only (camera.hpp:518-526) */ \
                else {                                                                                                                     \
                    V3 bg = background(sc, env, ray.d);                                                                                    \
                    if (MODE == 2) {                                                                                                       \
                        V3 scol = load_L() + load_beta() * bg;                                                                             \
                        const double luma = 0.2126 * len(scol);                  /* camera.hpp:499-503 */                                  \
                        if (luma > 2.0) scol = scol * (2.0 / luma);                                                                        \
                        contrib = att0_now * scol;                                                                                         \
                    } else {                                                                                                               \
                        contrib = miss_first ? bg : att0_now * (load_L() + load_beta() * bg);  /* camera.hpp:520 / 941,1000 */             \
                    }                                                                                                                      \
                    ended = true;                                                                                                          \
                }                                                                                                                          \
            }
            // every build compiles exactly one of the two calls: the builds without the escape stage keep the miss ahead of the hit, as their code has
            // always been laid out (their registers and instructions are what they were); the lean render runs it behind the hit stage
            constexpr bool ESC = LEAN && MODE == 0;
            if (!ESC && ki.x == NONE) ZR_MISS_STAGE()
            else if (ki.x != NONE) {
                const double t = t_hit;
                V3 em, att; Ray nr; bool sc_ok;
                uint32_t cls_now = 0;
                if (LEAN) {
                    RecL rec;
                    lean_rec(sc, ki.x, ki.y, ray, t, rec);
                    sc_ok = lean_shade(sc, ray, rec, em, att, nr, g);
                } else {
                    Rec rec;
                    object_rec<true, UV>(sc, ki.x, ki.y, ray, t, rec);
                    em = emitted(sc, rec);
                    if (MODE == 2 && first) {   // the stream continues where the beauty path of this sample stopped
                        const uint2 ke = B.kend[mb_now.x];
                        g.k = ke.x; g.bounce = ke.y;
                    }
                    sc_ok = scatter(sc, ray, rec, att, nr, g);
                    if (MODE == 2 && first && sc_ok) {   // camera.hpp:506-516
                        const V3 reflected_dir = reflect(unit(ray.d), unit(rec.n));
                        if (dot(unit(nr.d), reflected_dir) > 0.9) cls_now = 1;
                        else if (dot(nr.d, rec.n) < 0) cls_now = 2;
                    }
                }
                const bool has_em = em.x != 0.0 || em.y != 0.0 || em.z != 0.0;
                // decided before any state is stored; it takes effect only if the path does go on (depth, roulette)
                uint32_t esc_nodes = 0;
                const bool esc = ESC && sc_ok && sc.shade_escape && ray_escapes(nr, sc.root, sc.spheres, esc_nodes);
                if (first) {  // ray_color_from_hit, camera.hpp:989-1004
                    if (MODE != 2 && has_em) { add_now = em; has_add = true; }
                    if (!sc_ok || depth_inner <= 0) { ended = true; if (MODE == 2) no_output = true; }
                    else {
                        if (esc) { att0_now = att; have_L_now = true; }   // MISS gets att0 = att, L = 0 (L_now), beta = 1 (beta_now)
                        else S.st3(SF_ATT0, att);   // L = 0, beta = 1: implicit (F_LZERO | F_BONE below)
                        if (MODE == 2) { uint2 mb = mb_now; mb.y = cls_now; S.st2(SF_MB, mb); }
                        b_inner = 0;
                    }
                } else {      // body of ray_color's loop, camera.hpp:944-983
                    V3 beta = load_beta();
                    V3 L = mk(0, 0, 0);
                    bool have_L = false;
                    if (has_em) { L = load_L() + beta * em; have_L = true; }
                    bool stop = !sc_ok;
                    if (!stop) {
                        beta = beta * att;
                        if (b_inner > 10) {
                            if (len(beta) < 0.0001) stop = true;
                            else {
                                double p = fmax(fmax(beta.x, beta.y), beta.z);
                                p = clampd(p, 0.05, 0.95);
                                if (g.next() > p) stop = true; else beta = beta * (1 / p);
                            }
                        }
                    }
                    if (!stop) { b_inner++; if (b_inner >= depth_inner) stop = true; }
                    if (stop) {
                        if (!have_L) L = load_L();
                        if (MODE == 2) { const double luma = 0.2126 * len(L); if (luma > 2.0) L = L * (2.0 / luma); }
                        contrib = S.ld3(SF_ATT0) * L; ended = true;
                    } else if (esc) {   // MISS gets what the slot would have carried: att0 as stored, the new beta, the new L if there is one
                        att0_now = S.ld3(SF_ATT0); beta_now = beta;
                        if (have_L) { L_now = L; have_L_now = true; }
                    } else {
                        if (have_L) { S.st3(SF_L, L); keep_lzero = 0; }
                        S.st3(SF_BETA, beta);
                    }
                }
                if (!ended && esc) {
                    // the path continues and its ray leaves the world: nothing is published, MISS ends the path along the new ray
                    escaped = true; miss_first = false;
                    ray = nr;
                    if (COUNT) { c_esc++; c_esc_nodes += esc_nodes; }
                } else if (!ended) {
                    // the path continues: publish the scattered ray (a primary hit's emission waits in SF_SUM)
                    S.st3(SF_RAY, nr.o); S.st3(SF_RAY + 3, nr.d);
                    if (has_add) S.st3(SF_SUM, add_now);
                    m.x = (uint32_t)g.k;
                    m.y = (g.bounce & 0xFFu) | ((uint32_t)b_inner << 8) | F_ACTIVE | (first ? (has_add ? F_L0 : 0u) : (m.y & F_L0)) |
                          (first ? (F_LZERO | F_BONE) : keep_lzero);
                    S.st2(SF_MA, m);
                    active_after = true;
                }
            }
            if constexpr (RESERVE_EARLY) {
                // Which lanes will want a work unit is known here: in the lean render MISS always ends its path, so this is the exact set of lanes that reach
                // `ended` below.  The wave's one atomic on its block's shard and the pixel word of each lane's next unit are requested now, so that both round
                // trips run beside the background's texel fetch and arithmetic instead of behind them.  Units reserved == lanes that end, launch for launch.
                const bool will_end = ended || ki.x == NONE || escaped;
                const unsigned long long wm = __ballot(will_end);
                if (wm != 0ull) {
                    const uint32_t shard = sblock % ST_SHARDS;
                    const int wl = threadIdx.x & 63, first_lane = (int)__builtin_ctzll(wm);
                    uint32_t k0 = 0;
                    if (wl == first_lane) k0 = atomicAdd(&B.uctl[CTL_STRIDE * shard + CTL_SH_UNITS], (unsigned int)__popcll(wm));
                    k0 = __shfl(k0, first_lane, 64);
                    if (will_end) {
                        const unsigned long long k = (unsigned long long)k0 + (unsigned long long)__popcll(wm & ((1ull << wl) - 1ull));
                        const unsigned long long u = st_unit_of(B.unit_chunk, B.unit_base, shard, (unsigned long long)B.shard_k0 + k);
                        if (u < (unsigned long long)B.n_units) { next_unit = (uint32_t)u; next_pk = B.pixels[next_unit / B.spp]; }
                    }
                }
#ifdef ZR_SHADE_ASSERT
                reserved = will_end;
#endif
            }
            if (ESC && (ki.x == NONE || escaped)) ZR_MISS_STAGE()
#undef ZR_MISS_STAGE
            if (ended) {
                // radiance of this sample = L0 + att0 * L (camera.hpp:1000), written exactly once
                V3 rad = contrib;
                if (has_add) rad = add_now + rad;
                else if (MODE != 2 && !first && (m.y & F_L0)) rad = S.ld3(SF_SUM) + rad;
                const uint2 mb = mb_now;
                const uint32_t unit = mb.x;
                if (MODE != 2 || !no_output) {
                    double* pp = B.samples + (size_t)unit * 3;
                    pp[0] = rad.x; pp[1] = rad.y; pp[2] = rad.z;
                }
                if (MODE == 1) { uint2 ke; ke.x = (uint32_t)g.k; ke.y = g.bounce; B.kend[unit] = ke; }
                if (MODE == 2 && !no_output) B.cls[unit] = (unsigned char)mb.y;
                if (COUNT) {
                    if (MODE != 2) c_draws += g.k;
                    else if (!(first && ki.x == NONE)) c_draws += g.k - B.kend[unit].x;   // draws of the second path only
                }
                want_unit = true;
            }
        }
    }
    if constexpr (RESERVE_EARLY) {
        // the in-place build reserved the units ahead of its MISS stage: the sample starts from registers
#ifdef ZR_SHADE_ASSERT
        assert(want_unit == reserved);   // units reserved == lanes that ended (a -DZR_SHADE_ASSERT build only)
#endif
        if (want_unit) {
            if (next_unit != ST_NO_UNIT) { begin_sample(B, cam, seed, S, next_unit, next_pk, c_samp); active_after = true; }
            else { uint2 z; z.x = 0; z.y = 0; S.st2(SF_MA, z); B.ctl[CTL_INACTIVE] = 1u; }
        }
    } else {
        // hand out new work units: one atomic per wave on this block's shard
        const unsigned long long wm = __ballot(want_unit);
        if (wm != 0ull) {
            const uint32_t shard = sblock % ST_SHARDS;
            const int wl = threadIdx.x & 63;
            uint32_t k0 = 0;
            if (wl == (int)__builtin_ctzll(wm)) k0 = atomicAdd(&B.uctl[CTL_STRIDE * shard + CTL_SH_UNITS], (unsigned int)__popcll(wm));
            k0 = __shfl(k0, (int)__builtin_ctzll(wm), 64);
            if (want_unit) {
                const unsigned long long k = (unsigned long long)k0 + (unsigned long long)__popcll(wm & ((1ull << wl) - 1ull));
                const unsigned long long u = st_unit_of(B.unit_chunk, B.unit_base, shard, (unsigned long long)B.shard_k0 + k);
                if (u < (unsigned long long)B.n_units) { begin_sample(B, cam, seed, S, (uint32_t)u, c_samp); active_after = true; }
                else { uint2 z; z.x = 0; z.y = 0; S.st2(SF_MA, z); B.ctl[CTL_INACTIVE] = 1u; }
            }
        }
    }
    // active-slot count for the host's round loop: sharded like the other counters — one contended word would cost
    // ~3 ms per 16 M-slot round (262 144 wave atomics at ~90 per microsecond)
    const unsigned long long am = __ballot(active_after);
    if ((threadIdx.x & 63) == 0 && am != 0ull) atomicAdd(&B.ctl[CTL_SHARD0 + CTL_STRIDE * (sblock % ST_SHARDS) + CTL_SH_ACTIVE], (unsigned int)__popcll(am));
    if (COUNT && MODE == 0) {
        if (c_samp) atomicAdd(&gctr[CTR_SAMPLES], (unsigned long long)c_samp);
        if (c_draws) atomicAdd(&gctr[CTR_DRAWS], c_draws);
        if (c_seen) atomicAdd(&gctr[CTR_SHADE_LANES], (unsigned long long)c_seen);
        if (c_esc) {   // a segment finished here is a segment all the same, and its root boxes were tested (EXTEND would have counted both)
            atomicAdd(&gctr[CTR_SEGMENTS], (unsigned long long)c_esc); atomicAdd(&gctr[CTR_ESCAPED], (unsigned long long)c_esc);
            atomicAdd(&gctr[CTR_NODES], (unsigned long long)c_esc_nodes);
        }
    }
    if (MODE != 0) {
        if (c_samp) atomicAdd(&s_cnt[0], (unsigned long long)c_samp);
        if (c_seg2) atomicAdd(&s_cnt[1], (unsigned long long)c_seg2);
        if (c_hit2) atomicAdd(&s_cnt[2], (unsigned long long)c_hit2);
        if (c_draws) atomicAdd(&s_cnt[3], c_draws);
        __syncthreads();
        if (threadIdx.x < 4 && s_cnt[threadIdx.x]) B.cpart[(size_t)blockIdx.x * 4 + threadIdx.x] += s_cnt[threadIdx.x];
    }
}

// ---- FUSED small-scene path ---------------------------------------------------------------------------------------------------
// A world of a few dozen objects (cfg5: seven placed cubes, a sphere, a medium) needs no tree and no pool: streaming its paths
// through EXTEND and SHADE moved 405 bytes of path state per segment through HBM for nine objects (profiles/r2_cfg5_traffic.json:
// 979 GB per frame), and the frame's 486 ms were those round trips.  Here a lane keeps its whole path in registers and tests
// EVERY leaf object of the world each segment — the loop counter is wave-uniform, so the objects' records arrive through scalar
// loads, once per wave — then shades the winner in place; a lane whose path ends writes the sample and starts the next work unit
// (persistent threads with regeneration: the intersection loop always runs under a full exec mask, only the material branch
// diverges).  HBM sees 24 bytes per SAMPLE (samples[unit], reduced by stream_reduce as in the pipeline): the kernel is bound by
// FP64 vector issue.  Arithmetic and decisions are the pipeline's (the same zr_device.h routines in the same order), so a frame
// agrees with the pipeline's to the last bits of FMA contraction.
// Work units: waves reserve chunks of ST_FUSED_CHUNK consecutive units (one atomic per chunk, ST_SHARDS interleaved counters), so
// that the 64 lanes of a wave share a pixel; every wave reaches the exit: it leaves when its lanes are idle and every shard is dry.
#ifndef ST_FUSED_CHUNK
#define ST_FUSED_CHUNK 256
#endif
#ifndef ST_FUSED_WAVES
#define ST_FUSED_WAVES 2
#endif
struct FusedBuf {
    const uint32_t* pixels; double* samples; unsigned int* uctl;   // uctl: the unit-counter block; here shard s counts chunks of ST_FUSED_CHUNK units
    uint32_t spp, n_units;
    uint32_t sample0;              // as StreamBuf::sample0
    uint32_t chunk_lo, chunk_hi;   // this launch hands out the chunks [chunk_lo, chunk_hi) of ST_FUSED_CHUNK units (a frame in one launch, or in
                                   // parts when the caller polls for cancellation / progress between them)
};
// plain medium from a kernel-argument record (medium_plain_t's arithmetic: constant_medium.hpp:39-77 on a bare boundary)
__device__ __forceinline__ bool medium_rec_t(const double* q, const Ray& r, double tmin, double tmax, const Rng& g, double& t) {
    double t1, t2;
    const double inf = __builtin_huge_val();
    const uint32_t btype = (uint32_t)__double_as_longlong(q[8]);
    if (btype == ZR_PRIM_SPHERE) {
        if (!sphere_t(q, r, -inf, inf, t1)) return false;
        if (!sphere_t(q, r, t1 + 0.0001, inf, t2)) return false;
    } else {
        if (!cube_t(q, r, -inf, inf, t1)) return false;
        if (!cube_t(q, r, t1 + 0.0001, inf, t2)) return false;
    }
    if (t1 < tmin) t1 = tmin;
    if (t2 > tmax) t2 = tmax;
    if (t1 >= t2) return false;
    if (t1 < 0) t1 = 0;
    const double rl = len(r.d);
    const double inside = (t2 - t1) * rl;
    const double xi = zr_bits_to_unit(zr_medium_bits(g.key, g.bounce, (uint32_t)__double_as_longlong(q[7])));
    const double hd = q[6] * log(xi);
    if (hd > inside) return false;
    t = t1 + hd / rl;
    return true;
}
template <int LEVEL, bool COUNT>
__device__ __forceinline__ void brute_hit(const DScene& sc, const FusedObjs& fo, const Ray& ray, const Rng& g, double& tbest, uint32_t& kbest, uint32_t& ibest, uint32_t* cn) {
    const double INF = __builtin_huge_val();
    tbest = INF; kbest = 0xFFFFFFFFu; ibest = 0;
    double t;
    const V3 inv_d = mk(1.0 / ray.d.x, 1.0 / ray.d.y, 1.0 / ray.d.z);   // for the cubes that see the world ray's direction (cube_t_inv)
    // the table's objects: wave-uniform loop counter and kind, records through scalar loads
    for (uint32_t i = 0; i < fo.n; i++) {
        const uint32_t k = fo.kind[i];
        const double* q = fo.rec[i];
        bool h;
        if (k == ZR_PRIM_SPHERE) h = sphere_t(q, ray, 0.001, tbest, t);
        else if (k == ZR_PRIM_TRIANGLE) h = triangle_t(q, ray, 0.001, tbest, t);
        else if (k == ZR_PRIM_CUBE) h = cube_t_inv(q, ray, inv_d, 0.001, tbest, t);
        else if (k == ZR_KIND_PCUBE) h = pcube_t_inv<false>(q, ray, inv_d, 0.001, tbest, t);   // (no scaled placed cube reaches this kernel: zr_commit.cpp finish_commit)
        else h = medium_rec_t(q, ray, 0.001, tbest, g, t);
        if (h) { tbest = t; kbest = k; ibest = fo.index[i]; }
        if (COUNT) { if (k == ZR_PRIM_SPHERE) cn[0]++; else if (k == ZR_PRIM_TRIANGLE) cn[1]++; else if (k == ZR_PRIM_CUBE || k == ZR_KIND_PCUBE) cn[2]++; else cn[3]++; }
    }
    if (LEVEL >= 2) {   // what the table cannot hold: media with a wrapped boundary, objects under wrapper chains (the op-list interpreter)
        for (uint32_t i = 0; i < sc.leaf_cnt[ZR_PRIM_MEDIUM]; i++) {
            if (sc.media[i].chain_count == 0) continue;   // (plain ones are in the table)
            if (medium_t(sc, i, ray, 0.001, tbest, g, t)) { tbest = t; kbest = ZR_PRIM_MEDIUM; ibest = i; }
            if (COUNT) cn[3]++;
        }
        for (uint32_t i = 0; i < sc.leaf_cnt[ZR_KIND_WRAPPED]; i++) {
            if (object_t(sc, ZR_KIND_WRAPPED, i, ray, 0.001, tbest, g, t)) { tbest = t; kbest = ZR_KIND_WRAPPED; ibest = i; }
            if (COUNT) { const uint32_t kk = sc.wrapped[i].type; if (kk == ZR_PRIM_SPHERE) cn[0]++; else if (kk == ZR_PRIM_TRIANGLE) cn[1]++; else if (kk == ZR_PRIM_CUBE) cn[2]++; else cn[3]++; }
        }
    }
}

template <int LEVEL, bool COUNT, bool UV = false>
__global__ __launch_bounds__(256, ST_FUSED_WAVES) void fused_render(DScene sc, DCamera cam, DEnv env, uint64_t seed, FusedBuf B, unsigned long long* __restrict__ gctr, FusedObjs fo) {
    const int lane = threadIdx.x & 63;
    const uint32_t wave_id = blockIdx.x * 4 + (threadIdx.x >> 6);
    const uint32_t NONE = 0xFFFFFFFFu;
    const int depth_inner = cam.max_depth - 1;
    // the lane's path
    bool active = false, first = true;
    uint32_t unit = 0;
    Ray ray; ray.o = mk(0, 0, 0); ray.d = mk(0, 0, 1);
    Rng g; g.key = 0; g.k = 0; g.bounce = 0;
    V3 L0 = mk(0, 0, 0), att0 = mk(0, 0, 0), L = mk(0, 0, 0), beta = mk(1, 1, 1);
    int b_inner = 0;
    // the wave's chunk of work units
    uint32_t chunk_next = 0, chunk_end = 0, shard = wave_id % ST_SHARDS, shards_tried = 0;
    bool units_left = true;
    uint32_t cn[4] = {0, 0, 0, 0}, c_samp = 0, c_seg = 0, c_hit = 0;
    unsigned long long c_draws = 0;
    const unsigned long long n_chunks = B.chunk_hi;
    for (;;) {
        // ---- regeneration: idle lanes take the wave's next units
        const unsigned long long idle = __ballot(!active);
        if (idle != 0ull && units_left) {
            uint32_t want = (uint32_t)__popcll(idle);
            while (chunk_next >= chunk_end && units_left) {
                uint32_t nb = 0;
                if (lane == 0) nb = atomicAdd(&B.uctl[CTL_STRIDE * shard + CTL_SH_UNITS], 1u);
                nb = __builtin_amdgcn_readfirstlane(nb);
                const unsigned long long c = (unsigned long long)B.chunk_lo + (unsigned long long)nb * ST_SHARDS + shard;   // chunk index
                if (c < n_chunks) {
                    chunk_next = (uint32_t)(c * ST_FUSED_CHUNK);
                    const unsigned long long e = c * ST_FUSED_CHUNK + ST_FUSED_CHUNK;
                    chunk_end = e < (unsigned long long)B.n_units ? (uint32_t)e : B.n_units;
                } else {
                    shard = (shard + 1) % ST_SHARDS;
                    if (++shards_tried >= ST_SHARDS) units_left = false;
                }
            }
            if (!units_left) want = 0;
            if (want > chunk_end - chunk_next) want = chunk_end - chunk_next;
            const uint32_t base = chunk_next;
            chunk_next += want;
            if (!active) {
                const uint32_t my = (uint32_t)__popcll(idle & ((1ull << lane) - 1ull));
                if (my < want) {
                    unit = base + my;
                    const uint32_t pix_i = unit / B.spp, sample = unit - pix_i * B.spp + B.sample0;
                    const uint32_t pk = B.pixels[pix_i];
                    const int px = (int)(pk & 0xFFFFu), py = (int)(pk >> 16);
                    g.key = zr_stream_key(seed, (uint64_t)py * (uint64_t)cam.W + (uint64_t)px, (uint64_t)sample); g.k = 0; g.bounce = 0;
                    ray = camera_ray(cam, px, py, g);
                    first = true; active = true;
                    if (COUNT) c_samp++;
                }
            }
        }
        if (__ballot(active) == 0ull) { if (!units_left) break; else continue; }
        // ---- one segment for every active lane: closest hit over all leaf objects, then the shading of the winner
        double t_hit; uint32_t kind, idx;
        brute_hit<LEVEL, COUNT>(sc, fo, ray, g, t_hit, kind, idx, cn);
        if (active) {
            g.bounce++;
            if (COUNT) { c_seg++; if (kind != NONE) c_hit++; }
            bool ended = false;
            V3 rad = mk(0, 0, 0);
            if (kind == NONE) {
                const V3 bg = background(sc, env, ray.d);
                rad = first ? bg : L0 + att0 * (L + beta * bg);   // camera.hpp:520 / 941, 1000
                ended = true;
            } else {
                Rec rec;
                object_rec<false, UV>(sc, kind, idx, ray, t_hit, rec);
                const V3 em = emitted(sc, rec);
                V3 att; Ray nr;
                const bool sc_ok = scatter(sc, ray, rec, att, nr, g);
                if (first) {   // ray_color_from_hit, camera.hpp:989-1004
                    L0 = em;
                    if (!sc_ok || depth_inner <= 0) { rad = L0; ended = true; }
                    else { att0 = att; L = mk(0, 0, 0); beta = mk(1, 1, 1); b_inner = 0; first = false; ray = nr; }
                } else {       // body of ray_color's loop, camera.hpp:944-983
                    L = L + beta * em;
                    bool stop = !sc_ok;
                    if (!stop) {
                        beta = beta * att;
                        if (b_inner > 10) {
                            if (len(beta) < 0.0001) stop = true;
                            else {
                                double p = fmax(fmax(beta.x, beta.y), beta.z);
                                p = clampd(p, 0.05, 0.95);
                                if (g.next() > p) stop = true; else beta = beta * (1 / p);
                            }
                        }
                    }
                    if (!stop) { b_inner++; if (b_inner >= depth_inner) stop = true; }
                    if (stop) { rad = L0 + att0 * L; ended = true; } else ray = nr;
                }
            }
            if (ended) {
                double* pp = B.samples + (size_t)unit * 3;
                pp[0] = rad.x; pp[1] = rad.y; pp[2] = rad.z;
                if (COUNT) c_draws += g.k;
                active = false;
            }
        }
    }
    if (COUNT) {
        atomicAdd(&gctr[CTR_SAMPLES], (unsigned long long)c_samp); atomicAdd(&gctr[CTR_SEGMENTS], (unsigned long long)c_seg);
        atomicAdd(&gctr[CTR_SPHERES], (unsigned long long)cn[0]); atomicAdd(&gctr[CTR_TRIANGLES], (unsigned long long)cn[1]); atomicAdd(&gctr[CTR_CUBES], (unsigned long long)cn[2]); atomicAdd(&gctr[CTR_MEDIA], (unsigned long long)cn[3]);
        atomicAdd(&gctr[CTR_HITS], (unsigned long long)c_hit); atomicAdd(&gctr[CTR_DRAWS], c_draws);
    }
}

// THE DRAIN.  Once the last work unit has been handed out a frame lives on its longest paths: cfg5 (depth 50) spends 36 of its
// 118 rounds on a pool that is almost empty, and a round costs 0.8 ms however few paths it carries (every EXTEND wave still
// walks its share of the slot pool to find them).  So when no unit is left and fewer than 1/16 of the slots are active, the
// host has the survivors MOVED to the front of a small pool of their own (all 23 state rows of a slot: a slot is self-contained,
// its unit id travels with it) and runs the remaining rounds on that.  Which slot holds a path changes; nothing else does.
// A block takes ST_COMPACT_PER x 256 slots and reserves room for all its survivors with ONE atomic: every survivor count goes through one word, which sustains
// ~90 atomics/us (see ST_SHARDS), and with an atomic per wave that has a survivor the compaction of cfg3's two 52 Mi-slot sub-pools took 6.5 ms when 1 slot in
// 100 was alive (800 K atomics) against 1.3 ms at 1 in 900: the earlier the switch, the dearer.  Now at most 27 K atomics whatever the survivors' number.
#define ST_COMPACT_PER 16
__global__ __launch_bounds__(256) void stream_compact(StreamBuf S, StreamBuf D, unsigned int* __restrict__ counter) {
    __shared__ uint32_t s_wave[4];
    __shared__ uint32_t s_base;
    const int wl = threadIdx.x & 63, w = threadIdx.x >> 6;
    const uint32_t slot0 = blockIdx.x * (256u * ST_COMPACT_PER) + threadIdx.x;   // pass j: slot0 + 256 j (grid: ceil(S.P / (256 PER)) blocks, so slot0 < 2^32)
    unsigned long long bm[ST_COMPACT_PER];   // (wave-uniform)
    uint32_t wave_total = 0;
#pragma unroll
    for (int j = 0; j < ST_COMPACT_PER; j++) {
        const unsigned long long slot = (unsigned long long)slot0 + 256ull * (unsigned)j;
        const bool act = slot < S.P && (S.ld2(SF_MA, (uint32_t)slot).y & F_ACTIVE) != 0;
        bm[j] = __ballot(act);
        wave_total += (uint32_t)__popcll(bm[j]);
    }
    if (wl == 0) s_wave[w] = wave_total;
    __syncthreads();
    uint32_t before = 0, total = 0;
    for (int k = 0; k < 4; k++) { const uint32_t c = s_wave[k]; total += c; if (k < w) before += c; }
    if (total == 0) return;   // (the whole block)
    if (threadIdx.x == 0) s_base = atomicAdd(counter, total);
    __syncthreads();
    uint32_t base = s_base + before;
#pragma unroll
    for (int j = 0; j < ST_COMPACT_PER; j++) {
        if ((bm[j] >> wl) & 1ull) {
            const uint32_t slot = slot0 + 256u * (unsigned)j;
            const uint32_t d = base + (uint32_t)__popcll(bm[j] & ((1ull << wl) - 1ull));
            // (d >= D.P cannot happen: the host sized D from a poll's count, which bounds this one — zr_round_polls.h, drain_condition)
            if (d < D.P)
                for (int f = 0; f <= SF_MB; f++) D.st(f, d, S.ld(f, slot));   // the 23 rows in use (the 24th is spare)
        }
        base += (uint32_t)__popcll(bm[j]);
    }
}
// the slots behind the survivors: inactive.  How many survivors there are is *counter (stream_compact has run): the host's figure may be a few rounds old
__global__ __launch_bounds__(256) void stream_compact_pad(StreamBuf D, const unsigned int* __restrict__ counter) {
    const uint32_t slot = blockIdx.x * 256 + threadIdx.x;
    if (slot >= *counter && slot < D.P) { uint2 z; z.x = 0; z.y = 0; D.st2(SF_MA, slot, z); D.ctl[CTL_INACTIVE] = 1u; }
}

// THE POLL of a round (zr_round_polls.h), one wave behind a sub-pool's SHADE on its stream: lane s reads shard s.  `host` is pinned host memory: a kernel's store
// reaches it without leaving the stream for a copy engine, and the event the host records behind this launch says when it is there.
__global__ __launch_bounds__(64) void stream_poll(StreamBuf B, unsigned int* __restrict__ host) {
    const uint32_t sh = threadIdx.x;
    uint32_t active = B.ctl[CTL_SHARD0 + CTL_STRIDE * sh + CTL_SH_ACTIVE];
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) active += __shfl_xor(active, m, 64);   // (<= B.P: fits)
    // shard sh has handed out every k below its counter (SHADE: unit = st_unit_of(.., k)); the counters only grow
    const unsigned long long k = (unsigned long long)B.shard_k0 + B.uctl[CTL_STRIDE * sh + CTL_SH_UNITS];
    const bool left = st_unit_of(B.unit_chunk, B.unit_base, sh, k) < (unsigned long long)B.n_units;
    const unsigned long long any_left = __ballot(left);
    if (sh == 0) {
        host[POLL_ACTIVE] = active; host[POLL_CAPPED] = B.ctl[CTL_CAPPED]; host[POLL_UNITS_LEFT] = any_left != 0ull ? 1u : 0u;
        __threadfence_system();
    }
}

// one wave per pixel: lane l sums samples l, l + 64, ... in order, then a fixed xor butterfly — the order depends on
// spp only, never on which slot produced a sample
__global__ __launch_bounds__(256) void stream_reduce(StreamBuf B, DCamera cam, double* __restrict__ out) {
    const uint32_t i = blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (i >= B.n_pix) return;
    const double* pp = B.samples + (size_t)i * B.spp * 3;
    const V3 mean = wave_pixel_mean(lane, B.spp, cam.spp, [&](uint32_t sidx) { return mk(pp[sidx * 3], pp[sidx * 3 + 1], pp[sidx * 3 + 2]); });
    if (lane == 0) {
        const uint32_t pk = B.pixels[i];
        const int px = (int)(pk & 0xFFFFu), py = (int)(pk >> 16);
        double* o = out + ((size_t)py * cam.W + px) * 3;
        o[0] = mean.x; o[1] = mean.y; o[2] = mean.z;
    }
}

// ---- progressive accumulation (zr_accum) ----------------------------------------------------------------------------
// The lane sums of stream_reduce, kept between runs: partial[pixel][channel][lane] (64 x 3 doubles = 1536 contiguous bytes per pixel, one coalesced
// 512-byte row per channel).  Sample s of a pixel ALWAYS belongs to lane s % 64 and a lane adds its samples in increasing s, so after any split of
// [0, N) into consecutive batches the 64 sums are exactly those stream_reduce forms in registers for spp = N (0.0 + x is x).  One wave per pixel,
// no atomics, no LDS.  `samples` holds the batch as the pipeline wrote it ([n_pix][n][3], sample0 + sidx at index sidx); flip: that pixel list ran
// in the reverse of the accumulator's order (ZR_STREAM_BOTTOM_UP).
__global__ __launch_bounds__(256) void stream_accumulate(const double* __restrict__ samples, uint32_t n_pix, uint32_t n, uint32_t sample0, uint32_t flip,
                                                          double* __restrict__ partial) {
    const uint32_t i = blockIdx.x * 4 + (threadIdx.x >> 6);
    const uint32_t lane = threadIdx.x & 63u;
    if (i >= n_pix) return;
    const uint32_t first = (lane - sample0) & 63u;   // the batch's first sample of this lane: (sample0 + first) % 64 == lane
    if (first >= n) return;
    const double* pp = samples + (size_t)i * n * 3;
    double* q = partial + (size_t)(flip ? n_pix - 1u - i : i) * 192 + lane;
    double sx = q[0], sy = q[64], sz = q[128];
    for (uint32_t sidx = first; sidx < n; sidx += 64) { sx += pp[(size_t)sidx * 3]; sy += pp[(size_t)sidx * 3 + 1]; sz += pp[(size_t)sidx * 3 + 2]; }
    q[0] = sx; q[64] = sy; q[128] = sz;
}

// The stored lane sums -> the mean of the `done` samples they hold, into the accumulator's pixels of `out`.  The xor butterfly of the kernel that
// rendered the batches: stream_reduce pairs lanes 32, 16, ... 1 apart (asc_lanes = 1); the pixel-group kernel sums over L = asc_lanes lanes
// (lanes_for: sample s in lane s % L) and pairs them 1, 2, ... L/2 apart, which here is the steps 32 ... L first (lane l + lane l + L, the
// two samples a pixel-group lane adds) and then 1 ... L/2.  Either way every lane ends with the sum of all 64; the order is what makes the frame
// equal the one-shot frame of the same route bit for bit.
__global__ __launch_bounds__(256) void accum_resolve(const double* __restrict__ partial, const uint32_t* __restrict__ pixels, uint32_t n_pix, int W, int done,
                                                      int asc_lanes, double* __restrict__ out) {
    const uint32_t i = blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (i >= n_pix) return;
    const double* q = partial + (size_t)i * 192 + lane;
    double sx = q[0], sy = q[64], sz = q[128];
    for (int m = 32; m >= asc_lanes; m >>= 1) {
        sx += __hiloint2double(__shfl_xor(__double2hiint(sx), m, 64), __shfl_xor(__double2loint(sx), m, 64));
        sy += __hiloint2double(__shfl_xor(__double2hiint(sy), m, 64), __shfl_xor(__double2loint(sy), m, 64));
        sz += __hiloint2double(__shfl_xor(__double2hiint(sz), m, 64), __shfl_xor(__double2loint(sz), m, 64));
    }
    for (int m = 1; m < asc_lanes; m <<= 1) {
        sx += __hiloint2double(__shfl_xor(__double2hiint(sx), m, 64), __shfl_xor(__double2loint(sx), m, 64));
        sy += __hiloint2double(__shfl_xor(__double2hiint(sy), m, 64), __shfl_xor(__double2loint(sy), m, 64));
        sz += __hiloint2double(__shfl_xor(__double2hiint(sz), m, 64), __shfl_xor(__double2loint(sz), m, 64));
    }
    if (lane == 0) {
        const uint32_t pk = pixels[i];
        const int px = (int)(pk & 0xFFFFu), py = (int)(pk >> 16);
        const double scale = 1.0 / done;  // camera.hpp:437,531 with the samples that exist
        double* o = out + ((size_t)py * W + px) * 3;
        o[0] = sx * scale; o[1] = sy * scale; o[2] = sz * scale;
    }
}

// per-block counters of the split passes -> the context's counter words (samples, segments, hits, draws)
__global__ __launch_bounds__(256) void stream_sum_counters(const unsigned long long* __restrict__ cpart, size_t n_blocks, unsigned long long* __restrict__ gctr) {
    __shared__ unsigned long long s[4];
    if (threadIdx.x < 4) s[threadIdx.x] = 0;
    __syncthreads();
    unsigned long long a[4] = {0, 0, 0, 0};
    for (size_t b = threadIdx.x; b < n_blocks; b += 256) for (int k = 0; k < 4; k++) a[k] += cpart[b * 4 + k];
    for (int k = 0; k < 4; k++) if (a[k]) atomicAdd(&s[k], a[k]);
    __syncthreads();
    if (threadIdx.x == 0) { gctr[CTR_SAMPLES] += s[0]; gctr[CTR_SEGMENTS] += s[1]; gctr[CTR_HITS] += s[2]; gctr[CTR_DRAWS] += s[3]; }
}

// the split frames: the same order-fixed sum, every sample to the frame its class names
__global__ __launch_bounds__(256) void stream_reduce_split(StreamBuf B, DCamera cam, double* __restrict__ out_reflection, double* __restrict__ out_refraction) {
    const uint32_t i = blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (i >= B.n_pix) return;
    const double* pp = B.samples + (size_t)i * B.spp * 3;
    const unsigned char* cc = B.cls + (size_t)i * B.spp;
    double a[6] = {0, 0, 0, 0, 0, 0};
    for (uint32_t sidx = (uint32_t)lane; sidx < B.spp; sidx += 64) {
        const unsigned char c = cc[sidx];
        if (c == 1) { a[0] += pp[sidx * 3]; a[1] += pp[sidx * 3 + 1]; a[2] += pp[sidx * 3 + 2]; }
        else if (c == 2) { a[3] += pp[sidx * 3]; a[4] += pp[sidx * 3 + 1]; a[5] += pp[sidx * 3 + 2]; }
    }
    for (int m = 32; m >= 1; m >>= 1)
        for (int k = 0; k < 6; k++) a[k] += __hiloint2double(__shfl_xor(__double2hiint(a[k]), m, 64), __shfl_xor(__double2loint(a[k]), m, 64));
    if (lane == 0) {
        const uint32_t pk = B.pixels[i];
        const int px = (int)(pk & 0xFFFFu), py = (int)(pk >> 16);
        const double scale = 1.0 / cam.spp;  // camera.hpp:532-533
        const size_t o = ((size_t)py * cam.W + px) * 3;
        if (out_reflection) { out_reflection[o] = a[0] * scale; out_reflection[o + 1] = a[1] * scale; out_reflection[o + 2] = a[2] * scale; }
        if (out_refraction) { out_refraction[o] = a[3] * scale; out_refraction[o + 1] = a[4] * scale; out_refraction[o + 2] = a[5] * scale; }
    }
}

// ---- known-answer path: a batch of caller-supplied rays through EXTEND (zr_trace) ------------------------------------
// slot k = ray k, RNG key as in trace_rays (zr_kernels.hip) so that a medium's draw is the same on both engines
__global__ __launch_bounds__(256) void stream_load_rays(StreamBuf B, const double* __restrict__ rays, uint32_t n, uint64_t seed, uint64_t pixel,
                                                         uint32_t bounce) {
    const uint32_t slot = blockIdx.x * 256 + threadIdx.x;
    if (slot >= B.P) return;
    uint2 ma; ma.x = 0; ma.y = 0;
    if (slot < n) {
        B.st3(SF_RAY, slot, ld3(rays + (size_t)slot * 6)); B.st3(SF_RAY + 3, slot, ld3(rays + (size_t)slot * 6 + 3));
        B.st(SF_KEY, slot, __longlong_as_double((long long)zr_stream_key(seed, pixel, (uint64_t)slot)));
        ma.y = (bounce & 0xFFu) | F_ACTIVE;
    } else B.ctl[CTL_INACTIVE] = 1u;
    B.st2(SF_MA, slot, ma);
}

template <bool UV>
__global__ __launch_bounds__(256) void stream_hits_out(DScene sc, StreamBuf B, uint32_t n, zr_hit* __restrict__ out, uint2* __restrict__ out_ki) {
    const uint32_t slot = blockIdx.x * 256 + threadIdx.x;
    if (slot >= n) return;
    const uint2 ki = B.ld2(SF_HIT_KI, slot);
    zr_hit o;
    if (ki.x != 0xFFFFFFFFu) {
        Ray r; r.o = B.ld3(SF_RAY, slot); r.d = B.ld3(SF_RAY + 3, slot);
        Rec rec;
        object_rec<true, UV>(sc, ki.x, ki.y, r, B.ld(SF_HIT_T, slot), rec, true);
        o.p[0] = rec.p.x; o.p[1] = rec.p.y; o.p[2] = rec.p.z;
        o.normal[0] = rec.n.x; o.normal[1] = rec.n.y; o.normal[2] = rec.n.z;
        o.tangent[0] = rec.tan.x; o.tangent[1] = rec.tan.y; o.tangent[2] = rec.tan.z;
        o.bitangent[0] = rec.bit.x; o.bitangent[1] = rec.bit.y; o.bitangent[2] = rec.bit.z;
        o.t = rec.t; o.u = rec.u; o.v = rec.v; o.mat = rec.mat; o.front_face = rec.front ? 1u : 0u;
    } else {
        for (int c = 0; c < 3; c++) { o.p[c] = 0; o.normal[c] = 0; o.tangent[c] = 0; o.bitangent[c] = 0; }
        o.t = 0; o.u = 0; o.v = 0; o.mat = 0xFFFFFFFFu; o.front_face = 0;
    }
    out[slot] = o;
    if (out_ki) out_ki[slot] = ki.x != 0xFFFFFFFFu ? ki : make_uint2(0xFFFFFFFFu, 0xFFFFFFFFu);   // as trace_rays reports it
}

// ---- host-side launch helpers -----------------------------------------------------------------------------------
size_t stream_ctl_words() { return CTL_SHARD0 + CTL_STRIDE * ST_SHARDS; }
// spill slab of the EXTEND stack: `stack_demand` = worst-case entries of the committed tree (zr_scene_stats), ST_LDS_STACK of them live in LDS
uint32_t stream_overflow_levels(uint32_t stack_demand) { return stack_demand > ST_LDS_STACK ? stack_demand - ST_LDS_STACK : 1u; }
size_t stream_overflow_bytes(int blocks, uint32_t levels) { return (size_t)blocks * levels * 64 * sizeof(SEntry); }

// number of EXTEND waves that are resident at once (the persistent grid), a multiple of the workgroup's ST_EXT_GROUP
int stream_extend_blocks() {
    int dev = 0, cus = 256, per_cu = 2;
    if (hipGetDevice(&dev) == hipSuccess) {
        hipDeviceProp_t p;
        if (hipGetDeviceProperties(&p, dev) == hipSuccess) cus = p.multiProcessorCount;
    }
    int lean = 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, stream_extend<false, 2>, 64 * ST_EXT_GROUP, 0) != hipSuccess || per_cu < 1) per_cu = 2;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&lean, stream_extend<false, 0>, 64 * ST_EXT_GROUP, 0) == hipSuccess && lean > per_cu) per_cu = lean;
    if (std::getenv("ZR_COMMIT_STATS")) std::fprintf(stderr, "[zr] EXTEND workgroups per CU: %d (lean build %d) x %d waves\n", per_cu, lean, ST_EXT_GROUP);
    return cus * per_cu * ST_EXT_GROUP;
}

// layout of the slot pool inside one allocation; returns bytes needed
size_t stream_pool_bytes(uint32_t P) { return ((size_t)(P + 63) / 64) * SF_N * 64 * sizeof(double); }

static StreamBuf make_buf(void* pool, uint32_t P, uint32_t spp, uint32_t n_units, uint32_t n_pix, const uint32_t* pixels, double* samples,
                          unsigned int* ctl, unsigned int* uctl, uint32_t unit0, uint32_t unit_base) {
    StreamBuf B;
    B.pool = (double*)pool; B.pixels = pixels; B.samples = samples; B.ctl = ctl; B.uctl = uctl;
    B.P = P; B.spp = spp; B.n_units = n_units; B.n_pix = n_pix; B.unit0 = unit0; B.unit_base = unit_base; B.unit_chunk = 0; B.shard_k0 = 0; B.sample0 = 0;
    B.kend = nullptr; B.cls = nullptr; B.cpart = nullptr;
    return B;
}

// The control blocks of a run, zeroed on `stream`.  ZR_EXTEND_ALL_ACTIVE=0 (read per run, like ZR_SHADE_IN_PLACE) starts every pool's CTL_INACTIVE at 1: the lean
// EXTEND then tests the meta word of every slot it fetches, as it did before the word existed.
static hipError_t clear_ctl(unsigned int* ctl, hipStream_t stream) {
    const size_t W = stream_ctl_words();
    hipError_t e = hipMemsetAsync(ctl, 0, (ST_MAX_POOLS + 1) * W * sizeof(unsigned int), stream);
    const char* env = std::getenv("ZR_EXTEND_ALL_ACTIVE");
    if (env && std::atoi(env) == 0)
        for (int k = 0; k < ST_MAX_POOLS && e == hipSuccess; k++) e = hipMemsetD32Async((hipDeviceptr_t)(ctl + (size_t)k * W + CTL_INACTIVE), 1, 1, stream);
    return e;
}

// ---- which build serves a launch: per kernel family one table from the deciding facts to the kernel, and one call site --------------------------------------
using ExtendKernel = void (*)(DScene, StreamBuf, SEntry*, uint32_t, unsigned long long*, float);
using ShadeKernel = void (*)(DScene, DCamera, DEnv, uint64_t, StreamBuf, unsigned long long*);
using FusedKernel = void (*)(DScene, DCamera, DEnv, uint64_t, FusedBuf, unsigned long long*, FusedObjs);

// `blocks` counts waves (at most stream_extend_blocks(), a multiple of ST_EXT_GROUP: the overflow slabs are sized for that many)
static void launch_extend(bool count, int level, const DScene& sc, const StreamBuf& B, void* overflow, uint32_t ovf_levels, int blocks, unsigned long long* gctr, hipStream_t st) {
    static constexpr ExtendKernel build[2][4] = {   // [count][leaf level]
        {stream_extend<false, 0>, stream_extend<false, 1>, stream_extend<false, 2>, stream_extend<false, 3>},
        {stream_extend<true, 0>, stream_extend<true, 1>, stream_extend<true, 2>, stream_extend<true, 3>}};
    const ExtendKernel kernel = build[count ? 1 : 0][level < 0 ? 0 : (level > 3 ? 3 : level)];
    hipLaunchKernelGGL(kernel, dim3((blocks + ST_EXT_GROUP - 1) / ST_EXT_GROUP), dim3(64 * ST_EXT_GROUP), 0, st, sc, B, (SEntry*)overflow, ovf_levels, gctr, slab_id_limit(sc.root));
}

// SHADE.  in place: the lean build that shades a slot where it lies, one wave per workgroup; lean: same arithmetic as the general build, fewer registers, 6 waves
// per SIMD instead of 4 (see lean_rec, zr_device.h), sorted like it; uv: the general build that reads the triangles' texture coordinates.
enum ShadeFamily { SHADE_IN_PLACE = 0, SHADE_LEAN = 1, SHADE_UV = 2, SHADE_GENERAL = 3 };
static void launch_shade(ShadeFamily family, bool count, int mode, unsigned lds_pad, const DScene& sc, const DCamera& cam, const DEnv& env, uint64_t seed,
                         const StreamBuf& B, unsigned long long* gctr, hipStream_t st) {
    static constexpr ShadeKernel build[4][4] = {   // [family][variant]: plain, counting, the split's reflection pass, its refraction pass (the lean families serve mode 0 only)
        {stream_shade<false, 0, true, false, false>, stream_shade<true, 0, true, false, false>, nullptr, nullptr},
        {stream_shade<false, 0, true>, stream_shade<true, 0, true>, nullptr, nullptr},
        {stream_shade<false, 0, false, true>, stream_shade<true, 0, false, true>, stream_shade<true, 1, false, true>, stream_shade<true, 2, false, true>},
        {stream_shade<false, 0>, stream_shade<true, 0>, stream_shade<true, 1>, stream_shade<true, 2>}};
    const int variant = mode != 0 ? 1 + mode : (count ? 1 : 0);   // the split passes always count
    const unsigned lds = variant == 0 ? lds_pad : 0u;              // the LDS pad goes only to non-counting builds
    const uint32_t slot_blocks = (B.P + 255) / 256;
    const bool waves = family == SHADE_IN_PLACE;                   // one wave per workgroup, four per slot block
    hipLaunchKernelGGL(build[family][variant], dim3(waves ? slot_blocks * 4 : slot_blocks), dim3(waves ? 64 : 256), lds, st, sc, cam, env, seed, B, gctr);
}

// level: 1 = no wrapped objects and only plain media, 2 = everything but placements; uv: the builds that read the triangles' texture coordinates
static void launch_fused(int level, bool count, bool uv, dim3 grid, const DScene& sc, const DCamera& cam, const DEnv& env, uint64_t seed, const FusedBuf& B,
                         unsigned long long* gctr, const FusedObjs& fo, hipStream_t st) {
    static constexpr FusedKernel build[2][2][2] = {   // [level][count][uv]
        {{fused_render<1, false>, fused_render<1, false, true>}, {fused_render<1, true>, fused_render<1, true, true>}},
        {{fused_render<2, false>, fused_render<2, false, true>}, {fused_render<2, true>, fused_render<2, true, true>}}};
    hipLaunchKernelGGL(build[level <= 1 ? 0 : 1][count ? 1 : 0][uv ? 1 : 0], grid, dim3(256), 0, st, sc, cam, env, seed, B, gctr, fo);
}

// A polled frame's report, the stream idle: when the sink wants the frame, `out` gets the mean of the samples finished so far (samples[] began at zero: render_stream)
static hipError_t reduce_and_report(StreamProgress& sink, double finished_fraction, bool reducible, const StreamFrame& F, const StreamBuf& B, hipStream_t stream) {
    bool reduced = false;
    if (reducible && F.out && sink.wants_frame()) {
        hipLaunchKernelGGL(stream_reduce, dim3((F.n_pix + 3) / 4), dim3(256), 0, stream, B, *F.cam, F.out);
        const hipError_t e = hipStreamSynchronize(stream);
        if (e != hipSuccess) return e;
        reduced = true;
    }
    sink.report(finished_fraction, reduced);
    return hipSuccess;
}

struct StreamSwitches {
    unsigned shade_pad;   // ZR_SHADE_LDS_PAD (read once per process), a development aid: bytes of dynamic LDS per SHADE block lower the blocks a CU can hold
                          // (160 KB: 4 fit by registers; > 40 KB: 3, > 53 KB: 2)
    bool trace_polls;     // ZR_STREAM_POLL_TRACE (once per process), a development aid: one line per poll on stderr
    bool in_place;        // ZR_SHADE_IN_PLACE (per render): 0 forces the sorted SHADE build
    int lag;              // ZR_STREAM_POLL_LAG (per render): rounds the lagged loop's knowledge is behind, 0 .. POLL_MAX_LAG; 0 is the cadenced loop
};
static StreamSwitches read_switches() {
    static const unsigned shade_pad = std::getenv("ZR_SHADE_LDS_PAD") ? (unsigned)std::atoi(std::getenv("ZR_SHADE_LDS_PAD")) : 0u;
    static const bool trace_polls = std::getenv("ZR_STREAM_POLL_TRACE") != nullptr;
    const char* in_place_env = std::getenv("ZR_SHADE_IN_PLACE");
    const char* lag_env = std::getenv("ZR_STREAM_POLL_LAG");
    const int lag = lag_env ? std::atoi(lag_env) : 1;
    return StreamSwitches{shade_pad, trace_polls, !(in_place_env && std::atoi(in_place_env) == 0), lag < 0 ? 0 : (lag > POLL_MAX_LAG ? POLL_MAX_LAG : lag)};
}

// One frame of the pipeline on the device: its sub-pools, the launches of a round, and what the round loop (zr_round_polls.h: run_round_loop) asks of a device.
// The slot pool can be split into K sub-pools that run a fraction of a round apart on K HIP streams, so that one
// pool's EXTEND overlaps another's SHADE.  Measured on cfg3: K = 2 gains 1-3 % on a whole frame and 6 % on a rank's
// 1/8 shard, K >= 3 loses (the stages are throughput-bound, co-running launches only stretch each other).
// streams[0] is the caller's stream, the others are internal.
struct PipelineRun {
    const DScene& sc; const StreamJob& job; const int leaf_level; const StreamSwitches sw;
    const StreamFrame& F; const StreamContext& X; const StreamHooks& H;
    const size_t W = stream_ctl_words();
    StreamBuf Q[ST_MAX_POOLS]; void* ov[ST_MAX_POOLS];
    int K = 1;                        // sub-pools the frame begins on
    // The lean render of a world with one material kind shades its slots IN PLACE while work units are left: the pool is full of fresh paths and the sort would
    // only cost.  `units_left` is what the newest poll the loop holds says (true until one arrives); once the hand-out is over the pool thins out and the sorted
    // build packs the survivors into full waves.  Either build is correct for any launch, so a stale poll only costs time.
    const bool lean, in_place_ok;
    const bool cadenced;
    int shade_launches[2] = {0, 0};   // in place, sorted

    PipelineRun(const DScene& sc_, const StreamJob& job_, int leaf_level_, const StreamSwitches& sw_)
        : sc(sc_), job(job_), leaf_level(leaf_level_), sw(sw_), F(job_.frame), X(job_.ctx), H(job_.hooks), lean(sc_.shade_lean && job_.split.mode == 0),
          in_place_ok(lean && (sc_.mat_kinds & (sc_.mat_kinds - 1u)) == 0 && sw_.in_place), cadenced(sw_.lag == 0 || job_.hooks.keep_going || job_.hooks.progress) {}

    unsigned int* uctl() const { return X.ctl + (size_t)ST_MAX_POOLS * W; }   // the unit-counter block, behind the sub-pools' control blocks
    size_t cpart_blocks() const { return (size_t)job.pool.P / 256 + ST_MAX_POOLS + 1; }
    unsigned int* poll_words(int slot, int k) const { return X.h_polls + ((size_t)slot * ST_MAX_POOLS + (size_t)k) * POLL_WORDS; }
    hipEvent_t poll_event(int slot, int k) const { return X.poll_events[(size_t)slot * ST_MAX_POOLS + (size_t)k]; }

    // the pool as K sub-pools Q[] with their spill slabs ov[]
    hipError_t split_pool() {
        const uint32_t P = job.pool.P, unit_chunk = job.pool.unit_chunk, n_units = F.n_pix * F.spp;
        K = X.n_pools < 1 ? 1 : (X.n_pools > ST_MAX_POOLS ? ST_MAX_POOLS : X.n_pools);
        while (K > 1 && P / K < 64u * 1024u) K--;
        // affine hand-out (st_unit_of): a slot's shard is (slot / 256) % ST_SHARDS counted over ALL sub-pools, and the SHADE block that
        // serves it must agree (blockIdx % ST_SHARDS inside its sub-pool): pool and sub-pools are whole rounds of ST_SHARDS blocks
        const uint32_t pool_round = unit_chunk ? ST_SHARDS * 256u : 64u;
        if (unit_chunk && P % pool_round != 0) return hipErrorInvalidValue;
        while (K > 1 && P / K < pool_round) K--;
        uint32_t first = 0;
        unsigned char* base = (unsigned char*)job.pool.slots;
        for (int k = 0; k < K; k++) {
            uint32_t Pk = k == K - 1 ? P - first : (P / K + pool_round - 1) / pool_round * pool_round;
            Q[k] = make_buf(base, Pk, F.spp, n_units, F.n_pix, F.pixels, F.samples, X.ctl + (size_t)k * W, uctl(), first, P);
            Q[k].unit_chunk = unit_chunk; Q[k].shard_k0 = unit_chunk ? P / ST_SHARDS : 0u; Q[k].sample0 = F.sample0;
            Q[k].kend = (uint2*)job.split.kend; Q[k].cls = (unsigned char*)job.split.cls;
            Q[k].cpart = job.split.cpart ? job.split.cpart + ((size_t)first / 256 + (size_t)k) * 4 : nullptr;
            ov[k] = (unsigned char*)X.overflow + (size_t)k * stream_overflow_bytes(X.extend_blocks, X.ovf_levels);
            base += stream_pool_bytes(Pk);
            first += Pk;
        }
        return hipSuccess;
    }

    void init(int k) {
        const hipStream_t st = X.streams[k];
        if (H.timer) H.timer->begin(st, 0);
        if (F.count) hipLaunchKernelGGL(stream_init<true>, dim3((Q[k].P + 255) / 256), dim3(256), 0, st, Q[k], *F.cam, F.seed, X.gctr);
        else hipLaunchKernelGGL(stream_init<false>, dim3((Q[k].P + 255) / 256), dim3(256), 0, st, Q[k], *F.cam, F.seed, X.gctr);
        if (H.timer) H.timer->end(st, 0);
    }
    void extend(int k) {
        const hipStream_t st = X.streams[k];
        const uint32_t waves = (Q[k].P + 63) / 64;
        if (H.timer) H.timer->begin(st, 1);
        launch_extend(F.count, leaf_level, sc, Q[k], ov[k], X.ovf_levels, (int)(waves < (uint32_t)X.extend_blocks ? waves : (uint32_t)X.extend_blocks), X.gctr, st);
        if (H.timer) H.timer->end(st, 1);
    }
    void shade(int k, bool units_left) {
        const hipStream_t st = X.streams[k];
        const ShadeFamily family = in_place_ok && units_left ? SHADE_IN_PLACE : (lean ? SHADE_LEAN : (sc.tri_uv_at ? SHADE_UV : SHADE_GENERAL));
        if (H.timer) H.timer->begin(st, 2);
        shade_launches[family == SHADE_IN_PLACE ? 0 : 1]++;
        launch_shade(family, F.count, job.split.mode, sw.shade_pad, sc, *F.cam, *F.env, F.seed, Q[k], X.gctr, st);
        if (H.timer) H.timer->end(st, 2);
    }

    // start-up: pool k is initialised after the control words are cleared and starts once pool k-1 has a round in flight
    hipError_t start_up() {
        hipError_t e;
        if ((e = clear_ctl(X.ctl, X.streams[0])) != hipSuccess) return e;
        if (job.split.cpart && (e = hipMemsetAsync(job.split.cpart, 0, cpart_blocks() * 4 * sizeof(unsigned long long), X.streams[0])) != hipSuccess) return e;
        init(0);
        for (int k = 1; k < K; k++) {
            extend(k - 1);
            if ((e = hipEventRecord(X.event, X.streams[k - 1])) != hipSuccess) return e;
            if ((e = hipStreamWaitEvent(X.streams[k], X.event, 0)) != hipSuccess) return e;
            init(k);
            shade(k - 1, true);
        }
        return hipSuccess;
    }

    // ---- the round loop's device (zr_round_polls.h); a status is a hipError_t ----
    int enqueue_round(int slot, int pools, bool with_events, bool units_left) {
        hipError_t e = hipSuccess;
        for (int k = pools - 1; k >= 0; k--) {
            extend(k); shade(k, units_left);
            hipLaunchKernelGGL(stream_poll, dim3(1), dim3(64), 0, X.streams[k], Q[k], poll_words(slot, k));
            if (with_events && e == hipSuccess) e = hipEventRecord(poll_event(slot, k), X.streams[k]);
        }
        return (int)e;
    }
    int wait_poll(int slot, int k) { return (int)hipEventSynchronize(poll_event(slot, k)); }
    int wait_all(int pools) {
        hipError_t e = hipSuccess;
        for (int k = pools - 1; k >= 0 && e == hipSuccess; k--) e = hipStreamSynchronize(X.streams[k]);
        return (int)e;
    }
    int order_behind(int slot, int pools) {
        hipError_t e = hipSuccess;
        for (int k = 1; k < pools && e == hipSuccess; k++) e = hipStreamWaitEvent(X.streams[0], poll_event(slot, k), 0);
        return (int)e;
    }
    // the survivors of Q[0 .. pools) move to the drain pool of drain_P slots (see stream_compact), on stream 0, which the loop has ordered behind the other streams
    int compact(uint32_t drain_P, int pools) {
        StreamBuf D = Q[0];
        D.pool = (double*)job.pool.drain; D.P = drain_P; D.unit0 = 0;
        unsigned int* counter = X.ctl + CTL_COMPACT;   // (of pool 0)
        for (int k = 0; k < pools; k++) {
            const uint32_t per_block = 256u * ST_COMPACT_PER;
            hipLaunchKernelGGL(stream_compact, dim3((uint32_t)(((unsigned long long)Q[k].P + per_block - 1) / per_block)), dim3(256), 0, X.streams[0], Q[k], D, counter);
        }
        hipLaunchKernelGGL(stream_compact_pad, dim3(D.P / 256), dim3(256), 0, X.streams[0], D, counter);
        Q[0] = D;
        return 0;
    }
    // the finished fraction: the units started (the one figure no poll carries: the unit counters are copied for it) less those still on their way
    int report_progress(unsigned long long active) {
        if (!H.progress) return 0;
        unsigned int* h_units = X.h_active + (size_t)ST_MAX_POOLS * W;
        hipError_t e = hipMemcpyAsync(h_units, uctl(), W * sizeof(unsigned int), hipMemcpyDeviceToHost, X.streams[0]);
        if (e != hipSuccess || (e = hipStreamSynchronize(X.streams[0])) != hipSuccess) return (int)e;
        const uint32_t n_units = F.n_pix * F.spp;
        const unsigned long long started = units_started(job.pool.unit_chunk, job.pool.P, n_units, h_units + CTL_SH_UNITS, CTL_STRIDE);
        const double frac = started > active ? (double)(started - active) / (double)n_units : 0.0;
        return (int)reduce_and_report(*H.progress, frac, job.split.mode == 0, F, Q[0], X.streams[0]);
    }
    bool cancelled() const { return H.keep_going && *H.keep_going == 0; }
    size_t launches_logged() const { return H.timer ? H.timer->logged() : 0; }
    void polled(const RoundPolls& rp, const PollResult& p, bool compaction) const {
        if (!sw.trace_polls) return;
        const bool condition = drain_condition(p, job.pool.P, job.pool.drain_slots);
        if (!cadenced)
            std::fprintf(stderr, "[zr] poll of round %d (%d queued behind it): active %llu, units left %d, drain condition %d%s\n", rp.polled, rp.in_flight(), p.active,
                         (int)p.units_left, (int)condition, compaction ? " -> compaction" : "");
        else {
            std::fprintf(stderr, "[zr] poll of round %d (drained with %d behind it): active %llu, units left %d, drain condition %d\n", rp.polled, rp.in_flight(), p.active,
                         (int)p.units_left, (int)(p.active != 0 && condition));
            if (compaction) std::fprintf(stderr, "[zr] compaction behind round %d\n", rp.enqueued);
        }
    }

    // counters, the frame, and what the caller wanted to know
    hipError_t finish(const RoundLoopOutcome& loop) {
        const hipStream_t stream = X.streams[0];
        const int rounds = (K > 1 ? 1 : 0) + loop.rounds;   // (the start-up ran a round on all sub-pools but the last)
        // the rounds behind the one that emptied the pools changed nothing: the caller does not see them, nor their launches
        if (loop.emptied && H.timer) H.timer->drop_from(loop.log_keep);
        if (H.timer) H.timer->begin(stream, 3);
        if (job.split.cpart) hipLaunchKernelGGL(stream_sum_counters, dim3(1), dim3(256), 0, stream, job.split.cpart, cpart_blocks(), X.gctr);
        if (job.split.mode == 2) hipLaunchKernelGGL(stream_reduce_split, dim3((F.n_pix + 3) / 4), dim3(256), 0, stream, Q[0], *F.cam, F.out, F.out2);
        else if (F.out) hipLaunchKernelGGL(stream_reduce, dim3((F.n_pix + 3) / 4), dim3(256), 0, stream, Q[0], *F.cam, F.out);
        if (H.timer) H.timer->end(stream, 3);
        if (H.done_out) *H.done_out = loop.cancelled ? -rounds : rounds;
        if (H.drain_out) { H.drain_out[0] = loop.drain_round; H.drain_out[1] = K; }
        if (H.shade_out) { H.shade_out[0] = shade_launches[0]; H.shade_out[1] = shade_launches[1]; }
        return hipGetLastError();
    }
};

hipError_t stream_render(const DScene& sc, const StreamJob& job, int leaf_level) {
    if (!job.ctx.h_polls || !job.ctx.poll_events) return hipErrorInvalidValue;   // the round loop learns what the device did from its polls alone
    PipelineRun run(sc, job, leaf_level, read_switches());
    hipError_t e;
    if ((e = run.split_pool()) != hipSuccess || (e = run.start_up()) != hipSuccess) return e;
    const int max_run = job.hooks.progress ? 2 : POLL_RING;   // an interactive caller: report (and poll keep_going) every other round
    const RoundLoopOutcome loop = run_round_loop(run, RoundLoopPlan{run.cadenced, run.sw.lag, run.K, job.pool.P, job.pool.drain_slots, job.pool.drain != nullptr, max_run});
    if (loop.status != 0) return (hipError_t)loop.status;
    if (loop.runaway || loop.capped) return hipErrorLaunchFailure;  // capped: an EXTEND wave of some sub-pool hit its iteration cap, its rays were abandoned mid-walk
    return run.finish(loop);
}

// the fused small-scene render: one persistent launch over all units, then the pipeline's reduce.  `level`: 1 = no wrapped objects
// and only plain media, 2 = everything but placements
int fused_blocks() {
    int dev = 0, cus = 256, per_cu = 2;
    if (hipGetDevice(&dev) == hipSuccess) { hipDeviceProp_t p; if (hipGetDeviceProperties(&p, dev) == hipSuccess) cus = p.multiProcessorCount; }
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, fused_render<2, false>, 256, 0) != hipSuccess || per_cu < 1) per_cu = 2;
    return cus * per_cu;
}
hipError_t fused_render_frame(const DScene& sc, const StreamFrame& F, const StreamContext& X, int blocks, int level, const FusedObjs& fo, const StreamHooks& H) {
    hipStream_t stream = X.streams[0];
    const uint32_t n_units = F.n_pix * F.spp;
    const size_t W = stream_ctl_words();
    hipError_t e;
    FusedBuf B; B.pixels = F.pixels; B.samples = F.samples; B.uctl = X.ctl + (size_t)ST_MAX_POOLS * W; B.spp = F.spp; B.n_units = n_units; B.sample0 = F.sample0;
    const unsigned long long n_chunks = ((unsigned long long)n_units + ST_FUSED_CHUNK - 1) / ST_FUSED_CHUNK;
    // one launch for the whole frame — or, for a caller that polls (render_flag, lines_rendered, the live preview of camera.hpp:548-552 /
    // main.cpp:1576), sixteen launches over consecutive parts of the unit range with the poll between them (samples[] was zeroed, so the
    // reduce of a partial frame is the mean of the samples finished so far, as in the pipeline)
    const int parts = (H.keep_going || H.progress) && n_chunks >= 64 ? 16 : 1;
    StreamBuf R = make_buf(nullptr, 0, F.spp, n_units, F.n_pix, F.pixels, F.samples, X.ctl, X.ctl, 0, 0);
    bool cancelled = false;
    int done = 0;
    for (int p = 0; p < parts && !cancelled; p++) {
        B.chunk_lo = (uint32_t)(n_chunks * (unsigned long long)p / (unsigned long long)parts);
        B.chunk_hi = (uint32_t)(n_chunks * (unsigned long long)(p + 1) / (unsigned long long)parts);
        if (B.chunk_hi == B.chunk_lo) continue;
        if ((e = hipMemsetAsync(X.ctl, 0, (ST_MAX_POOLS + 1) * W * sizeof(unsigned int), stream)) != hipSuccess) return e;
        const unsigned long long want_blocks = ((unsigned long long)(B.chunk_hi - B.chunk_lo) + 3) / 4;   // no more waves than chunks
        const dim3 grid((unsigned)(want_blocks < (unsigned long long)blocks ? (want_blocks ? want_blocks : 1) : blocks));
        if (H.timer) H.timer->begin(stream, 1);
        launch_fused(level, F.count, sc.tri_uv_at != 0, grid, sc, *F.cam, *F.env, F.seed, B, X.gctr, fo, stream);
        if (H.timer) H.timer->end(stream, 1);
        done = p + 1;
        if (parts > 1 && p + 1 < parts) {
            if ((e = hipStreamSynchronize(stream)) != hipSuccess) return e;
            if (H.progress && (e = reduce_and_report(*H.progress, (double)(p + 1) / parts, true, F, R, stream)) != hipSuccess) return e;
            if (H.keep_going && *H.keep_going == 0) cancelled = true;
        }
    }
    if (H.timer) H.timer->begin(stream, 3);
    if (F.out) hipLaunchKernelGGL(stream_reduce, dim3((F.n_pix + 3) / 4), dim3(256), 0, stream, R, *F.cam, F.out);
    if (H.timer) H.timer->end(stream, 3);
    if (H.done_out) *H.done_out = cancelled ? -done : done;
    return hipGetLastError();
}

hipError_t launch_accumulate(const double* samples, uint32_t n_pix, uint32_t n, uint32_t sample0, bool flip, double* partial, hipStream_t stream) {
    if (n_pix == 0 || n == 0) return hipSuccess;
    hipLaunchKernelGGL(stream_accumulate, dim3((n_pix + 3) / 4), dim3(256), 0, stream, samples, n_pix, n, sample0, flip ? 1u : 0u, partial);
    return hipGetLastError();
}
hipError_t launch_accum_resolve(const double* partial, const uint32_t* pixels, uint32_t n_pix, int W, int done, int asc_lanes, double* out, hipStream_t stream) {
    if (n_pix == 0) return hipSuccess;
    hipLaunchKernelGGL(accum_resolve, dim3((n_pix + 3) / 4), dim3(256), 0, stream, partial, pixels, n_pix, W, done, asc_lanes, out);
    return hipGetLastError();
}

// closest hits of n rays in [0.001, inf) through the EXTEND kernel; `pool` holds stream_pool_bytes(round_up(n, 64)) bytes
hipError_t stream_trace(const DScene& sc, const double* d_rays, uint32_t n, uint64_t seed, uint64_t pixel, uint32_t bounce, zr_hit* d_out, uint2* d_out_ki, void* pool,
                        const StreamContext& X, int leaf_level) {
    hipStream_t stream = X.streams[0];
    if (n == 0) return hipSuccess;
    const uint32_t P = (n + 63u) / 64u * 64u;
    const size_t W = stream_ctl_words();
    StreamBuf B = make_buf(pool, P, 1, n, n, nullptr, nullptr, X.ctl, X.ctl + (size_t)ST_MAX_POOLS * W, 0, P);
    hipError_t e;
    if ((e = clear_ctl(X.ctl, stream)) != hipSuccess) return e;
    hipLaunchKernelGGL(stream_load_rays, dim3((P + 255) / 256), dim3(256), 0, stream, B, d_rays, n, seed, pixel, bounce);
    const int eb = (int)(P / 64 < (uint32_t)X.extend_blocks ? P / 64 : (uint32_t)X.extend_blocks);
    launch_extend(false, leaf_level, sc, B, X.overflow, X.ovf_levels, eb, X.gctr, stream);
    if (sc.tri_uv_at) hipLaunchKernelGGL(stream_hits_out<true>, dim3((n + 255) / 256), dim3(256), 0, stream, sc, B, n, d_out, d_out_ki);
    else hipLaunchKernelGGL(stream_hits_out<false>, dim3((n + 255) / 256), dim3(256), 0, stream, sc, B, n, d_out, d_out_ki);
    return hipGetLastError();
}

}  // namespace zr
