// zr_units.h — how the pipeline's work units (one per primary sample) are dealt to the slots (zr_stream.hip).  No HIP in here: the kernels and the host's progress
// figure share these functions, and tests/native/round_polls_check.cpp checks the host's against them.
#pragma once
#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define ZR_UNITS_HD __host__ __device__
#else
#define ZR_UNITS_HD
#endif

namespace zr {

#define ST_SHARDS 64     /* sharded counters of the control block (zr_stream.hip: CTL_*): a single contended word sustains only ~90 atomics/us */

// Which unit is the k-th of shard `shard`.
//  striped (G = 0): unit_base + k * ST_SHARDS + shard — every shard sweeps the whole frame, one unit in ST_SHARDS.
//  affine  (G > 0): the frame's units (pixel list in tile order x spp) are cut into chunks of G units and chunk c belongs to
//    the shard at position c % ST_SHARDS of a round; within its chunks a shard deals consecutive units.  A shard is served by
//    the SHADE blocks and the EXTEND waves with blockIdx % ST_SHARDS == shard, i.e. by ONE XCD class (blocks b and b + 8 share
//    an XCD: MI355X_MICROARCH.md, workgroup dispatch), and position (shard % 8) * 8 + shard / 8 puts the eight shards of a class
//    side by side: at any time an XCD's L2 sees the rays of ~8 neighbouring chunks (screen tiles) instead of every 64th unit of
//    a front that spans the frame.  The image cannot depend on it: samples[unit] is written once, by whichever slot got the unit.
ZR_UNITS_HD inline unsigned long long st_unit_of(uint32_t G, uint32_t unit_base, uint32_t shard, unsigned long long k) {
    if (G == 0) return (unsigned long long)unit_base + k * ST_SHARDS + shard;
    const uint32_t k32 = (uint32_t)k, q = k32 / G, r = k32 - q * G;
    const uint32_t pos = (shard & 7u) * (ST_SHARDS / 8u) + (shard >> 3);
    return ((unsigned long long)q * ST_SHARDS + pos) * G + r;
}
// the unit slot g (index over all sub-pools) starts on
ZR_UNITS_HD inline unsigned long long st_first_unit(uint32_t G, uint32_t g) {
    if (G == 0) return g;
    const uint32_t c = g >> 8;
    return st_unit_of(G, 0, c % ST_SHARDS, (unsigned long long)(c / ST_SHARDS) * 256u + (g & 255u));
}

// The units of a frame that have been started on a pool of P slots: the first P are dealt at initialisation (st_first_unit), the rest through the sharded counters,
// dealt[stride * s] by shard s.  Host only (the round loop's progress fraction).
//  striped: P + the counters' sum, at most n_units (a shard counts the units it asked for beyond the frame's end too).
//  affine:  of a shard's sequence (its P / ST_SHARDS initial units, then the dealt ones), the units that exist: a shard's last chunks may lie beyond the frame.
inline unsigned long long units_started(uint32_t G, uint32_t P, uint32_t n_units, const unsigned int* dealt, size_t stride) {
    unsigned long long started = 0;
    if (G == 0) { started = P; for (uint32_t sh = 0; sh < ST_SHARDS; sh++) started += dealt[stride * sh]; }
    else for (uint32_t sh = 0; sh < ST_SHARDS; sh++) {
        const unsigned long long k_sh = (unsigned long long)(P / ST_SHARDS) + dealt[stride * sh];
        const uint32_t pos = (sh & 7u) * (ST_SHARDS / 8u) + (sh >> 3);
        const unsigned long long full = k_sh / G, part = k_sh % G;
        for (unsigned long long q = 0; q <= full; q++) {
            const unsigned long long c0 = (q * ST_SHARDS + pos) * G, len = q < full ? G : part;
            if (c0 < n_units) started += c0 + len <= n_units ? len : n_units - c0;
        }
    }
    return started > n_units ? n_units : started;
}

}  // namespace zr
