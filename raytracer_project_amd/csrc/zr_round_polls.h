// zr_round_polls.h — the host's bookkeeping of the round loop's polls (zr_stream.hip: stream_render).  No HIP in here: tests/native/round_polls_check.cpp drives it
// alone, with scripted poll results.
//
// A POLL of loop round r is what a sub-pool's stream writes to pinned host memory after round r's SHADE (stream_poll): the slots that SHADE left active, whether an
// EXTEND wave hit its iteration cap, whether any shard still has a work unit to hand out; an event recorded behind it says when it is there.  The polls of the
// rounds in flight live in a ring: round r (counted from 1) uses slot r % ring.  The lagged loop keeps `lag + 1` rounds in flight (ring = lag + 1) and waits for
// the oldest one only, so a stream always holds a queued round; the cadenced loop (polled frames, lag 0) enqueues up to POLL_RING rounds and then drains.
#pragma once
#include <stddef.h>
#include <stdint.h>

namespace zr {

constexpr int POLL_RING = 8;      // ring slots the context owns per sub-pool: the cadenced loop's longest run of rounds between two drains
constexpr int POLL_MAX_LAG = 3;   // ZR_STREAM_POLL_LAG is clamped to this
enum { POLL_ACTIVE = 0, POLL_CAPPED = 1, POLL_UNITS_LEFT = 2, POLL_WORDS = 4 };   // words of one sub-pool's poll

struct PollResult {   // one round's polls, folded over the sub-pools it ran on
    unsigned long long active = 0;
    bool units_left = false, capped = false;
    void add(const volatile unsigned int* w) { active += w[POLL_ACTIVE]; capped = capped || w[POLL_CAPPED] != 0; units_left = units_left || w[POLL_UNITS_LEFT] != 0; }
};

// When the survivors move to the drain pool (stream_compact).  WHY A STALE `active` STILL SIZES THAT POOL: a slot becomes active only when SHADE starts a new work
// unit in it, and the unit counters only grow.  A sub-pool's poll reads the counters after that sub-pool's own SHADE of round r, so once it says that no shard has
// a unit left, no later SHADE of that sub-pool can start one: its active count can only fall from round r on.  The condition asks this of every sub-pool's own
// poll, so the sum polled for round r bounds the slots that are active when the compaction runs, however many rounds later that is.
inline bool drain_condition(const PollResult& p, uint32_t P, uint32_t drain_slots) {
    return !p.units_left && p.active * 16ull <= (unsigned long long)P && p.active <= (unsigned long long)drain_slots;
}
inline uint32_t drain_pool_slots(unsigned long long active) { return (uint32_t)((active + 255ull) / 256ull * 256ull); }

struct RoundPolls {
    struct Action { bool finished, drain; uint32_t drain_P; };
    int ring;                          // slots in use (<= POLL_RING)
    int enqueued = 0, polled = 0;      // loop rounds enqueued / whose poll has been taken; rounds are counted from 1
    int emptied = 0;                   // the round whose poll first showed no active slot (0: none yet)
    bool capped = false, drained = false;
    int pools[POLL_RING] = {};         // per slot: the sub-pools the round ran on
    size_t log_mark[POLL_RING] = {};   // per slot: launches logged up to and including the round

    explicit RoundPolls(int ring_slots) : ring(ring_slots < 1 ? 1 : (ring_slots > POLL_RING ? POLL_RING : ring_slots)) {}
    int slot(int round) const { return round % ring; }
    int in_flight() const { return enqueued - polled; }
    bool may_enqueue() const { return emptied == 0 && in_flight() < ring; }
    int oldest() const { return polled + 1; }
    // a round has been enqueued on `n_pools` sub-pools, and the launch log holds `mark` launches behind it; returns its ring slot
    int push(int n_pools, size_t mark) {
        const int s = slot(++enqueued);
        pools[s] = n_pools; log_mark[s] = mark;
        return s;
    }
    // the poll of round oldest() is here: what follows from it
    Action take(const PollResult& p, uint32_t P, uint32_t drain_slots, bool drain_allowed) {
        ++polled;
        Action a{false, false, 0};
        if (p.capped) capped = true;
        if (emptied != 0) return a;   // (a round behind the emptying one: it ran on an empty pool)
        if (p.active == 0) { emptied = polled; a.finished = true; return a; }
        if (!drained && drain_allowed && drain_condition(p, P, drain_slots)) { drained = true; a.drain = true; a.drain_P = drain_pool_slots(p.active); }
        return a;
    }
    // the rounds the caller sees, and the launches of the log that belong to them (meaningful once a poll has emptied the pools)
    int rounds_done() const { return emptied != 0 ? emptied : polled; }
    size_t log_keep() const { return log_mark[slot(rounds_done())]; }
};

}  // namespace zr
