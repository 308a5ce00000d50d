// zr_round_polls.h — the host's side of the pipeline's round loop (zr_stream.hip: stream_render): the bookkeeping of the polls (RoundPolls) and the loop itself
// (run_round_loop), which reaches the device through an interface only.  No HIP in here: stream_render supplies the HIP device, tests/native/round_polls_check.cpp
// a scripted one, and both run the same loop.
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

// THE ROUND LOOP.  A loop round is EXTEND, SHADE and the round's poll (stream_poll) on every sub-pool's stream.  The host has to learn three things from
// the device: that the pools are empty, that the survivors are few enough for the drain pool, that a wave was capped.
//  - The LAGGED loop (a frame nobody polls: the timed path) keeps lag + 1 rounds in flight and waits for the event behind the OLDEST round's poll only, so a
//    stream never runs dry and one sub-pool's SHADE always has the other's EXTEND beside it.  What it learns is `lag` rounds old: the frame ends with up to
//    `lag` rounds on empty pools, which nobody sees (the round count and the launch log stop at the round that emptied the pools), the drain switch and a
//    capped wave are noticed up to `lag` rounds late.
//  - The CADENCED loop (ZR_STREAM_POLL_LAG=0, and every frame with keep_going or progress: camera::render cancels within two rounds and previews what is
//    finished) enqueues a run of rounds, synchronises every stream and takes the run's polls in order: the newest one says what the pools hold now.
// Both count their rounds in RoundPolls, which also says why a poll's stale count may size the drain pool.
// Measured on cfg3 (profiles/r25_round_loop_ab.txt): the streams were never empty for long (0.55 ms of a frame without any kernel, before and after); what the
// lag buys is the drain switch one round after its condition holds instead of four (the cadenced loop was in a run of 8 rounds when it came true, and each late round walks two
// 52 Mi-slot pools for a few hundred thousand paths): 296.5 against 300.5 ms, lag 0 299.8, lag 2 298.2 (a second queued round on the big pools).
struct RoundLoopPlan {
    bool cadenced; int lag;           // lagged: lag + 1 rounds in flight
    int pools;                        // sub-pools the loop begins on; one after the drain
    uint32_t P, drain_slots;          // slots of all sub-pools together; of the drain pool
    bool drain_allowed;
    int max_run = POLL_RING;          // cadenced: the longest run of rounds between two synchronisations (2 with a progress sink: an interactive caller)
};
struct RoundLoopOutcome {
    int status = 0;        // the device's first status that was not 0: the loop stopped there
    bool runaway = false;  // ... or at its round guard
    int rounds = 0;        // loop rounds the caller sees: up to the one that emptied the pools, or those enqueued when the frame was cancelled
    int drain_round = 0;   // the round behind which the survivors moved to the drain pool (0: never)
    bool emptied = false, capped = false, cancelled = false;
    size_t log_keep = 0;   // emptied: the launches of the log that belong to `rounds`
};
constexpr int ROUND_GUARD = 1 << 22;

// the cadenced loop's next run: the fuller the pools, the longer
inline int next_run(unsigned long long active, uint32_t P, int max_run) {
    const int n = active > P / 2 ? 8 : (active > P / 16 ? 4 : 2);
    return n < max_run ? n : max_run;
}

// Device: what the loop asks of the GPU side.  Every int is an opaque status, 0 = success.
//   int enqueue_round(int slot, int pools, bool with_events, bool units_left)   EXTEND, SHADE and poll into ring slot `slot` on sub-pools [0, pools), an event behind each
//                                                                               poll if asked; units_left: what the newest poll taken says (true before the first)
//   int wait_poll(int slot, int k)  /  int wait_all(int pools)                  until the poll of sub-pool k in `slot` is there / until the streams of [0, pools) are idle
//   const volatile unsigned int* poll_words(int slot, int k)                    that poll's POLL_WORDS words
//   int order_behind(int slot, int pools)                                       stream 0 waits for the events of `slot` on the other streams.  No host wait
//   int compact(uint32_t drain_P, int pools)                                    the survivors of [0, pools) into drain_P slots of the drain pool, on stream 0: sub-pool 0 from now on
//   int report_progress(unsigned long long active)                              cadenced, the streams idle: tell the frame's progress sink, if there is one
//   bool cancelled()  /  size_t launches_logged()
//   void polled(const RoundPolls&, const PollResult&, bool compaction)          a poll has been taken (a trace line; the scripted device's checks)
template <class Device>
PollResult fold_oldest(Device& dev, const RoundPolls& rp) {
    PollResult p;
    const int s = rp.slot(rp.oldest());
    for (int k = 0; k < rp.pools[s]; k++) p.add(dev.poll_words(s, k));
    return p;
}

template <class Device>
RoundLoopOutcome run_round_loop(Device& dev, const RoundLoopPlan& plan) {
    RoundLoopOutcome out;
    RoundPolls rp(plan.cadenced ? POLL_RING : plan.lag + 1);
    int& st = out.status;
    int K = plan.pools;
    bool units_left = true;
    auto enqueue = [&](bool with_events) {
        st = dev.enqueue_round(rp.slot(rp.enqueued + 1), K, with_events, units_left);
        rp.push(K, dev.launches_logged());
    };
    if (!plan.cadenced) {
        for (;;) {
            while (rp.may_enqueue() && st == 0) enqueue(true);
            const int s = rp.slot(rp.oldest());
            for (int k = 0; k < rp.pools[s] && st == 0; k++) st = dev.wait_poll(s, k);
            if (st != 0) return out;
            const PollResult p = fold_oldest(dev, rp);
            const RoundPolls::Action a = rp.take(p, plan.P, plan.drain_slots, plan.drain_allowed);
            units_left = p.units_left;
            dev.polled(rp, p, a.drain);
            if (a.finished) break;
            if (a.drain) {   // stream 0 waits for what the other streams still hold: the event of the newest round stands behind a stream's last queued launch
                if ((st = dev.order_behind(rp.slot(rp.enqueued), K)) != 0 || (st = dev.compact(a.drain_P, K)) != 0) return out;
                K = 1; out.drain_round = rp.enqueued;
            }
            if (rp.enqueued > ROUND_GUARD) { out.runaway = true; return out; }
        }
        // the rounds queued behind the emptying one run on empty pools; the frame's last kernels (stream 0) follow the other streams' share of them
        if ((st = dev.order_behind(rp.slot(rp.enqueued), K)) != 0) return out;
    } else {
        int run = plan.max_run < POLL_RING ? plan.max_run : POLL_RING;
        for (;;) {
            for (int i = 0; i < run && st == 0; i++) enqueue(false);
            if (st != 0 || (st = dev.wait_all(K)) != 0) return out;
            PollResult p;
            RoundPolls::Action a{false, false, 0};
            while (rp.in_flight() > 0) {   // every poll of the run says whether its round emptied the pools; the newest one decides the rest
                p = fold_oldest(dev, rp);
                a = rp.take(p, plan.P, plan.drain_slots, plan.drain_allowed && rp.in_flight() == 1);
                dev.polled(rp, p, a.drain);
            }
            if (rp.emptied != 0) break;
            if ((st = dev.report_progress(p.active)) != 0) return out;
            units_left = p.units_left;
            if (a.drain) {
                if ((st = dev.compact(a.drain_P, K)) != 0 || (st = dev.wait_all(1)) != 0) return out;
                K = 1; out.drain_round = rp.enqueued;
            }
            run = next_run(p.active, plan.P, plan.max_run);
            if (dev.cancelled()) { out.cancelled = true; break; }
            if (rp.enqueued > ROUND_GUARD) { out.runaway = true; return out; }
        }
    }
    out.capped = rp.capped;
    out.emptied = rp.emptied != 0;
    out.rounds = out.emptied ? rp.emptied : rp.enqueued;
    out.log_keep = rp.log_keep();
    return out;
}

}  // namespace zr
