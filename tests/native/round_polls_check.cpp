// round_polls_check.cpp — the pipeline's round loop (raytracer_project_amd/csrc/zr_round_polls.h: run_round_loop, the loop stream_render runs) on its own, no HIP:
// a scripted device says what every round leaves behind and checks, in its callbacks, every step the loop takes against what the script knows.  Also the
// host's count of started work units (zr_units.h) against an enumeration of the hand-out.
//   g++ -std=c++20 -fsanitize=address,undefined -I raytracer_project_amd/csrc tests/native/round_polls_check.cpp && ./a.out
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <utility>
#include <vector>
#include "zr_round_polls.h"
#include "zr_units.h"

using namespace zr;

static int failures = 0;
#define CHECK(c, ...) do { if (!(c)) { failures++; std::printf("FAIL %s:%d (%s): ", __FILE__, __LINE__, #c); std::printf(__VA_ARGS__); std::printf("\n"); } } while (0)

struct Round { unsigned long long active; bool units_left; bool capped; };   // what round r (from 1) leaves, summed over the pools it ran on

struct Outcome { int rounds; size_t launches_kept; int drain_after_round; uint32_t drain_P; bool capped; int enqueued; bool cancelled; std::vector<int> runs; };

// The device of run_round_loop, scripted; `script` must end in a round with active == 0 (or the run in a cancellation).  Rounds past its end are empty.
struct ScriptedDevice {
    const std::vector<Round>& script; const RoundLoopPlan plan; const char* name;
    int cancel_after_runs = 0;   // cadenced: keep_going is cleared once that many runs have been synchronised (0: never)
    struct Slot { bool full = false; int round = 0; bool waited[POLL_RING] = {}; unsigned int words[POLL_RING][POLL_WORDS] = {}; };
    std::vector<Slot> ring;
    std::vector<int> launch_round;   // the launch log: the round of every logged launch
    std::vector<int> runs;           // cadenced: the rounds between two synchronisations
    int ring_slots, pools, enqueued = 0, polled_rounds = 0, synced = 0, ordered_behind = -1, reports = 0;
    int first_true = 0;      // the first poll the switch may be decided from whose drain condition holds
    int decided_at = 0, drain_after = 0;
    uint32_t drain_P = 0;
    bool newest_units_left = true, said_cancelled = false;

    ScriptedDevice(const std::vector<Round>& s, const RoundLoopPlan& p, const char* n)
        : script(s), plan(p), name(n), ring_slots(p.cadenced ? POLL_RING : p.lag + 1), pools(p.pools) { ring.resize((size_t)ring_slots); }
    Round at(int r) const { return r <= (int)script.size() ? script[(size_t)r - 1] : Round{0, false, false}; }

    int enqueue_round(int s, int n_pools, bool with_events, bool units_left) {
        const int r = ++enqueued;
        CHECK(!said_cancelled, "%s: round %d enqueued after the cancellation", name, r);
        CHECK(n_pools == pools, "%s: round %d on %d pools, the frame is on %d", name, r, n_pools, pools);
        CHECK(with_events == !plan.cadenced, "%s: round %d %s events", name, r, with_events ? "with" : "without");
        CHECK(units_left == newest_units_left, "%s: round %d told units_left %d, the newest poll taken said %d", name, r, (int)units_left, (int)newest_units_left);
        CHECK(s == r % ring_slots, "%s: round %d in slot %d", name, r, s);
        CHECK(!ring[(size_t)s].full, "%s: round %d overwrites the unread poll of round %d", name, r, ring[(size_t)s].round);
        ring[(size_t)s] = Slot{}; ring[(size_t)s].full = true; ring[(size_t)s].round = r;
        const Round d = at(r);   // the device "runs" the round: pool 0 carries the remainder, so that the fold is exercised
        for (int k = 0; k < n_pools; k++) {
            launch_round.push_back(r);
            unsigned int* w = ring[(size_t)s].words[k];
            w[POLL_ACTIVE] = (unsigned int)(d.active / (unsigned)n_pools + (k == 0 ? d.active % (unsigned)n_pools : 0));
            w[POLL_CAPPED] = d.capped && k == n_pools - 1; w[POLL_UNITS_LEFT] = d.units_left && k == 0;
        }
        if (!plan.cadenced) CHECK(enqueued - polled_rounds <= plan.lag + 1, "%s: %d rounds in flight", name, enqueued - polled_rounds);
        return 0;
    }
    int wait_poll(int s, int k) {
        CHECK(!plan.cadenced, "%s: the cadenced loop waits for a single poll", name);
        CHECK(ring[(size_t)s].full && ring[(size_t)s].round == polled_rounds + 1, "%s: slot %d holds round %d, wanted %d", name, s, ring[(size_t)s].round, polled_rounds + 1);
        ring[(size_t)s].waited[k] = true;
        return 0;
    }
    int wait_all(int n_pools) {
        CHECK(plan.cadenced, "%s: the lagged loop synchronises the streams", name);
        CHECK(n_pools == pools, "%s: %d streams synchronised, the frame is on %d", name, n_pools, pools);
        if (enqueued > synced) runs.push_back(enqueued - synced);
        synced = enqueued;
        return 0;
    }
    const volatile unsigned int* poll_words(int s, int k) {
        const Slot& sl = ring[(size_t)s];
        CHECK(sl.full && sl.round == polled_rounds + 1, "%s: slot %d holds round %d, wanted %d", name, s, sl.round, polled_rounds + 1);
        CHECK(plan.cadenced ? sl.round <= synced : sl.waited[k], "%s: the poll of round %d, pool %d is read before it is there", name, sl.round, k);
        return sl.words[k];
    }
    void polled(const RoundPolls& rp, const PollResult& p, bool compaction) {
        const int q = ++polled_rounds, s = rp.slot(q);
        CHECK(rp.polled == q, "%s: poll %d taken as %d", name, q, rp.polled);
        CHECK(ring[(size_t)s].full && ring[(size_t)s].round == q, "%s: slot %d holds round %d, wanted %d", name, s, ring[(size_t)s].round, q);
        ring[(size_t)s].full = false;
        CHECK(p.active == at(q).active && p.units_left == at(q).units_left && p.capped == at(q).capped, "%s: poll of round %d folded wrongly", name, q);
        newest_units_left = p.units_left;
        const bool decides = !plan.cadenced || rp.in_flight() == 0;   // the cadenced loop decides from the newest poll of a run
        if (first_true == 0 && decides && p.active != 0 && drain_condition(p, plan.P, plan.drain_slots)) first_true = q;
        if (compaction) {
            CHECK(plan.drain_allowed, "%s: a compaction without a drain pool", name);
            CHECK(decided_at == 0, "%s: a second compaction", name);
            CHECK(q == first_true, "%s: the switch was decided at poll %d, the condition held from poll %d", name, q, first_true);
            decided_at = q;
        }
    }
    int order_behind(int s, int n_pools) {
        CHECK(!plan.cadenced, "%s: the cadenced loop orders streams by events", name);
        CHECK(s == enqueued % ring_slots && n_pools == pools, "%s: stream 0 ordered behind slot %d of %d pools, the newest round %d is on %d", name, s, n_pools, enqueued, pools);
        ordered_behind = enqueued;
        return 0;
    }
    int compact(uint32_t to_P, int n_pools) {
        CHECK(drain_after == 0, "%s: a second compaction", name);
        CHECK(decided_at != 0 && n_pools == pools, "%s: compaction of %d pools (the frame is on %d), decided at poll %d", name, n_pools, pools, decided_at);
        CHECK(plan.cadenced ? synced == enqueued : ordered_behind == enqueued, "%s: the compaction is not behind round %d on every stream", name, enqueued);
        drain_after = enqueued; drain_P = to_P; pools = 1;
        CHECK(drain_after - decided_at <= (plan.cadenced ? 0 : plan.lag), "%s: compaction %d rounds behind its poll", name, drain_after - decided_at);
        // the bound: what is active when the compaction runs (after the newest queued round) fits the pool sized from the older poll
        CHECK(at(drain_after).active <= (unsigned long long)drain_P, "%s: %llu survivors, drain pool of %u", name, at(drain_after).active, drain_P);
        CHECK(drain_P % 256u == 0 && drain_P >= 256u && drain_P <= plan.drain_slots, "%s: drain pool of %u slots (limit %u)", name, drain_P, plan.drain_slots);
        return 0;
    }
    int report_progress(unsigned long long active) {
        CHECK(plan.cadenced && synced == enqueued, "%s: progress asked for with rounds in flight", name);
        CHECK(active != 0 && active == at(enqueued).active, "%s: progress with %llu active, round %d left %llu", name, active, enqueued, at(enqueued).active);
        reports++;
        return 0;
    }
    bool cancelled() { return said_cancelled = cancel_after_runs != 0 && (int)runs.size() >= cancel_after_runs; }
    size_t launches_logged() const { return launch_round.size(); }

    Outcome run() {
        const RoundLoopOutcome o = run_round_loop(*this, plan);
        CHECK(o.status == 0 && !o.runaway, "%s: status %d, runaway %d", name, o.status, (int)o.runaway);
        CHECK(o.drain_round == drain_after, "%s: drain round %d, the compaction came behind round %d", name, o.drain_round, drain_after);
        CHECK(o.cancelled == said_cancelled && o.emptied != o.cancelled, "%s: cancelled %d, emptied %d", name, (int)o.cancelled, (int)o.emptied);
        if (!plan.cadenced) CHECK(ordered_behind == enqueued, "%s: the frame's last kernels are not ordered behind round %d", name, enqueued);
        if (plan.cadenced && !o.cancelled) CHECK(reports == (int)runs.size() - 1, "%s: %d progress reports for %zu runs (every run but the emptying one)", name, reports, runs.size());
        if (o.emptied) {
            size_t kept = 0;
            for (int r : launch_round) if (r <= o.rounds) kept++;
            CHECK(o.log_keep == kept, "%s: log_keep %zu, launches of the rounds seen %zu", name, o.log_keep, kept);
            for (size_t i = 0; i < o.log_keep && i < launch_round.size(); i++) CHECK(launch_round[i] <= o.rounds, "%s: a kept launch of round %d", name, launch_round[i]);
        }
        return Outcome{o.rounds, o.log_keep, drain_after, drain_P, o.capped, enqueued, o.cancelled, runs};
    }
};

static Outcome run_lagged(const std::vector<Round>& script, int lag, int pools0, uint32_t P, uint32_t drain_slots, bool drain_allowed, const char* name) {
    RoundLoopPlan plan{false, lag, pools0, P, drain_slots, drain_allowed};
    return ScriptedDevice(script, plan, name).run();
}

// max_run: POLL_RING for a frame without a progress sink, 2 with one
static Outcome run_cadenced(const std::vector<Round>& script, int max_run, int pools, uint32_t P, uint32_t drain_slots, bool drain_allowed, const char* name, int cancel_after_runs = 0) {
    RoundLoopPlan plan{true, 0, pools, P, drain_slots, drain_allowed, max_run};
    ScriptedDevice dev(script, plan, name);
    dev.cancel_after_runs = cancel_after_runs;
    return dev.run();
}

// the units started, by enumeration: shard s has dealt the first P / ST_SHARDS + dealt[s] units of its sequence, those beyond the frame included
static unsigned long long started_by_enumeration(uint32_t G, uint32_t P, uint32_t n_units, const std::vector<unsigned int>& dealt, size_t stride) {
    unsigned long long n = 0;
    for (uint32_t sh = 0; sh < ST_SHARDS; sh++)
        for (unsigned long long k = 0; k < (unsigned long long)(P / ST_SHARDS) + dealt[stride * sh]; k++)
            if (st_unit_of(G, P, sh, k) < (unsigned long long)n_units) n++;
    return n;
}

static void check_units_started() {
    const uint32_t P = ST_SHARDS * 256;   // the smallest pool the affine hand-out accepts
    const uint32_t beyond = 3 * P + 77;   // affine, chunks of 256: the fourth chunk of the shard at position 0 is cut at 77 units, every other shard's lies beyond the frame
    for (size_t stride : {(size_t)1, (size_t)32})
        for (int pattern = 0; pattern < 3; pattern++) {
            std::vector<unsigned int> dealt(stride * ST_SHARDS, 0xDEADu);   // (the words between the counters are not the function's to read)
            unsigned long long sum = 0;
            for (uint32_t sh = 0; sh < ST_SHARDS; sh++) { dealt[stride * sh] = pattern == 0 ? 0u : (pattern == 1 ? (sh * 37u + 5u) % 300u : 700u + (sh * 53u) % 400u); sum += dealt[stride * sh]; }
            for (uint32_t n_units : {3u, 21u, P, P + 1u, beyond}) {
                for (uint32_t G : {1u, 3u, 256u}) {
                    const unsigned long long got = units_started(G, P, n_units, dealt.data(), stride), want = started_by_enumeration(G, P, n_units, dealt, stride);
                    CHECK(got == want, "units_started affine G %u, n_units %u, pattern %d, stride %zu: %llu, enumeration %llu", G, n_units, pattern, stride, got, want);
                }
                const unsigned long long got = units_started(0, P, n_units, dealt.data(), stride), want = std::min<unsigned long long>(P + sum, n_units);
                CHECK(got == want, "units_started striped, n_units %u, pattern %d, stride %zu: %llu, wanted %llu", n_units, pattern, stride, got, want);
            }
        }
    // st_first_unit deals the first P units of a pool to its slots: what the enumeration above takes for granted
    for (uint32_t G : {0u, 1u, 3u, 256u}) {
        std::vector<unsigned char> seen(P, 0);
        for (uint32_t g = 0; g < P; g++) {
            const unsigned long long u = st_first_unit(G, g);
            const uint32_t sh = (g >> 8) % ST_SHARDS;
            if (G != 0) CHECK(u == st_unit_of(G, P, sh, g & 255u), "st_first_unit G %u slot %u", G, g);
            if (u < P) seen[(size_t)u]++;
        }
        if (G == 0 || G == 1 || G == 256) for (uint32_t u = 0; u < P; u++) if (seen[u] != 1) { CHECK(false, "G %u: unit %u starts in %d slots", G, u, (int)seen[u]); break; }
    }
}

int main() {
    const uint32_t P = 65536, drain_slots = P / 16 / 256 * 256 + 256;   // (zr_render.cpp: size_slot_pool)
    CHECK(RoundPolls(0).ring == 1 && RoundPolls(99).ring == POLL_RING, "ring is not clamped");
    CHECK(POLL_MAX_LAG + 1 <= POLL_RING, "the ring cannot hold the longest lag");
    // the drain condition itself, at its edges
    {
        PollResult p; p.active = P / 16; p.units_left = false;
        CHECK(drain_condition(p, P, drain_slots), "active * 16 == P must switch");
        p.active = P / 16 + 1; CHECK(!drain_condition(p, P, drain_slots), "active * 16 > P must not switch");
        p.active = 100; p.units_left = true; CHECK(!drain_condition(p, P, drain_slots), "units left must not switch");
        p.units_left = false; CHECK(!drain_condition(p, P, 64), "more survivors than the drain pool holds must not switch");
        CHECK(drain_pool_slots(1) == 256 && drain_pool_slots(256) == 256 && drain_pool_slots(257) == 512, "drain pool rounding");
    }
    for (int lag = 0; lag <= 2; lag++) {
        for (int pools = 1; pools <= 3; pools++) {
            char name[64];
            // empty at round 1
            std::snprintf(name, sizeof name, "empty-at-1 lag %d pools %d", lag, pools);
            Outcome o = run_lagged({{0, false, false}}, lag, pools, P, drain_slots, true, name);
            CHECK(o.rounds == 1 && o.launches_kept == (size_t)pools && o.enqueued == 1 + lag && o.drain_after_round == 0, "%s: rounds %d, kept %zu, enqueued %d", name, o.rounds, o.launches_kept, o.enqueued);
            // empty exactly at a ring wrap: round lag + 1 is the last of the first lap, round 2 * (lag + 1) of the second
            for (int laps = 1; laps <= 2; laps++) {
                const int n = laps * (lag + 1);
                std::vector<Round> s;
                for (int r = 1; r < n; r++) s.push_back({50000, true, false});
                s.push_back({0, false, false});
                std::snprintf(name, sizeof name, "empty-at-wrap %d lag %d pools %d", n, lag, pools);
                o = run_lagged(s, lag, pools, P, drain_slots, true, name);
                CHECK(o.rounds == n && o.launches_kept == (size_t)(n * pools) && o.enqueued == n + lag && o.drain_after_round == 0, "%s: rounds %d, kept %zu, enqueued %d", name, o.rounds, o.launches_kept, o.enqueued);
                // ... and one round past it
                s.back() = {50000, true, false}; s.push_back({0, false, false});
                o = run_lagged(s, lag, pools, P, drain_slots, true, name);
                CHECK(o.rounds == n + 1 && o.enqueued == n + 1 + lag, "%s + 1: rounds %d, enqueued %d", name, o.rounds, o.enqueued);
            }
            // the drain condition true for one poll only: the next poll shows the pools empty
            std::snprintf(name, sizeof name, "drain-one-poll lag %d pools %d", lag, pools);
            o = run_lagged({{60000, true, false}, {30000, false, false}, {4000, false, false}, {0, false, false}}, lag, pools, P, drain_slots, true, name);
            CHECK(o.rounds == 4 && o.drain_after_round == 3 + lag && o.drain_P == 4096, "%s: rounds %d, drain after %d into %u", name, o.rounds, o.drain_after_round, o.drain_P);
            CHECK(o.launches_kept == (size_t)(pools * 3 + (lag == 0 ? 1 : pools)), "%s: kept %zu", name, o.launches_kept);
            // a long tail: the switch comes once, from the first poll that allows it, and the pool sized from that poll holds the later, smaller count
            std::snprintf(name, sizeof name, "drain-tail lag %d pools %d", lag, pools);
            o = run_lagged({{65000, true, false}, {9000, false, false}, {4090, false, false}, {4000, false, false}, {900, false, false}, {30, false, false}, {2, false, false}, {0, false, false}},
                           lag, pools, P, drain_slots, true, name);
            CHECK(o.rounds == 8 && o.drain_after_round == 3 + lag && o.drain_P == 4096, "%s: rounds %d, drain after %d into %u", name, o.rounds, o.drain_after_round, o.drain_P);
            // no drain pool: never
            o = run_lagged({{65000, true, false}, {900, false, false}, {0, false, false}}, lag, pools, P, drain_slots, false, name);
            CHECK(o.rounds == 3 && o.drain_after_round == 0, "%s without a drain pool: rounds %d, drain after %d", name, o.rounds, o.drain_after_round);
            // a capped wave is seen whichever round it comes from, the emptying one and the rounds behind it included
            for (int at_round = 1; at_round <= 3; at_round++) {
                std::vector<Round> s = {{65000, true, false}, {900, false, false}, {0, false, false}};
                s[(size_t)at_round - 1].capped = true;
                std::snprintf(name, sizeof name, "capped-at-%d lag %d pools %d", at_round, lag, pools);
                o = run_lagged(s, lag, pools, P, drain_slots, true, name);
                CHECK(o.capped && o.rounds == 3, "%s: capped %d, rounds %d", name, (int)o.capped, o.rounds);
            }
        }
    }
    // the cadenced loop: the round count stops at the emptying round wherever in a run of check_every rounds that is (the pools stay more than half full, so
    // every run is as long as the loop allows)
    for (int check_every : {1, 2, 4, 8})
        for (int empty_at = 1; empty_at <= 17; empty_at++) {
            std::vector<Round> s;
            for (int r = 1; r < empty_at; r++) s.push_back({P, false, false});
            s.push_back({0, false, false});
            char name[64]; std::snprintf(name, sizeof name, "cadenced every %d empty at %d", check_every, empty_at);
            const Outcome o = run_cadenced(s, check_every, 2, P, 4096, false, name);
            CHECK(o.rounds == empty_at && o.launches_kept == (size_t)(2 * empty_at) && o.enqueued == (empty_at + check_every - 1) / check_every * check_every, "%s: rounds %d, kept %zu, enqueued %d", name,
                  o.rounds, o.launches_kept, o.enqueued);
        }
    // the cadenced loop's drain switch, decided from the newest poll of a run; with a progress sink (runs of 2) and without (a first run of 8, then by `active`)
    for (int max_run : {2, POLL_RING})
        for (int pools = 1; pools <= 3; pools++) {
            char name[64];
            std::vector<Round> lead;   // eight rounds, a whole number of runs whatever max_run: units are left; the last one leaves few active, so runs of 2 follow
            for (int r = 0; r < 7; r++) lead.push_back({60000, true, false});
            lead.push_back({4000, true, false});
            auto with = [&](std::initializer_list<Round> tail) { std::vector<Round> s = lead; s.insert(s.end(), tail); return s; };
            // active at P / 16 exactly: the switch, once, and the rounds behind it on one pool
            std::snprintf(name, sizeof name, "cadenced drain at P/16, max run %d pools %d", max_run, pools);
            Outcome o = run_cadenced(with({{5000, false, false}, {P / 16, false, false}, {4000, false, false}, {3000, false, false}, {100, false, false}, {0, false, false}}), max_run, pools, P, drain_slots, true, name);
            CHECK(o.rounds == 14 && o.drain_after_round == 10 && o.drain_P == 4096 && o.enqueued == 14, "%s: rounds %d, drain after %d into %u, enqueued %d", name, o.rounds, o.drain_after_round, o.drain_P, o.enqueued);
            CHECK(o.launches_kept == (size_t)(10 * pools + 4), "%s: kept %zu launches", name, o.launches_kept);
            // at P / 16 + 1 it does not switch (and a run of 4 follows where the loop may: its newest poll is the emptying one); two rounds later it may
            std::snprintf(name, sizeof name, "cadenced no drain at P/16 + 1, max run %d pools %d", max_run, pools);
            o = run_cadenced(with({{5000, false, false}, {P / 16 + 1, false, false}, {4097, false, false}, {P / 16 + 1, false, false}, {4000, false, false}, {0, false, false}}), max_run, pools, P, drain_slots, true, name);
            CHECK(o.rounds == 14 && o.drain_after_round == 0 && o.launches_kept == (size_t)(14 * pools), "%s: rounds %d, drain after %d, kept %zu", name, o.rounds, o.drain_after_round, o.launches_kept);
            o = run_cadenced(with({{5000, false, false}, {P / 16 + 1, false, false}, {4097, false, false}, {4000, false, false}, {100, false, false}, {0, false, false}}), max_run, pools, P, drain_slots, true, name);
            CHECK(o.rounds == 14 && o.drain_after_round == (max_run == 2 ? 12 : 0) && o.drain_P == (max_run == 2 ? 4096u : 0u), "%s, then 4000: rounds %d, drain after %d into %u", name, o.rounds, o.drain_after_round, o.drain_P);
            // units left: no switch, however few are active
            std::snprintf(name, sizeof name, "cadenced units left, max run %d pools %d", max_run, pools);
            o = run_cadenced(with({{500, true, false}, {400, true, false}, {300, true, false}, {0, false, false}}), max_run, pools, P, drain_slots, true, name);
            CHECK(o.rounds == 12 && o.drain_after_round == 0, "%s: rounds %d, drain after %d", name, o.rounds, o.drain_after_round);
            // more survivors than the drain pool holds: no switch until they fit
            std::snprintf(name, sizeof name, "cadenced small drain pool, max run %d pools %d", max_run, pools);
            o = run_cadenced(with({{300, false, false}, {257, false, false}, {257, false, false}, {0, false, false}}), max_run, pools, P, 256, true, name);
            CHECK(o.rounds == 12 && o.drain_after_round == 0, "%s: rounds %d, drain after %d", name, o.rounds, o.drain_after_round);
            o = run_cadenced(with({{300, false, false}, {256, false, false}, {200, false, false}, {0, false, false}}), max_run, pools, P, 256, true, name);
            CHECK(o.rounds == 12 && o.drain_after_round == 10 && o.drain_P == 256, "%s, then 256: rounds %d, drain after %d into %u", name, o.rounds, o.drain_after_round, o.drain_P);
            // no drain pool: never
            std::snprintf(name, sizeof name, "cadenced without a drain pool, max run %d pools %d", max_run, pools);
            o = run_cadenced(with({{5000, false, false}, {4000, false, false}, {100, false, false}, {0, false, false}}), max_run, pools, P, drain_slots, false, name);
            CHECK(o.rounds == 12 && o.drain_after_round == 0 && o.launches_kept == (size_t)(12 * pools), "%s: rounds %d, drain after %d", name, o.rounds, o.drain_after_round);
            // a capped wave, in any round of a run (the emptying one and the rounds behind it in its run included)
            for (int at_round = 1; at_round <= 12; at_round++) {
                std::vector<Round> s = with({{0, false, false}, {0, false, false}, {0, false, false}, {0, false, false}});
                s[(size_t)at_round - 1].capped = true;
                std::snprintf(name, sizeof name, "cadenced capped-at-%d max run %d pools %d", at_round, max_run, pools);
                o = run_cadenced(s, max_run, pools, P, drain_slots, true, name);
                CHECK(o.capped == (at_round <= 10) && o.rounds == 9 && o.enqueued == 10, "%s: capped %d, rounds %d, enqueued %d", name, (int)o.capped, o.rounds, o.enqueued);
            }
            // cancelled after the first run: the rounds enqueued so far, and no further round (the device checks that)
            std::snprintf(name, sizeof name, "cadenced cancelled, max run %d pools %d", max_run, pools);
            o = run_cadenced(lead, max_run, pools, P, drain_slots, true, name, 1);
            CHECK(o.cancelled && o.rounds == max_run && o.enqueued == max_run && o.runs.size() == 1, "%s: cancelled %d, rounds %d, enqueued %d", name, (int)o.cancelled, o.rounds, o.enqueued);
        }
    // the runs of the cadenced loop: 8 rounds first, then 8 / 4 / 2 by what is active against P / 2 and P / 16; 2 throughout with a progress sink
    for (int max_run : {2, POLL_RING})
        for (const auto& [active, want] : std::vector<std::pair<unsigned long long, int>>{{P / 2 + 1, 8}, {P / 2, 4}, {P / 16 + 1, 4}, {P / 16, 2}}) {
            std::vector<Round> s;
            for (int r = 1; r <= 20; r++) s.push_back({active, true, false});
            s.push_back({0, false, false});
            char name[64]; std::snprintf(name, sizeof name, "runs with %llu active, max run %d", active, max_run);
            const Outcome o = run_cadenced(s, max_run, 2, P, drain_slots, true, name);
            std::vector<int> runs;
            for (int n = 0; n < 21; n += runs.back()) runs.push_back(max_run == 2 ? 2 : (n == 0 ? 8 : want));
            CHECK(o.runs == runs && o.rounds == 21, "%s: %zu runs (wanted %zu) of %d ... %d rounds, %d rounds seen", name, o.runs.size(), runs.size(), o.runs.front(), o.runs.back(), o.rounds);
            CHECK(next_run(active, P, POLL_RING) == want && next_run(active, P, 2) == 2, "%s: next_run", name);
        }
    check_units_started();
    if (failures) { std::printf("%d failure(s)\n", failures); return 1; }
    std::printf("round polls: ok\n");
    return 0;
}
