// Host-side bookkeeping of the scan lanes that one-query-per-call traffic rotates over (dense_single_enqueue and
// hybrid_lane_enqueue, api.hip) -- no HIP in this file; host_slots.hpp is its sibling for the host-pointer ring.
// Consecutive queries take consecutive lanes.  A lane owns per_lane = kPipeSlots / lanes list sets and four back-pressure
// events; anrag_index::ScanLane (common.hpp) keeps its stream, the events themselves and the merge still pending.  Here:
// which lane and set the next query takes, which event the host waits for before the set is overwritten, which event to
// record behind the query's launches.
//
// INVARIANT.  A lane's queries -- its "launches": one scan for a dense single, scan + K3 + tail for a hybrid one -- are
// numbered from 0 since the last drain (reset).  With every = per_lane / 4, event m is recorded behind launch
// (m + 1) * every - 1, into slot m % 4.  Launch ls writes set ls % per_lane, whose previous user was launch
// ls - per_lane.  A hybrid query reads its lists in its own launch (its tail); a dense single's merge rides in the NEXT
// launch of the lane, ls - per_lane + 1.  The event to wait for is the first one recorded at or behind that later launch:
// m = ceil((ls - per_lane + 2) / every) - 1.  It has been recorded, because (m + 1) * every - 1 <= ls - per_lane + every
// <= ls - 1 (per_lane = 4 * every), and its slot still holds it, because event m + 4 comes behind launch
// (m + 5) * every - 1 >= ls + 1.  No wait while ls < per_lane: the set has had no user since the drain.
// tests/native/scan_lanes_model.cpp checks exactly this against a fake device (tests/test_scan_lanes_cpu.py).
#pragma once
#include <cstdint>

namespace anrag {

constexpr int kPipeSlots = 32;     // queries in flight in the hybrid pipeline (list sets, events): four exchange
                                   // groups of 8, so a slow collective on the communication stream (which the tails
                                   // queue behind) does not stall the scans two groups later
constexpr int kScanLanesMax = 4;   // scan streams that single queries rotate over (api.hip)

struct ScanLanes {
    bool active = false;                 // a run of single queries owns the list sets
    int in_use = 1;                      // lanes of the current run: 1 (big corpora), 2 or 4
    int per_lane = kPipeSlots, every = kPipeSlots / 4;  // list sets per lane, launches per event: set by activate
    uint64_t rr = 0;                     // queries of the run: the next one takes lane rr % in_use
    uint64_t count[kScanLanesMax] = {};  // launches per lane since the last drain
    struct Ticket { int lane, set, wait_ev; };  // wait_ev: the lane's event (0..3) to wait for before the set is written, or -1
    // start a run of single queries (the caller has drained whatever else used the list sets); a no-op inside a run
    void activate(int n_lanes, bool one_lane) {
        if (active) return;
        active = true;
        rr = 0;
        in_use = one_lane ? 1 : n_lanes;
        per_lane = kPipeSlots / in_use;
        every = per_lane / 4;
    }
    int peek() const { return (int)(rr % (uint64_t)in_use); }  // the lane the next query will take
    Ticket acquire() {
        const int l = peek();
        ++rr;
        const int64_t ls = (int64_t)count[l], pl = per_lane, ev = every;
        return Ticket{l, (int)(l * pl + ls % pl), ls < pl ? -1 : (int)(((ls - pl + 2 + ev - 1) / ev - 1) % 4)};
    }
    // behind the launches of the lane's query: the event (0..3) to record after them, or -1
    int commit(int lane) {
        const uint64_t n = ++count[lane], ev = (uint64_t)every;
        return n % ev == 0 ? (int)((n / ev - 1) % 4) : -1;
    }
    void reset() {  // the lanes' streams are drained (sync_all)
        active = false;
        for (uint64_t &c : count) c = 0;
    }
};

}  // namespace anrag
