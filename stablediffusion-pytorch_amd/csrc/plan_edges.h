// Edge pass of the launch plans (plan.hip): compiles the recorded op list of a step into the list the replay issues,
// with fewer event records and stream waits and the same happens-before relation between the ops that do work
// (launches, all-reduces, callouts). Plain C++ over {kind, stream id, event id} records: no HIP, so the rules are
// compiled and tested on the CPU (tests/plan_edges/edges_check.cpp).
//
// Model. An event record on stream s captures everything s is ordered after at that point: its own work so far and,
// transitively, whatever its earlier waits brought in. A wait on d orders d's LATER ops after that capture. The pass
// keeps, per stream, a vector clock over (stream, number of work ops issued on it) of what the stream's next op is
// already ordered after, and per event the clock its latest record captured. The clocks start at zero with every
// replay; component s of a capture is 1 + the work ops s has issued in this replay, the 1 standing for everything s
// ran in earlier replays (stream order carries it along), which a zero clock does not know either. A kept wait on a
// carried-over or opaque event (below) orders its stream after work the clocks cannot name: it bumps a second,
// per-stream component, so that a later record on that stream is never taken for a copy of an earlier one.
//
// Rules (each keeps the relation exactly: nothing is lost and nothing is added):
//   * duplicate record: a plan-owned event recorded on s directly behind another plan-owned record on s (no op of any
//     kind on s and no callout in between) captures the same clock: it aliases to the earlier event and is not issued;
//   * folded record: a record on s whose previous op on s is a launch is issued with that launch (its stop event)
//     when the caller asks for folding -- unless a wait on the event, another record of it or a callout sits between
//     the two in plan order (the wait would see the new record instead of the one it was issued against, the other
//     record would no longer be overwritten by this one);
//   * dominated wait: a wait whose event's capture is already covered by the waiting stream's clock is dropped;
//   * wait cluster: among the waits a stream issues with no op of its own (and no callout) in between, a wait whose
//     capture a LATER wait of the cluster covers is dropped (29 waits -> one per source stream).
// Conservatism:
//   * a callout is work on every stream, and Python may record or wait on any event that is not plan-owned inside it:
//     after a callout every such event is opaque (its waits are kept and teach the clock nothing) until the plan
//     records it again;
//   * a wait on an event the plan has not recorded yet in this replay refers to the PREVIOUS replay's last record of
//     it (the forward waiting on the last step's optimizer chunks). It is never dropped on current-replay knowledge,
//     only against another carried-over wait of the same stream whose event's last record is on the same source
//     stream and later in plan order. An event the plan never records is opaque.
#pragma once
#include <algorithm>
#include <vector>

namespace sdmi_edges {

enum Kind { LAUNCH = 0, EVENT = 1, WAIT = 2, CALLOUT = 3, ALLREDUCE = 4 };
enum Fate { KEPT = 0, FOLDED = 1, ALIASED = 2, DROPPED = 3 };

struct Rec {
  int kind;
  int stream;  // dense stream id; -1 for callouts
  int event;   // dense event id for EVENT / WAIT, else -1
  bool owned;  // EVENT / WAIT: the event is plan-owned (a private edge: never visible outside the plan)
};

struct COp {
  int src;    // index of the recorded op this compiled op issues
  int event;  // EVENT / WAIT: the event id to use (after aliasing); LAUNCH: the event it stops with, or -1
};

struct Stats {
  int recorded = 0, compiled = 0, folded = 0, aliased = 0, waits_dropped = 0, owned_events = 0;
};

struct Result {
  std::vector<COp> ops;
  std::vector<int> fate;          // per recorded op (Fate)
  std::vector<char> system_fence; // per event id: 1 = keep default (system-scope) flags
  Stats stats;
};

inline Result compile(const std::vector<Rec>& recs, bool fold) {
  const int n = (int)recs.size();
  int S = 0, E = 0;
  bool any_callout = false;
  for (const Rec& r : recs) {
    S = std::max(S, r.stream + 1);
    E = std::max(E, r.event + 1);
    any_callout |= r.kind == CALLOUT;
  }
  Result out;
  out.fate.assign(n, KEPT);
  out.stats.recorded = n;
  std::vector<char> owned(E, 0), has_allreduce(S, 0);
  std::vector<int> last_rec(E, -1);  // plan index of the event's last record
  for (int i = 0; i < n; ++i) {
    const Rec& r = recs[i];
    if (r.kind == EVENT) last_rec[r.event] = i;
    if ((r.kind == EVENT || r.kind == WAIT) && r.owned) owned[r.event] = 1;
    if (r.kind == ALLREDUCE) has_allreduce[r.stream] = 1;
  }
  for (int e = 0; e < E; ++e) out.stats.owned_events += owned[e];

  typedef std::vector<int> Clock;
  enum EvState { CARRIED = 0, VALID = 1, OPAQUE = 2 };
  std::vector<int> cnt(S, 0);                 // work ops issued on each stream (a callout counts on all)
  std::vector<Clock> clock(S, Clock(2 * S, 0));  // what the stream's next op is ordered after (S + s: unknowns)
  std::vector<Clock> snap(E);                 // capture of the event's latest record (state VALID)
  std::vector<int> state(E, CARRIED), alias(E);
  for (int e = 0; e < E; ++e) {
    alias[e] = e;
    if (last_rec[e] < 0) state[e] = OPAQUE;   // recorded outside the plan only
  }
  struct Pending {  // a kept wait of the stream's open cluster
    int cidx;       // its index in the compiled list
    Clock cap;      // VALID: the capture it waited for
    int src, ord;   // CARRIED: source stream and plan index of the event's last record; src -1 otherwise
  };
  std::vector<std::vector<Pending>> cluster(S);
  std::vector<int> dup_event(S, -1);          // plan-owned event recorded on s with no op on s (or callout) since
  std::vector<int> last_op(S, -1);            // recorded index of the last op on s
  std::vector<int> last_wait(E, -1);          // recorded index of the last wait on the event
  std::vector<int> last_seen_rec(E, -1);      // recorded index of the last record of the event so far
  std::vector<std::vector<int>> carried(S, std::vector<int>(S, -1));  // per (waiter, source): latest carried record
  std::vector<std::vector<char>> consumers(E, std::vector<char>(S, 0));
  int last_callout = -1;
  std::vector<char> dead;                     // per compiled op: dropped by a later wait of its cluster

  auto emit = [&](int src, int event) {
    out.ops.push_back(COp{src, event});
    dead.push_back(0);
    return (int)out.ops.size() - 1;
  };
  std::vector<int> cidx_of(n, -1);

  for (int i = 0; i < n; ++i) {
    const Rec& r = recs[i];
    switch (r.kind) {
      case LAUNCH:
      case ALLREDUCE:
        ++cnt[r.stream];
        cluster[r.stream].clear();
        dup_event[r.stream] = -1;
        cidx_of[i] = emit(i, -1);
        break;
      case CALLOUT:
        for (int s = 0; s < S; ++s) {
          ++cnt[s];
          cluster[s].clear();
          dup_event[s] = -1;
          std::fill(carried[s].begin(), carried[s].end(), -1);
        }
        for (int e = 0; e < E; ++e)
          if (!owned[e]) state[e] = OPAQUE;
        last_callout = i;
        emit(i, -1);
        break;
      case EVENT: {
        const int s = r.stream, e = r.event;
        cluster[s].clear();  // the record captures the waits issued so far: they stay
        if (owned[e] && dup_event[s] >= 0) {
          alias[e] = dup_event[s];
          out.fate[i] = ALIASED;
          ++out.stats.aliased;
          break;
        }
        alias[e] = e;
        snap[e] = clock[s];
        snap[e][s] = cnt[s] + 1;
        state[e] = VALID;
        const int j = last_op[s];
        if (fold && j >= 0 && recs[j].kind == LAUNCH && out.ops[cidx_of[j]].event < 0 && last_wait[e] < j &&
            last_seen_rec[e] < j && last_callout < j) {
          out.ops[cidx_of[j]].event = e;
          out.fate[i] = FOLDED;
          ++out.stats.folded;
        } else {
          emit(i, e);
        }
        last_seen_rec[e] = i;
        dup_event[s] = owned[e] ? e : -1;
        break;
      }
      case WAIT: {
        const int d = r.stream, e = alias[r.event];
        last_wait[r.event] = i;
        last_wait[e] = i;
        consumers[e][d] = 1;
        dup_event[d] = -1;
        Pending p;
        p.src = -1;
        p.ord = -1;
        bool drop = false;
        if (state[e] == VALID) {
          const Clock& cap = snap[e];
          bool covered = true;
          for (int s = 0; s < 2 * S && covered; ++s) covered = cap[s] <= (s == d ? cnt[d] + 1 : clock[d][s]);
          if (covered) {
            drop = true;
          } else {
            for (int s = 0; s < 2 * S; ++s) clock[d][s] = std::max(clock[d][s], cap[s]);
            for (Pending& q : cluster[d]) {
              if (q.cap.empty() || dead[q.cidx]) continue;
              bool le = true;
              for (int s = 0; s < 2 * S && le; ++s) le = q.cap[s] <= cap[s];
              if (le) dead[q.cidx] = 1;
            }
            p.cap = cap;
          }
        } else if (state[e] == CARRIED) {
          const int src = recs[last_rec[e]].stream, ord = last_rec[e];
          if (carried[d][src] >= ord) {
            drop = true;
          } else {
            carried[d][src] = ord;
            for (Pending& q : cluster[d])
              if (q.src == src && q.ord <= ord && !dead[q.cidx]) dead[q.cidx] = 1;
            p.src = src;
            p.ord = ord;
          }
        }
        if (drop) {
          out.fate[i] = DROPPED;
          ++out.stats.waits_dropped;
        } else {
          if (state[e] != VALID) ++clock[d][S + d];  // d is now ordered after something the clocks cannot name
          p.cidx = emit(i, e);
          cluster[d].push_back(p);
        }
        break;
      }
    }
    if (r.stream >= 0) last_op[r.stream] = i;
  }
  // compact: waits a later wait of their cluster made redundant
  std::vector<COp> kept;
  kept.reserve(out.ops.size());
  for (size_t c = 0; c < out.ops.size(); ++c) {
    if (dead[c]) {
      out.fate[out.ops[c].src] = DROPPED;
      ++out.stats.waits_dropped;
    } else {
      kept.push_back(out.ops[c]);
    }
  }
  out.ops.swap(kept);
  out.stats.compiled = (int)out.ops.size();
  // a plan-owned event may drop the system-scope fence of its record unless a stream that waits on it carries an
  // all-reduce or the plan has a callout (work the plan cannot see, possibly read by the host or a peer device)
  out.system_fence.assign(E, 1);
  for (int e = 0; e < E; ++e) {
    if (!owned[e] || any_callout) continue;
    bool fence = false;
    for (int s = 0; s < S; ++s) fence |= consumers[e][s] && has_allreduce[s];
    out.system_fence[e] = fence ? 1 : 0;
  }
  return out;
}

}  // namespace sdmi_edges
