// Host-only check of the launch plans' edge pass (stablediffusion-pytorch_amd/csrc/plan_edges.h), built with
// -fsanitize=address,undefined and run by tests/test_plan_edges_cpu.py.
//   * hand-written op lists, one per rule, with the exact counters the pass must report;
//   * a seeded random check: for every list, the happens-before relation over the ops that do work (launches,
//     all-reduces, callouts -- a callout is work on every stream), computed by a small stream / event simulator
//     from the compiled list, equals the one computed from the recorded list. Three replays are unrolled, so waits
//     that refer to the previous replay's record (carried-over edges) are part of the relation.
// Usage: edges_check [lists] [seed]
#include <bitset>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

#include "plan_edges.h"

using namespace sdmi_edges;

namespace {

struct Builder {
  std::vector<Rec> recs;
  int next_owned = 1000;  // ids handed to plan-owned events, made dense by finish()
  void launch(int s) { recs.push_back(Rec{LAUNCH, s, -1, false}); }
  void allreduce(int s) { recs.push_back(Rec{ALLREDUCE, s, -1, false}); }
  void callout() { recs.push_back(Rec{CALLOUT, -1, -1, false}); }
  void record(int e, int s) { recs.push_back(Rec{EVENT, s, e, false}); }
  void wait(int d, int e) { recs.push_back(Rec{WAIT, d, e, false}); }
  void edge(int src, int dst) {  // what sdmi_plan_note_edge records
    recs.push_back(Rec{EVENT, src, next_owned, true});
    recs.push_back(Rec{WAIT, dst, next_owned, true});
    ++next_owned;
  }
  std::vector<Rec> finish() {
    std::vector<int> ids;
    for (Rec& r : recs) {
      if (r.event < 0) continue;
      size_t k = 0;
      while (k < ids.size() && ids[k] != r.event) ++k;
      if (k == ids.size()) ids.push_back(r.event);
      r.event = (int)k;
    }
    return recs;
  }
};

int g_fail = 0;

void expect(const char* name, const std::vector<Rec>& recs, bool fold, int compiled, int folded, int aliased,
            int dropped, int owned) {
  const Result r = compile(recs, fold);
  const Stats& s = r.stats;
  const bool ok = s.recorded == (int)recs.size() && s.compiled == compiled && s.folded == folded &&
                  s.aliased == aliased && s.waits_dropped == dropped && s.owned_events == owned &&
                  (int)r.ops.size() == compiled;
  if (!ok) {
    ++g_fail;
    std::printf("FAIL %s (fold %d): compiled %d folded %d aliased %d dropped %d owned %d, expected %d %d %d %d %d\n",
                name, (int)fold, s.compiled, s.folded, s.aliased, s.waits_dropped, s.owned_events, compiled, folded,
                aliased, dropped, owned);
  }
}

// ---- the simulator: what each work op is ordered after --------------------------------------------------------
constexpr int kMaxOps = 40, kMaxStreams = 4, kReplays = 3;
constexpr int kNodes = kMaxOps * kMaxStreams * kReplays;
typedef std::bitset<kNodes> Set;

struct ExecOp {
  int kind, stream, event, stop, src;
};

std::vector<Set> simulate(const std::vector<ExecOp>& list, int n, int S, int E) {
  std::vector<Set> pred(kNodes);
  std::vector<Set> dep(S), evset(E);
  for (int rep = 0; rep < kReplays; ++rep) {
    for (const ExecOp& op : list) {
      switch (op.kind) {
        case LAUNCH:
        case ALLREDUCE: {
          const int id = (rep * n + op.src) * kMaxStreams;
          pred[id] = dep[op.stream];
          dep[op.stream].set(id);
          if (op.stop >= 0) evset[op.stop] = dep[op.stream];
          break;
        }
        case CALLOUT:
          for (int s = 0; s < S; ++s) {
            const int id = (rep * n + op.src) * kMaxStreams + s;
            pred[id] = dep[s];
            dep[s].set(id);
          }
          break;
        case EVENT: evset[op.event] = dep[op.stream]; break;
        case WAIT: dep[op.stream] |= evset[op.event]; break;
      }
    }
  }
  return pred;
}

bool same_relation(const std::vector<Rec>& recs, bool fold) {
  const int n = (int)recs.size();
  int S = 1, E = 1;
  for (const Rec& r : recs) {
    S = std::max(S, r.stream + 1);
    E = std::max(E, r.event + 1);
  }
  std::vector<ExecOp> a, b;
  for (int i = 0; i < n; ++i) a.push_back(ExecOp{recs[i].kind, recs[i].stream, recs[i].event, -1, i});
  const Result res = compile(recs, fold);
  int work_a = 0, work_b = 0;
  for (const Rec& r : recs) work_a += r.kind == LAUNCH || r.kind == ALLREDUCE || r.kind == CALLOUT;
  for (const COp& c : res.ops) {
    const Rec& r = recs[c.src];
    const bool launch = r.kind == LAUNCH;
    work_b += r.kind == LAUNCH || r.kind == ALLREDUCE || r.kind == CALLOUT;
    b.push_back(ExecOp{r.kind, r.stream, launch ? -1 : c.event, launch ? c.event : -1, c.src});
  }
  if (work_a != work_b) return false;  // every work op is issued, once
  for (size_t k = 1; k < res.ops.size(); ++k)
    if (res.ops[k].src <= res.ops[k - 1].src) return false;  // in recorded order
  return simulate(a, n, S, E) == simulate(b, n, S, E);
}

std::vector<Rec> random_list(std::mt19937& g) {
  Builder b;
  const int S = 1 + (int)(g() % kMaxStreams), P = 1 + (int)(g() % 5), n = 4 + (int)(g() % (kMaxOps - 3));
  while ((int)b.recs.size() < n) {
    const int roll = (int)(g() % 100), s = (int)(g() % S), d = (int)(g() % S), e = (int)(g() % P);
    if (roll < 34) b.launch(s);
    else if (roll < 37) b.allreduce(s);
    else if (roll < 41) b.callout();
    else if (roll < 54) b.record(e, s);
    else if (roll < 72) b.wait(d, e);
    else if ((int)b.recs.size() + 2 <= n) b.edge(s, d);
  }
  return b.finish();
}

}  // namespace

int main(int argc, char** argv) {
  const int lists = argc > 1 ? std::atoi(argv[1]) : 4000;
  const unsigned seed = argc > 2 ? (unsigned)std::atoi(argv[2]) : 20240611u;
  {  // duplicate record: two private edges off stream 0 with nothing on it in between
    Builder b;
    b.launch(0); b.edge(0, 1); b.edge(0, 2); b.launch(1); b.launch(2);
    const std::vector<Rec> r = b.finish();
    expect("duplicate record", r, false, 6, 0, 1, 0, 2);
    expect("duplicate record", r, true, 5, 1, 1, 0, 2);
    const Result res = compile(r, false);
    if (res.system_fence[0] != 0 || res.fate[3] != ALIASED || res.ops[3].event != 0) {
      ++g_fail;
      std::printf("FAIL duplicate record: alias target / fence flags\n");
    }
  }
  {  // a launch between the two records: no alias
    Builder b;
    b.launch(0); b.edge(0, 1); b.launch(0); b.edge(0, 2); b.launch(1); b.launch(2);
    expect("record after work", b.finish(), false, 8, 0, 0, 0, 2);
  }
  {  // a wait on the recording stream between the two records changes what the second captures: no alias
    Builder b;
    b.launch(0); b.launch(3); b.record(0, 3); b.edge(0, 1); b.wait(0, 0); b.edge(0, 2); b.launch(1); b.launch(2);
    expect("record after wait", b.finish(), false, 10, 0, 0, 0, 2);
  }
  {  // doubled wait
    Builder b;
    b.launch(1); b.record(0, 1); b.wait(0, 0); b.wait(0, 0); b.launch(0);
    expect("doubled wait", b.finish(), false, 4, 0, 0, 1, 0);
  }
  {  // a wait already implied transitively: 0 waits on 1 after 1 waited on 2
    Builder b;
    b.launch(2); b.record(0, 2); b.wait(1, 0); b.launch(1); b.record(1, 1); b.wait(0, 1); b.wait(0, 0); b.launch(0);
    expect("transitive wait", b.finish(), false, 7, 0, 0, 1, 0);
  }
  {  // cluster of k = 6 waits from two side streams collapses to one per source stream
    Builder b;
    for (int i = 0; i < 6; ++i) { b.launch(1 + i % 2); b.record(i, 1 + i % 2); }
    for (int i = 0; i < 6; ++i) b.wait(0, i);
    b.launch(0);
    expect("wait cluster", b.finish(), false, 15, 0, 0, 4, 0);
    expect("wait cluster", b.finish(), true, 9, 6, 0, 4, 0);
  }
  {  // the same waits with a launch of the waiting stream between them are no cluster
    Builder b;
    for (int i = 0; i < 4; ++i) { b.launch(1); b.record(i, 1); }
    for (int i = 0; i < 4; ++i) { b.wait(0, i); b.launch(0); }
    expect("waits apart", b.finish(), false, 16, 0, 0, 0, 0);
  }
  {  // carried-over wait (the event is recorded later in plan order: the previous replay's record) is kept,
     // even though stream 0 already knows everything stream 1 has issued in this replay
    Builder b;
    b.launch(1); b.edge(1, 0); b.wait(0, 0); b.launch(0); b.launch(1); b.record(0, 1);
    expect("carried-over wait kept", b.finish(), false, 7, 0, 0, 0, 1);
  }
  {  // two carried-over waits in a row on events of one source stream: only the later record's wait stays
    Builder b;
    b.wait(0, 0); b.wait(0, 1); b.launch(0); b.launch(1); b.record(0, 1); b.launch(1); b.record(1, 1);
    expect("carried-over pair", b.finish(), false, 6, 0, 0, 1, 0);
  }
  {  // ... but not when their records are on different streams
    Builder b;
    b.wait(0, 0); b.wait(0, 1); b.launch(0); b.launch(1); b.record(0, 1); b.launch(2); b.record(1, 2);
    expect("carried-over, two sources", b.finish(), false, 7, 0, 0, 0, 0);
  }
  {  // a callout between two private records blocks aliasing (and keeps every system-scope fence)
    Builder b;
    b.launch(0); b.edge(0, 1); b.callout(); b.edge(0, 2); b.launch(1); b.launch(2);
    const std::vector<Rec> r = b.finish();
    expect("callout blocks alias", r, false, 8, 0, 0, 0, 2);
    const Result res = compile(r, false);
    if (res.system_fence[0] != 1 || res.system_fence[1] != 1) {
      ++g_fail;
      std::printf("FAIL callout keeps fences\n");
    }
  }
  {  // a callout makes a caller's event opaque: the doubled wait behind it stays
    Builder b;
    b.launch(1); b.record(0, 1); b.wait(0, 0); b.callout(); b.wait(0, 0); b.launch(0);
    expect("callout blocks dominated wait", b.finish(), false, 6, 0, 0, 0, 0);
  }
  {  // fold only directly behind a launch
    Builder a, b, c, d, e;
    a.launch(0); a.record(0, 0); a.wait(1, 0); a.launch(1);
    expect("fold", a.finish(), true, 3, 1, 0, 0, 0);
    expect("fold off", a.finish(), false, 4, 0, 0, 0, 0);
    b.launch(1); b.record(1, 1); b.launch(0); b.wait(0, 1); b.record(0, 0);
    expect("no fold behind a wait", b.finish(), true, 4, 1, 0, 0, 0);  // (only stream 1's record folds)
    c.launch(0); c.callout(); c.record(0, 0);
    expect("no fold across a callout", c.finish(), true, 3, 0, 0, 0, 0);
    d.launch(0); d.wait(1, 0); d.record(0, 0); d.launch(1);
    expect("no fold past a carried-over wait", d.finish(), true, 4, 0, 0, 0, 0);
    e.allreduce(0); e.record(0, 0);
    expect("no fold behind an all-reduce", e.finish(), true, 2, 0, 0, 0, 0);
  }
  {  // a private edge into a stream that carries an all-reduce keeps its system-scope fence, the others drop it
    Builder b;
    b.launch(0); b.edge(0, 1); b.allreduce(1); b.launch(0); b.edge(0, 2); b.launch(2);
    const Result res = compile(b.finish(), true);
    if (res.system_fence[0] != 1 || res.system_fence[1] != 0) {
      ++g_fail;
      std::printf("FAIL all-reduce consumer keeps the fence\n");
    }
  }
  std::mt19937 g(seed);
  int bad = 0;
  long recorded = 0, compiled = 0;
  for (int i = 0; i < lists; ++i) {
    const std::vector<Rec> r = random_list(g);
    for (int fold = 0; fold < 2; ++fold) {
      if (!same_relation(r, fold != 0)) {
        if (++bad <= 3) {
          std::printf("FAIL relation differs (list %d, fold %d):", i, fold);
          for (const Rec& x : r) std::printf(" %d/%d/%d%s", x.kind, x.stream, x.event, x.owned ? "o" : "");
          std::printf("\n");
        }
      }
    }
    recorded += (long)r.size();
    compiled += compile(r, true).stats.compiled;
  }
  g_fail += bad;
  std::printf("%d random lists: %ld recorded ops -> %ld compiled, %d with a different relation\n", lists, recorded,
              compiled, bad);
  std::printf(g_fail ? "FAILED %d\n" : "ok\n", g_fail);
  return g_fail ? 1 : 0;
}
