// Native launch plans: a training step recorded once and re-issued from C++.
//
// While a plan records (sdmi_plan_begin .. sdmi_plan_end) the step runs for real; every kernel launch of the library
// (launch.h) is appended with its marshalled arguments, and the host layer notes the stream / event edges it issues
// (sdmi_plan_note_event / sdmi_plan_note_wait) and the points where it must run something the library does not
// own -- an RCCL collective, a torch copy -- as numbered callouts (sdmi_plan_note_callout). sdmi_plan_replay then
// re-issues the ops in recorded order, same pointers, grids and streams, until the next callout (returned to the
// caller, who runs it and resumes) or the end. Per launch this costs one hipLaunchKernel: no Python, no ctypes
// marshalling, no GEMM planning (split / tile choice, descriptor validation) on the replay path.
#include <hip/hip_ext.h>

#include <cstdlib>
#include <cstring>
#include <map>
#include <memory>
#include <new>
#include <vector>

#include "../../include/sdmi.h"
#include "launch.h"
#include "plan_edges.h"

namespace sdmi_rt {

void* g_recording = nullptr;

namespace {

enum OpKind { OP_LAUNCH = 0, OP_EVENT = 1, OP_WAIT = 2, OP_CALLOUT = 3, OP_ALLREDUCE = 4 };

struct alignas(16) Chunk16 {
  unsigned char b[16];
};

struct Op {
  int kind;
  const void* fn = nullptr;
  dim3 grid, block;
  unsigned shmem = 0;
  hipStream_t stream = nullptr;
  hipEvent_t event = nullptr;  // the caller's handle; nullptr for a plan-owned event (sdmi_plan_note_edge)
  int eid = -1;                // OP_EVENT / OP_WAIT: dense event id inside the plan
  int callout = -1;
  void* comm = nullptr;  // OP_ALLREDUCE: communicator, buffer, element count, dtype (0 fp32, 1 bf16)
  void* buf = nullptr;
  size_t count = 0;
  int dtype = 0;
  std::vector<Chunk16> args;   // copy of the argument tuple (16-B aligned)
  std::vector<unsigned> offs;  // byte offset of each argument inside it
};

// one op of the compiled list (plan_edges.h): the recorded op it issues and the event it uses -- for a launch the
// event folded into it (recorded at the kernel's end through hipExtLaunchKernel's stop event), or nullptr
struct CompiledOp {
  int src;
  hipEvent_t event;
};

struct Plan {
  std::vector<Op> ops;
  int launches = 0;
  std::vector<void*> scratch;  // argument pointer array reused by replay
  std::map<hipEvent_t, int> event_ids;  // caller's handle -> dense id
  int nevents = 0;
  std::vector<char> owned;              // per event id: plan-owned
  // Plan-owned events. `plain` (hipEventDisableTiming, what torch creates) serves the verbatim replay; `fast` the
  // compiled one, without the system-scope fence where plan_edges.h allows it. Neither has been recorded when the
  // first replay starts; a wait on a never-recorded event is a no-op, and no compiled wait precedes its event's
  // record anyway (an edge's record directly precedes its wait). The caller synchronises the device after recording
  // (sdmi.plan.StepPlan), so nothing of the recording run is still in flight then.
  std::vector<hipEvent_t> plain, fast;
  std::vector<CompiledOp> compiled[2];  // [0] records folded into their producers, [1] not folded
  std::vector<int> fate;                // per recorded op, of the default compiled list (sdmi_edges::Fate)
  sdmi_edges::Stats stats;
  int mode = 1;                         // the edge mode of the replay in progress (taken at start == 0)

  ~Plan() {
    for (hipEvent_t e : plain)
      if (e) (void)hipEventDestroy(e);
    for (hipEvent_t e : fast)
      if (e) (void)hipEventDestroy(e);
  }
};

// Process-wide edge mode (sdmi_plan_set_edges): 0 replays the recorded list verbatim, 1 the compiled list,
// 2 the compiled list with no record folded into its producer (diagnostic).
// Starts from the environment (SDMI_PLAN_EDGES = 0 / 1 / 2), so that a whole bench run can be A/B'd unchanged.
int initial_edges() {
  const char* v = getenv("SDMI_PLAN_EDGES");
  return v && v[0] >= '0' && v[0] <= '2' && !v[1] ? v[0] - '0' : 1;
}
int g_edges = initial_edges();
// which compiled list mode 1 replays: 0 = records folded into their producing launch, 1 = not folded
// (what the edge-cost probe measured)
constexpr int kDefaultList = 0;

int event_id(Plan* p, hipEvent_t ev) {
  auto it = p->event_ids.find(ev);
  if (it != p->event_ids.end()) return it->second;
  p->event_ids[ev] = p->nevents;
  p->owned.push_back(0);
  return p->nevents++;
}

hipEvent_t handle(const Plan* p, const Op& op, bool fast) {
  return op.event ? op.event : (fast ? p->fast : p->plain)[op.eid];
}

// run the edge pass over the recorded list and create the plan-owned events
int compile_plan(Plan* p) {
  std::map<hipStream_t, int> sid;
  std::vector<sdmi_edges::Rec> recs;
  recs.reserve(p->ops.size());
  for (const Op& op : p->ops) {
    sdmi_edges::Rec r;
    r.kind = op.kind;
    r.stream = -1;
    if (op.kind != OP_CALLOUT) r.stream = sid.emplace(op.stream, (int)sid.size()).first->second;
    r.event = op.eid;
    r.owned = op.eid >= 0 && p->owned[op.eid];
    recs.push_back(r);
  }
  p->plain.assign(p->nevents, nullptr);
  p->fast.assign(p->nevents, nullptr);
  for (int v = 0; v < 2; ++v) {
    const sdmi_edges::Result res = sdmi_edges::compile(recs, v == 0);
    if (v == 0) {
      for (int e = 0; e < p->nevents; ++e) {
        if (!p->owned[e]) continue;
        const unsigned flags = hipEventDisableTiming | (res.system_fence[e] ? 0u : (unsigned)hipEventDisableSystemFence);
        if (hipEventCreateWithFlags(&p->plain[e], hipEventDisableTiming) != hipSuccess) return -3;
        if (hipEventCreateWithFlags(&p->fast[e], flags) != hipSuccess) return -3;
      }
    }
    if (v == kDefaultList) {
      p->fate = res.fate;
      p->stats = res.stats;
    }
    std::vector<Op*> by_event(p->nevents, nullptr);  // any recorded op naming the event: resolves its handle
    for (Op& op : p->ops)
      if (op.eid >= 0) by_event[op.eid] = &op;
    for (const sdmi_edges::COp& c : res.ops) {
      CompiledOp co{c.src, nullptr};
      if (c.event >= 0) co.event = handle(p, *by_event[c.event], true);
      p->compiled[v].push_back(co);
    }
  }
  return 0;
}

}  // namespace

void record_launch(const void* fn, dim3 grid, dim3 block, unsigned shmem, hipStream_t stream, const void* args,
                   size_t bytes, const unsigned* offsets, int nargs) {
  Plan* p = (Plan*)g_recording;
  Op op;
  op.kind = OP_LAUNCH;
  op.fn = fn;
  op.grid = grid;
  op.block = block;
  op.shmem = shmem;
  op.stream = stream;
  op.args.resize((bytes + 15) / 16);
  if (bytes) memcpy(op.args.data(), args, bytes);
  op.offs.assign(offsets, offsets + nargs);
  if ((int)p->scratch.size() < nargs) p->scratch.resize(nargs);
  p->ops.push_back(std::move(op));
  ++p->launches;
}

void record_allreduce(void* comm, void* buf, size_t count, int dtype, hipStream_t stream) {
  Plan* p = (Plan*)g_recording;
  Op op;
  op.kind = OP_ALLREDUCE;
  op.comm = comm;
  op.buf = buf;
  op.count = count;
  op.dtype = dtype;
  op.stream = stream;
  p->ops.push_back(std::move(op));
}

}  // namespace sdmi_rt

using sdmi_rt::Plan;

extern "C" int sdmi_plan_begin(void) {
  if (sdmi_rt::g_recording) return -1;  // not re-entrant
  sdmi_rt::g_recording = new (std::nothrow) Plan();
  return sdmi_rt::g_recording ? 0 : -2;
}

extern "C" int sdmi_plan_end(void** plan) {
  if (!plan || !sdmi_rt::g_recording) return -1;
  *plan = sdmi_rt::g_recording;
  sdmi_rt::g_recording = nullptr;
  return sdmi_rt::compile_plan((Plan*)*plan);
}

extern "C" int sdmi_plan_recording(void) { return sdmi_rt::g_recording != nullptr; }

extern "C" int sdmi_plan_note_event(void* event, sdmi_stream_t stream) {
  Plan* p = (Plan*)sdmi_rt::g_recording;
  if (!p) return 0;
  if (!event) return -1;
  sdmi_rt::Op op;
  op.kind = sdmi_rt::OP_EVENT;
  op.event = (hipEvent_t)event;
  op.eid = sdmi_rt::event_id(p, op.event);
  op.stream = (hipStream_t)stream;
  p->ops.push_back(std::move(op));
  return 0;
}

extern "C" int sdmi_plan_note_wait(sdmi_stream_t stream, void* event) {
  Plan* p = (Plan*)sdmi_rt::g_recording;
  if (!p) return 0;
  if (!event) return -1;
  sdmi_rt::Op op;
  op.kind = sdmi_rt::OP_WAIT;
  op.event = (hipEvent_t)event;
  op.eid = sdmi_rt::event_id(p, op.event);
  op.stream = (hipStream_t)stream;
  p->ops.push_back(std::move(op));
  return 0;
}

// A private edge: dst waits for everything issued so far on src, through an event only the plan ever sees (the
// caller has already issued the edge itself for the recording run). Recorded as an event record on src and a wait on
// dst, on an event the plan creates and owns.
extern "C" int sdmi_plan_note_edge(sdmi_stream_t src, sdmi_stream_t dst) {
  Plan* p = (Plan*)sdmi_rt::g_recording;
  if (!p) return 0;
  const int eid = p->nevents++;
  p->owned.push_back(1);
  sdmi_rt::Op rec, wait;
  rec.kind = sdmi_rt::OP_EVENT;
  rec.stream = (hipStream_t)src;
  wait.kind = sdmi_rt::OP_WAIT;
  wait.stream = (hipStream_t)dst;
  rec.eid = wait.eid = eid;
  p->ops.push_back(std::move(rec));
  p->ops.push_back(std::move(wait));
  return 0;
}

extern "C" int sdmi_plan_note_callout(int id) {
  Plan* p = (Plan*)sdmi_rt::g_recording;
  if (!p) return 0;
  sdmi_rt::Op op;
  op.kind = sdmi_rt::OP_CALLOUT;
  op.callout = id;
  p->ops.push_back(std::move(op));
  return 0;
}

extern "C" int sdmi_plan_info(const void* plan, int* ops, int* launches) {
  const Plan* p = (const Plan*)plan;
  if (!p) return -1;
  if (ops) *ops = (int)p->ops.size();
  if (launches) *launches = p->launches;
  return 0;
}

// what the edge pass made of the recorded list: recorded ops, ops of the compiled list, records folded into their
// producing launch, records aliased to an earlier one, waits dropped, plan-owned events
extern "C" int sdmi_plan_edge_info(const void* plan, int* recorded, int* compiled, int* folded, int* aliased,
                                   int* waits_dropped, int* owned_events) {
  const Plan* p = (const Plan*)plan;
  if (!p) return -1;
  if (recorded) *recorded = p->stats.recorded;
  if (compiled) *compiled = p->stats.compiled;
  if (folded) *folded = p->stats.folded;
  if (aliased) *aliased = p->stats.aliased;
  if (waits_dropped) *waits_dropped = p->stats.waits_dropped;
  if (owned_events) *owned_events = p->stats.owned_events;
  return 0;
}

// recorded op i, if an event record or a stream wait: the event's dense id inside the plan, whether the plan owns it,
// and what the compiled list does with the op (0 kept, 1 folded into its producer, 2 aliased, 3 dropped)
extern "C" int sdmi_plan_op_edge(const void* plan, int i, int* event, int* owned, int* fate) {
  const Plan* p = (const Plan*)plan;
  if (!p || i < 0 || i >= (int)p->ops.size()) return -1;
  const sdmi_rt::Op& op = p->ops[i];
  if (op.eid < 0) return -2;
  if (event) *event = op.eid;
  if (owned) *owned = p->owned[op.eid];
  if (fate) *fate = p->fate[i];
  return 0;
}

extern "C" int sdmi_plan_set_edges(int mode) {
  if (mode < 0 || mode > 2) return -1;
  sdmi_rt::g_edges = mode;
  return 0;
}

// `start` / `next` index the list being replayed (the recorded one in edge mode 0, else the compiled one): opaque to
// the caller, who passes 0 first and then whatever `next` returned. The mode is taken when a replay starts.
extern "C" int sdmi_plan_replay(void* plan, int start, int* callout, int* next) {
  Plan* p = (Plan*)plan;
  if (!p || start < 0 || !callout || !next) return -1;
  if (start == 0) p->mode = sdmi_rt::g_edges;
  void** ptrs = p->scratch.data();
  const bool verbatim = p->mode == 0;
  const std::vector<sdmi_rt::CompiledOp>& list = p->compiled[p->mode == 2 ? 1 : sdmi_rt::kDefaultList];
  const int n = verbatim ? (int)p->ops.size() : (int)list.size();
  for (int i = start; i < n; ++i) {
    const sdmi_rt::Op& op = p->ops[verbatim ? i : list[i].src];
    const hipEvent_t ev = verbatim ? (op.eid >= 0 ? sdmi_rt::handle(p, op, false) : nullptr) : list[i].event;
    hipError_t e = hipSuccess;
    switch (op.kind) {
      case sdmi_rt::OP_LAUNCH: {
        const unsigned char* base = (const unsigned char*)op.args.data();
        for (size_t a = 0; a < op.offs.size(); ++a) ptrs[a] = (void*)(base + op.offs[a]);
        if (ev)  // the record behind this launch, folded: the event is recorded when the kernel ends
          e = hipExtLaunchKernel(op.fn, op.grid, op.block, ptrs, op.shmem, op.stream, nullptr, ev, 0);
        else
          e = hipLaunchKernel(op.fn, op.grid, op.block, ptrs, op.shmem, op.stream);
        break;
      }
      case sdmi_rt::OP_EVENT: e = hipEventRecord(ev, op.stream); break;
      case sdmi_rt::OP_WAIT: e = hipStreamWaitEvent(op.stream, ev, 0); break;
      case sdmi_rt::OP_ALLREDUCE: {
        const int rc = sdmi_rt::issue_allreduce(op.comm, op.buf, op.count, op.dtype, op.stream);
        if (rc != 0) {
          *callout = -1;
          *next = i;
          return rc;
        }
        break;
      }
      default:
        *callout = op.callout;
        *next = i + 1;
        return 0;
    }
    if (e != hipSuccess) {
      *callout = -1;
      *next = i;
      return (int)e;
    }
  }
  *callout = -1;
  *next = n;
  return 0;
}

// the stream an op was recorded on (launches, event records, waits, all-reduces; nullptr for callouts)
extern "C" int sdmi_plan_op_stream(const void* plan, int i, sdmi_stream_t* stream) {
  const Plan* p = (const Plan*)plan;
  if (!p || i < 0 || i >= (int)p->ops.size() || !stream) return -1;
  *stream = (sdmi_stream_t)p->ops[i].stream;
  return 0;
}

// Per-op inspection for profiling tools (scripts/plan_profile.py): op kind (0 launch, 1 event record, 2 stream wait,
// 3 callout, 4 all-reduce), kernel name, grid / block, LDS bytes.
extern "C" int sdmi_plan_op_info(const void* plan, int i, int* kind, const char** name, int* grid, int* block,
                                 int* shmem) {
  const Plan* p = (const Plan*)plan;
  if (!p || i < 0 || i >= (int)p->ops.size()) return -1;
  const sdmi_rt::Op& op = p->ops[i];
  if (kind) *kind = op.kind;
  if (name) *name = op.kind == sdmi_rt::OP_LAUNCH ? hipKernelNameRefByPtr(op.fn, op.stream) : nullptr;
  if (grid) {
    grid[0] = (int)op.grid.x;
    grid[1] = (int)op.grid.y;
    grid[2] = (int)op.grid.z;
  }
  if (block) *block = (int)(op.block.x * op.block.y * op.block.z);
  if (shmem) *shmem = (int)op.shmem;
  return 0;
}

// Re-issue launch op i alone `iters` times on its stream between two events (after `warm` untimed issues) and
// return the average device time in microseconds. The plan's buffers are live (private pool), so the op reads and
// writes exactly the memory it does inside the step (in-place accumulating ops change values; timing only).
extern "C" int sdmi_plan_time_op(void* plan, int i, int warm, int iters, float* us) {
  Plan* p = (Plan*)plan;
  if (!p || i < 0 || i >= (int)p->ops.size() || iters < 1 || !us) return -1;
  const sdmi_rt::Op& op = p->ops[i];
  if (op.kind != sdmi_rt::OP_LAUNCH) return -2;
  void** ptrs = p->scratch.data();
  const unsigned char* base = (const unsigned char*)op.args.data();
  for (size_t a = 0; a < op.offs.size(); ++a) ptrs[a] = (void*)(base + op.offs[a]);
  hipEvent_t e0, e1;
  if (hipEventCreate(&e0) != hipSuccess) return -3;
  if (hipEventCreate(&e1) != hipSuccess) return -3;
  hipError_t e = hipSuccess;
  for (int w = 0; w < warm && e == hipSuccess; ++w) e = hipLaunchKernel(op.fn, op.grid, op.block, ptrs, op.shmem, op.stream);
  if (e == hipSuccess) e = hipEventRecord(e0, op.stream);
  for (int r = 0; r < iters && e == hipSuccess; ++r) e = hipLaunchKernel(op.fn, op.grid, op.block, ptrs, op.shmem, op.stream);
  if (e == hipSuccess) e = hipEventRecord(e1, op.stream);
  if (e == hipSuccess) e = hipEventSynchronize(e1);
  float ms = 0.f;
  if (e == hipSuccess) e = hipEventElapsedTime(&ms, e0, e1);
  (void)hipEventDestroy(e0);
  (void)hipEventDestroy(e1);
  if (e != hipSuccess) return (int)e;
  *us = ms * 1000.f / (float)iters;
  return 0;
}

// ---------------------------------------------------------------------------------------------------------------
// Edge-cost probe (scripts/plan_edge_cost.py): what one cross-stream edge costs the stream it sits on. A chain of
// `chain` short dependent kernels on stream A (each rewrites the same `bytes` buffer), timed by two events on A,
// with per boundary:
//   variant 0  nothing (the baseline span);
//   variant 1  hipEventRecord(ev_i, A) and stream B waiting on it (then a tiny kernel on B);
//   variant 2  no separate record: kernel i launched with hipExtLaunchKernel(stopEvent = ev_i), B waiting on it;
//   variant 3  k hipStreamWaitEvent on A, back to back, on events of B that completed long ago;
//   variant 4  hipEventRecord(ev_i, A) alone, nothing waiting on it;
//   variant 5  as 1, with no kernel on B behind its wait.
// nofence: the edge events carry hipEventDisableSystemFence besides hipEventDisableTiming (torch's default flags).
// Returns the span in microseconds, averaged over `reps` timed chains after one untimed.
namespace {

__global__ void edge_probe_kernel(float* p, size_t n) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) p[i] = p[i] * 0.5f + 1.0f;
}

}  // namespace

extern "C" int sdmi_plan_edge_probe(int variant, int nofence, int k, int chain, size_t bytes, int reps, float* span_us) {
  if (variant < 0 || variant > 5 || chain < 1 || chain > 4096 || k < 1 || k > 64 || reps < 1 || bytes < 4 ||
      bytes > ((size_t)256 << 20) || !span_us)
    return -1;
  const size_t n = bytes / 4, nb = 4096;
  const int nev = variant == 3 ? chain * k : chain;
  hipStream_t A = nullptr, B = nullptr;
  float *bufA = nullptr, *bufB = nullptr;
  hipEvent_t t0 = nullptr, t1 = nullptr;
  std::vector<hipEvent_t> evs(nev, nullptr);
  hipError_t e = hipStreamCreateWithFlags(&A, hipStreamNonBlocking);
  if (e == hipSuccess) e = hipStreamCreateWithFlags(&B, hipStreamNonBlocking);
  if (e == hipSuccess) e = hipMalloc((void**)&bufA, n * 4);
  if (e == hipSuccess) e = hipMalloc((void**)&bufB, nb * 4);
  if (e == hipSuccess) e = hipMemsetAsync(bufA, 0, n * 4, A);
  if (e == hipSuccess) e = hipMemsetAsync(bufB, 0, nb * 4, B);
  if (e == hipSuccess) e = hipEventCreate(&t0);
  if (e == hipSuccess) e = hipEventCreate(&t1);
  const unsigned flags = hipEventDisableTiming | (nofence ? (unsigned)hipEventDisableSystemFence : 0u);
  for (int i = 0; i < nev && e == hipSuccess; ++i) e = hipEventCreateWithFlags(&evs[i], flags);
  if (variant == 3)  // the awaited events: recorded on B once, complete before the chain starts
    for (int i = 0; i < nev && e == hipSuccess; ++i) e = hipEventRecord(evs[i], B);
  if (e == hipSuccess) e = hipDeviceSynchronize();
  const dim3 block(256), grid((unsigned)((n + 255) / 256)), gridB((unsigned)((nb + 255) / 256));
  void* argsA[2] = {(void*)&bufA, (void*)&n};
  void* argsB[2] = {(void*)&bufB, (void*)&nb};
  float total = 0.f;
  for (int r = 0; r <= reps && e == hipSuccess; ++r) {
    e = hipEventRecord(t0, A);
    for (int i = 0; i < chain && e == hipSuccess; ++i) {
      if (variant == 3)
        for (int w = 0; w < k && e == hipSuccess; ++w) e = hipStreamWaitEvent(A, evs[i * k + w], 0);
      if (e != hipSuccess) break;
      if (variant == 2)
        e = hipExtLaunchKernel((const void*)edge_probe_kernel, grid, block, argsA, 0, A, nullptr, evs[i], 0);
      else
        e = hipLaunchKernel((const void*)edge_probe_kernel, grid, block, argsA, 0, A);
      if (e == hipSuccess && (variant == 1 || variant >= 4)) e = hipEventRecord(evs[i], A);
      if (e == hipSuccess && (variant == 1 || variant == 2 || variant == 5)) {
        e = hipStreamWaitEvent(B, evs[i], 0);
        if (e == hipSuccess && variant != 5) e = hipLaunchKernel((const void*)edge_probe_kernel, gridB, block, argsB, 0, B);
      }
    }
    if (e == hipSuccess) e = hipEventRecord(t1, A);
    if (e == hipSuccess) e = hipDeviceSynchronize();
    float ms = 0.f;
    if (e == hipSuccess) e = hipEventElapsedTime(&ms, t0, t1);
    if (r > 0) total += ms;
  }
  if (e != hipSuccess) (void)hipDeviceSynchronize();
  for (hipEvent_t ev : evs)
    if (ev) (void)hipEventDestroy(ev);
  if (t0) (void)hipEventDestroy(t0);
  if (t1) (void)hipEventDestroy(t1);
  if (bufA) (void)hipFree(bufA);
  if (bufB) (void)hipFree(bufB);
  if (A) (void)hipStreamDestroy(A);
  if (B) (void)hipStreamDestroy(B);
  if (e != hipSuccess) return (int)e;
  *span_us = total * 1000.f / (float)reps;
  return 0;
}

extern "C" int sdmi_plan_destroy(void* plan) {
  delete (Plan*)plan;
  return 0;
}
