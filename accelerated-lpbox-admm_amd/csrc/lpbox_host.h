// lpbox_host.h -- the HIP-side plumbing every host file (*_capi.hip) shares: the error-check macros, use_device, the owning device
// buffer, the stream timer, the cache of captured graphs and the drivers of a single-problem launch chain and of the lockstep chain of
// a batch (their decisions are those of lpbox_chain.h).  Not part of the C-ABI.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <map>
#include <utility>
#include <vector>

#include "../../include/lpbox_hip.h"
#include "lpbox_capi_internal.h"
#include "lpbox_chain.h"

#define HIPCHK(expr)                                                                                         \
    do {                                                                                                     \
        hipError_t e_ = (expr);                                                                              \
        if (e_ != hipSuccess) return lpbox_fail(LPBOX_E_HIP, "%s failed: %s", #expr, hipGetErrorString(e_)); \
    } while (0)
#define CHK(expr) do { int rc_ = (expr); if (rc_ < 0) return rc_; } while (0)

inline int use_device(int device) {
    int cnt = 0;
    if (hipGetDeviceCount(&cnt) != hipSuccess || cnt <= 0) return lpbox_fail(LPBOX_E_NODEVICE, "no HIP device available");
    HIPCHK(hipSetDevice(device));
    return LPBOX_OK;
}

// `count` elements on the device, freed with the owner.  alloc(0) leaves p == nullptr ("not allocated" is tested through p); `floor`
// asks for at least that many elements behind an unchanged count (the generic BQP path hands its kernels a pointer for empty vectors).
template <typename Tp>
struct DevBuf {
    Tp *p = nullptr;
    size_t count = 0;
    DevBuf() = default;
    DevBuf(const DevBuf &) = delete;
    DevBuf &operator=(const DevBuf &) = delete;
    ~DevBuf() { release(); }
    hipError_t alloc(size_t c, size_t floor = 0) {
        release();
        count = c;
        c = std::max(c, floor);
        return c ? hipMalloc((void **)&p, c * sizeof(Tp)) : hipSuccess;
    }
    void release() {
        if (p) (void)hipFree(p);
        p = nullptr; count = 0;
    }
    hipError_t upload(const std::vector<Tp> &v, size_t floor = 0) {
        hipError_t e = alloc(v.size(), floor);
        if (e != hipSuccess || v.empty()) return e;
        return hipMemcpy(p, v.data(), v.size() * sizeof(Tp), hipMemcpyHostToDevice);
    }
};

// the time a stream spends between start() and stop(), from two events
struct StreamTimer {
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    hipError_t create() {
        if (ev0) return hipSuccess;
        hipError_t e = hipEventCreate(&ev0);
        return e != hipSuccess ? e : hipEventCreate(&ev1);
    }
    void destroy() {
        if (ev0) (void)hipEventDestroy(ev0);
        if (ev1) (void)hipEventDestroy(ev1);
        ev0 = ev1 = nullptr;
    }
    hipError_t start(hipStream_t s) { return hipEventRecord(ev0, s); }
    hipError_t stop(hipStream_t s) { return hipEventRecord(ev1, s); }
    hipError_t read(double *ms) {                                    // once the stream has been synchronised behind stop()
        float f = 0.f;
        hipError_t e = hipEventElapsedTime(&f, ev0, ev1);
        *ms = f;
        return e;
    }
    hipError_t stop_sync(hipStream_t s, double *ms) {
        hipError_t e = stop(s);
        if (e == hipSuccess) e = hipStreamSynchronize(s);
        return e != hipSuccess ? e : read(ms);
    }
};

// where a chain's launches go and what they count; the members point into the front end's handle
struct ChainIo {
    hipStream_t stream;
    int &parity;                   // the state ping-pong: every launch of the chain flips it
    long long &launches, &collectives;
    bool &use_graph;               // cleared for good when a capture fails
    bool can_capture;              // false: a transport that runs host code at enqueue time
};

// The static launch sequence of iters_per_graph outer iterations, captured once per (kmax, start parity) and replayed: short kernels are
// launch-bound without it.  Every entry knows the launches and collectives of one replay of ITS graph.
struct GraphCache {
    struct Entry { hipGraph_t graph = nullptr; hipGraphExec_t exec = nullptr; long long launches = 0, collectives = 0; };
    std::map<std::pair<int, int>, Entry> entries;
    int last_kmax = -1;            // of the entry captured last
    long long revisits = 0;        // hits on an entry of another kmax than the one captured last (kmax moved away and came back)
    GraphCache() = default;
    GraphCache(const GraphCache &) = delete;
    GraphCache &operator=(const GraphCache &) = delete;
    ~GraphCache() { clear(); }
    void clear() {                 // also when a buffer the captured launches carry is reallocated
        for (auto &kv : entries) { (void)hipGraphExecDestroy(kv.second.exec); (void)hipGraphDestroy(kv.second.graph); }
        entries.clear();
    }
    // enqueue() issues the launches (flipping io.parity, counting into io.launches / io.collectives) and returns an LPBOX status
    template <class Enqueue>
    int get(int kmax, ChainIo &io, Enqueue &&enqueue, const Entry **out) {
        const auto key = std::make_pair(kmax, io.parity);
        auto it = entries.find(key);
        if (it != entries.end()) { revisits += kmax != last_kmax; *out = &it->second; return LPBOX_OK; }
        const int par0 = io.parity;
        const long long l0 = io.launches, c0 = io.collectives;
        Entry e;
        HIPCHK(hipStreamBeginCapture(io.stream, hipStreamCaptureModeThreadLocal));
        const int rc = enqueue();
        const hipError_t e2 = hipStreamEndCapture(io.stream, &e.graph);
        e.launches = io.launches - l0; e.collectives = io.collectives - c0;
        io.launches = l0; io.collectives = c0;
        if (rc < 0 || e2 != hipSuccess || io.parity != par0) {
            io.parity = par0;
            if (e.graph) (void)hipGraphDestroy(e.graph);
            return rc < 0 ? rc : lpbox_fail(LPBOX_E_HIP, "graph capture failed: %s", hipGetErrorString(e2));
        }
        const hipError_t e3 = hipGraphInstantiate(&e.exec, e.graph, nullptr, nullptr, 0);
        if (e3 != hipSuccess) {
            (void)hipGraphDestroy(e.graph);
            return lpbox_fail(LPBOX_E_HIP, "hipGraphInstantiate failed: %s", hipGetErrorString(e3));
        }
        last_kmax = kmax;
        *out = &(entries[key] = e);
        return LPBOX_OK;
    }
};

// `batch` outer iterations at kmax: replays of the graph of per_graph iterations while that many are left, the rest eagerly;
// enqueue(n) issues n iterations.  A capture that fails makes the chain go on with eager launches for good.
template <class Enqueue>
int chain_enqueue_batch(GraphCache &graphs, ChainIo &io, int per_graph, int kmax, int batch, Enqueue &&enqueue) {
    if (io.use_graph && io.can_capture && batch >= per_graph) {
        const GraphCache::Entry *g = nullptr;
        if (graphs.get(kmax, io, [&] { return enqueue(per_graph); }, &g) < 0) {
            io.use_graph = false;
            (void)hipGetLastError();
        } else {
            for (; batch >= per_graph; batch -= per_graph) {
                HIPCHK(hipGraphLaunch(g->exec, io.stream));
                io.launches += g->launches; io.collectives += g->collectives;
            }
        }
    }
    if (batch > 0) CHK(enqueue(batch));
    return LPBOX_OK;
}

// The host loop of a single-problem chain up to iter_end: read the control state, resume a PCG that ran out of launch groups, re-pick
// kmax, enqueue a batch as graph replays plus an eager tail, finalise.  Ops supplies the front end's launches:
//   int read_state(ChainView &v)   copy the control state back (synchronises)
//   int resume_pcg()               CHAIN_PAIRS_PER_RESUME more launch groups for the halted PCG
//   int batch_head()               what precedes the iterations of a batch (pcg_max = 0 for it)
//   int enqueue(int n)             n outer iterations at the controller's kmax
//   int finalize()                 finalise the last iteration of the batch
template <class Ops>
int chain_run(ChainController &ctl, GraphCache &graphs, ChainIo io, int iter_end, Ops &&ops) {
    ctl.begin();
    for (;;) {
        ChainView v;
        CHK(ops.read_state(v));
        const ChainStep step = ctl.next(v, iter_end);
        if (step.kind == ChainStep::DONE) return LPBOX_OK;
        if (step.kind == ChainStep::STUCK)
            return lpbox_fail(LPBOX_E_STATE, "iteration %d: the PCG is still halted at k = %d after %d resumes in a row", v.iter, v.pcg_k, step.resumes);
        if (step.kind == ChainStep::RESUME) { CHK(ops.resume_pcg()); continue; }
        CHK(ops.batch_head());
        CHK(chain_enqueue_batch(graphs, io, ctl.rules.iters_per_graph, step.kmax, step.iters, [&](int n) { return ops.enqueue(n); }));
        CHK(ops.finalize());
    }
}

// The host loop of the ONE chain A members of a batch share, up to iter_end (decisions: ChainLockstep).  resumes[A] is raised for every
// member whose own state showed the halt at a resume; act[k] is the batch index of the member in slot k (nullptr: k) for the error text.
// A front end that launches eagerly passes use_graph = false and an empty cache.  Ops as for chain_run, but collect(ChainView *v) reads
// the A control states, and batch_head(iters, kmax) and enqueue(n, kmax) are told the step: a count that must be the same for a replay
// and for eager launches is made by formula in batch_head (enqueue runs once, inside a capture).
template <class Ops>
int chain_run_lockstep(ChainLockstep &ctl, int A, const int *act, GraphCache &graphs, ChainIo io, int iter_end, long long *resumes, Ops &&ops) {
    std::vector<ChainView> v((size_t)A);
    ctl.begin(A);
    for (;;) {
        CHK(ops.collect(v.data()));
        const ChainStep step = ctl.next(v.data(), iter_end, resumes);
        if (step.kind == ChainStep::DONE) return LPBOX_OK;
        if (step.kind == ChainStep::STUCK)
            return lpbox_fail(LPBOX_E_STATE, "problem %d of the batch, iteration %d: the PCG is still halted at k = %d after %d resumes in a row", act ? act[ctl.stuck_slot] : ctl.stuck_slot, ctl.stuck_iter, ctl.stuck_pcg_k, step.resumes);
        if (step.kind == ChainStep::RESUME) { CHK(ops.resume_pcg()); continue; }
        CHK(ops.batch_head(step.iters, step.kmax));
        CHK(chain_enqueue_batch(graphs, io, ctl.rules.iters_per_graph, step.kmax, step.iters, [&](int n) { return ops.enqueue(n, step.kmax); }));
        CHK(ops.finalize());
    }
}

// the indices of the members a batch's mask leaves active, ascending
inline std::vector<int> active_members(const std::vector<uint8_t> &active) {
    std::vector<int> act;
    for (size_t i = 0; i < active.size(); i++) if (active[i]) act.push_back((int)i);
    return act;
}
