// lpbox_chain.h -- what the host loops of the adaptive launch chains decide, written once and free of HIP (plain C++: a host compiler
// builds it, tests/chain_check.cpp runs it under the host sanitizers).  A chain enqueues kmax PCG launch groups per outer iteration; the
// kernels fall through once a PCG has converged, a PCG that needs more halts the chain (halt = 3) and the host resumes it with 16 more
// groups.  The segmentation (lpbox_seg_capi.hip), generic BQP (lpbox_gen_capi.hip) and large-LP (lpbox_big_capi.hip) front ends differ
// in the numbers of ChainRules and in their launches, nothing else.  ChainController decides for the chain of one problem, ChainLockstep
// for the one chain a batch shares; the drivers that issue the launches are chain_run and chain_run_lockstep in lpbox_host.h.
#pragma once
#include <algorithm>
#include <vector>

constexpr int CHAIN_HALT_NONE = 0, CHAIN_HALT_PCG_MORE = 3;   // SEG_/GEN_/BIG_HALT_* agree on these two (static_asserts at the front ends)
constexpr int CHAIN_PAIRS_PER_RESUME = 16;                    // PCG launch groups a resume enqueues

struct ChainRules {
    const char *name;
    int kmax_start;        // launch groups per iteration of a fresh handle
    int kmax_floor;        // least kmax the batch rule picks
    int kmax_cap;          // most kmax either rule picks (0: none)
    int halt_bump;         // after a halt at pcg_k: kmax >= pcg_k + halt_bump
    int margin;            // spare groups beyond the largest PCG count of the previous batch
    int iters_per_batch;   // outer iterations between two reads of the control state
    int iters_per_graph;   // outer iterations of one captured graph (even: the state ping-pong returns to its start parity)
    int pcg_cap;           // the PCG's iteration cap, for the resume limit
    // a PCG of at most pcg_cap iterations is complete after this many resumes of 16 groups whatever kmax was: a chain that asks for more
    // is broken, and the loops return an error instead of resuming for ever
    constexpr int resume_limit() const { return pcg_cap / CHAIN_PAIRS_PER_RESUME + 2; }
};
// margin: a spare group is a launch that falls through (~3 us), a miss is a host round trip.  Segmentation, measured over 100 images at
// 10^4 nodes and the full-resolution one: 0 spare groups 8 % / 7 % faster than 2, 1 in between (the counts drift slowly, misses are rare);
// the lockstep chain of a batch, 100 problems, fastest / median of five: margin 2 119 / 120 ms, 1 111 / 112 ms, 0 108 / 108 ms.
constexpr ChainRules CHAIN_RULES_SEG = {"seg", 10, 2, 24, 4, 0, 32, 4, 1000};
constexpr ChainRules CHAIN_RULES_GEN = {"gen", 12, 3, 0, 8, 1, 16, 2, 1000};      // pcg_cap: GenParams::pcg_maxiters of the solve
constexpr ChainRules CHAIN_RULES_BIG = {"big", 28, 4, 0, 8, 1, 16, 2, 1000};

// the fields of SegState / GenState / BigState the loops read
struct ChainView { int halt, iter, pcg_k, pcg_max, outer_total, have_prev; };
template <class State>
ChainView chain_view(const State &s) { return ChainView{s.halt, s.iter, s.pcg_k, s.pcg_max, s.outer_total, s.have_prev}; }

inline int chain_cap(const ChainRules &r, int kmax) { return r.kmax_cap > 0 ? std::min(r.kmax_cap, kmax) : kmax; }

// rule 1, after a halt: the PCG stood at pcg_k when it ran out of launch groups
inline int chain_kmax_after_halt(const ChainRules &r, int kmax, int pcg_k) { return chain_cap(r, std::max(kmax, pcg_k + r.halt_bump)); }

// rule 2, before a batch: track the largest PCG count of the previous one.  A problem that completed no PCG there (pcg_max == 0: the
// batch only finalised an iteration that had been resumed, or nothing has run yet) has nothing to track and votes for the kmax in use --
// it used to vote 0, and the window after one whose last iteration had been resumed began at the floor, with a halt.
inline int chain_pcg_vote(const ChainRules &r, int kmax, const ChainView &v) {
    return v.outer_total > 0 && v.pcg_max > 0 ? v.pcg_max : kmax - r.margin;
}
inline int chain_kmax_for_vote(const ChainRules &r, int vote) { return chain_cap(r, std::max(r.kmax_floor, vote + r.margin)); }
inline int chain_kmax_before_batch(const ChainRules &r, int kmax, const ChainView &v) {
    return v.outer_total > 0 && v.pcg_max > 0 ? chain_kmax_for_vote(r, chain_pcg_vote(r, kmax, v)) : kmax;
}

inline int chain_batch_iters(const ChainRules &r, int remaining) { return std::min(std::max(remaining, 0), r.iters_per_batch); }

struct ChainStep {
    enum Kind { RESUME, BATCH, DONE, STUCK } kind;
    int kmax;      // RESUME, BATCH: the launch count to go on with
    int iters;     // BATCH: outer iterations to enqueue; 0 = only finalise the one that is waiting
    int resumes;   // STUCK: resumes in a row that did not complete the iteration
};

// one problem's chain: owns the launch count and the resume bookkeeping, answers "what next?" from the control state
struct ChainController {
    ChainRules rules = CHAIN_RULES_SEG;
    int kmax = 0;
    bool adaptive = true;        // false: kmax is forced (LPBOX_*_KMAX) and never moves
    int resumed = 0;             // resumes since an outer iteration last completed
    long long pcg_resumes = 0;   // halts resumed since the owner last reset it
    long long kept = 0;          // batches before which rule 2 had nothing to track although iterations had run (pcg_max == 0)

    explicit ChainController(const ChainRules &r) : rules(r), kmax(r.kmax_start) {}
    void force_kmax(int v) { kmax = v; adaptive = false; }
    void begin() { resumed = 0; }                                   // a host loop starts (a window, a solve)

    ChainStep next(const ChainView &v, int iter_end) {
        if (v.halt == CHAIN_HALT_PCG_MORE) {
            if (++resumed > rules.resume_limit()) return ChainStep{ChainStep::STUCK, kmax, 0, resumed - 1};
            pcg_resumes++;
            if (adaptive) kmax = chain_kmax_after_halt(rules, kmax, v.pcg_k);
            return ChainStep{ChainStep::RESUME, kmax, 0, 0};
        }
        if (v.halt != CHAIN_HALT_NONE) return ChainStep{ChainStep::DONE, kmax, 0, 0};
        resumed = 0;
        const int remaining = iter_end - v.iter;
        if (remaining <= 0 && !v.have_prev) return ChainStep{ChainStep::DONE, kmax, 0, 0};
        if (adaptive) kmax = chain_kmax_before_batch(rules, kmax, v);
        if (adaptive && v.outer_total > 0 && v.pcg_max == 0) kept++;
        return ChainStep{ChainStep::BATCH, kmax, chain_batch_iters(rules, remaining), 0};
    }
};

// A members advanced in lockstep by ONE chain (a batch): one launch count for all, every member on its own control state.  A halt of
// any member resumes the chain (the others fall through); halted members neither vote for kmax nor count towards the iterations left; a
// batch runs as far as the member that has most left, at the largest vote.  A = 1, kmax inside [floor, cap]: ChainController's steps.
struct ChainLockstep {
    ChainRules rules;
    int kmax;
    bool adaptive;               // false: kmax is forced and never moves
    std::vector<int> resumed;    // per member: resumes since one of its outer iterations last completed
    int stuck_slot = -1, stuck_iter = 0, stuck_pcg_k = 0;   // STUCK: the member that did not come out of its halt, and where it stands

    ChainLockstep(const ChainRules &r, int kmax_, bool adaptive_ = true) : rules(r), kmax(kmax_), adaptive(adaptive_) {}
    void begin(int A) { resumed.assign((size_t)A, 0); }              // a host loop starts (a window, a solve) over A members

    // v[A]: the members' control states; resumes[A] is raised for every member whose own state shows the halt at a resume
    ChainStep next(const ChainView *v, int iter_end, long long *resumes) {
        bool more = false, any_run = false;
        int remaining = 0, vote = 0, pcg_k = 0;
        for (int i = 0; i < (int)resumed.size(); i++) {
            if (v[i].halt == CHAIN_HALT_PCG_MORE) {
                if (++resumed[i] <= rules.resume_limit()) { resumes[i]++; more = true; pcg_k = std::max(pcg_k, v[i].pcg_k); continue; }
                stuck_slot = i; stuck_iter = v[i].iter; stuck_pcg_k = v[i].pcg_k;
                return ChainStep{ChainStep::STUCK, kmax, 0, resumed[i] - 1};
            }
            resumed[i] = 0;
            if (v[i].halt != CHAIN_HALT_NONE) continue;
            const int rem = iter_end - v[i].iter;
            if (rem <= 0 && !v[i].have_prev) continue;
            any_run = true; remaining = std::max(remaining, rem);
            vote = std::max(vote, chain_pcg_vote(rules, kmax, v[i]));
        }
        if (more && adaptive) kmax = chain_kmax_after_halt(rules, kmax, pcg_k);      // some PCG ran out of launch groups
        if (more) return ChainStep{ChainStep::RESUME, kmax, 0, 0};
        if (!any_run) return ChainStep{ChainStep::DONE, kmax, 0, 0};
        if (adaptive) kmax = chain_kmax_for_vote(rules, vote);
        return ChainStep{ChainStep::BATCH, kmax, chain_batch_iters(rules, remaining), 0};
    }
};
