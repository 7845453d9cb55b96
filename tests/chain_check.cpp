// chain_check.cpp -- the decisions of the adaptive launch chains (csrc/lpbox_chain.h) against a table, as a stand-alone program meant
// to run under AddressSanitizer + UBSan (tests/test_chain.py builds and runs it):
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I<csrc> chain_check.cpp
// The expectations are literals worked out from the formulas of the host loops as they stood before the header existed (run_window and
// batch_run_chain of lpbox_seg_capi.hip, the loop of lpbox_bqp_solve, run_window of lpbox_big_capi.hip), with the two deliberate
// changes of DESIGN.md section 25: the large-LP chain has the resume limit, and all three keep kmax after a batch that completed no PCG.
// The lockstep chain of a batch (ChainLockstep) is held against the two loops it replaced in the same way.
// `chain_check rules` prints the rules, one line per front end, for the Python side.
#include "lpbox_chain.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

namespace {

const char *g_what = "";
long g_checks = 0;

#define REQUIRE(cond)                                                                         \
    do {                                                                                      \
        g_checks++;                                                                           \
        if (!(cond)) { printf("FAILED %s: %s (line %d)\n", g_what, #cond, __LINE__); exit(1); } \
    } while (0)

// per front end: the rules as the table of DESIGN.md section 25 states them, and what the rules give at chosen points
struct Expect {
    const char *name;
    ChainRules rules;
    int start, floor, cap, bump, margin, per_batch, per_graph, resume_limit;
    int halt_at_5;         // kmax after a halt at pcg_k = 5 from the starting kmax: max(start, 5 + bump)
    int halt_at_30;        // ... at pcg_k = 30: max(start, 30 + bump), under the cap
    int halt_at_30_from_40;   // kmax = 40 before (forced up by hand): never lowered by a halt; under the cap
    int batch_pcg_1;       // kmax before a batch after pcg_max = 1: max(floor, 1 + margin)
    int batch_pcg_7;       // ... pcg_max = 7
    int batch_pcg_100;     // ... pcg_max = 100, under the cap
};
const Expect TABLE[] = {
    //                         start floor cap bump margin batch graph limit | h5  h30 h30/40 | b1  b7  b100
    {"seg", CHAIN_RULES_SEG,   10,   2,    24, 4,   0,     32,   4,    64,     10, 24, 24,      2,  7,  24},
    {"gen", CHAIN_RULES_GEN,   12,   3,    0,  8,   1,     16,   2,    64,     13, 38, 40,      3,  8,  101},
    {"big", CHAIN_RULES_BIG,   28,   4,    0,  8,   1,     16,   2,    64,     28, 38, 40,      4,  8,  101},
};

ChainView view(int halt, int iter, int pcg_k, int pcg_max, int outer_total, int have_prev) {
    return ChainView{halt, iter, pcg_k, pcg_max, outer_total, have_prev};
}

void check_front_end(const Expect &e) {
    g_what = e.name;
    const ChainRules &r = e.rules;
    REQUIRE(!strcmp(r.name, e.name));
    REQUIRE(r.kmax_start == e.start && r.kmax_floor == e.floor && r.kmax_cap == e.cap && r.halt_bump == e.bump && r.margin == e.margin);
    REQUIRE(r.iters_per_batch == e.per_batch && r.iters_per_graph == e.per_graph && r.iters_per_graph % 2 == 0);
    REQUIRE(r.pcg_cap == 1000 && r.resume_limit() == e.resume_limit);

    // ---- a resume raises kmax to max(kmax, pcg_k + bump) under the cap
    {
        ChainController c(r);
        REQUIRE(c.kmax == e.start && c.adaptive && c.pcg_resumes == 0);
        ChainStep s = c.next(view(3, 0, 5, 0, 0, 0), 10);
        REQUIRE(s.kind == ChainStep::RESUME && s.kmax == e.halt_at_5 && c.kmax == e.halt_at_5 && c.pcg_resumes == 1);
        s = c.next(view(3, 0, 30, 0, 0, 0), 10);
        REQUIRE(s.kind == ChainStep::RESUME && s.kmax == e.halt_at_30 && c.pcg_resumes == 2 && c.resumed == 2);
        c.kmax = 40;
        s = c.next(view(3, 0, 30, 0, 0, 0), 10);
        REQUIRE(s.kind == ChainStep::RESUME && s.kmax == e.halt_at_30_from_40);
        REQUIRE(chain_kmax_after_halt(r, e.start, 5) == e.halt_at_5 && chain_kmax_after_halt(r, e.start, 30) == e.halt_at_30);
    }
    // ---- resume number limit + 1 in a row is "stuck"; a completed iteration resets the count
    {
        ChainController c(r);
        c.begin();
        for (int k = 1; k <= e.resume_limit; k++) REQUIRE(c.next(view(3, 7, 16 * k, 0, 5, 0), 10).kind == ChainStep::RESUME);
        REQUIRE(c.pcg_resumes == e.resume_limit);
        ChainStep s = c.next(view(3, 7, 2000, 0, 5, 0), 10);
        REQUIRE(s.kind == ChainStep::STUCK && s.resumes == e.resume_limit && c.pcg_resumes == e.resume_limit);

        ChainController d(r);
        for (int k = 1; k <= e.resume_limit; k++) REQUIRE(d.next(view(3, 7, 16 * k, 0, 5, 0), 10).kind == ChainStep::RESUME);
        REQUIRE(d.next(view(0, 8, 0, 9, 6, 1), 10).kind == ChainStep::BATCH && d.resumed == 0);       // iteration 7 completed
        for (int k = 1; k <= e.resume_limit; k++) REQUIRE(d.next(view(3, 8, 16 * k, 0, 6, 0), 10).kind == ChainStep::RESUME);
        REQUIRE(d.next(view(3, 8, 2000, 0, 6, 0), 10).kind == ChainStep::STUCK);
        d.begin();                                                                                    // a new host loop starts over
        REQUIRE(d.next(view(3, 8, 2000, 0, 6, 0), 10).kind == ChainStep::RESUME && d.pcg_resumes == 2 * e.resume_limit + 1);
    }
    // ---- the batch rule
    {
        ChainController c(r);
        ChainStep s = c.next(view(0, 0, 0, 7, 0, 0), 100);                       // outer_total == 0: nothing has run, kmax stays
        REQUIRE(s.kind == ChainStep::BATCH && s.kmax == e.start && s.iters == e.per_batch);
        s = c.next(view(0, 10, 0, 7, 10, 1), 100);
        REQUIRE(s.kind == ChainStep::BATCH && s.kmax == e.batch_pcg_7 && c.kmax == e.batch_pcg_7);
        s = c.next(view(0, 20, 0, 0, 20, 1), 100);                               // pcg_max == 0: no PCG completed, kmax stays
        REQUIRE(s.kind == ChainStep::BATCH && s.kmax == e.batch_pcg_7);
        s = c.next(view(0, 30, 0, 1, 30, 1), 100);                               // at the floor
        REQUIRE(s.kmax == e.batch_pcg_1 && e.batch_pcg_1 == e.floor);
        s = c.next(view(0, 40, 0, 100, 40, 1), 100);                             // at the cap (seg) / unbounded (gen, big)
        REQUIRE(s.kmax == e.batch_pcg_100);
        REQUIRE(chain_kmax_before_batch(r, 9, view(0, 1, 0, 7, 1, 0)) == e.batch_pcg_7);
        REQUIRE(chain_kmax_before_batch(r, 9, view(0, 1, 0, 0, 1, 0)) == 9 && chain_kmax_before_batch(r, 9, view(0, 0, 0, 7, 0, 0)) == 9);
    }
    // ---- a forced kmax never moves
    for (int forced : {1, 2, 24, 1000}) {
        ChainController c(r);
        c.force_kmax(forced);
        REQUIRE(!c.adaptive && c.kmax == forced);
        REQUIRE(c.next(view(3, 0, 900, 0, 0, 0), 10).kmax == forced && c.pcg_resumes == 1);
        REQUIRE(c.next(view(0, 1, 0, 50, 1, 1), 10).kmax == forced);
        REQUIRE(c.next(view(0, 5, 0, 0, 5, 1), 10).kmax == forced && c.kmax == forced);
    }
    // ---- batch sizes: remaining 0 without / with an iteration waiting, 1, iters_per_batch, iters_per_batch + 1, past the end; other halts
    {
        ChainController c(r);
        REQUIRE(c.next(view(0, 50, 0, 3, 50, 0), 50).kind == ChainStep::DONE);
        ChainStep s = c.next(view(0, 50, 0, 3, 50, 1), 50);
        REQUIRE(s.kind == ChainStep::BATCH && s.iters == 0);
        REQUIRE(c.next(view(0, 49, 0, 3, 49, 1), 50).iters == 1);
        REQUIRE(c.next(view(0, 50 - e.per_batch, 0, 3, 9, 1), 50).iters == e.per_batch);
        REQUIRE(c.next(view(0, 49 - e.per_batch, 0, 3, 9, 1), 50).iters == e.per_batch);
        REQUIRE(c.next(view(0, 60, 0, 3, 60, 0), 50).kind == ChainStep::DONE);
        s = c.next(view(0, 60, 0, 3, 60, 1), 50);
        REQUIRE(s.kind == ChainStep::BATCH && s.iters == 0);
        REQUIRE(chain_batch_iters(r, -3) == 0 && chain_batch_iters(r, 0) == 0 && chain_batch_iters(r, 1) == 1);
        REQUIRE(chain_batch_iters(r, e.per_batch) == e.per_batch && chain_batch_iters(r, e.per_batch + 1) == e.per_batch);
        for (int halt : {1, 2, 4}) REQUIRE(c.next(view(halt, 3, 0, 3, 3, 1), 50).kind == ChainStep::DONE);     // stop, window / end, all fixed
    }
}

// the lockstep chain of a segmentation batch (ChainLockstep): one kmax for B problems from their votes
void check_aggregated() {
    g_what = "seg batch";
    ChainRules r = CHAIN_RULES_SEG;
    auto agree = [&](int kmax, const std::vector<ChainView> &members) {
        ChainLockstep c(r, kmax);
        c.begin((int)members.size());
        std::vector<long long> resumes(members.size(), 0);
        const ChainStep s = c.next(members.data(), 100, resumes.data());
        REQUIRE(s.kind == ChainStep::BATCH && s.kmax == c.kmax);
        return s.kmax;
    };
    // margin 0: the largest PCG count of the previous batch, between 2 and 24
    REQUIRE(agree(10, {view(0, 10, 0, 4, 10, 1), view(0, 10, 0, 21, 10, 1)}) == 21);
    REQUIRE(agree(10, {view(0, 10, 0, 1, 10, 1), view(0, 10, 0, 1, 10, 1)}) == 2);
    REQUIRE(agree(10, {view(0, 10, 0, 4, 10, 1), view(0, 10, 0, 44, 10, 1)}) == 24);
    // a member that completed no PCG votes for the kmax in use: alone it keeps it, next to a larger count it is outvoted
    REQUIRE(chain_pcg_vote(r, 20, view(0, 10, 0, 0, 10, 1)) == 20 && chain_pcg_vote(r, 20, view(0, 0, 0, 5, 0, 0)) == 20);
    REQUIRE(agree(20, {view(0, 10, 0, 0, 10, 1), view(0, 10, 0, 4, 10, 1)}) == 20);
    REQUIRE(agree(20, {view(0, 10, 0, 0, 10, 1), view(0, 10, 0, 23, 10, 1)}) == 23);
    REQUIRE(agree(20, {view(0, 10, 0, 0, 10, 1)}) == 20);
    // LPBOX_SEG_KMARGIN = 2: counts carry the margin, a "keep" vote does not add it twice
    r.margin = 2;
    REQUIRE(chain_pcg_vote(r, 20, view(0, 10, 0, 0, 10, 1)) == 18);
    REQUIRE(agree(20, {view(0, 10, 0, 0, 10, 1), view(0, 10, 0, 4, 10, 1)}) == 20);
    REQUIRE(agree(20, {view(0, 10, 0, 7, 10, 1), view(0, 10, 0, 4, 10, 1)}) == 9);
    REQUIRE(agree(20, {view(0, 10, 0, 23, 10, 1)}) == 24);
    // one problem of a batch is the single-problem chain
    r.margin = 0;
    for (int pcg_max : {0, 1, 2, 9, 24, 30})
        REQUIRE(agree(12, {view(0, 5, 0, pcg_max, 5, 1)}) == chain_kmax_before_batch(r, 12, view(0, 5, 0, pcg_max, 5, 1)));
    // the halt rule with the largest pcg_k of the halted members
    REQUIRE(chain_kmax_after_halt(r, 10, 17) == 21 && chain_kmax_after_halt(r, 10, 40) == 24 && chain_kmax_after_halt(r, 24, 3) == 24);
}

// The decisions of a lockstep chain (ChainLockstep), for the rules of the two front ends that run one.  The expectations are literals
// from the two loops as they stood before the controller existed (batch_run_chain of lpbox_seg_capi.hip, bigb_run_chain of
// lpbox_big_capi.hip: the same procedure); kmax_at_1024: kmax after a halt at pcg_k = 1024 (uncapped: 1024 + bump).
void check_lockstep(const Expect &e, int kmax_at_1024) {
    g_what = e.name;
    const ChainRules &r = e.rules;
    const ChainView running = view(0, 45, 0, 7, 45, 1);                       // 5 iterations left of 50, votes 7
    // ---- member 0 halts resume_limit + 1 times in a row while member 1 completes iterations: stuck, and only member 0's count is raised
    {
        ChainLockstep c(r, r.kmax_start);
        REQUIRE(c.kmax == e.start && c.adaptive);
        c.begin(2);
        long long res[2] = {0, 0};
        for (int k = 1; k <= 64; k++) {
            const ChainView v[2] = {view(3, 7, 16 * k, 0, 5, 0), view(0, 7 + k, 0, 3, 5 + k, 1)};
            const ChainStep s = c.next(v, 100, res);
            REQUIRE(s.kind == ChainStep::RESUME && s.iters == 0 && c.resumed[0] == k && c.resumed[1] == 0 && c.stuck_slot == -1);
        }
        REQUIRE(e.resume_limit == 64 && res[0] == 64 && res[1] == 0 && c.kmax == kmax_at_1024);
        const ChainView v[2] = {view(3, 7, 2000, 0, 5, 0), view(0, 72, 0, 3, 70, 1)};
        const ChainStep s = c.next(v, 100, res);
        REQUIRE(s.kind == ChainStep::STUCK && s.resumes == 64 && c.stuck_slot == 0 && c.stuck_iter == 7 && c.stuck_pcg_k == 2000);
        REQUIRE(res[0] == 64 && res[1] == 0 && c.kmax == kmax_at_1024);
        c.begin(2);                                                           // a new host loop starts over
        REQUIRE(c.next(v, 100, res).kind == ChainStep::RESUME && res[0] == 65 && c.resumed[0] == 1);
    }
    // ---- a member whose state stops showing the halt resets its own count and nobody else's; the stuck member is named by its slot
    {
        ChainLockstep c(r, r.kmax_start);
        c.begin(3);
        long long res[3] = {0, 0, 0};
        const ChainView both[3] = {view(3, 7, 20, 0, 5, 0), running, view(3, 9, 20, 0, 5, 0)};
        for (int k = 0; k < 3; k++) REQUIRE(c.next(both, 50, res).kind == ChainStep::RESUME);
        REQUIRE(c.resumed[0] == 3 && c.resumed[1] == 0 && c.resumed[2] == 3);
        const ChainView one[3] = {view(0, 8, 0, 20, 6, 1), running, view(3, 9, 36, 0, 5, 0)};
        REQUIRE(c.next(one, 50, res).kind == ChainStep::RESUME);
        REQUIRE(c.resumed[0] == 0 && c.resumed[2] == 4 && res[0] == 3 && res[1] == 0 && res[2] == 4);
        for (int k = 5; k <= 64; k++) REQUIRE(c.next(both, 50, res).kind == ChainStep::RESUME);
        REQUIRE(c.resumed[0] == 60 && c.resumed[2] == 64);
        const ChainStep s = c.next(both, 50, res);                            // member 0 is raised before member 2 is found stuck
        REQUIRE(s.kind == ChainStep::STUCK && s.resumes == 64 && c.stuck_slot == 2 && c.stuck_iter == 9 && c.stuck_pcg_k == 20);
        REQUIRE(res[0] == 64 && res[1] == 0 && res[2] == 64);
    }
    // ---- halted members neither vote nor count towards the iterations left, and a halt anywhere resumes; after the resume kmax follows
    //      the largest pcg_k among the HALTED members (a stale pcg_k of a running one is not looked at)
    {
        ChainLockstep c(r, r.kmax_start);
        c.begin(2);
        long long res[2] = {0, 0};
        const ChainView v[2] = {view(3, 0, 5, 23, 9, 0), view(0, 98, 0, 3, 98, 1)};
        ChainStep s = c.next(v, 100, res);
        REQUIRE(s.kind == ChainStep::RESUME && s.kmax == e.halt_at_5 && s.iters == 0 && res[0] == 1 && res[1] == 0);
        ChainLockstep d(r, r.kmax_start);
        d.begin(3);
        long long res3[3] = {0, 0, 0};
        const ChainView w[3] = {view(3, 0, 5, 0, 9, 0), view(0, 3, 900, 3, 3, 1), view(3, 0, 30, 0, 9, 0)};
        s = d.next(w, 100, res3);
        REQUIRE(s.kind == ChainStep::RESUME && s.kmax == e.halt_at_30 && d.kmax == e.halt_at_30);
        // the batch that follows: the member that had halted has completed no PCG in it (pcg_max == 0) and votes for the kmax in use
        const ChainView x[2] = {view(0, 1, 0, 0, 10, 1), view(0, 98, 0, 3, 98, 1)};
        s = c.next(x, 100, res);
        REQUIRE(s.kind == ChainStep::BATCH && s.kmax == e.halt_at_5 && s.iters == e.per_batch);
    }
    // ---- who runs: not a member that has stopped (1), ended its window (2) or is all fixed (4), nor one at the end with nothing waiting
    {
        ChainLockstep c(r, r.kmax_start);
        c.begin(5);
        long long res[5] = {0, 0, 0, 0, 0};
        const ChainView idle[5] = {view(1, 3, 0, 23, 3, 1), view(2, 3, 0, 23, 3, 1), view(4, 3, 0, 23, 3, 1), view(0, 50, 0, 23, 50, 0), view(0, 60, 0, 23, 60, 0)};
        ChainStep s = c.next(idle, 50, res);
        REQUIRE(s.kind == ChainStep::DONE && s.kmax == e.start && c.kmax == e.start);
        ChainView some[5] = {idle[0], idle[1], idle[2], idle[3], running};
        s = c.next(some, 50, res);                                            // their counts of 23 and iterations left do not reach the batch
        REQUIRE(s.kind == ChainStep::BATCH && s.iters == 5 && s.kmax == e.batch_pcg_7 && c.kmax == e.batch_pcg_7);
        // the iterations left are the maximum over the running members, cut at iters_per_batch
        some[3] = view(0, 40, 0, 2, 40, 1);
        REQUIRE(c.next(some, 50, res).iters == 10);
        some[3] = view(0, 10, 0, 2, 10, 1);
        REQUIRE(c.next(some, 100, res).iters == e.per_batch);
        // only a member with a finished iteration waiting is left: finalise it, enqueue nothing
        some[3] = view(0, 50, 0, 2, 50, 1); some[4] = idle[3];
        s = c.next(some, 50, res);
        REQUIRE(s.kind == ChainStep::BATCH && s.iters == 0);
        some[3] = view(0, 60, 0, 2, 60, 1);
        s = c.next(some, 50, res);
        REQUIRE(s.kind == ChainStep::BATCH && s.iters == 0);
        for (int k = 0; k < 5; k++) REQUIRE(res[k] == 0 && c.resumed[k] == 0);
    }
    // ---- a forced kmax never moves
    for (int forced : {1, 2, 24, 1000}) {
        ChainLockstep c(r, forced, false);
        c.begin(2);
        long long res[2] = {0, 0};
        const ChainView halted[2] = {view(3, 0, 900, 0, 0, 0), running}, batch[2] = {view(0, 1, 0, 50, 1, 1), running};
        const ChainView kept[2] = {view(0, 5, 0, 0, 5, 1), view(0, 5, 0, 0, 5, 1)};
        REQUIRE(!c.adaptive && c.next(halted, 50, res).kmax == forced && res[0] == 1);
        REQUIRE(c.next(batch, 50, res).kmax == forced);
        REQUIRE(c.next(kept, 50, res).kmax == forced && c.kmax == forced);
    }
    // ---- one member, kmax inside [floor, cap]: the steps of ChainController
    {
        const ChainView script[] = {view(3, 0, 6, 0, 0, 0), view(3, 0, 9, 0, 0, 0), view(0, 1, 0, 9, 1, 1), view(0, 17, 0, 0, 17, 1),
                                    view(0, 33, 0, 5, 33, 1), view(0, 50, 0, 5, 50, 0)};
        const ChainStep::Kind kinds[] = {ChainStep::RESUME, ChainStep::RESUME, ChainStep::BATCH, ChainStep::BATCH, ChainStep::BATCH, ChainStep::DONE};
        ChainLockstep c(r, r.kmax_start);
        ChainController solo(r);
        c.begin(1); solo.begin();
        long long res[1] = {0};
        for (int k = 0; k < 6; k++) {
            const ChainStep a = c.next(&script[k], 50, res), b = solo.next(script[k], 50);
            REQUIRE(a.kind == kinds[k] && a.kind == b.kind && a.kmax == b.kmax && a.iters == b.iters && c.kmax == solo.kmax);
        }
        REQUIRE(res[0] == 2 && solo.pcg_resumes == 2 && solo.kept == 1);
    }
}

}  // namespace

int main(int argc, char **argv) {
    if (argc > 1 && !strcmp(argv[1], "rules")) {
        for (const ChainRules &r : {CHAIN_RULES_SEG, CHAIN_RULES_GEN, CHAIN_RULES_BIG})
            printf("%s kmax_start=%d kmax_floor=%d kmax_cap=%d halt_bump=%d margin=%d iters_per_batch=%d iters_per_graph=%d pcg_cap=%d "
                   "resume_limit=%d pairs_per_resume=%d\n", r.name, r.kmax_start, r.kmax_floor, r.kmax_cap, r.halt_bump, r.margin,
                   r.iters_per_batch, r.iters_per_graph, r.pcg_cap, r.resume_limit(), CHAIN_PAIRS_PER_RESUME);
        return 0;
    }
    for (const Expect &e : TABLE) check_front_end(e);
    check_aggregated();
    check_lockstep(TABLE[0], 24);
    check_lockstep(TABLE[2], 1032);
    printf("%ld checks, chain ok\n", g_checks);
    return 0;
}
