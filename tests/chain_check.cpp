// chain_check.cpp -- the decisions of the adaptive launch chains (csrc/lpbox_chain.h) against a table, as a stand-alone program meant
// to run under AddressSanitizer + UBSan (tests/test_chain.py builds and runs it):
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I<csrc> chain_check.cpp
// The expectations are literals worked out from the formulas of the host loops as they stood before the header existed (run_window and
// batch_run_chain of lpbox_seg_capi.hip, the loop of lpbox_bqp_solve, run_window of lpbox_big_capi.hip), with the two deliberate
// changes of DESIGN.md section 25: the large-LP chain has the resume limit, and all three keep kmax after a batch that completed no PCG.
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

// the lockstep chain of a segmentation batch (batch_run_chain): one kmax for B problems from their votes
void check_aggregated() {
    g_what = "seg batch";
    ChainRules r = CHAIN_RULES_SEG;
    auto agree = [&](int kmax, const std::vector<ChainView> &members) {
        int vote = 0;
        for (const ChainView &v : members) vote = std::max(vote, chain_pcg_vote(r, kmax, v));
        return chain_kmax_for_vote(r, vote);
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
    printf("%ld checks, chain ok\n", g_checks);
    return 0;
}
