// lpbox_lp_layout.cpp -- the host-only layout planner of the batched LP kernels (lpbox_lp_layout.h).  No HIP header: g++ compiles it.
#include "lpbox_lp_layout.h"

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <utility>

LpLayoutOptions lp_layout_options_from_env() {
    LpLayoutOptions o;
    if (const char *e = getenv("LPBOX_LP_THREADS")) o.threads = atoi(e);
    o.nosort = getenv("LPBOX_LP_NOSORT") != nullptr;
    o.nosplit = getenv("LPBOX_LP_NOSPLIT") != nullptr;
    if (const char *e = getenv("LPBOX_LP_BANKAWARE")) o.bankaware = atoi(e) != 0 ? 1 : 0;
    o.noconflict = getenv("LPBOX_LP_NOCONFLICT") != nullptr;
    o.snakerows = getenv("LPBOX_LP_SNAKEROWS") != nullptr;
    o.snakecols = getenv("LPBOX_LP_SNAKECOLS") != nullptr;
    o.nocolsplit = getenv("LPBOX_LP_NOCOLSPLIT") != nullptr;
    if (const char *e = getenv("LPBOX_LP_SPLITBIAS")) o.splitbias = atoi(e);
    if (const char *e = getenv("LPBOX_LP_PCGLOOP")) o.pcg_generic = strcmp(e, "generic") == 0;
    if (const char *e = getenv("LPBOX_LP_REF_VALS")) o.ref_vals = strcmp(e, "lds") == 0 ? 1 : 0;
    return o;
}

// 8 wavefronts (two per SIMD of the CU) with as few slots per thread as the instance allows (1, 2 or 4; the 4-slot variant keeps the
// vectors the PCG loop never reads out of registers); beyond 2048 positions 4 wavefronts x 8 slots.  LPBOX_LP_THREADS overrides
// (tuning only; the reference order has one workgroup size).
int lp_choose_geometry(int nmax, int lmax, int zmax, bool reference_order, const LpLayoutOptions &opt, LpGeometry *geo, std::string *err) {
    char buf[256];
    if (nmax > 65534 || lmax > 65534) {
        *err = "n or l exceeds the uint16 index range of the on-chip kernel";
        return LPBOX_E_UNSUPPORTED;
    }
    const int big = std::max(nmax, lmax);
    int T = 512;                          // 8 waves with short lists beat 4 waves with long ones also at n = 2000 (512 x 4, register-lean variant)
    if (!reference_order && (opt.threads == 256 || opt.threads == 512 || opt.threads == 1024)) T = opt.threads;
    const int max_ept = T == 256 ? 8 : (T == 1024 ? 2 : 4);
    int EPT = 1;
    while (EPT < max_ept && (long)T * EPT < big) EPT *= 2;
    if ((long)T * EPT < big && T == 512) { T = 256; EPT = 1; while (EPT < 8 && (long)T * EPT < big) EPT *= 2; }
    if ((long)T * EPT < big) {
        snprintf(buf, sizeof(buf), "instance with max(n,l)=%d exceeds the on-chip kernel's %d register slots", big, T * EPT);
        *err = buf;
        return LPBOX_E_TOOLARGE;
    }
    geo->colsplit = T == 512 || T == 1024 || (T == 256 && EPT == 2);              // variants compiled with helper lists (LP_DISPATCH)
    geo->T = T; geo->EPT = EPT;
    geo->NS = T * EPT;
    geo->LS = (lmax + 31) & ~31; geo->ZS = (zmax + 7) & ~7;
    return LPBOX_OK;
}

void lp_wave_class_rule(int lanes, const int *row_len, const int *col_len, const int *help_len, const int caps[3], int *class4) {
    const int *len[3] = {row_len, col_len, help_len};
    class4[0] = class4[1] = class4[2] = class4[3] = 0;
    for (int t = 0; t < 3; t++)
        for (int p = 0; p < lanes; p++) {
            class4[t] = std::max(class4[t], (std::min(len[t][p], caps[t]) + 1) / 2);
            if (len[t][p] > caps[t]) class4[3] = 1;
        }
}

// the indices 0 .. size-1 by decreasing key, equal keys in index order (every ordering of the planner is this one)
static std::vector<int> by_decreasing(const std::vector<int> &key) {
    std::vector<int> order(key.size());
    for (size_t i = 0; i < key.size(); i++) order[i] = (int)i;
    std::stable_sort(order.begin(), order.end(), [&](int a, int c) { return key[a] > key[c]; });
    return order;
}

int lp_plan_direct_rows(const LpProblemView &P, std::vector<int> *gidx_of_row) {
    std::vector<int> key(P.l), used(P.n, 0);
    for (int r = 0; r < P.l; r++) key[r] = -(P.rowptr[r + 1] - P.rowptr[r]);        // ascending length
    std::vector<char> isD(P.l, 0);
    for (int r : by_decreasing(key)) {
        bool disjoint = true;
        for (int e = P.rowptr[r]; e < P.rowptr[r + 1] && disjoint; e++) disjoint = !used[P.colidx[e]];
        if (!disjoint) continue;
        isD[r] = 1;
        for (int e = P.rowptr[r]; e < P.rowptr[r + 1]; e++) used[P.colidx[e]] = 1;
    }
    gidx_of_row->assign(P.l, -1);
    int nG = 0;
    for (int r = 0; r < P.l; r++) if (!isD[r]) (*gidx_of_row)[r] = nG++;
    return nG;
}

namespace {

void size_tables(const LpProblemView &P, int NS, LpInstanceLayout &L) {
    L.rs_ptr.assign(NS + 1, 0); L.cs_ptr.assign(NS + 1, 0); L.hs_ptr.assign(NS + 1, 0);
    L.rs_col.assign(P.nnz, 0); L.cs_row.assign(P.nnz, 0);
    L.rid.assign(NS, 0xFFFF); L.rgl.assign(NS, 0); L.rmeta.assign(NS, 0x10); L.cmeta.assign(NS, 0);
}

struct Task { int row, g, G; };                    // lane g of the G lanes that share a row
struct Quad { int v[4]; int tau, tail, slot; };    // a long column and three short ones in four adjacent lanes; the long one keeps tau entries

// The state the steps of lp_plan_layout hand on to each other.
struct Plan {
    const LpProblemView &P;
    const LpGeometry &geo;
    const LpLayoutOptions &opt;
    LpInstanceLayout &L;
    const int NS, W;                   // storage positions, wavefronts
    const bool bank_aware;
    std::vector<int> rorder;           // the rows in task order
    std::vector<Task> task_of_slot;
    std::vector<int> slot_of_row;      // storage slot of lane 0 of the row's task group (lanes are consecutive)
    int max_chain = 1;                 // longest list of a row task
    std::vector<int> var_of_pos;
    std::vector<int> rpos;             // row storage index in the gathered l-vectors
    // bank-aware column placement.  occ[j]: occurrences of column j in the row-gather instructions, (half-wave group of the task slot,
    // entry index k); cnt: how many variables placed so far read bank class c in that instruction
    std::vector<std::vector<std::pair<int, int>>> occ;
    std::vector<int> cnt;

    Plan(const LpProblemView &P_, const LpGeometry &g, const LpLayoutOptions &o, LpInstanceLayout &L_)
        : P(P_), geo(g), opt(o), L(L_), NS(g.NS), W(g.T / 64),
          bank_aware(!o.nosort && !(o.noconflict || !(o.bankaware >= 0 ? o.bankaware != 0 : g.EPT >= 4))) {}

    int clen(int j) const { return j < 0 ? 0 : P.colptr[j + 1] - P.colptr[j]; }
    int rlen(int r) const { return P.rowptr[r + 1] - P.rowptr[r]; }
    int chain(int r) const { return (rlen(r) + L.rowG[r] - 1) / L.rowG[r]; }
    // block b of 64 consecutive (sorted) items -> storage slot: slots are dealt to the waves in snake order so that every
    // wave receives a similar amount of gather work
    int block_base(int blk) const {
        const int slot = blk / W, r = blk % W;
        const int wv = (slot & 1) ? (W - 1 - r) : r;
        return slot * geo.T + wv * 64;
    }
    long place_cost(int j, int c) const {
        long cost = 0;
        for (auto &o : occ[j]) cost += cnt[((size_t)o.first * max_chain + o.second) * 32 + c];
        return cost;
    }
    void place_commit(int j, int p) {
        for (auto &o : occ[j]) cnt[((size_t)o.first * max_chain + o.second) * 32 + (p % 32)]++;
        L.cpos[j] = p; var_of_pos[p] = j;
    }
};

// Blocks of 64 lanes -> first storage slot of the block, longest-first to the least loaded wave that has a free slot.  A wave walks
// every slot to the longest list of its 64 lanes, in chunks of 4 gathers, and the phase ends when the slowest wave does; the sort that
// forms the blocks leaves their maxima not monotone, and the snake deal left the waves of a multi-slot layout up to 35 % apart
// (j=500/k=2000: 24 ... 44 chunks-of-4 entries per wave).
std::vector<int> deal_longest_first(const std::vector<int> &cost, const LpGeometry &geo) {
    const int nb = (int)cost.size(), W = geo.T / 64;
    std::vector<int> base(nb, 0), load(W, 0), used(W, 0);
    for (int b : by_decreasing(cost)) {
        int best = -1;
        for (int w = 0; w < W; w++) if (used[w] < geo.EPT && (best < 0 || load[w] < load[best])) best = w;
        base[b] = used[best] * geo.T + best * 64;
        used[best]++; load[best] += cost[b];
    }
    return base;
}

// ---- rows: G lanes share a row so that no lane walks more than ~L entries; lane g takes entries g, g+G, ... ----
void split_rows(Plan &s) {
    s.L.rowG.assign(s.P.l, 1);
    if (s.opt.nosplit) return;
    for (int Lt = 4; Lt <= 65536; Lt++) {
        long tot = 0;
        for (int r = 0; r < s.P.l; r++) {
            const int m = s.rlen(r);
            int G = 1;
            while (G < 8 && (m + G - 1) / G > Lt) G *= 2;
            s.L.rowG[r] = G; tot += G;
        }
        if (tot <= (long)s.NS) break;
    }
}

// Row tasks sorted by (lanes per row, list length), in blocks of 64 -> (wave, slot): snake order, or (multi-slot variants) by load.
// Where a row's task sits changes nothing in the arithmetic (a row sum is the same sum in any lane), only the time.
void deal_row_tasks(Plan &s) {
    const std::vector<int> &rowG = s.L.rowG;
    const bool nosort = s.opt.nosort;
    std::vector<int> key(s.P.l);
    for (int r = 0; r < s.P.l; r++) key[r] = rowG[r] * 65536 + (nosort ? 0 : s.chain(r));      // a list holds < 65536 entries
    s.rorder = by_decreasing(key);
    std::vector<int> row_block_base;
    if (!nosort && s.geo.EPT >= 2 && !s.opt.snakerows) {
        long ntask = 0;
        for (int r = 0; r < s.P.l; r++) ntask += rowG[r];
        std::vector<int> cost((size_t)((ntask + 63) / 64), 0);
        long qq = 0;
        for (int r : s.rorder) { for (int g = 0; g < rowG[r]; g++, qq++) cost[qq / 64] = std::max(cost[qq / 64], s.chain(r)); }
        for (int &c : cost) c = (c + 3) / 4 * 4;
        row_block_base = deal_longest_first(cost, s.geo);
    }
    s.task_of_slot.assign(s.NS, Task{-1, 0, 1});
    s.slot_of_row.assign(s.P.l, 0);
    int q = 0;
    for (int r : s.rorder) {
        s.max_chain = std::max(s.max_chain, s.chain(r));
        for (int g = 0; g < rowG[r]; g++, q++) {
            const int tp = nosort ? q : (row_block_base.empty() ? s.block_base(q / 64) : row_block_base[q / 64]) + q % 64;
            if (g == 0) s.slot_of_row[r] = tp;
            s.task_of_slot[tp] = Task{r, g, rowG[r]};
        }
    }
}

// Columns by decreasing length (stable), whole and unplaced; with the bank-aware choice on, where the row gathers read each of them.
void order_columns(Plan &s) {
    const LpProblemView &P = s.P;
    std::vector<int> key(P.n, 0);
    for (int j = 0; j < P.n && !s.opt.nosort; j++) key[j] = s.clen(j);
    s.L.cperm = by_decreasing(key);
    s.L.cpos.resize(P.n);
    s.var_of_pos.assign(s.NS, -1);
    s.L.col_own.assign(P.n, 0); s.L.col_help.assign((size_t)4 * P.n, 0);
    for (int j = 0; j < P.n; j++) s.L.col_own[j] = s.clen(j);
    s.L.help_of_pos.clear();
    s.occ.assign(P.n, {});
    if (!s.bank_aware) return;
    s.cnt.assign((size_t)(s.NS / 32) * s.max_chain * 32, 0);
    for (int r = 0; r < P.l; r++) {
        const int G = s.L.rowG[r];
        for (int e = P.rowptr[r]; e < P.rowptr[r + 1]; e++) {
            const int ee = e - P.rowptr[r];
            s.occ[P.colidx[e]].push_back({(s.slot_of_row[r] + ee % G) / 32, ee / G});
        }
    }
}

// LPBOX_LP_NOSORT: variable j at position j.
void place_cols_unsorted(Plan &s) {
    for (int q = 0; q < s.P.n; q++) { s.L.cpos[s.L.cperm[q]] = q; s.var_of_pos[q] = s.L.cperm[q]; }
}

// Blocks of 64 by decreasing column length (stable) are dealt to the waves; INSIDE a block the lane (= LDS bank class pos % 32 of the
// variable in the gathered vector) is chosen greedily so that the 32 lanes of a half-wave gather from different banks in as many
// row-gather instructions as possible (an instruction = the k-th list entry of the 32 row tasks of one half-wave).
void place_cols_blocks(Plan &s) {
    for (int blk = 0; blk * 64 < s.P.n; blk++) {
        bool used[64] = {false};
        const int base = s.block_base(blk);
        for (int q = blk * 64; q < std::min(s.P.n, blk * 64 + 64); q++) {
            const int j = s.L.cperm[q];
            int best = -1; long best_cost = 0;
            for (int c = 0; c < 32; c++) {
                if (used[c] && used[c + 32]) continue;
                const long cost = s.bank_aware ? s.place_cost(j, c) : 0;
                if (best < 0 || cost < best_cost) { best = c; best_cost = cost; }
            }
            const int lane = used[best] ? best + 32 : best;
            used[lane] = true;
            s.place_commit(j, base + lane);
        }
    }
}

constexpr int QW = 16, CH = 8;         // quads per wave (= per block of 64 positions), register capacity of a helper list

// The per-wave issue rate of LDS gathers, not the LDS array, bounds a sparse product, so what counts is the LONGEST list of a wave.
// Columns are grouped in quads of adjacent lanes, one long column with three short ones (long ranks ascending meet short ranks
// descending, so the quads of a wave look alike): the long column keeps its first tau entries (tau = longest companion), the rest is
// dealt in consecutive chunks to the other three lanes (helper lists, summed into a second accumulator and combined over the quad,
// lp_window_kernel cols_gather).  A block splits only where that shortens its longest list.  Returns the cost of every block (own list
// + helper list, in chunks of 4).
std::vector<int> form_quads(const Plan &s, std::vector<Quad> &quad, std::vector<int> &quad_of_var) {
    const int Q = s.NS / 4;
    auto var_of_rank = [&](int r) { return r < s.P.n ? s.L.cperm[r] : -1; };
    auto r2 = [](int v) { return (v + 1) & ~1; };
    quad.assign(Q, Quad{});
    quad_of_var.assign(s.P.n, -1);
    std::vector<int> blk_cost(Q / QW, 0);
    for (int w = 0; w < Q / QW; w++) {
        int A = 0, Bm = 0, Lm = 0;
        for (int qi = 0; qi < QW; qi++) {
            Quad &qd = quad[w * QW + qi];
            qd.v[0] = var_of_rank(w * QW + qi);
            for (int t = 0; t < 3; t++) qd.v[1 + t] = var_of_rank(s.NS - 1 - (3 * (w * QW + qi) + t));
            const int L = s.clen(qd.v[0]);
            const int s1 = std::max(s.clen(qd.v[1]), std::max(s.clen(qd.v[2]), s.clen(qd.v[3])));
            qd.tau = std::min(L, std::max(s1, L - 3 * CH));
            qd.tail = L - qd.tau; qd.slot = -1;
            A = std::max(A, std::max(qd.tau, s1)); Bm = std::max(Bm, (qd.tail + 2) / 3); Lm = std::max(Lm, std::max(L, s1));
            for (int t = 0; t < 4; t++) if (qd.v[t] >= 0) quad_of_var[qd.v[t]] = w * QW + qi;
        }
        bool split = true;
        if (r2(A) + r2(Bm) + s.opt.splitbias >= r2(Lm)) {      // splitting does not shorten this wave's longest list
            split = false;
            for (int qi = 0; qi < QW; qi++) { Quad &qd = quad[w * QW + qi]; qd.tau = s.clen(qd.v[0]); qd.tail = 0; }
        }
        blk_cost[w] = split ? (A + 3) / 4 * 4 + (Bm + 3) / 4 * 4 : (Lm + 3) / 4 * 4;
    }
    return blk_cost;
}

// chunks of the tails, in lane order over the helper lanes of the quad
void deal_helper_chunks(Plan &s, const std::vector<Quad> &quad) {
    s.L.help_of_pos.assign(s.NS, {-1, 0, 0});
    for (auto &qd : quad) {
        if (qd.tail <= 0 || qd.v[0] < 0) continue;
        const int jl = qd.v[0], pl = s.L.cpos[jl];
        s.L.col_own[jl] = qd.tau;
        int given = 0, hl = 0;
        for (int p = 4 * qd.slot; p < 4 * qd.slot + 4; p++) {
            if (p == pl) continue;
            const int c = qd.tail / 3 + (hl < qd.tail % 3 ? 1 : 0);
            s.L.help_of_pos[p] = {jl, qd.tau + given, c};
            s.L.col_help[(size_t)4 * jl + (p - 4 * qd.slot)] = c;
            given += c; hl++;
        }
    }
}

// Quads with helper chunks.  Multi-slot layouts deal the logical blocks of columns to (wave, slot) by load like the row tasks; unlike
// the rows this moves variables to other lanes, i.e. it is part of the layout the oracle mirrors through lpbox_get_layout.
void place_cols_quads(Plan &s) {
    const int Q = s.NS / 4;
    std::vector<Quad> quad;
    std::vector<int> quad_of_var;
    const std::vector<int> blk_cost = form_quads(s, quad, quad_of_var);
    std::vector<int> col_block_base;
    if (s.geo.EPT >= 2 && !s.opt.snakecols) col_block_base = deal_longest_first(blk_cost, s.geo);
    // lane of every column: bank-aware greedy as in place_cols_blocks, inside the wave's free quad slots / the quad's free lanes
    std::vector<char> used(s.NS, 0), slot_used(Q, 0);
    auto qbase = [&](int w) { return (col_block_base.empty() ? s.block_base(w) : col_block_base[w]) / 4; };    // first quad slot of the 64 positions that hold logical block w
    for (int qq = 0; qq < s.P.n; qq++) {
        const int j = s.L.cperm[qq];
        Quad &qd = quad[quad_of_var[j]];
        const int w = quad_of_var[j] / QW;
        int best = -1; long best_cost = 0;
        for (int t = (qd.slot >= 0 ? qd.slot : qbase(w)); t < (qd.slot >= 0 ? qd.slot + 1 : qbase(w) + QW); t++) {
            if (qd.slot < 0 && slot_used[t]) continue;
            for (int p = 4 * t; p < 4 * t + 4; p++) {
                if (used[p]) continue;
                const long cost = s.bank_aware ? s.place_cost(j, p % 32) : 0;
                if (best < 0 || cost < best_cost) { best = p; best_cost = cost; }
            }
        }
        if (qd.slot < 0) { qd.slot = best / 4; slot_used[qd.slot] = 1; }
        used[best] = 1;
        s.place_commit(j, best);
    }
    for (int qd_i = 0; qd_i < Q; qd_i++) {               // quads made of holes only still need a slot (nothing is stored there)
        Quad &qd = quad[qd_i];
        if (qd.slot >= 0) continue;
        for (int t = qbase(qd_i / QW); t < qbase(qd_i / QW) + QW; t++) if (!slot_used[t]) { qd.slot = t; slot_used[t] = 1; break; }
    }
    deal_helper_chunks(s, quad);
}

// ---- row storage index in the gathered l-vectors (bank class rpos % 32), chosen like the lanes of the columns, for the column gathers ----
void place_rows_in_bank_classes(Plan &s) {
    const LpProblemView &P = s.P;
    const LpInstanceLayout &L = s.L;
    s.rpos.resize(P.l);
    for (int r = 0; r < P.l; r++) s.rpos[r] = r;
    if (!s.bank_aware) return;
    s.L.identity_rows = false;
    int max_col = 1;
    for (int j = 0; j < P.n; j++) max_col = std::max(max_col, s.clen(j));
    const int ngrp = s.NS / 32, cap = s.geo.LS / 32;
    std::vector<int> cnt((size_t)ngrp * 2 * max_col * 32, 0), usedc(32, 0);
    std::vector<int> key(P.l);
    for (int r = 0; r < P.l; r++) key[r] = s.rlen(r);
    // the column-gather instruction that reads row r for column j: (half-wave group of the reading lane, entry index in its
    // list); helper lists are separate instructions, numbered after the own lists
    auto instr_of = [&](int j, int r) {
        const int rank = (int)(std::lower_bound(P.rowidx + P.colptr[j], P.rowidx + P.colptr[j + 1], r) - (P.rowidx + P.colptr[j]));
        if (rank < L.col_own[j]) return (size_t)(L.cpos[j] / 32) * 2 * max_col + rank;
        int first = L.col_own[j];
        const int q0 = L.cpos[j] & ~3;
        for (int q = 0; q < 4; q++) {
            const int c = L.col_help[(size_t)4 * j + q];
            if (rank < first + c) return (size_t)((q0 + q) / 32) * 2 * max_col + max_col + (rank - first);
            first += c;
        }
        return (size_t)0;
    };
    std::vector<size_t> ins(P.nnz);                 // gather instruction of every entry, row-major
    for (int r = 0; r < P.l; r++)
        for (int e = P.rowptr[r]; e < P.rowptr[r + 1]; e++) ins[e] = instr_of(P.colidx[e], r) * 32;
    // (re-choosing every row's class against all the others in further passes was measured: 77.9 / 78.1 / 78.2 us per iteration
    // of the four-slot variant with 0 / 3 / 10 passes -- nothing; one greedy pass stays)
    for (int r : by_decreasing(key)) {
        int best = -1; long best_cost = 0;
        for (int c = 0; c < 32; c++) {
            if (usedc[c] >= cap) continue;
            long cost = 0;
            for (int e = P.rowptr[r]; e < P.rowptr[r + 1]; e++) cost += cnt[ins[e] + c];
            if (best < 0 || cost < best_cost) { best = c; best_cost = cost; }
        }
        for (int e = P.rowptr[r]; e < P.rowptr[r + 1]; e++) cnt[ins[e] + best]++;
        s.rpos[r] = best + 32 * usedc[best]++;
    }
}

void emit_tables(Plan &s) {
    const LpProblemView &P = s.P;
    LpInstanceLayout &L = s.L;
    size_tables(P, s.NS, L);
    int k = 0;
    for (int p = 0; p < s.NS; p++) {
        L.cs_ptr[p] = k;
        const int j = s.var_of_pos[p];
        if (j < 0) continue;
        for (int e = P.colptr[j]; e < P.colptr[j] + L.col_own[j]; e++) L.cs_row[k++] = (uint16_t)s.rpos[P.rowidx[e]];
        L.cmeta[p] = (uint16_t)(s.clen(j) | (L.col_own[j] < s.clen(j) ? 0x8000 : 0));
    }
    L.cs_ptr[s.NS] = k;
    for (int p = 0; p < s.NS; p++) {                          // helper chunks follow the own parts in the same index pool
        L.hs_ptr[p] = k;
        if (L.help_of_pos.empty() || L.help_of_pos[p].var < 0) continue;
        const LpHelpChunk &hp = L.help_of_pos[p];
        for (int e = P.colptr[hp.var] + hp.first; e < P.colptr[hp.var] + hp.first + hp.count; e++) L.cs_row[k++] = (uint16_t)s.rpos[P.rowidx[e]];
    }
    L.hs_ptr[s.NS] = k;
    k = 0;
    for (int tp = 0; tp < s.NS; tp++) {
        L.rs_ptr[tp] = k;
        const Task &t = s.task_of_slot[tp];
        if (t.row < 0) continue;
        for (int e = P.rowptr[t.row] + t.g; e < P.rowptr[t.row + 1]; e += t.G) L.rs_col[k++] = (uint16_t)L.cpos[P.colidx[e]];
        L.rid[tp] = (uint16_t)t.row;
        L.rgl[tp] = (uint16_t)s.rpos[t.row];
        L.rmeta[tp] = (uint16_t)((t.G << 4) | t.g);
    }
    L.rs_ptr[s.NS] = k;
}

// class of every wavefront in the 512 x 1 kernel's PCG loop, from the emitted pointer tables
void classify_waves(Plan &s, const int caps[3]) {
    s.L.wave_class.clear();
    if (s.geo.T != 512 || s.geo.EPT != 1) return;
    const int *ptr[3] = {s.L.rs_ptr.data(), s.L.cs_ptr.data(), s.L.hs_ptr.data()};
    for (int w = 0; w < s.W; w++) {
        int len[3][64], cls[4];
        for (int t = 0; t < 3; t++)
            for (int p = 0; p < 64; p++) len[t][p] = ptr[t][64 * w + p + 1] - ptr[t][64 * w + p];
        lp_wave_class_rule(64, len[0], len[1], len[2], caps, cls);
        s.L.wave_class.insert(s.L.wave_class.end(), cls, cls + 4);
    }
}

}  // namespace

void lp_plan_layout(const LpProblemView &P, const LpGeometry &geo, const LpLayoutOptions &opt, const int caps[3], LpInstanceLayout *out) {
    *out = LpInstanceLayout();
    Plan s(P, geo, opt, *out);
    split_rows(s);
    deal_row_tasks(s);
    order_columns(s);
    if (opt.nosort) place_cols_unsorted(s);
    else if (!(geo.colsplit && !opt.nocolsplit)) place_cols_blocks(s);
    else place_cols_quads(s);
    place_rows_in_bank_classes(s);
    emit_tables(s);
    classify_waves(s, caps);
}

void lp_plan_identity_layout(const LpProblemView &P, const LpGeometry &geo, LpInstanceLayout *out) {
    LpInstanceLayout &L = *out;
    L = LpInstanceLayout();
    L.cpos.resize(P.n); L.cperm.resize(P.n);
    for (int j = 0; j < P.n; j++) { L.cpos[j] = j; L.cperm[j] = j; }
    L.rowG.assign(P.l, 1);
    L.col_own.resize(P.n);
    for (int j = 0; j < P.n; j++) L.col_own[j] = P.colptr[j + 1] - P.colptr[j];
    L.col_help.assign((size_t)4 * P.n, 0);
    size_tables(P, geo.NS, L);
    for (int p = 0; p <= geo.NS; p++) {
        L.cs_ptr[p] = P.colptr[std::min(p, P.n)];
        L.rs_ptr[p] = P.rowptr[std::min(p, P.l)];
        L.hs_ptr[p] = P.nnz;
    }
    for (int k = 0; k < P.nnz; k++) { L.cs_row[k] = (uint16_t)P.rowidx[k]; L.rs_col[k] = (uint16_t)P.colidx[k]; }
    for (int j = 0; j < P.n; j++) L.cmeta[j] = (uint16_t)L.col_own[j];
    for (int r = 0; r < P.l; r++) { L.rid[r] = (uint16_t)r; L.rgl[r] = (uint16_t)r; }
}
