// lp_layout_check.cpp -- invariants of the host layout planner (csrc/lpbox_lp_layout.h) on generated instances, as a stand-alone
// program meant to run under AddressSanitizer + UBSan (tests/test_lp_layout.py builds and runs it):
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I<csrc> lp_layout_check.cpp <csrc>/lpbox_lp_layout.cpp
// Every instance is planned under every geometry lp_choose_geometry can return for it and under the knob combinations of the layout
// fixture; what is checked is what the kernels rely on, whatever the planner decided.
#include "lpbox_lp_layout.h"

#include <algorithm>
#include <cstdio>
#include <cstdlib>

namespace {

unsigned long long g_state = 88172645463325252ULL;
unsigned rnd() { g_state = g_state * 6364136223846793005ULL + 1442695040888963407ULL; return (unsigned)(g_state >> 33); }
int rnd_in(int lo, int hi) { return lo + (int)(rnd() % (unsigned)(hi - lo + 1)); }

const int CAPS[3] = {12, 12, 8};      // register entries of a lane's row, own-column and helper list (include/lpbox_hip.h)
const char *g_what = "";
long g_plans = 0;

#define REQUIRE(cond)                                                                         \
    do {                                                                                      \
        if (!(cond)) { printf("FAILED %s: %s (line %d)\n", g_what, #cond, __LINE__); exit(1); } \
    } while (0)

struct Instance {
    int n = 0, l = 0;
    std::vector<int> colptr, rowidx, rowptr, colidx;
    LpProblemView view() const {
        LpProblemView P;
        P.n = n; P.l = l; P.nnz = (int)rowidx.size();
        P.colptr = colptr.data(); P.rowidx = rowidx.data(); P.rowptr = rowptr.data(); P.colidx = colidx.data();
        return P;
    }
};

// shape 0: random, with empty rows and columns; 1: plus one column of length l; 2: plus one row of length n
Instance make_instance(int n, int l, int per_col, int shape) {
    Instance I;
    I.n = n; I.l = l;
    std::vector<char> in_col(l);
    const int dense_col = shape == 1 ? rnd_in(0, n - 1) : -1, dense_row = shape == 2 ? rnd_in(0, l - 1) : -1;
    const int empty_row = l > 1 ? (dense_row + 1) % l : -1;
    I.colptr.assign(1, 0);
    for (int j = 0; j < n; j++) {
        std::fill(in_col.begin(), in_col.end(), 0);
        const int k = (j % 7 == 3 && j != dense_col) ? 0 : rnd_in(0, std::min(l, 2 * per_col));     // every seventh column is empty
        for (int t = 0; t < k; t++) in_col[rnd_in(0, l - 1)] = 1;
        if (j == dense_col) std::fill(in_col.begin(), in_col.end(), 1);
        if (dense_row >= 0) in_col[dense_row] = 1;
        if (empty_row >= 0 && j != dense_col) in_col[empty_row] = 0;
        for (int r = 0; r < l; r++) if (in_col[r]) I.rowidx.push_back(r);
        I.colptr.push_back((int)I.rowidx.size());
    }
    I.rowptr.assign(l + 1, 0);
    for (int r : I.rowidx) I.rowptr[r + 1]++;
    for (int r = 0; r < l; r++) I.rowptr[r + 1] += I.rowptr[r];
    I.colidx.assign(I.rowidx.size(), 0);
    std::vector<int> cur(I.rowptr.begin(), I.rowptr.end() - 1);
    for (int j = 0; j < n; j++)
        for (int k = I.colptr[j]; k < I.colptr[j + 1]; k++) I.colidx[cur[I.rowidx[k]]++] = j;
    return I;
}

void check_plan(const Instance &I, const LpGeometry &geo, const LpInstanceLayout &L, bool reference_order) {
    const int n = I.n, l = I.l, nnz = (int)I.rowidx.size(), NS = geo.NS, LS = geo.LS;
    g_plans++;
    // cpos is injective into [0, NS)
    REQUIRE((int)L.cpos.size() == n);
    std::vector<int> var_of_pos(NS, -1);
    for (int j = 0; j < n; j++) {
        REQUIRE(L.cpos[j] >= 0 && L.cpos[j] < NS && var_of_pos[L.cpos[j]] < 0);
        var_of_pos[L.cpos[j]] = j;
    }
    // the three pointer tables are monotone and chained
    for (const std::vector<int> *t : {&L.rs_ptr, &L.cs_ptr, &L.hs_ptr}) {
        REQUIRE((int)t->size() == NS + 1);
        for (int p = 0; p < NS; p++) REQUIRE((*t)[p] <= (*t)[p + 1]);
    }
    REQUIRE(L.rs_ptr[0] == 0 && L.rs_ptr[NS] == nnz && L.cs_ptr[0] == 0 && L.cs_ptr[NS] == L.hs_ptr[0] && L.hs_ptr[NS] == nnz);
    REQUIRE((int)L.rs_col.size() == nnz && (int)L.cs_row.size() == nnz);
    REQUIRE((int)L.rid.size() == NS && (int)L.rgl.size() == NS && (int)L.rmeta.size() == NS && (int)L.cmeta.size() == NS);
    // rows: rgl is injective over the rows and below LS; every lane of a row agrees on it; lanes g = 0 .. G-1 are all there
    std::vector<int> rpos(l, -1), row_of_rpos(LS, -1), lanes_seen(l, 0);
    REQUIRE((int)L.rowG.size() == l);
    for (int tp = 0; tp < NS; tp++) {
        if (L.rid[tp] == 0xFFFF) { REQUIRE(L.rs_ptr[tp] == L.rs_ptr[tp + 1]); continue; }
        const int r = L.rid[tp], G = L.rmeta[tp] >> 4, g = L.rmeta[tp] & 15;
        REQUIRE(r < l && L.rgl[tp] < LS && G == L.rowG[r] && g < G && (G == 1 || G == 2 || G == 4 || G == 8));
        REQUIRE(rpos[r] < 0 || rpos[r] == L.rgl[tp]);
        REQUIRE(row_of_rpos[L.rgl[tp]] < 0 || row_of_rpos[L.rgl[tp]] == r);
        rpos[r] = L.rgl[tp]; row_of_rpos[L.rgl[tp]] = r;
        lanes_seen[r] |= 1 << g;
    }
    for (int r = 0; r < l; r++) REQUIRE(lanes_seen[r] == (1 << L.rowG[r]) - 1);
    // every entry of E occurs exactly once over the row-task lists (as the storage position of its variable)
    std::vector<char> seen(nnz, 0);
    auto csr_entry = [&](int r, int j) {
        const int *b = I.colidx.data() + I.rowptr[r], *e = I.colidx.data() + I.rowptr[r + 1], *at = std::lower_bound(b, e, j);
        return at != e && *at == j ? (int)(at - I.colidx.data()) : -1;
    };
    for (int tp = 0; tp < NS; tp++)
        for (int k = L.rs_ptr[tp]; k < L.rs_ptr[tp + 1]; k++) {
            REQUIRE(L.rs_col[k] < NS && var_of_pos[L.rs_col[k]] >= 0);
            const int e = csr_entry(L.rid[tp], var_of_pos[L.rs_col[k]]);
            REQUIRE(e >= 0 && !seen[e]);
            seen[e] = 1;
        }
    REQUIRE(std::count(seen.begin(), seen.end(), 1) == nnz);
    // every entry of E occurs exactly once over the own plus helper lists of its column (as the storage index of its row)
    std::fill(seen.begin(), seen.end(), 0);
    auto take = [&](int j, int k) {
        REQUIRE(L.cs_row[k] < LS && row_of_rpos[L.cs_row[k]] >= 0);
        const int e = csr_entry(row_of_rpos[L.cs_row[k]], j);
        REQUIRE(e >= 0 && !seen[e]);
        seen[e] = 1;
    };
    REQUIRE((int)L.col_own.size() == n && (int)L.col_help.size() == 4 * n);
    REQUIRE(L.help_of_pos.empty() || (int)L.help_of_pos.size() == NS);
    for (int p = 0; p < NS; p++) {
        const int j = var_of_pos[p], own = L.cs_ptr[p + 1] - L.cs_ptr[p], help = L.hs_ptr[p + 1] - L.hs_ptr[p];
        if (j < 0) REQUIRE(own == 0 && L.cmeta[p] == 0);
        else {
            const int len = I.colptr[j + 1] - I.colptr[j];
            REQUIRE(own == L.col_own[j] && L.cmeta[p] == (len | (own < len ? 0x8000 : 0)));
            REQUIRE(own + L.col_help[4 * j] + L.col_help[4 * j + 1] + L.col_help[4 * j + 2] + L.col_help[4 * j + 3] == len);
            REQUIRE(L.col_help[4 * j + p % 4] == 0);
            for (int k = L.cs_ptr[p]; k < L.cs_ptr[p + 1]; k++) take(j, k);
        }
        if (L.help_of_pos.empty() || L.help_of_pos[p].var < 0) { REQUIRE(help == 0); continue; }
        // helper chunks sit only in the other lanes of the owner's quad
        const int jl = L.help_of_pos[p].var;
        REQUIRE(jl < n && L.cpos[jl] / 4 == p / 4 && L.cpos[jl] != p && help == L.help_of_pos[p].count && help == L.col_help[4 * jl + p % 4]);
        for (int k = L.hs_ptr[p]; k < L.hs_ptr[p + 1]; k++) take(jl, k);
    }
    REQUIRE(std::count(seen.begin(), seen.end(), 1) == nnz);
    // wave_class is the rule applied to the emitted pointer tables (512 x 1, default order), else empty
    if (reference_order || geo.T != 512 || geo.EPT != 1) { REQUIRE(L.wave_class.empty()); return; }
    REQUIRE((int)L.wave_class.size() == 4 * 8);
    const std::vector<int> *ptr[3] = {&L.rs_ptr, &L.cs_ptr, &L.hs_ptr};
    for (int w = 0; w < 8; w++) {
        int cls[4] = {0, 0, 0, 0};
        for (int t = 0; t < 3; t++)
            for (int p = 64 * w; p < 64 * w + 64; p++) {
                const int len = (*ptr[t])[p + 1] - (*ptr[t])[p];
                cls[t] = std::max(cls[t], (std::min(len, CAPS[t]) + 1) / 2);
                if (len > CAPS[t]) cls[3] = 1;
            }
        for (int c = 0; c < 4; c++) REQUIRE(L.wave_class[4 * w + c] == cls[c]);
    }
}

void check_instance(const Instance &I) {
    static char what[160];
    g_what = what;
    const LpProblemView P = I.view();
    std::vector<LpLayoutOptions> knobs(9);
    knobs[1].bankaware = 1; knobs[2].bankaware = 0; knobs[3].nosort = true; knobs[4].nosplit = true; knobs[5].nocolsplit = true;
    knobs[6].splitbias = 0; knobs[7].snakerows = true; knobs[8].snakecols = true;
    for (int threads : {0, 256, 1024}) {             // 0: the default (512, or 256 x 8 beyond 2048 positions)
        for (size_t k = 0; k < knobs.size(); k++) {
            LpLayoutOptions opt = knobs[k];
            opt.threads = threads;
            LpGeometry geo;
            std::string err;
            snprintf(what, sizeof(what), "n=%d l=%d nnz=%d threads=%d knobs=%zu", I.n, I.l, P.nnz, threads, k);
            if (lp_choose_geometry(I.n, I.l, P.nnz, false, opt, &geo, &err) != LPBOX_OK) { REQUIRE(!err.empty()); continue; }
            REQUIRE(geo.NS == geo.T * geo.EPT && geo.NS >= std::max(I.n, I.l) && geo.LS >= I.l && geo.LS % 32 == 0 && geo.ZS >= P.nnz);
            LpInstanceLayout L;
            lp_plan_layout(P, geo, opt, CAPS, &L);
            check_plan(I, geo, L, false);
        }
    }
    LpGeometry geo;
    std::string err;
    snprintf(what, sizeof(what), "n=%d l=%d nnz=%d reference order", I.n, I.l, P.nnz);
    REQUIRE(lp_choose_geometry(I.n, I.l, P.nnz, true, LpLayoutOptions(), &geo, &err) == LPBOX_OK && geo.T == 512);
    LpInstanceLayout L;
    lp_plan_identity_layout(P, geo, &L);
    check_plan(I, geo, L, true);
    for (int j = 0; j < I.n; j++) REQUIRE(L.cpos[j] == j);
    // the direct mode's row choice: the closed-form rows are pairwise disjoint, the dense ones are numbered in row order
    std::vector<int> gidx, owner(I.n, -1);
    const int nG = lp_plan_direct_rows(P, &gidx);
    int next = 0;
    for (int r = 0; r < I.l; r++) {
        if (gidx[r] >= 0) { REQUIRE(gidx[r] == next); next++; continue; }
        for (int e = I.rowptr[r]; e < I.rowptr[r + 1]; e++) { REQUIRE(owner[I.colidx[e]] < 0); owner[I.colidx[e]] = r; }
    }
    REQUIRE(next == nG);
}

}  // namespace

int main(int argc, char **argv) {
    const int extra = argc > 1 ? atoi(argv[1]) : 6;           // random sizes on top of the fixed ones
    const int fixed_n[] = {2, 3, 64, 65, 511, 512, 513, 1024, 1025, 2048};
    int shape = 0;
    for (int n : fixed_n) {
        int l = n <= 3 ? n + 1 : rnd_in(1, std::min(2048, 2 * n));
        if (l == n) l--;
        check_instance(make_instance(n, l, rnd_in(1, 6), shape++ % 3));
    }
    check_instance(make_instance(700, 2048, 2, 0));             // l at the limit, more rows than variables
    check_instance(make_instance(2047, 1, 1, 2));               // a single row that holds every variable
    check_instance(make_instance(40, 300, 150, 1));             // long columns: split over their quads
    for (int t = 0; t < extra; t++) {
        const int n = rnd_in(2, 2048);
        int l = rnd_in(1, 2048);
        if (l == n) l = l > 1 ? l - 1 : l + 1;
        check_instance(make_instance(n, l, rnd_in(1, 8), t % 3));
    }
    printf("lp_layout_check: %ld plans ok\n", g_plans);
    return 0;
}
