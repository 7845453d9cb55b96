// lpbox_lp_layout.h -- host-only planner of the storage layout of the batched LP kernels (lpbox_lp_kernels.hip,
// lpbox_lp_ref_kernels.hip): which lane holds which variable, which lanes share a row, which index lists every lane walks.
// Plain C++17, no HIP: everything here is a pure function of the instance, the geometry and the options, so it runs (and is tested)
// on a machine without a GPU.  lpbox_capi.hip plans with it and uploads what it returns ("Host layout planner").
#ifndef LPBOX_LP_LAYOUT_H
#define LPBOX_LP_LAYOUT_H

#include "../../include/lpbox_hip.h"

#include <cstdint>
#include <string>
#include <vector>

// The LPBOX_LP_* environment knobs (tuning, A/B runs and tests; none of them changes a result beyond the summation order the oracle
// mirrors through the layout getters).  Read once per handle, when its layout is planned.
struct LpLayoutOptions {
    int threads = 0;            // LPBOX_LP_THREADS=256|512|1024: workgroup size of the default order (0 = not set: 512)
    bool nosort = false;        // LPBOX_LP_NOSORT: variables and row tasks stay in input order (no blocks, no bank classes, no column split)
    bool nosplit = false;       // LPBOX_LP_NOSPLIT: one lane per row, however long
    int bankaware = -1;         // LPBOX_LP_BANKAWARE=1|0: bank-aware lane choice on / off (-1 = not set: on with four slots per thread).
                                // O(n * 32 * row length) host work.  One slot per thread: worth < 3 % per iteration once the long columns
                                // are split, and the direct x-update wants the plain row placement: off.  Four slots per thread
                                // (n > 1024): 4-5 % per iteration, measured over all eight rank shards of the j=500/k=2000 stream: on
                                // (tools/lottery.sh measures both).
    bool noconflict = false;    // LPBOX_LP_NOCONFLICT: bank-aware lane choice off, whatever LPBOX_LP_BANKAWARE says
    bool snakerows = false;     // LPBOX_LP_SNAKEROWS: multi-slot layouts deal the blocks of row tasks in snake order, not by load
    bool snakecols = false;     // LPBOX_LP_SNAKECOLS: the same for the blocks of columns (this one moves variables: part of lpbox_get_layout)
    bool nocolsplit = false;    // LPBOX_LP_NOCOLSPLIT: whole columns, no quads with helper chunks
    int splitbias = 2;          // LPBOX_LP_SPLITBIAS: cost of the quad combine, in list entries (a wave splits only where it gains more)
    bool pcg_generic = false;   // LPBOX_LP_PCGLOOP=generic: no wave takes a PCG loop specialised for its list lengths (A/B and tests; same
                                // results either way)
    int ref_vals = -1;          // LPBOX_LP_REF_VALS=lds (1) / anything else, e.g. global (0): where a valued reference-order batch keeps
                                // its values (-1 = not set: in LDS where they fit; lds fails when they do not)
};
LpLayoutOptions lp_layout_options_from_env();

// Workgroup geometry of a batch: T threads x EPT slots per thread = NS storage positions / row-task slots per instance; LS and ZS are the
// strides of the l-vectors (a whole number of 32-row bank classes) and of the index pools.
struct LpGeometry {
    int T = 0, EPT = 0, NS = 0, LS = 0, ZS = 0;
    bool colsplit = false;      // the kernel variant of this geometry is compiled with helper lists
};
// LPBOX_OK, or the LPBOX_E_* code of the refusal with its text in *err.
int lp_choose_geometry(int nmax, int lmax, int zmax, bool reference_order, const LpLayoutOptions &opt, LpGeometry *geo, std::string *err);

// E of one instance: CSC as read, and the CSR of the same matrix (columns ascending inside a row).
struct LpProblemView {
    int n = 0, l = 0, nnz = 0;
    const int *colptr = nullptr, *rowidx = nullptr, *rowptr = nullptr, *colidx = nullptr;
};

struct LpHelpChunk { int var, first, count; };     // entries first .. first + count - 1 of column var (var < 0: none)

struct LpInstanceLayout {
    // what the layout getters report (and the oracle mirrors)
    std::vector<int> cpos, cperm;      // variable j sits at storage position cpos[j]; cperm = the variables by decreasing column length
    std::vector<int> rowG;             // lanes that share the sum of row r (1,2,4,8)
    std::vector<int> col_own;          // entries of column j summed by its own lane (= its length unless the column is split)
    std::vector<int> col_help;         // [4*j + q]: entries of column j summed by lane q of its quad as a helper (0 = none)
    std::vector<LpHelpChunk> help_of_pos;   // storage position -> helper chunk (empty: no column is split)
    std::vector<int> wave_class;       // 512 x 1 kernel: (rn, cn, hn, tail) of every wavefront, else empty
    bool identity_rows = true;         // row storage index == row id (bank-aware placement off)
    // the tables the kernels read, as the device sees them.  Pointer tables: NS + 1 entries; index pools: nnz entries (rs_col: storage
    // positions by row task, cs_row: row storage indices by position, own parts first, helper chunks from hs_ptr[0] on); per slot: NS
    // entries (rid = row of the task, 0xFFFF none; rgl = its storage index; rmeta = lanes << 4 | lane, 0x10 none; cmeta = column length,
    // bit 15: split)
    std::vector<int> rs_ptr, cs_ptr, hs_ptr;
    std::vector<uint16_t> rs_col, cs_row, rid, rgl, rmeta, cmeta;
};

// Default order: split rows, order and deal the row tasks, place the columns, place the rows in bank classes, emit the tables, classify
// the waves.  caps = register entries of a lane's row, own-column and helper list (lp_pcg_list_caps).
void lp_plan_layout(const LpProblemView &P, const LpGeometry &geo, const LpLayoutOptions &opt, const int caps[3], LpInstanceLayout *out);
// Reference order (lp_ref_window_kernel): variable j at position j, row i at row slot i, one lane per row, whole columns;
// rs_ptr / rs_col = CSR of E (columns ascending), cs_ptr / cs_row = CSC (rows ascending).
void lp_plan_identity_layout(const LpProblemView &P, const LpGeometry &geo, LpInstanceLayout *out);
// Direct x-update: rows with pairwise disjoint columns (D) are inverted in closed form, the rest (G) through a dense |G| x |G| inverse.
// Greedy choice of D: rows by ascending length (the XOR "dummy item" rows of an auction are short and mutually disjoint), rows of equal
// length by ascending row index; a row is D if none of its columns belongs to a D row chosen before it (an empty row always is).
// gidx_of_row[r] = dense index of row r among the G rows, numbered in row order, -1 = D row; returns |G|.
// (tests/direct_cases.py::greedy_split restates the rule; tests/test_direct_edges.py compares the two element for element.)
int lp_plan_direct_rows(const LpProblemView &P, std::vector<int> *gidx_of_row);
// Class of one wavefront of the 512 x 1 kernel's PCG loop from the list lengths of its lanes: chunks of two register entries of its
// longest row, own-column and helper list (what build_list's wlen gives), and whether some lane's list goes beyond the registers.
void lp_wave_class_rule(int lanes, const int *row_len, const int *col_len, const int *help_len, const int caps[3], int *class4);

#endif
