#pragma once
#include "gh_internal.h"

// Kernel argument block of the lattice Viterbi (all pointers are device pointers).
struct gh_vit_args {
    const gh_lattices::desc* descs;
    const int32_t* row_state;
    const uint8_t* row_start;
    const int32_t* pred_ptr;
    const uint32_t* pred_row;
    const double* pred_cost;
    const int32_t* order;
    const int32_t* level_ptr;
    const int32_t* level_narrow;  // rows of each level with <= 2 arcs (first in `order`)
    const int32_t* end_rows;
    const void* nll;  // [N,S] float or double
    int S;
    int r_pad;                // LDS column stride (>= max R, even)
    int em_chunk;             // lean kernel: columns of emissions prefetched per chunk, >= 1
    int arc_cap;              // lean kernel: LDS slots for a graph's arc list
    int lds_bytes;            // lean kernel: dynamic LDS of the launch (the back-trace re-uses all of it)
    int bpc_off;              // lean kernel: LDS byte offset of the 8-column back-pointer staging block
    int beam;                 // generic kernel: rank beam per column (0 = off), gh_lattices_set_beam
    const int64_t* utt_off;   // [U+1] frame offsets
    const int32_t* utt_lat;   // [U] graph of each utterance, or null (graph 0)
    const int64_t* perm;      // launch slot -> utterance (longest first), or null
    int64_t u_begin;          // first launch slot of this chunk
    uint16_t* bp;             // back-pointer scratch of this chunk
    const int64_t* bp_off;    // [slots] offset of each launch slot's [T,R] block
    double* end_cost;         // [sum n_end]
    const int64_t* end_off;   // [U]
    int32_t* best_end;        // [U]
    int32_t* path;            // [.., 2]
    const int64_t* path_off;  // [U+1]
    int32_t* path_len;        // [U]
    double* costs;            // optional full matrices
    const int64_t* costs_off; // [U+1]
    int* flag;
};

int gh_launch_viterbi(gh_ctx* ctx, const gh_vit_args& a, int64_t n_utts, int block, size_t lds_bytes,
                      bool f64, bool want_path);
// lean kernel (gh_viterbi_lean.hip): <= 3 levels, one row per lane per level, no NaN / self arcs
int gh_launch_viterbi_lean(gh_ctx* ctx, const gh_vit_args& a, int64_t n_utts, int block, size_t lds_bytes,
                           bool f64, bool want_path, int levels);

// Chain kernel (gh_viterbi_chain.hip): left-to-right graphs (arcs from r, r-1, r-2 only), one graph
// for the whole batch.  All pointers are device pointers.
struct gh_chain_args {
    const double* cost0;      // [R] self-arc cost, +inf = absent
    const double* cost1;      // [R] arc from r-1
    const double* cost2;      // [R] arc from r-2
    const uint8_t* row_info;  // [R] bits 0-1: code of the first (lowest-origin) arc, 3 = none; bit 2: start row
    const int32_t* row_state; // [R]
    const int32_t* end_slot;  // [R] position in the end list or -1
    const int32_t* end_rows;  // [n_end]
    const int32_t* group_row0;  // [n_groups+1] row ranges of the 64-lane groups (whole chains)
    int n_groups, R, S, n_end;
    const void* nll;
    const int64_t* utt_off;
    const int64_t* perm;
    int64_t slot0;
    uint8_t* bp;              // [T,R] bytes per launch slot
    const int64_t* bp_off;
    double* end_cost;         // [U, n_end]
    int32_t* best_end;        // [U]
    int32_t* path;
    const int64_t* path_off;
    int32_t* path_len;
    double* costs;
    const int64_t* costs_off;
    int* flag;
    int unit_chains;          // lane = chain form: chains per utterance (R / rows per chain)
    int64_t n_slots;          // lane = chain form: launch slots of this launch (slot0 .. slot0 + n_slots - 1)
    int64_t n_lane_waves;     // lane = chain form: grid positions of this launch (the grid may be smaller: strided walk)
};
int gh_launch_viterbi_chain(gh_ctx* ctx, const gh_chain_args& a, int64_t u_begin, int64_t n_utts, bool f64,
                            bool want_bp, bool want_costs, bool skip);
// lane = chain form of the same sweep for graphs whose chains all have `unit` rows (gh_chain_lanes_ok: 1 .. 8) with
// consecutive states; *selected: best_end is written, gh_launch_chain_backtrace is not needed for the end selection
bool gh_chain_lanes_ok(int unit);
int gh_launch_viterbi_chain_lanes(gh_ctx* ctx, const gh_chain_args& a, int unit, int64_t u_begin, int64_t n_utts, bool f64,
                                  bool want_bp, bool want_costs, bool skip, bool* selected);
int gh_launch_chain_backtrace(gh_ctx* ctx, const gh_chain_args& a, int64_t u_begin, int64_t n_utts);

// Fused single-Gaussian decode (gh_viterbi_fused.hip): the chain kernel's graph and outputs, but every lane scores its
// own state's Gaussian against the frame instead of reading the [N, S] likelihood matrix (c.nll / c.S unused).
struct gh_fused_args {
    gh_chain_args c;
    const void* feats;   // [N, D] features of the batch's dtype
    const double* par;   // [2 DVp + 2][Rp]: sqrt(1/(2 var)) rows, -mean sqrt(1/(2 var)) rows, -logc, underflow threshold
    int D, Rp, skip;     // feature dimension, padded row count, any r-2 -> r arc
    int DVp;             // rows per half of the constants table (gh_fused_dv(D))
    int select_end;      // 1: the sweep also picks the best end row (one lane group, no path wanted): no back-trace launch
    int lin;             // 1: the linear-domain underflow rule of GMM.evaluate is on (finite threshold in the table)
    int64_t n_items;     // (utterance, row group) pairs of the launch
    int pw, period;      // packed form: rows per wave window (0: one utterance per wave), windows per repeat of the row pattern
    int64_t n_windows;
};
int gh_fused_window(int R, int unit, int* period_out);   // rows per packed window (0: one utterance per wave)
int gh_fused_dv(int D);  // rows per half of the constants table for D dimensions (0: D not covered)
int gh_launch_fused_params(gh_ctx* ctx, const gh_gmm* g, const int32_t* d_row_state, int R, int Rp, int DV, double thr,
                           double* d_par);
int gh_launch_viterbi_fused(gh_ctx* ctx, const gh_fused_args& fa, int64_t u_begin, int64_t n_utts, bool f64,
                            bool want_bp, bool want_costs);

// Layer-form kernel (gh_viterbi_layers.hip): K identical layers of W words x N states (gh_layerform), one graph for
// the whole batch, one wave per utterance.  All pointers are device pointers.
struct gh_layers_args {
    const gh_layerform* lf;
    const int32_t* end_slot;   // [R] position of a row in the end list or -1
    const int32_t* end_rows;   // [n_end]
    int n_end, S;
    const void* nll;
    const int64_t* utt_off;
    const int64_t* perm;
    int64_t slot0;
    uint16_t* bp;              // decision words; bp_off in uint16 units (multiples of 8)
    const int64_t* bp_off;
    double* end_cost;          // [U, n_end]
    int32_t* best_end;         // [U]
    int32_t* path;             // timed label mode (MODE 2 of the back-trace kernels): the begin column of every label, laid out like
                               // `labels` -- a label launch writes no path, and the block keeps its size and offsets
    const int64_t* path_off;
    int32_t* path_len;
    // sequence form (gh_seq.hip): per-utterance graphs made of shared word templates
    const gh_seqgraph* seqgraphs;
    const gh_seqword* seqwords;
    const int32_t* utt_lat;    // [U] graph of every utterance, or null (graph 0)
    const int64_t* end_off;    // [U] offset of the utterance's end costs, or null (u * n_end)
    int seq_N;
    const int32_t* row_label;  // label mode (gh_viterbi_labels): label per row, < 0 on non-emitting rows
    int32_t* labels;           // utterance u at label_off[u]
    const int64_t* label_off;  // [U+1]
    int32_t* n_labels;         // [U]
    int* flag;
};
size_t gh_layers_bp_entries(const gh_layerform& f, int64_t T);
int gh_launch_viterbi_layers(gh_ctx* ctx, const gh_layers_args& a, const gh_layerform& f, int64_t u_begin, int64_t n_utts,
                             bool f64, bool want_path);
int gh_launch_lattice_backtrace(gh_ctx* ctx, const gh_layers_args& a, const gh_layerform& f, int64_t u_begin, int64_t n_utts,
        bool timed = false);   // timed: label mode with begins in a.path
// more than GH_LAYERS_ROWW words per layer (gh_viterbi_layers_wide.hip: lane = word); the two launchers above hand over to these
size_t gh_layers_wide_bp_entries(int64_t T);
size_t gh_loop_wide_bp_entries(int64_t T);
int gh_launch_viterbi_layers_wide(gh_ctx* ctx, const gh_layers_args& a, const gh_layerform& f, int64_t u_begin, int64_t n_utts,
                                  bool f64, bool want_path);
int gh_launch_lattice_backtrace_wide(gh_ctx* ctx, const gh_layers_args& a, const gh_layerform& f, int64_t u_begin, int64_t n_utts,
        bool timed = false);   // timed: label mode with begins in a.path
// sequence form (forced-alignment lattices, gh_seq.hip): forward sweep, four utterances per wave, and its back-trace
size_t gh_seq_bp_entries(int N, int skip, int64_t T);
int gh_launch_viterbi_seq(gh_ctx* ctx, const gh_layers_args& a, int N, int skip, int64_t u_begin, int64_t n_utts, bool f64,
                          bool want_path);
int gh_launch_seq_backtrace(gh_ctx* ctx, const gh_layers_args& a, int N, int skip, int64_t u_begin, int64_t n_utts);
// bigram form (gh_viterbi_bigram.hip: the loop form with one entry row per word): forward sweep, four utterances per wave,
// and its back-trace (path or label mode); gh_bigram_n_ok: the word sizes the kernel is instantiated for
bool gh_bigram_n_ok(int N, int skip);
size_t gh_bigram_bp_entries(const gh_layerform& f, int64_t T);
int gh_launch_viterbi_bigram(gh_ctx* ctx, const gh_layers_args& a, const gh_layerform& f, int64_t u_begin, int64_t n_utts,
                             bool f64, bool want_path, const gh_bigram_wide* wide = nullptr);
int gh_launch_bigram_backtrace(gh_ctx* ctx, const gh_layers_args& a, const gh_layerform& f, int64_t u_begin, int64_t n_utts,
        bool timed = false, const gh_bigram_wide* wide = nullptr);   // timed: label mode with begins in a.path
// more than GH_LAYERS_ROWW words (gh_viterbi_bigram_wide.hip: one utterance per wave, lane = word, the word-to-word costs `wide`
// in LDS); the three functions above hand over to these
size_t gh_bigram_wide_bp_entries(int64_t T);
int gh_launch_viterbi_bigram_wide(gh_ctx* ctx, const gh_layers_args& a, const gh_layerform& f, const gh_bigram_wide* wide,
                                  int64_t u_begin, int64_t n_utts, bool f64, bool want_path);
int gh_launch_bigram_backtrace_wide(gh_ctx* ctx, const gh_layers_args& a, const gh_layerform& f, const gh_bigram_wide* wide,
                                    int64_t u_begin, int64_t n_utts, bool timed);

// ---------------------------------------------------------------------------------------------------------------------
// Decision-word layout of the register forms above, ONE definition for the sweep that writes the words, the back-trace that
// reads them and the host function that sizes the scratch: decision bits per column and lane (layer forms: and register
// set / layer) for words of N states, and the columns that share one decision word.
constexpr int gh_layer_hb(int N, bool skip) { return N + 1 + (skip ? N - 2 : 0); }    // layer form, narrow and wide
constexpr int gh_loop_hb(int N, bool skip) { return N + 2 + (skip ? N - 2 : 0); }     // loop form, narrow and wide
constexpr int gh_bigram_hb(int N, bool skip) { return N + 5 + (skip ? N - 2 : 0); }   // in-word bits, 4 bits of predecessor word, 2 bits of state 0
constexpr int gh_bigram_wide_hb(int N, bool skip) { return N + 7 + (skip ? N - 2 : 0); }   // the same with 6 bits of predecessor word
constexpr int gh_seq_hb(int N, bool skip) { return N + (skip ? N - 2 : 0); }
// layer form: `sets` register sets (2: up to 8 layers, 4: up to 16) share a word, 64 bits wide when 32 do not hold them
constexpr int gh_layer_word_bits(int N, bool skip, int sets) { return sets * gh_layer_hb(N, skip) > 32 ? 64 : 32; }
constexpr int gh_layer_cpw(int N, bool skip, int sets) { return gh_layer_word_bits(N, skip, sets) / (sets * gh_layer_hb(N, skip)); }
constexpr int gh_loop_cpw(int N, bool skip) { return 32 / gh_loop_hb(N, skip); }
constexpr int gh_bigram_cpw(int N, bool skip) { return 32 / gh_bigram_hb(N, skip); }
constexpr int gh_seq_cpw(int N, bool skip) { return 32 / gh_seq_hb(N, skip); }
// back-pointer scratch of T frames in uint16 units (the lattice kernels' common unit): `lanes` words per cpw columns
constexpr size_t gh_bp_entries(int64_t T, int cpw, int lanes, int word_bits) {
    return (size_t)((T + cpw - 1) / cpw) * lanes * (word_bits / 16);
}

// columns per word for N = 2 .. 8, 12, 16 without and with skip arcs (0: not built; a two-state word has no skip arc)
namespace gh_layout_check {
constexpr int NS[9] = {2, 3, 4, 5, 6, 7, 8, 12, 16};
template <typename F> constexpr bool same(F cpw, const int (&plain)[9], const int (&skip)[9]) {
    for (int i = 0; i < 9; ++i)
        if ((plain[i] && cpw(NS[i], false) != plain[i]) || (skip[i] && cpw(NS[i], true) != skip[i])) return false;
    return true;
}
static_assert(same([](int N, bool s) { return gh_layer_cpw(N, s, 2); }, {5, 4, 3, 2, 2, 2, 1, 1, 1}, {5, 3, 2, 1, 1, 1, 1, 1, 1}), "layer form, two sets");
static_assert(same([](int N, bool s) { return gh_layer_cpw(N, s, 4); }, {2, 2, 1, 1, 1, 1, 1, 0, 0}, {2, 1, 1, 1, 1, 1, 1, 0, 0}), "layer form, four sets");
static_assert(same(gh_loop_cpw, {8, 6, 5, 4, 4, 3, 3, 2, 1}, {8, 5, 4, 3, 2, 2, 2, 1, 1}), "loop form");
static_assert(same(gh_bigram_cpw, {4, 4, 3, 3, 2, 2, 2, 1, 1}, {4, 3, 2, 2, 2, 1, 1, 1, 0}), "bigram form");
static_assert(same(gh_seq_cpw, {16, 10, 8, 6, 5, 4, 4, 2, 2}, {16, 8, 5, 4, 3, 2, 2, 1, 1}), "sequence form");
static_assert(gh_layer_word_bits(16, false, 2) == 64 && gh_layer_word_bits(12, false, 2) == 32 && gh_layer_word_bits(8, true, 2) == 32 &&
              gh_layer_word_bits(12, true, 2) == 64 && gh_layer_word_bits(7, false, 4) == 32 && gh_layer_word_bits(8, false, 4) == 64 &&
              gh_layer_word_bits(4, true, 4) == 32 && gh_layer_word_bits(5, true, 4) == 64, "layer form: where the words turn 64 bits wide");
static_assert(4 * gh_layer_hb(8, true) <= 64 && gh_loop_hb(8, true) <= 32, "wide forms: one word per column (and four layers)");
static_assert(gh_bigram_wide_hb(8, true) <= 32, "wide bigram form: one word per column");
static_assert(gh_bigram_hb(16, true) > 32, "bigram form: 16 states with skip arcs do not fit a word");
}  // namespace gh_layout_check

// ---------------------------------------------------------------------------------------------------------------------
// The one switch over states per word x skip arcs that picks a template instantiation: CALL(ET, N, SKIP) is a statement,
// ET is handed through untouched, MAXN names the word sizes a form is built for -- 8; 16 (also 12 and 16); 16_NO_SKIP16
// (the same without 16 states with skip arcs).  Anything else sets the error text (printf arguments) and returns
// GH_ERR_UNSUPPORTED from the calling function.
#define GH_NSKIP_CASE(NN, skip, CALL, ET) case NN: if (skip) CALL(ET, NN, true); else CALL(ET, NN, false); break;
#define GH_NSKIP_FROM_12_8(skip, CALL, ET)
#define GH_NSKIP_FROM_12_16(skip, CALL, ET) GH_NSKIP_CASE(12, skip, CALL, ET) GH_NSKIP_CASE(16, skip, CALL, ET)
#define GH_NSKIP_FROM_12_16_NO_SKIP16(skip, CALL, ET) GH_NSKIP_CASE(12, skip, CALL, ET) case 16: if (!(skip)) { CALL(ET, 16, false); break; }
#define GH_NSKIP_SWITCH(n, skip, MAXN, CALL, ET, ...)                                     \
    switch (n) {                                                                          \
        case 2: CALL(ET, 2, false); break;                                                \
        GH_NSKIP_CASE(3, skip, CALL, ET) GH_NSKIP_CASE(4, skip, CALL, ET) GH_NSKIP_CASE(5, skip, CALL, ET) \
        GH_NSKIP_CASE(6, skip, CALL, ET) GH_NSKIP_CASE(7, skip, CALL, ET) GH_NSKIP_CASE(8, skip, CALL, ET) \
        GH_NSKIP_FROM_12_##MAXN(skip, CALL, ET)                                           \
        default: gh_set_error(__VA_ARGS__); return GH_ERR_UNSUPPORTED;                    \
    }
