// The online session (gh_online_*).  gh_online.hip is the session itself: create, push, result, commit, tail and the end kernel.
// What a session does with a chunk and with its history depends on its FORM alone, and the table below says per form which
// launcher does it: the carried sweeps (gh_viterbi_online.hip, gh_viterbi_bigram_online.hip, gh_viterbi_online_wide.hip,
// gh_viterbi_bigram_online_wide.hip, gh_viterbi_layers_online.hip) and the settle and segment walks of commit and tail
// (gh_online_settle.hip: both narrow forms; gh_online_wide_settle.hip, gh_online_bigram_wide_settle.hip).
#pragma once
#include "gh_internal.h"
#include "gh_host.h"
#include "gh_viterbi.h"

// one stream of one push: `count` frames from row `row0` of the batch's [N, S] likelihood matrix continue stream `stream`
// at absolute column `t0`
struct gh_online_slot {
    int64_t row0;
    int32_t stream, count, t0, pad;
};

// the settled prefix of a stream ends in this cell (column < 0: nothing is settled yet)
struct gh_online_anchor {
    int32_t col, word, state, pad;
};

// argument block of the carried sweeps (viterbi_online_kernel, viterbi_bigram_online_kernel, viterbi_online_wide_kernel,
// viterbi_bigram_online_wide_kernel, viterbi_layers_online_kernel)
struct gh_online_args {
    const gh_layerform* lf;
    const void* nll;
    int S;
    const gh_online_slot* slots;
    int64_t n_slots;
    double* prev;          // [n_streams][register sets of the form][N][lanes of the form]
    uint32_t* open;        // [n_streams][lanes of the form] (a form without an open word: null)
    uint16_t* hist;        // decision words, stream k at k * hist_stride (uint16 units, as gh_layers_args::bp)
    int64_t hist_stride;
    int ring_words;        // word index i of a stream lives at i % ring_words (gh_online::ring_words)
};

// one stream of a commit or a tail: `T` frames taken, `has_anchor`: d_anchor[stream] is valid
struct gh_settle_task {
    int32_t stream, T, has_anchor, pad;
};

// argument block of the settle and segment walks (the wide bigram segment walk takes the graph's cost table as a second kernel
// argument)
struct gh_settle_args {
    const gh_layerform* lf;
    const int32_t* end_rows;
    const gh_settle_task* tasks;
    int64_t n;
    const double* prev;            // [n_streams][N][lanes of the form]
    const uint16_t* hist;          // stream k at k * hist_stride (uint16 units), word index i at i % ring_words
    int64_t hist_stride;
    int ring_words;
    gh_online_anchor* anchor;      // [n_streams]
    gh_online_anchor* cand;        // [n]: the settle walk's result (commit), null in tail mode
    const int32_t* best_end;       // [n] (tail mode)
    const int32_t* row_label;
    int32_t* labels;
    const int64_t* label_off;
    int32_t* n_labels;
    int64_t* settled_frames;       // [n] (commit)
    int* flag;
    int32_t* begins;               // timed twins: the begin column of every label, laid out like `labels` (appended: no older field moves)
};

// argument block of the forced commit (online_force_kernel, gh_online_force.hip): the narrow loop form only
struct gh_force_args {
    const gh_layerform* lf;
    const int32_t* end_slot;       // [R]: the end slot of a row, -1 where it is no end row (gh_lattices::d_lf_end_slot)
    const gh_settle_task* tasks;
    int64_t n;
    double* prev;                  // [n_streams][N][16]: the carried column, the ONE thing the kernel writes besides `pruned`
    const uint16_t* hist;          // as gh_settle_args
    int64_t hist_stride;
    int ring_words;
    int max_tail;                  // M: the column to force is T - 1 - M
    const gh_online_anchor* anchor;
    int32_t* pruned;               // [n]: cells set to +inf
    int* flag;
};

struct gh_online;

// ------------------------------------------------------------------------------------------------------- the five forms
// Every launcher of a family has the family's signature; the graph (on->lat->h_layers, and the cost table on->lat->d_bigram_wide
// of the wide bigram form) comes from the session.
//   sweep: the chunks of a.slots continue their streams (f64: the batch's likelihoods are doubles);
//   walk:  the settle walk (settle) or the segment walk of commit and tail, `who` is the caller for messages;
//   trace: the one-shot decode's own back-trace on the history of n streams as utterances 0 .. n - 1 (timed: label mode with
//          begins in a.path) -- it runs unchanged, because a session with full history lays its decision words out exactly as
//          the one-shot sweep of the same frames does.
typedef int gh_online_sweep_fn(gh_ctx* ctx, const gh_online* on, const gh_online_args& a, bool f64);
typedef int gh_online_walk_fn(gh_ctx* ctx, const gh_online* on, const gh_settle_args& a, bool settle, const char* who);
typedef int gh_online_trace_fn(gh_ctx* ctx, const gh_online* on, const gh_layers_args& a, int64_t n, bool timed);
gh_online_sweep_fn gh_launch_online_loop, gh_launch_online_bigram, gh_launch_online_wide, gh_launch_online_bigram_wide,
    gh_launch_online_layers;
gh_online_walk_fn gh_launch_online_loop_settle, gh_launch_online_bigram_settle, gh_launch_online_wide_settle,
    gh_launch_online_bigram_wide_settle;
gh_online_trace_fn gh_online_loop_trace, gh_online_bigram_trace;     // (gh_online.hip; each hands a wide graph on by itself)
int gh_launch_online_loop_force(gh_ctx* ctx, const gh_online* on, const gh_force_args& a);   // gh_online_force.hip
constexpr int gh_one_cpw(int, bool) { return 1; }
constexpr int gh_layer2_cpw(int N, bool skip) { return gh_layer_cpw(N, skip, 2); }   // layer form, two register sets (up to 8 layers)

struct gh_online_form {
    const char* grammar;             // "loop", "bigram" or "layers": the rows of the graph and the word of gh_online_push's messages
    int lanes;                       // lanes per stream: 16 -- up to GH_LAYERS_ROWW words, four streams to a wave, DPP row = stream
                                     // -- or 64 -- a wave per stream: 17 .. GH_LAYERS_MAXW words, lane = word, or the K-layer lattice,
                                     // lane = (layer mod 4, word)
    int sets;                        // register sets per lane: 1, or 2 in the K-layer lattice (layers 0-3 and 4-7).
                                     // State: [n_streams][sets][N][lanes] doubles
    bool open_word;                  // a decision word holds several columns, so a chunk may end inside one: [n_streams][lanes] open
                                     // words are carried beside the state.  false: one complete word per column and lane
    bool bigram_rows;                // state 0 of word w is row loop_row + W + w (the loop numbering: loop_row + 1 + w)
    int (*cpw)(int N, bool skip);    // columns per decision word.  A history of `frames` frames is ceil(frames / cpw) words -- one
                                     // more where it is a window: the word the anchor lies in is kept -- of `lanes` x 4 B each, and
                                     // that count is ring_words: full history never wraps
    gh_online_sweep_fn* sweep;
    gh_online_walk_fn* walk;         // (null: no entry point makes a session of this form that settles)
    gh_online_trace_fn* trace;
};

enum gh_online_form_id { GH_ONLINE_LOOP, GH_ONLINE_BIGRAM, GH_ONLINE_WIDE, GH_ONLINE_BIGRAM_WIDE, GH_ONLINE_LAYERS };
inline constexpr gh_online_form gh_online_forms[] = {
    {"loop", 16, 1, true, false, gh_loop_cpw, gh_launch_online_loop, gh_launch_online_loop_settle, gh_online_loop_trace},
    {"bigram", 16, 1, true, true, gh_bigram_cpw, gh_launch_online_bigram, gh_launch_online_bigram_settle, gh_online_bigram_trace},
    {"loop", 64, 1, false, false, gh_one_cpw, gh_launch_online_wide, gh_launch_online_wide_settle, gh_online_loop_trace},
    {"bigram", 64, 1, false, true, gh_one_cpw, gh_launch_online_bigram_wide, gh_launch_online_bigram_wide_settle, gh_online_bigram_trace},
    {"layers", 64, 2, true, false, gh_layer2_cpw, gh_launch_online_layers, nullptr, gh_online_loop_trace},
};

struct gh_online {
    gh_ctx* ctx;
    const gh_lattices* lat;        // must outlive the session
    const gh_online_form* form;    // a row of gh_online_forms: push, end, back-trace and the walks each ask it, nothing else
    bool settles;                  // gh_online_commit / gh_online_tail serve the session: it has anchors (a narrow loop session
                                   // always, the others from their gh_online_create_*_settle; a layer session never)
    int64_t n_streams, max_frames, hist_stride;
    int64_t window;                // > 0: the history is a ring that holds `window` unsettled frames; gh_online_result is refused
    int32_t ring_words;            // decision words per lane in a stream's history: word index i lives at i % ring_words
    void* d_arena;
    double* d_prev;
    uint32_t* d_open;              // (null in a form without an open word)
    uint16_t* d_hist;
    gh_online_anchor* d_anchor;    // [n_streams], valid where settled[stream] > 0 (null in a session that does not settle)
    gh_online_slot* d_slots;       // [n_streams]: the table of the push in flight
    gh_online_slot* h_slots;       // page-locked staging of the same size
    hipEvent_t copied;             // behind the last upload of h_slots
    bool copy_pending;
    std::vector<int64_t> frames;   // [n_streams] frames taken so far
    std::vector<int64_t> settled;  // [n_streams] anchor column + 1 (0: none): host mirror of d_anchor for the push check
    std::vector<uint8_t> seen;     // [n_streams] scratch of the duplicate check
};
