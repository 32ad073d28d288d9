// The online session (gh_online_*): what gh_viterbi_online.hip (create, push, result), gh_viterbi_bigram_online.hip (the carried
// bigram sweep), gh_viterbi_online_wide.hip (the carried wide loop sweep), gh_viterbi_bigram_online_wide.hip (the carried wide
// bigram sweep), gh_online_settle.hip (commit, tail), gh_online_wide_settle.hip (the two walks of commit and tail over a
// wide session's history) and gh_online_bigram_wide_settle.hip (the same two walks over a wide bigram session's) share.
#pragma once
#include "gh_internal.h"
#include "gh_host.h"

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
// viterbi_bigram_online_wide_kernel)
struct gh_online_args {
    const gh_layerform* lf;
    const void* nll;
    int S;
    const gh_online_slot* slots;
    int64_t n_slots;
    double* prev;          // [n_streams][N][16] (wide session: [n_streams][N][64])
    uint32_t* open;        // [n_streams][16] (wide session: none, null)
    uint16_t* hist;        // decision words, stream k at k * hist_stride (uint16 units, as gh_layers_args::bp)
    int64_t hist_stride;
    int ring_words;        // word index i of a stream lives at i % ring_words (a wide session: one word per column and lane, so
                           // this is its ring in COLUMNS; one that keeps its full history passes a ring it never fills)
};

// one stream of a commit or a tail: `T` frames taken, `has_anchor`: d_anchor[stream] is valid
struct gh_settle_task {
    int32_t stream, T, has_anchor, pad;
};

// argument block of the settle and segment walks (gh_online_settle.hip; gh_online_wide_settle.hip for a wide session,
// gh_online_bigram_wide_settle.hip for a wide bigram one, whose segment walk takes the cost table as a second kernel argument)
struct gh_settle_args {
    const gh_layerform* lf;
    const int32_t* end_rows;
    const gh_settle_task* tasks;
    int64_t n;
    const double* prev;            // [n_streams][N][16] (wide session: [n_streams][N][64])
    const uint16_t* hist;          // stream k at k * hist_stride (uint16 units), word index i at i % ring_words
    int64_t hist_stride;
    int ring_words;                // (wide session: columns, column j at (j % ring_words) * 64 + lane)
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

struct gh_online {
    gh_ctx* ctx;
    const gh_lattices* lat;        // must outlive the session
    bool bigram;                   // the graph is in bigram form (gh_online_create_bigram[_settle]): wider records
    bool settles;                  // gh_online_commit / gh_online_tail serve the session (a loop session always; a bigram one
                                   // only from gh_online_create_bigram_settle, which alone may give it a window)
    bool wide;                     // the graph is a word loop of 17 .. 64 words (gh_online_create_wide[_settle]): lane = word, a wave
                                   // per stream, one 32-bit decision word per column and lane.  From gh_online_create_wide: full
                                   // history, no settled prefix; from gh_online_create_wide_settle: `settles`, and a ring of columns
                                   // where it has a window.  With `bigram` (gh_online_create_bigram_wide[_settle]): the WIDE BIGRAM
                                   // form, the same state and history shapes, the records of viterbi_bigram_wide_kernel; full history
                                   // and no settled prefix from gh_online_create_bigram_wide, `settles` (and a ring of columns where
                                   // it has a window) from gh_online_create_bigram_wide_settle
    int64_t n_streams, max_frames, hist_stride;
    int64_t window;                // > 0: the history is a ring that holds `window` unsettled frames (gh_online_create_window)
    int32_t ring_words;            // decision words per lane in a stream's history: word index i lives at i % ring_words
                                   // (a wide session: columns, CPW = 1)
    void* d_arena;
    double* d_prev;
    uint32_t* d_open;              // (null in a wide session: it has no open word)
    uint16_t* d_hist;
    gh_online_anchor* d_anchor;    // [n_streams], valid where settled[stream] > 0
    gh_online_slot* d_slots;       // [n_streams]: the table of the push in flight
    gh_online_slot* h_slots;       // page-locked staging of the same size
    hipEvent_t copied;             // behind the last upload of h_slots
    bool copy_pending;
    std::vector<int64_t> frames;   // [n_streams] frames taken so far
    std::vector<int64_t> settled;  // [n_streams] anchor column + 1 (0: none): host mirror of d_anchor for the push check
    std::vector<uint8_t> seen;     // [n_streams] scratch of the duplicate check
};

// End costs and end selection of n streams from their carried columns (gh_viterbi_online.hip)
int gh_launch_online_end(gh_ctx* ctx, const gh_online* on, const int64_t* d_ids, const int64_t* d_utt_off, int64_t n, double* d_end_cost,
                         int32_t* d_best_end);
// The same for a bigram session, and its carried sweep (gh_viterbi_bigram_online.hip); the sweep writes the history through
// the ring like viterbi_online_kernel
int gh_launch_online_bigram_end(gh_ctx* ctx, const gh_online* on, const int64_t* d_ids, const int64_t* d_utt_off, int64_t n,
                                double* d_end_cost, int32_t* d_best_end);
int gh_launch_online_bigram(gh_ctx* ctx, const gh_online_args& a, const gh_layerform& f, bool f64);
// ... and for a wide session (gh_viterbi_online_wide.hip): one wave per stream; the sweep writes column ta of a stream at word
// index (ta % ring_words) * 64 + lane of its history
int gh_launch_online_wide_end(gh_ctx* ctx, const gh_online* on, const int64_t* d_ids, const int64_t* d_utt_off, int64_t n,
                              double* d_end_cost, int32_t* d_best_end);
int gh_launch_online_wide(gh_ctx* ctx, const gh_online_args& a, const gh_layerform& f, bool f64);
// ... and for a wide BIGRAM session (gh_viterbi_bigram_online_wide.hip): one wave per stream, four streams per block around one
// LDS image of `wide`'s word-to-word costs; the same history addressing
int gh_launch_online_bigram_wide_end(gh_ctx* ctx, const gh_online* on, const int64_t* d_ids, const int64_t* d_utt_off, int64_t n,
                                     double* d_end_cost, int32_t* d_best_end);
int gh_launch_online_bigram_wide(gh_ctx* ctx, const gh_online_args& a, const gh_layerform& f, const gh_bigram_wide* wide, bool f64);
// The settle walk (settle) or the segment walk of a wide session that settles (gh_online_wide_settle.hip); launch_settle of
// gh_online_settle.hip hands over to it where the graph has more than GH_LAYERS_ROWW words
int gh_launch_online_wide_settle(gh_ctx* ctx, const gh_settle_args& a, const gh_layerform& f, bool settle, const char* who);
// ... and of a wide BIGRAM session that settles (gh_online_bigram_wide_settle.hip); launch_settle hands over to it where the
// graph is in the wide bigram form, `wide` is the graph's cost table (the segment walk reads its arc masks)
int gh_launch_online_bigram_wide_settle(gh_ctx* ctx, const gh_settle_args& a, const gh_layerform& f, const gh_bigram_wide* wide,
                                        bool settle, const char* who);
