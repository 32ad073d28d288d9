// The word-stream session (gh_wordstream_*) and what its two carried sweeps share: the Viterbi cost column
// (gh_viterbi_chain_online.hip, the session itself) and the log-alpha column of a SOFT session (gh_forward_chain.hip).
#pragma once
#include "gh_online.h"

struct gh_wordstream {
    gh_ctx* ctx;
    const gh_lattices* lat;        // must outlive the session
    int64_t n_streams;
    int N, C;                      // states per chain, chains per stream
    void* d_arena;
    double* d_state;               // [n_streams][N][C]
    double* d_alpha;               // [n_streams][N][C] log-alphas of a soft session (gh_wordstream_create_soft), else null
    gh_online_slot* d_slots;       // [n_streams]: the table of the push in flight
    gh_online_slot* h_slots;       // page-locked staging of the same size
    hipEvent_t copied;             // behind the last upload of h_slots
    bool copy_pending;
    std::vector<int64_t> frames;   // [n_streams] frames taken so far
    std::vector<uint8_t> seen;     // [n_streams] scratch of the duplicate check
};

// argument block of both sweeps (viterbi_chain_online_kernel, forward_chain_kernel)
struct gh_wordstream_args {
    const double *cost0, *cost1, *cost2;   // [R] arc costs of the chain form (gh_chain_args)
    const uint8_t* row_info;               // [R] bit 2: start row
    const int32_t* row_state;              // [R]
    const void* nll;                       // [rows, S] likelihoods of the batch
    int S, C;
    const gh_online_slot* slots;
    int64_t n_slots;
    double* state;                         // [n_streams][N][C]: costs (Viterbi sweep) or log-alphas (forward sweep)
};

// Why `lat` is not ONE graph of stacked word chains that the lane = chain sweeps take (equal length, 1 .. 8 rows, consecutive
// states, no beam), as the tail of a sentence; an empty string: it is one.  (gh_viterbi_chain_online.hip)
void gh_wordchain_refusal(const gh_lattices* lat, char* why, size_t n);
// the argument block of a sweep of `lat` over the likelihoods of `b` (slots, n_slots and state are the caller's)
gh_wordstream_args gh_wordchain_args(const gh_lattices* lat, const gh_batch* b);
// forward_chain_kernel on the slots of `a` (gh_forward_chain.hip)
int gh_launch_forward_chain(gh_ctx* ctx, const gh_wordstream_args& a, int N, bool skip, bool f64);
