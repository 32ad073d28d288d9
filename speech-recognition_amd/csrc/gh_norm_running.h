// Causal running mean / variance normalisation: what gh_norm_running.hip offers the streaming front-end.
#pragma once
#include "gh_host.h"

// one run of consecutive rows of a resident batch: an utterance (offline) or what one stream emits in a push
struct NormSlot {
    int64_t row0, nf;      // first row in the batch; rows (0: the kernel touches nothing)
    int64_t c0;            // frames the carried sums hold before this run (0: they are not read)
    int64_t id;            // stream whose sums are carried (unused without a state array)
};

// every check of the rule's parameters (mean / sd [D]); GH_ERR_INVALID with the error text set
int gh_norm_check(const char* who, const double* mean, const double* sd, int D, double prior_frames, double min_std);

// the per-coefficient constants of the rule as the kernel reads them, [3][D]: m | P s s | (phi s)(phi s), each product
// rounded once, in that order
std::vector<double> gh_norm_prior(const double* mean, const double* sd, int D, double prior_frames, double min_std);

// enqueue the pass over n_slots runs of `feats` ([.., D] of `dtype`, in place); state [n_streams][2][D] or null (every
// run starts from zero and nothing is carried)
hipError_t gh_norm_launch(hipStream_t st, gh_dtype dtype, void* feats, int D, const NormSlot* d_slot, int64_t n_slots,
                          const double* d_prior, double prior_frames, double* state);
