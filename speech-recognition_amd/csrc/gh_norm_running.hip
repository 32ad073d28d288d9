// Causal running mean / variance normalisation of a resident batch, in place.  THE RULE, per stream
// (offline: per utterance) and coefficient k, with the prior (m, s), its weight P in frames and the floor phi:
//     r = (double)x            the resident value, already rounded to the batch dtype
//     d = r - m ;  S += d ;  Q += d d ;  c += 1 ;  n = P + c
//     a = S / n ;  v = (P s s + Q) / n - a a ;  sd = sqrt(max(v, (phi s)(phi s))) ;  y = (OT)((d - a) / sd)
// every operation one correctly rounded fp64 operation, in the order written: this file is compiled with
// -ffp-contract=off (build.py) and the host forms P s s and (phi s)(phi s) once.  The sums run strictly in frame order, so
// a stream's output is a function of its frames alone, not of how its audio was cut; S and Q are carried per stream in
// [n_streams][2][D] fp64 (624 B at D = 39), the count c lives on the host, and a run with c = 0 reads no carried state.
// One kernel serves the streaming front-end (after stream_stack_kernel wrote the raw rows) and gh_batch_running_norm
// (every utterance from zero, nothing carried).
#include "gh_norm_running.h"

namespace {

// A lane owns one (run, coefficient) and walks the run's rows serially; the G = min(D, 256) coefficient lanes of a run sit
// side by side, so that a row is one contiguous read and write, and 256 / G runs share a workgroup.
template <typename OT>
__global__ __launch_bounds__(256) void running_norm_kernel(OT* __restrict__ x, int D, int G, const NormSlot* __restrict__ slot,
                                                           int64_t n_slots, const double* __restrict__ prior, double P,
                                                           double* __restrict__ state) {
    const int per_block = 256 / G;
    const int sl = threadIdx.x / G, k0 = threadIdx.x % G;
    const int64_t u = (int64_t)blockIdx.x * per_block + sl;
    if (sl >= per_block || u >= n_slots) return;
    const NormSlot s = slot[u];
    if (s.nf == 0) return;                                  // a stream that emits nothing touches nothing
    for (int k = k0; k < D; k += G) {
        const double m = prior[k], ps2 = prior[D + k], fl2 = prior[2 * D + k];
        double* keep = state ? state + s.id * 2 * D + k : nullptr;
        double S = 0.0, Q = 0.0, c = (double)s.c0;
        if (keep && s.c0 > 0) { S = keep[0]; Q = keep[D]; }
        OT* p = x + s.row0 * D + k;
        OT cur = *p;
        for (int64_t t = 0; t < s.nf; ++t, p += D) {
            const OT nxt = t + 1 < s.nf ? p[D] : cur;       // the next row's value is on its way while this one is worked
            const double d = (double)cur - m;
            S = S + d;
            Q = Q + d * d;
            c = c + 1.0;
            const double n = P + c;
            const double a = S / n;
            const double v = (ps2 + Q) / n - a * a;
            const double sd = __dsqrt_rn(v > fl2 ? v : fl2);
            *p = (OT)((d - a) / sd);
            cur = nxt;
        }
        if (keep) { keep[0] = S; keep[D] = Q; }
    }
}

}  // namespace

int gh_norm_check(const char* who, const double* mean, const double* sd, int D, double prior_frames, double min_std) {
    GH_REQUIRE(mean && sd, "%s: mean and std are needed", who);
    for (int k = 0; k < D; ++k)
        GH_REQUIRE(std::isfinite(mean[k]) && std::isfinite(sd[k]) && sd[k] > 0.0, "%s: mean[%d]=%g std[%d]=%g (finite, std > 0)", who, k,
                   mean[k], k, sd[k]);
    GH_REQUIRE(std::isfinite(prior_frames) && prior_frames >= 0.0 && prior_frames == std::floor(prior_frames) && prior_frames <= 0x1p52,
               "%s: prior_frames=%g (a whole number >= 0)", who, prior_frames);
    GH_REQUIRE(std::isfinite(min_std) && min_std > 0.0 && min_std <= 1.0, "%s: min_std=%g (0 < min_std <= 1)", who, min_std);
    return GH_OK;
}

std::vector<double> gh_norm_prior(const double* mean, const double* sd, int D, double prior_frames, double min_std) {
    std::vector<double> p((size_t)3 * D);
    for (int k = 0; k < D; ++k) {
        const double ps = prior_frames * sd[k], fs = min_std * sd[k];
        p[(size_t)k] = mean[k];
        p[(size_t)D + k] = ps * sd[k];
        p[(size_t)2 * D + k] = fs * fs;
    }
    return p;
}

hipError_t gh_norm_launch(hipStream_t st, gh_dtype dtype, void* feats, int D, const NormSlot* d_slot, int64_t n_slots,
                          const double* d_prior, double prior_frames, double* state) {
    if (n_slots == 0) return hipSuccess;
    const int G = D < 256 ? D : 256, per_block = 256 / G;
    const dim3 grid((unsigned)((n_slots + per_block - 1) / per_block)), block(256);
    if (dtype == GH_F64)
        hipLaunchKernelGGL((running_norm_kernel<double>), grid, block, 0, st, (double*)feats, D, G, d_slot, n_slots, d_prior, prior_frames, state);
    else
        hipLaunchKernelGGL((running_norm_kernel<float>), grid, block, 0, st, (float*)feats, D, G, d_slot, n_slots, d_prior, prior_frames, state);
    return hipGetLastError();
}

extern "C" int gh_batch_running_norm(gh_ctx* ctx, gh_batch* b, const double* mean, const double* std_, double prior_frames,
                                     double min_std) {
    const char* who = "gh_batch_running_norm";
    GH_REQUIRE(ctx && b, "%s: NULL argument", who);
    GH_REQUIRE(b->D >= 1, "%s: a batch of %d columns", who, b->D);
    int rc = gh_norm_check(who, mean, std_, b->D, prior_frames, min_std);
    if (rc) return rc;
    if (b->N == 0) return GH_OK;
    std::vector<NormSlot> slot((size_t)b->U);
    for (int64_t u = 0; u < b->U; ++u) slot[(size_t)u] = NormSlot{b->offsets[(size_t)u], b->offsets[(size_t)u + 1] - b->offsets[(size_t)u], 0, 0};
    const std::vector<double> prior = gh_norm_prior(mean, std_, b->D, prior_frames, min_std);
    GH_HIP(hipSetDevice(ctx->device));
    NormSlot* d_slot;
    double* d_prior;
    Carver cv;
    cv.add(&d_slot, slot.size());
    cv.add(&d_prior, prior.size());
    if ((rc = cv.commit(ctx))) return rc;
    hipStream_t st = ctx->stream;
    GH_HIP(hipMemcpyAsync(d_slot, slot.data(), slot.size() * sizeof(NormSlot), hipMemcpyHostToDevice, st));
    GH_HIP(hipMemcpyAsync(d_prior, prior.data(), prior.size() * 8, hipMemcpyHostToDevice, st));
    GH_HIP(gh_norm_launch(st, b->dtype, b->feats, b->D, d_slot, b->U, d_prior, prior_frames, nullptr));
    GH_HIP(hipStreamSynchronize(st));   // (the uploads come from this call's host memory)
    b->nll_serial = 0;                  // likelihoods the batch may hold belong to the features it had
    return GH_OK;
}
