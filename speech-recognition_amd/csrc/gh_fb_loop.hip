// Forward-backward over the LOOP form (gh_layerform with loop == 1), and from it the WORD POSTERIORS q_t(w) and the
// per-word confidences of a decode (gh_word_posteriors, include/gmmhmm.h).  NOT IN THE REFERENCE; the sum-product twin of
// viterbi_loop_wide_kernel (gh_viterbi_layers_wide.hip) in that kernel's mapping: ONE utterance per wave, lane = word, the
// N log-alphas (then the N log-betas) of the lane's word in registers, 1 .. 64 words on the one mapping.
//
// Log domain, fp64, every sum written the way the host statement of the definition writes it (a term is
// (origin - arc cost) - emission, a log-sum-exp is max + log(sum exp(term - max)), gamma is exp((alpha + beta) - logP)):
// with costs of order 1e6 a log-alpha is of order 1e7 and one unit in its last place is 1e-9, so the two sides agree to
// 1e-8 in a posterior only where they round alike.  The file is compiled without contraction for the same reason.
//
// FORWARD, column t, a[] = the previous column (all -inf before column 0):
//   s >= 1 (descending, in place):  a[s] = LSE(a[s] - c0[s], a[s-1] - c1[s], a[s-2] - c2[s]) - e[s][t]
//   L_t = LSE over the lanes of a[N-1] - cout                 the loop row's alpha: the only cross-lane step
//   a[0] = LSE(a[0] - c0[0], L_t - cin, t == 0 ? -cin0 : -inf) - e[0][t]
//   the column goes to alpha scratch, dense [T][N][W] doubles
// logP = LSE over the end rows of the last column.
// BACKWARD, column t descending, b[] = the next column (all -inf behind the last), en[] = its emissions:
//   1. b[0] = LSE(end term, b[0] - c0[0] - en[0], b[1] - c1[1] - en[1], b[2] - c2[2] - en[2])
//   2. BL_t = LSE over the lanes of b[0] - cin - e[0][t]      the loop row's beta
//   3. s >= 1 ascending, in place; the last state also takes BL_t - cout
//   4. q_t(w) = sum_s exp(alpha[s] + b[s] - logP) - exp(alpha[N-1] - cout + BL_t - logP), clamped at 0; one coalesced row
//      of W doubles per column
//   5. confidences: the span index k is wave-uniform and steps down when t passes begins[k]; every lane adds its own q,
//      lane labels[k] stores the mean when t == begins[k].  Descending t is the one order of summation, whatever the
//      batch position or the chunking.
// Lanes w >= W carry +inf arc costs: everything of theirs is -inf, exp() of it 0, and they store nothing.  Every
// cross-lane reduction sits under wave-uniform control flow (the column loops, and tests of values read off lanes).
#include "gh_internal.h"
#include "gh_fb.h"
#include "gh_viterbi.h"
#include "gh_wave.h"

namespace {

__device__ __forceinline__ double lane_of(double v, int l) {
    return __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(v), l), __builtin_amdgcn_readlane(__double2loint(v), l));
}
// maximum / sum over the 64 lanes, the same value in every lane: row_ror 1, 2, 4, 8 inside the 16-lane rows, then one lane
// of each row (wave_min of gh_viterbi_layers_wide.hip).  A wave owns its utterance, so EXEC is full.
__device__ __forceinline__ double wave_max(double v) {
    v = vmax(v, row_rot<0x121>(v));
    v = vmax(v, row_rot<0x122>(v));
    v = vmax(v, row_rot<0x124>(v));
    v = vmax(v, row_rot<0x128>(v));
    return vmax(vmax(lane_of(v, 0), lane_of(v, 16)), vmax(lane_of(v, 32), lane_of(v, 48)));
}
__device__ __forceinline__ double wave_sum(double v) {
    v += row_rot<0x121>(v);
    v += row_rot<0x122>(v);
    v += row_rot<0x124>(v);
    v += row_rot<0x128>(v);
    return (lane_of(v, 0) + lane_of(v, 16)) + (lane_of(v, 32) + lane_of(v, 48));
}
// log-sum-exp over the lanes (one term per lane); the test is on a wave-uniform value
__device__ __forceinline__ double wave_lse(double v) {
    const double m = wave_max(v);
    if (m == -INFINITY) return m;
    return m + log(wave_sum(exp(v - m)));
}
// log-sum-exp inside a lane: -inf terms add exp(-inf) = 0, and an all -inf set gives -inf (never -inf - -inf)
__device__ __forceinline__ double lse2(double x, double y) {
    const double m = vmax(x, y);
    if (m == -INFINITY) return m;
    return m + log(exp(x - m) + exp(y - m));
}
__device__ __forceinline__ double lse3(double x, double y, double z) {
    const double m = vmax(vmax(x, y), z);
    if (m == -INFINITY) return m;
    return m + log((exp(x - m) + exp(y - m)) + exp(z - m));
}
__device__ __forceinline__ double lse4(double x, double y, double z, double v) {
    const double m = vmax(vmax(x, y), vmax(z, v));
    if (m == -INFINITY) return m;
    return m + log(((exp(x - m) + exp(y - m)) + exp(z - m)) + exp(v - m));
}

template <typename ET, int N, bool SKIP>
__global__ __launch_bounds__(64) void fb_loop_kernel(gh_fbloop_args a) {
    const int lane = threadIdx.x, w = lane;
    const gh_layerform* __restrict__ lf = a.lf;
    const int W = lf->W, Lr = lf->loop_row;
    const int64_t slot = a.slot0 + blockIdx.x;
    const int64_t u = a.perm ? a.perm[slot] : slot;
    const int64_t f0 = a.utt_off[u];
    const int T = (int)(a.utt_off[u + 1] - f0);
    const double NEG = -INFINITY, INF = INFINITY;
    const bool wact = w < W;
    const int wc = wact ? w : 0;
    if (T <= 0) {
        if (lane == 0) a.logp[u] = NEG;
        return;
    }
    double c0[N], c1[N], c2[N];
    unsigned sto[N];
    bool is_end[N];
#pragma unroll
    for (int s = 0; s < N; ++s) {
        c0[s] = wact ? lf->c0[wc][s] : INF;
        c1[s] = wact ? lf->c1[wc][s] : INF;
        c2[s] = (SKIP && wact) ? lf->c2[wc][s] : INF;
        sto[s] = (unsigned)lf->state[wc][s] * (unsigned)sizeof(ET);
        const int r = s == 0 ? Lr + 1 + wc : 1 + wc * (N - 1) + (s - 1);
        is_end[s] = wact && a.end_slot[r] >= 0;
    }
    const double cin = wact ? lf->cin[wc] : INF, cin0 = wact ? lf->cin0[wc] : INF, cout = wact ? lf->cout[wc] : INF;
    const char* nllb = static_cast<const char*>(a.nll) + f0 * a.S * (int64_t)sizeof(ET);
    const int64_t rowb = (int64_t)a.S * (int64_t)sizeof(ET);
    double* __restrict__ al = a.alpha_scratch + a.scratch_off[slot] + wc;     // cell (t, s) of this lane at (t N + s) W

    // ------------------------------------------------------------------------------------------------ forward
    double v[N];
    ET en[N];
#pragma unroll
    for (int s = 0; s < N; ++s) {
        v[s] = NEG;
        en[s] = *reinterpret_cast<const ET*>(nllb + sto[s]);
    }
    for (int t = 0; t < T; ++t) {
        double e[N];
#pragma unroll
        for (int s = 0; s < N; ++s) e[s] = (double)en[s];
        {   // the next column's emissions travel while this one is summed
            const char* colp = nllb + (int64_t)((t + 1 < T) ? t + 1 : t) * rowb;
#pragma unroll
            for (int s = 0; s < N; ++s) en[s] = *reinterpret_cast<const ET*>(colp + sto[s]);
        }
        const double self0 = v[0] - c0[0];
#pragma unroll
        for (int s = N - 1; s >= 1; --s) {
            const double t0 = v[s] - c0[s], t1 = v[s - 1] - c1[s];
            double r;
            if (SKIP && s >= 2) r = lse3(t0, t1, v[s - 2] - c2[s]);
            else r = lse2(t0, t1);
            v[s] = r - e[s];
        }
        const double L = wave_lse(v[N - 1] - cout);
        v[0] = lse3(self0, L - cin, (t == 0) ? -cin0 : NEG) - e[0];
        if (wact) {
#pragma unroll
            for (int s = 0; s < N; ++s) al[((int64_t)t * N + s) * W] = v[s];
        }
    }
    // log P: one log-sum-exp over the end rows of the last column
    double logp;
    {
        double m = NEG;
#pragma unroll
        for (int s = 0; s < N; ++s) m = vmax(m, is_end[s] ? v[s] : NEG);
        m = wave_max(m);
        if (m == NEG) logp = NEG;
        else {
            double sm = 0.0;
#pragma unroll
            for (int s = 0; s < N; ++s) sm += is_end[s] ? exp(v[s] - m) : 0.0;
            logp = m + log(wave_sum(sm));
        }
    }
    if (lane == 0) a.logp[u] = logp;
    if (!a.post && !a.conf) return;

    // ----------------------------------------------------------------------------------------------- backward
    double* __restrict__ post = a.post ? a.post + f0 * W + wc : nullptr;
    int k = -1, k_begin = -1, k_label = -1, k_end = T;       // the span the sweep is in (wave-uniform)
    const int32_t* __restrict__ labs = nullptr;
    const int32_t* __restrict__ begs = nullptr;
    double* __restrict__ conf = nullptr;
    if (a.conf) {
        const int64_t lo = a.label_off[u];
        labs = a.labels + lo;
        begs = a.begins + lo;
        conf = a.conf + lo;
        k = a.n_labels[u] - 1;
        if (k >= 0) { k_begin = begs[k]; k_label = labs[k]; }
    }
    if (logp == NEG) {   // no path: every posterior is 0, every confidence 0.0
        if (post && wact)
            for (int t = 0; t < T; ++t) post[(int64_t)t * W] = 0.0;
        if (conf && lane == 0)
            for (int j = 0; j <= k; ++j) conf[j] = 0.0;
        return;
    }
    double acc = 0.0;
    ET ec[N];                                                // this column's emissions, loaded a column ahead
    double xe[N];                                            // emissions of the column behind: nothing lies behind the last
    double av[N];                                            // this column's alphas, loaded a column ahead
#pragma unroll
    for (int s = 0; s < N; ++s) {
        v[s] = NEG;
        xe[s] = 0.0;
        ec[s] = *reinterpret_cast<const ET*>(nllb + (int64_t)(T - 1) * rowb + sto[s]);
        av[s] = al[((int64_t)(T - 1) * N + s) * W];
    }
    for (int t = T - 1; t >= 0; --t) {
        const bool last = t == T - 1;
        double ac[N];
#pragma unroll
        for (int s = 0; s < N; ++s) ac[s] = av[s];
        ET ep[N];
        {   // the column in front travels while this one is summed: its alphas and its emissions
            const int tp = t > 0 ? t - 1 : 0;
            const char* colp = nllb + (int64_t)tp * rowb;
#pragma unroll
            for (int s = 0; s < N; ++s) {
                av[s] = al[((int64_t)tp * N + s) * W];
                ep[s] = *reinterpret_cast<const ET*>(colp + sto[s]);
            }
        }
        // the arcs into state s of the column behind, as terms: (beta - arc cost) - emission
        double f0t[N], f1t[N], f2t[N];
#pragma unroll
        for (int s = 0; s < N; ++s) {
            f0t[s] = (v[s] - c0[s]) - xe[s];                                    // from s
            f1t[s] = (s >= 1) ? (v[s] - c1[s]) - xe[s] : NEG;                   // from s - 1
            f2t[s] = (SKIP && s >= 2) ? (v[s] - c2[s]) - xe[s] : NEG;           // from s - 2
        }
        // 1. state 0, 2. the loop row's beta, 3. the other states (the last one also leaves through the loop row)
        const double endt0 = (last && is_end[0]) ? 0.0 : NEG;
        if (SKIP && N >= 3) v[0] = lse4(endt0, f0t[0], f1t[1], f2t[N >= 3 ? 2 : 0]);
        else v[0] = lse3(endt0, f0t[0], f1t[1]);
        const double BL = wave_lse((v[0] - cin) - (double)ec[0]);
#pragma unroll
        for (int s = 1; s < N; ++s) {
            const double endt = (last && is_end[s]) ? 0.0 : NEG;
            const double nx = (s + 1 < N) ? f1t[s + 1 < N ? s + 1 : s] : (BL - cout);
            if (SKIP && s + 2 < N) v[s] = lse4(endt, f0t[s], nx, f2t[s + 2 < N ? s + 2 : s]);
            else v[s] = lse3(endt, f0t[s], nx);
        }
        // 4. the word posterior of this column
        double q = 0.0;
#pragma unroll
        for (int s = 0; s < N; ++s) q += exp((ac[s] + v[s]) - logp);
        q -= exp(((ac[N - 1] - cout) + BL) - logp);
        q = (q > 0.0) ? q : 0.0;                             // below 0 by rounding: 0
        if (post && wact) post[(int64_t)t * W] = q;
        // 5. the confidence of the span this column lies in
        if (k >= 0) {
            acc += q;
            if (t == k_begin) {
                if (lane == k_label) conf[k] = acc / (double)(k_end - k_begin);
                acc = 0.0;
                k_end = k_begin;
                --k;
                if (k >= 0) { k_begin = begs[k]; k_label = labs[k]; }
            }
        }
#pragma unroll
        for (int s = 0; s < N; ++s) { xe[s] = (double)ec[s]; ec[s] = ep[s]; }
    }
}

}  // namespace

#define GH_FBL(ET, NN, SK) hipLaunchKernelGGL((fb_loop_kernel<ET, NN, SK>), grid, blk, 0, ctx->stream, b)

int gh_launch_fb_loop(gh_ctx* ctx, const gh_fbloop_args& a, const gh_layerform& f, int64_t u_begin, int64_t n_utts, bool f64) {
    if (n_utts <= 0) return GH_OK;
    gh_fbloop_args b = a;
    b.slot0 = u_begin;
    const dim3 grid((unsigned)n_utts), blk(64);
    if (f64) { GH_NSKIP_SWITCH(f.N, f.skip, 8, GH_FBL, double, "gh_word_posteriors: loop form with %d states per word", f.N) }
    else { GH_NSKIP_SWITCH(f.N, f.skip, 8, GH_FBL, float, "gh_word_posteriors: loop form with %d states per word", f.N) }
    GH_HIP(hipGetLastError());
    return GH_OK;
}
