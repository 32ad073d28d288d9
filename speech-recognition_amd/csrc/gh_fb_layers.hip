// Forward-backward over the narrow LAYER form (gh_layerform with loop == 0: the K-layer lattice of the reference's continuous
// recogniser), and from it the WORD POSTERIORS q_t(w) and the per-word confidences of a decode (gh_word_posteriors_layers,
// include/gmmhmm.h).  NOT IN THE REFERENCE; the sum-product twin of viterbi_layers_kernel (gh_viterbi_layers.hip) in that
// kernel's mapping: ONE utterance per wave, lane = 16 (k mod 4) + w, SETS = ceil(K / 4) register sets (layers 0-3, 4-7) of
// the N log-alphas (then the N log-betas) of the lane's word, arc costs in registers, emissions read a column ahead; the
// lanes of different layers of one word read the same emission.  1 .. 8 layers of 1 .. 16 words of 2 .. 8 states.
//
// Log domain, fp64, every term written the way fb_loop_kernel (gh_fb_loop.hip) writes it: a term is (origin - arc cost) -
// emission, a log-sum-exp is max + log(sum exp(term - max)) and returns -inf for an all -inf set before any subtraction,
// gamma is exp((alpha + beta) - logP).  The file is compiled without contraction, like that one.
//
// No chain over the layers inside a column: a word has >= 2 states, so its last state never depends on its first state
// of the same column.
// FORWARD, column t, a[h][] = the previous column of register set h (all -inf before column 0), sets ascending:
//   s >= 1 (descending, in place):  a[s] = LSE(a[s] - c0[s], a[s-1] - c1[s], a[s-2] - c2[s]) - e[s][t]
//   NES_{k+1}(t) = LSE over the 16-lane row of a[N-1] - cout   (row rotations; lane 0 of the row is THE value)
//   it is handed to row (k+1) mod 4; row 3 of set 0 hands its value to row 0 of set 1; NES_0 = 0 in column 0, -inf after
//   a[0] = LSE(NES_k(t) - cin, a[0] - c0[0]) - e[0][t]
//   the column goes to alpha scratch, dense [T][K][N][W] doubles
// logP = LSE over the end rows of the last column.
// BACKWARD, column t descending, b[h][] = the next column (all -inf behind the last), sets DESCENDING:
//   1. b[0] = LSE(end term, b[0] - c0[0] - en[0], b[1] - c1[1] - en[1], b[2] - c2[2] - en[2])
//   2. BNES_k(t) = LSE over the row of b[0] - cin - e[0][t]     (lane 0 of the row is THE value), handed DOWN one row to the
//      last states of layer k-1; row 0 of set 1 hands its value to row 3 of set 0; BNES_K = -inf
//   3. s >= 1 ascending, in place; the last state also takes BNES_{k+1} - cout
//   4. q_t(k, w) = sum_s exp(alpha[s] + b[s] - logP) - exp(alpha[N-1] - cout + BNES_{k+1} - logP), clamped at 0
//      q_t(w) = ((q(0,w) + q(4,w)) + (q(1,w) + q(5,w))) + ((q(2,w) + q(6,w)) + (q(3,w) + q(7,w)))    THE order of the layer sum:
//      set 0 + set 1 inside a lane, then the lane 16 away, then the lane 32 away; absent layers add 0.0.  One coalesced
//      row of W doubles per column.
//   5. confidences as in fb_loop_kernel: the span index is wave-uniform and steps down when t passes begins[k]; every lane
//      adds its own q, lane labels[k] stores the mean when t == begins[k].  Descending t is the one order of summation.
// Lanes w >= W and layer slots k >= K carry +inf entry and exit costs and -inf alphas: everything of theirs is -inf, exp()
// of it 0; they store nothing and read alpha scratch of cell (layer 0, word 0) only to discard it.  Every cross-lane step
// sits under wave-uniform control flow (the column and set loops, and tests of values read off lanes).
#include "gh_internal.h"
#include "gh_fb.h"
#include "gh_viterbi.h"
#include "gh_wave.h"

namespace {

__device__ __forceinline__ double lane_of(double v, int l) {
    return __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(v), l), __builtin_amdgcn_readlane(__double2loint(v), l));
}
// maximum / sum over the 64 lanes, the same value in every lane (wave_max / wave_sum of gh_fb_loop.hip)
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
// log-sum-exp over each 16-lane row (one term per lane).  No branch: the four rows differ, so an all -inf row is a select.
// The maximum is the same in all lanes of a row; the sum is rounded in a lane's own order, so callers read lane 0 of a row.
__device__ __forceinline__ double row_lse(double v) {
    double m = v;
    m = vmax(m, row_rot<0x121>(m));
    m = vmax(m, row_rot<0x122>(m));
    m = vmax(m, row_rot<0x124>(m));
    m = vmax(m, row_rot<0x128>(m));
    const bool none = m == -INFINITY;
    double s = exp(v - (none ? 0.0 : m));                   // never -inf - -inf
    s += row_rot<0x121>(s);
    s += row_rot<0x122>(s);
    s += row_rot<0x124>(s);
    s += row_rot<0x128>(s);
    return none ? -INFINITY : m + log(s);
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

template <typename ET, int N, bool SKIP, int SETS>
__global__ __launch_bounds__(64) void fb_layers_kernel(gh_fbloop_args a) {
    const int lane = threadIdx.x, kk = lane >> 4, w = lane & 15;
    const gh_layerform* __restrict__ lf = a.lf;
    const int K = lf->K, W = lf->W, P = lf->P;
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
#pragma unroll
    for (int s = 0; s < N; ++s) {
        c0[s] = wact ? lf->c0[wc][s] : INF;
        c1[s] = wact ? lf->c1[wc][s] : INF;
        c2[s] = (SKIP && wact) ? lf->c2[wc][s] : INF;
        sto[s] = (unsigned)lf->state[wc][s] * (unsigned)sizeof(ET);
    }
    bool act[SETS];
    double cin[SETS], cout[SETS];
    unsigned endm[SETS];                                      // bit s: state s of the lane's word in this layer is an end row
    double* __restrict__ al[SETS];                            // cell (t, s) of this lane's layer and word at (t K N + s) W
#pragma unroll
    for (int h = 0; h < SETS; ++h) {
        const int layer = 4 * h + kk;
        act[h] = wact && layer < K;                           // unused layer slots / word lanes: everything stays -inf
        const int lc = act[h] ? layer : 0, wl = act[h] ? w : 0;
        cin[h] = act[h] ? lf->cin[wc] : INF;
        cout[h] = act[h] ? lf->cout[wc] : INF;
        endm[h] = 0;
#pragma unroll
        for (int s = 0; s < N; ++s)
            if (act[h] && a.end_slot[lc * (P + 1) + 1 + wl * N + s] >= 0) endm[h] |= 1u << s;
        al[h] = a.alpha_scratch + a.scratch_off[slot] + (int64_t)lc * N * W + wl;
    }
    const char* nllb = static_cast<const char*>(a.nll) + f0 * a.S * (int64_t)sizeof(ET);
    const int64_t rowb = (int64_t)a.S * (int64_t)sizeof(ET);

    // ------------------------------------------------------------------------------------------------ forward
    double v[SETS][N];
    ET en[N];
#pragma unroll
    for (int s = 0; s < N; ++s) {
#pragma unroll
        for (int h = 0; h < SETS; ++h) v[h][s] = NEG;
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
        double carry = (t == 0) ? 0.0 : NEG;                  // NES_0: the start row, log alpha 0 in column 0 only
#pragma unroll
        for (int h = 0; h < SETS; ++h) {
            const double self0 = v[h][0] - c0[0];
#pragma unroll
            for (int s = N - 1; s >= 1; --s) {
                const double t0 = v[h][s] - c0[s], t1 = v[h][s - 1] - c1[s];
                double r;
                if (SKIP && s >= 2) r = lse3(t0, t1, v[h][s - 2] - c2[s]);
                else r = lse2(t0, t1);
                v[h][s] = r - e[s];
            }
            // the non-emitting row behind every layer of the set, handed to the next row; row 0 takes what the set before left
            const double L = row_lse(v[h][N - 1] - cout[h]);
            const double l0 = lane_of(L, 0), l1 = lane_of(L, 16), l2 = lane_of(L, 32), l3 = lane_of(L, 48);
            const double nin = kk == 0 ? carry : kk == 1 ? l0 : kk == 2 ? l1 : l2;
            carry = l3;
            v[h][0] = lse2(nin - cin[h], self0) - e[0];
            if (act[h]) {
#pragma unroll
                for (int s = 0; s < N; ++s) al[h][((int64_t)t * K * N + s) * W] = v[h][s];
            }
        }
    }
    // log P: one log-sum-exp over the end rows of the last column
    double logp;
    {
        double m = NEG;
#pragma unroll
        for (int h = 0; h < SETS; ++h)
#pragma unroll
            for (int s = 0; s < N; ++s) m = vmax(m, ((endm[h] >> s) & 1u) ? v[h][s] : NEG);
        m = wave_max(m);
        if (m == NEG) logp = NEG;
        else {
            double sm = 0.0;
#pragma unroll
            for (int h = 0; h < SETS; ++h)
#pragma unroll
                for (int s = 0; s < N; ++s) sm += ((endm[h] >> s) & 1u) ? exp(v[h][s] - m) : 0.0;
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
        if (post && wact && kk == 0)
            for (int t = 0; t < T; ++t) post[(int64_t)t * W] = 0.0;
        if (conf && lane == 0)
            for (int j = 0; j <= k; ++j) conf[j] = 0.0;
        return;
    }
    double acc = 0.0;
    ET ec[N];                                                // this column's emissions, loaded a column ahead
    double xe[N];                                            // emissions of the column behind: nothing lies behind the last
#pragma unroll
    for (int s = 0; s < N; ++s) {
        xe[s] = 0.0;
        ec[s] = *reinterpret_cast<const ET*>(nllb + (int64_t)(T - 1) * rowb + sto[s]);
#pragma unroll
        for (int h = 0; h < SETS; ++h) v[h][s] = NEG;
    }
    for (int t = T - 1; t >= 0; --t) {
        const bool last = t == T - 1;
        ET ep[N];
        {   // the emissions of the column in front travel while this one is summed
            const char* colp = nllb + (int64_t)(t > 0 ? t - 1 : 0) * rowb;
#pragma unroll
            for (int s = 0; s < N; ++s) ep[s] = *reinterpret_cast<const ET*>(colp + sto[s]);
        }
        double q = 0.0;
        double carry = NEG;                                   // BNES_K: nothing follows the last layer
#pragma unroll
        for (int h = SETS - 1; h >= 0; --h) {
            // this set's alphas of the column: asked for here, used in step 4, behind the set's logarithms (a column ahead
            // for both sets at once, they were the registers that did not fit at 8 states with skip arcs)
            double ac[N];
#pragma unroll
            for (int s = 0; s < N; ++s) {
                const double x = al[h][((int64_t)t * K * N + s) * W];
                ac[s] = act[h] ? x : NEG;
            }
            // the arcs into state s of the column behind, as terms: (beta - arc cost) - emission
            double f0t[N], f1t[N], f2t[N];
#pragma unroll
            for (int s = 0; s < N; ++s) {
                f0t[s] = (v[h][s] - c0[s]) - xe[s];                                    // from s
                f1t[s] = (s >= 1) ? (v[h][s] - c1[s]) - xe[s] : NEG;                   // from s - 1
                f2t[s] = (SKIP && s >= 2) ? (v[h][s] - c2[s]) - xe[s] : NEG;           // from s - 2
            }
            // 1. state 0, 2. the non-emitting rows' betas, handed down a row, 3. the other states
            const double endt0 = (last && (endm[h] & 1u)) ? 0.0 : NEG;
            if (SKIP && N >= 3) v[h][0] = lse4(endt0, f0t[0], f1t[1], f2t[N >= 3 ? 2 : 0]);
            else v[h][0] = lse3(endt0, f0t[0], f1t[1]);
            const double BL = row_lse((v[h][0] - cin[h]) - (double)ec[0]);
            const double r0 = lane_of(BL, 0), r1 = lane_of(BL, 16), r2 = lane_of(BL, 32), r3 = lane_of(BL, 48);
            const double nb = kk == 0 ? r1 : kk == 1 ? r2 : kk == 2 ? r3 : carry;
            carry = r0;
#pragma unroll
            for (int s = 1; s < N; ++s) {
                const double endt = (last && ((endm[h] >> s) & 1u)) ? 0.0 : NEG;
                const double nx = (s + 1 < N) ? f1t[s + 1 < N ? s + 1 : s] : (nb - cout[h]);
                if (SKIP && s + 2 < N) v[h][s] = lse4(endt, f0t[s], nx, f2t[s + 2 < N ? s + 2 : s]);
                else v[h][s] = lse3(endt, f0t[s], nx);
            }
            // 4. the posterior of this layer's word in this column
            double qh = 0.0;
#pragma unroll
            for (int s = 0; s < N; ++s) qh += exp((ac[s] + v[h][s]) - logp);
            qh -= exp(((ac[N - 1] - cout[h]) + nb) - logp);
            qh = (qh > 0.0) ? qh : 0.0;                      // below 0 by rounding: 0
            q = (h == SETS - 1) ? qh : qh + q;               // set 0 + set 1
        }
        q = q + __shfl_xor(q, 16);                           // the layer sum: the lane 16 away, then the lane 32 away
        q = q + __shfl_xor(q, 32);
        if (post && wact && kk == 0) post[(int64_t)t * W] = q;
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

#define GH_FBY(ET, NN, SK)                                                                              \
    do {                                                                                                \
        if (f.K > 4) hipLaunchKernelGGL((fb_layers_kernel<ET, NN, SK, 2>), grid, blk, 0, ctx->stream, b);  \
        else hipLaunchKernelGGL((fb_layers_kernel<ET, NN, SK, 1>), grid, blk, 0, ctx->stream, b);          \
    } while (0)

int gh_launch_fb_layers(gh_ctx* ctx, const gh_fbloop_args& a, const gh_layerform& f, int64_t u_begin, int64_t n_utts, bool f64) {
    if (n_utts <= 0) return GH_OK;
    gh_fbloop_args b = a;
    b.slot0 = u_begin;
    const dim3 grid((unsigned)n_utts), blk(64);
    if (f64) { GH_NSKIP_SWITCH(f.N, f.skip, 8, GH_FBY, double, "gh_word_posteriors_layers: layer form with %d states per word", f.N) }
    else { GH_NSKIP_SWITCH(f.N, f.skip, 8, GH_FBY, float, "gh_word_posteriors_layers: layer form with %d states per word", f.N) }
    GH_HIP(hipGetLastError());
    return GH_OK;
}
