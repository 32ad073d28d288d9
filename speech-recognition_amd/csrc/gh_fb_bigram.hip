// Forward-backward over the BIGRAM form (gh_lattices::bigram_ok / bigram_wide_ok, gh_internal.h), and from it the WORD
// POSTERIORS q_t(w) and the per-word confidences of a decode under a language model (gh_word_posteriors_bigram,
// include/gmmhmm.h).  NOT IN THE REFERENCE; the sum-product twin of viterbi_bigram_wide_kernel (gh_viterbi_bigram_wide.hip)
// and the bigram-form twin of fb_loop_kernel (gh_fb_loop.hip), in that kernel's mapping: ONE utterance per wave, lane =
// word, the N log-alphas (then the N log-betas) of the lane's word in registers, 2 .. 64 words on the one mapping.
//
// Arithmetic as in gh_fb_loop.hip: log domain, fp64, a term is (origin - arc cost) - emission, a log-sum-exp is
// max + log(sum exp(term - max)) and -inf when the maximum is -inf, gamma is exp((alpha + beta) - logP); compiled without
// contraction.  What is new are the two W x W steps that take the place of the loop form's one wave_lse per direction:
//   forward    EN_t(w) = LSE_v( a_v[N-1] - B[v][w] )      the entry row of w, from the last states of THIS column
//   backward   BE_t(u) = b_u[0] - e[s0_u][t]              the entry row's beta (one arc, cost 0: no reduction)
//              LV_t(v) = LSE_u( BE_t(u) - B[v][u] )       what the last state of v sees through the entry rows
// The other lane's value (a_v[N-1], BE_t(u)) is wave-uniform for a given v or u and comes from v_readlane, as in
// viterbi_bigram_wide_kernel.  THE MAXIMUM OF EVERY LOG-SUM-EXP IS THE LANE'S OWN: two passes over the candidates, the
// first takes the maximum of the lane's 64 terms, the second sums exp(term - max).  (One wave-wide maximum of a_v and a
// table of exp(-B) would need one exp per candidate less; a word whose only allowed predecessors lie far below the wave's
// maximum would then underflow to -inf where the true value is finite.  Not built.)  Candidates run in ascending order up
// to the next multiple of 16 behind the last word (wave-uniform trip count): 17 words pay for 32 candidates, not 64.
//
// B IN LDS, TWICE: the forward pass reads COLUMN w at a fixed v -- image [v][w], lane w reads 8 bytes at v 512 + w 8,
// consecutive lanes, consecutive banks (the image of gh_viterbi_bigram_wide.hip).  The backward pass reads ROW v at a fixed u;
// on that image every lane would hit one bank, so a TRANSPOSED image [u][v] stands beside it: 2 x 32 KB per block, both
// filled once in front of the ONE __syncthreads() of the kernel, shared by the four waves (utterances) of the block.
// Every wave reaches that barrier: the tests of the launch's last slot and of an utterance without frames sit BEHIND it,
// and there is no barrier after them.  64 KB per block is two blocks, eight waves, per CU: two waves per SIMD (DESIGN.md
// 4.26 weighs this against re-filling one image between the passes).
//
// FORWARD, column t:  states N-1 .. 1 in place (fb_loop_kernel's), then EN_t, then
//   a[0] = LSE(a[0] - c0[0], EN_t(w), t == 0 ? -cin0 : -inf) - e[0][t];  the column goes to alpha scratch [T][N][W].
// BACKWARD, column t descending:  state 0, BE_t, LV_t, states 1 .. N-1 (the last one also takes LV_t), then
//   q_t(w) = sum_s exp(alpha[s] + b[s] - logP) - exp(alpha[N-1] + LV_t(w) - logP), clamped at 0,
// and the confidences of the span table exactly as in fb_loop_kernel (descending t, one order of summation).
// Lanes w >= W carry +inf arc costs: everything of theirs is -inf, exp() of it 0, and they store nothing.
#include "gh_internal.h"
#include "gh_fb.h"
#include "gh_viterbi.h"
#include "gh_wave.h"

namespace {

constexpr int FBB_WAVES = 4;               // utterances (waves) per block: they share the two LDS images of B
constexpr int FBB_W = GH_LAYERS_MAXW;      // 64: rows and columns of the cost table

// the value of lane l (wave-uniform) as a wave-uniform double
__device__ __forceinline__ double lane_of(double v, int l) {
    return __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(v), l), __builtin_amdgcn_readlane(__double2loint(v), l));
}
// maximum / sum over the 64 lanes, the same value in every lane (gh_fb_loop.hip).  A wave owns its utterance, so EXEC is full.
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

// LSE over c = 0 .. n16 - 1 of ( x of lane c  -  img[c 64 + lane] ), the maximum the lane's own.  n16 is wave-uniform, so
// every lane runs both loops and the readlanes sit under uniform control; a lane whose terms are all -inf subtracts 0
// instead of its maximum (every exp is then exp(-inf) = 0) and is given -inf at the end: no -inf - -inf anywhere.
__device__ __forceinline__ double cross_lse(double x, const double* img, unsigned lane_off, int n16) {
    double m = -INFINITY;
#pragma unroll 4
    for (int c = 0; c < n16; ++c) m = vmax(m, lane_of(x, c) - img[c * FBB_W + lane_off]);
    const bool none = m == -INFINITY;
    const double mm = none ? 0.0 : m;
    double sm = 0.0;
#pragma unroll 4
    for (int c = 0; c < n16; ++c) sm += exp((lane_of(x, c) - img[c * FBB_W + lane_off]) - mm);
    return none ? -INFINITY : mm + log(sm);
}

template <typename ET, int N, bool SKIP>
__global__ __launch_bounds__(64 * FBB_WAVES) void fb_bigram_kernel(gh_fbloop_args a, const double* __restrict__ bg, int64_t slot_end) {
    __shared__ double s_b[FBB_W * FBB_W];                     // [v][w]: cost of word w after word v (+inf: none)
    __shared__ double s_bt[FBB_W * FBB_W];                    // [u][v] = B[v][u]: the backward pass reads row v at a fixed u
    for (int i = threadIdx.x; i < FBB_W * FBB_W; i += 64 * FBB_WAVES) {
        s_b[i] = bg[i];
        s_bt[i] = bg[(i & (FBB_W - 1)) * FBB_W + (i >> 6)];
    }
    static_assert(FBB_W == 64, "the transposed fill splits an index into 6 + 6 bits");
    __syncthreads();                                          // the only barrier: every wave of the block is here
    const int lane = threadIdx.x & 63, w = lane;
    const int64_t slot = a.slot0 + (int64_t)blockIdx.x * FBB_WAVES + (threadIdx.x >> 6);
    if (slot >= slot_end) return;                             // (wave-uniform; no barrier behind this line)
    const gh_layerform* __restrict__ lf = a.lf;
    const int W = lf->W, Lr = lf->loop_row;
    const int64_t u = a.perm ? a.perm[slot] : slot;
    const int64_t f0 = a.utt_off[u];
    const int T = (int)(a.utt_off[u + 1] - f0);
    const double NEG = -INFINITY, INF = INFINITY;
    const bool wact = w < W;
    const int wc = wact ? w : 0;
    const int n16 = (W + 15) & ~15;                           // candidates: whole groups of 16, none behind the last word's group
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
        const int r = s == 0 ? Lr + W + wc : 1 + wc * (N - 1) + (s - 1);
        is_end[s] = wact && a.end_slot[r] >= 0;
    }
    const double cin0 = wact ? lf->cin0[wc] : INF;
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
        // the images never change; the lane's offset is made opaque once per column so that none of them is kept in registers
        unsigned wo = (unsigned)w;
        asm volatile("" : "+v"(wo));
        const double EN = cross_lse(v[N - 1], s_b, wo, n16);
        v[0] = lse3(self0, EN, (t == 0) ? -cin0 : NEG) - e[0];
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
        // 1. state 0, 2. the entry rows' betas and what the last states see through them, 3. the other states
        const double endt0 = (last && is_end[0]) ? 0.0 : NEG;
        if (SKIP && N >= 3) v[0] = lse4(endt0, f0t[0], f1t[1], f2t[N >= 3 ? 2 : 0]);
        else v[0] = lse3(endt0, f0t[0], f1t[1]);
        const double BE = v[0] - (double)ec[0];               // (the arc entry row -> state 0 costs 0)
        unsigned wo = (unsigned)w;
        asm volatile("" : "+v"(wo));
        const double LV = cross_lse(BE, s_bt, wo, n16);
#pragma unroll
        for (int s = 1; s < N; ++s) {
            const double endt = (last && is_end[s]) ? 0.0 : NEG;
            const double nx = (s + 1 < N) ? f1t[s + 1 < N ? s + 1 : s] : LV;
            if (SKIP && s + 2 < N) v[s] = lse4(endt, f0t[s], nx, f2t[s + 2 < N ? s + 2 : s]);
            else v[s] = lse3(endt, f0t[s], nx);
        }
        // 4. the word posterior of this column: the cells of the word, less the paths that leave it in this column
        double q = 0.0;
#pragma unroll
        for (int s = 0; s < N; ++s) q += exp((ac[s] + v[s]) - logp);
        q -= exp((ac[N - 1] + LV) - logp);
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

// the narrow form's costs (gh_layerform::bg, 16 x 16) as the 64 x 64 table the kernel takes: +inf behind the words
__global__ __launch_bounds__(256) void fb_bigram_table_kernel(const gh_layerform* __restrict__ lf, double* __restrict__ bg) {
    for (int i = threadIdx.x; i < FBB_W * FBB_W; i += 256) {
        const int v = i >> 6, w = i & (FBB_W - 1);
        bg[i] = (v < GH_LAYERS_ROWW && w < GH_LAYERS_ROWW) ? lf->bg[v][w] : INFINITY;
    }
}

}  // namespace

int gh_fill_fb_bigram_table(gh_ctx* ctx, const gh_layerform* d_lf, double* d_bg) {
    hipLaunchKernelGGL(fb_bigram_table_kernel, dim3(1), dim3(256), 0, ctx->stream, d_lf, d_bg);
    GH_HIP(hipGetLastError());
    return GH_OK;
}

#define GH_FBB(ET, NN, SK) hipLaunchKernelGGL((fb_bigram_kernel<ET, NN, SK>), grid, blk, 0, ctx->stream, b, d_bg, slot_end)

int gh_launch_fb_bigram(gh_ctx* ctx, const gh_fbloop_args& a, const gh_layerform& f, const double* d_bg, int64_t u_begin, int64_t n_utts,
                        bool f64) {
    if (n_utts <= 0) return GH_OK;
    GH_REQUIRE(d_bg, "gh_word_posteriors_bigram: internal: no cost table");
    gh_fbloop_args b = a;
    b.slot0 = u_begin;
    const dim3 grid((unsigned)((n_utts + FBB_WAVES - 1) / FBB_WAVES)), blk(64 * FBB_WAVES);
    const int64_t slot_end = u_begin + n_utts;
    if (f64) { GH_NSKIP_SWITCH(f.N, f.skip, 8, GH_FBB, double, "gh_word_posteriors_bigram: bigram form with %d states per word", f.N) }
    else { GH_NSKIP_SWITCH(f.N, f.skip, 8, GH_FBB, float, "gh_word_posteriors_bigram: bigram form with %d states per word", f.N) }
    GH_HIP(hipGetLastError());
    return GH_OK;
}
