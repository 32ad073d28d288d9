// ONLINE decode over the WIDE BIGRAM form (gh_lattices::bigram_wide_ok: the bigram grammar with 17 .. 64 words of 2 .. 8
// states): the sweep of gh_viterbi_bigram_wide.hip (viterbi_bigram_wide_kernel, WANT_BP) CARRIED ACROSS CHUNKS of an
// utterance that is still arriving, as gh_viterbi_online_wide.hip carries the wide loop sweep.  A stream is fully described by
//   * the previous column: the N state costs of its 64 word lanes                [stream][N][64] doubles (512 N B),
//   * the number of frames it has taken (host side: the absolute column of the next frame),
// and its decision history: the one-shot kernel writes ONE COMPLETE 32-bit record per column and lane -- the in-word bits, 6
// bits of predecessor word, the two bits of state 0 (gh_bigram_wide_hb) -- at [column][64 lanes], so the record of absolute
// column ta goes to hist[stream][ta % ring_cols][lane], 256 B per frame.  A session that keeps its full history passes a ring
// it never fills, and column ta then lies exactly where viterbi_bigram_wide_kernel puts column ta of a whole utterance.  There
// is no open word to carry.  bigram_backtrace_wide_kernel reads nothing but those records and the arc masks of the graph, an
// entry row's predecessor from the 6-bit field of the SAME record, so gh_launch_bigram_backtrace runs UNCHANGED on the history
// (path, labels, timed labels), and "the result after k frames" is bitwise the one-shot decode of the first k frames.
//
// gfx950 mapping: as the one-shot kernel -- ONE STREAM PER WAVE, lane = word, the N states of the word in registers, FOUR WAVES
// (four slots of the push) PER BLOCK sharing one LDS image [v][w] of the 64 x 64 word-to-word costs (32 KB, +inf where there is
// no arc or no word).  The image is filled once per block, one __syncthreads() in front of the column loop and none inside; a
// wave whose slot lies behind the push's last one takes part in the fill and the barrier and returns behind it (the guard is
// wave-uniform).  gh_online_push orders the slots longest first, so the four waves of a block end close to each other.  The
// column step is a copy of the one-shot kernel's, operation for operation: in-word candidates in ascending origin order under
// a strict '<'; entry[w] = min_v (last[v] + B[v][w]) over v_readlane scalars and the LDS column, four groups of 16 in ascending
// v with the fences that keep a group's arg beside its minimum, the wave-uniform skip of groups behind the last word, the
// merges with the lower group on the left; word = (word << 6) | v; then b_l, b_s.  What differs is where `prev` comes from and
// goes to, that the start-row term and the history address use the absolute column, and that there is no end selection in the
// sweep (online_end_kernel of gh_online.hip).  A chunk of t frames moves 512 N B of state in and out and t 256 B of records beside
// its emissions, and its block reads the 32 KB of costs once.
//
// THE RING.  A stream owns its wave, so the column, its ring position and the wrap are wave-uniform: the position starts from
// t0 % ring_cols once per launch and moves on by compare-and-subtract, as in viterbi_online_wide_kernel.  A session from
// gh_online_create_bigram_wide keeps its full history and does not settle: gh_online_commit* / gh_online_tail* refuse it.  One
// from gh_online_create_bigram_wide_settle settles, and with a window its ring holds the unsettled frames and the column the
// anchor lies in; the settle walk over these records is in gh_online_bigram_wide_settle.hip.  NOT OFFERED: a forced commit,
// and words of 12 or 16 states.
// No scratch and no runtime-indexed private array for any instantiation (profiles/online_bigram_wide_kernel_resources.txt).
#include "gh_online.h"
#include "gh_viterbi.h"
#include "gh_wave.h"

namespace {

constexpr int OBW_WAVES = 4;               // streams (waves) per block: they share the LDS image of B

// (a, ia) <- the smaller of (a, ia) and (b, ib); ia < ib always, so a tie keeps the lower word
#define GH_OBW_MERGE(a, ia, b, ib) do { const bool lt_ = (b) < (a); a = vmin(a, b); ia = lt_ ? (ib) : (ia); } while (0)

// the value of lane L (a constant) as a wave-uniform double
template <int L> __device__ __forceinline__ double lane_value(double x) {
    return __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(x), L), __builtin_amdgcn_readlane(__double2loint(x), L));
}

// candidates v = V0 .. V0 + 15 in ascending order: (best, arg) <- first minimum of last[v] + B[v][w]
template <int V0, int I = 0> __device__ __forceinline__ void entry_group(double x, const double* s_bg, unsigned w, double& best, uint32_t& arg) {
    if constexpr (I < 16) {
        const double q = lane_value<V0 + I>(x) + s_bg[(V0 + I) * GH_LAYERS_MAXW + w];
        GH_OBW_MERGE(best, arg, q, (uint32_t)(V0 + I));
        entry_group<V0, I + 1>(x, s_bg, w, best, arg);
    }
}

template <typename ET, int N, bool SKIP>
__global__ __launch_bounds__(64 * OBW_WAVES) void viterbi_bigram_online_wide_kernel(gh_online_args a, const gh_bigram_wide* __restrict__ bgw) {
    constexpr int PF = 4;
    static_assert(gh_bigram_wide_hb(N, SKIP) <= 32, "the decision bits of a column must fit one word");
    __shared__ double s_bg[GH_LAYERS_MAXW * GH_LAYERS_MAXW];
    for (int i = threadIdx.x; i < GH_LAYERS_MAXW * GH_LAYERS_MAXW; i += 64 * OBW_WAVES) s_bg[i] = (&bgw->bg[0][0])[i];
    __syncthreads();
    const int lane = threadIdx.x & 63, w = lane;
    const int64_t slot = (int64_t)blockIdx.x * OBW_WAVES + (threadIdx.x >> 6);
    if (slot >= a.n_slots) return;                            // (wave-uniform; no barrier behind this line)
    const gh_layerform* __restrict__ lf = a.lf;
    const int W = lf->W;
    const gh_online_slot sl = a.slots[slot];
    const int T = sl.count, tb = sl.t0;
    if (T <= 0) return;                                       // (gh_online_push drops such a slot on the host)
    const double INF = INFINITY;
    const bool wact = w < W;
    const int wc = wact ? w : 0;
    double c0[N], c1[N], c2[N];
    unsigned sto[N];
#pragma unroll
    for (int s = 0; s < N; ++s) {
        c0[s] = wact ? lf->c0[wc][s] : INF;
        c1[s] = wact ? lf->c1[wc][s] : INF;
        c2[s] = (SKIP && wact) ? lf->c2[wc][s] : INF;
        sto[s] = (unsigned)lf->state[wc][s] * (unsigned)sizeof(ET);
    }
    const double cin0 = wact ? lf->cin0[wc] : INF;
    const char* nllb = static_cast<const char*>(a.nll) + sl.row0 * a.S * (int64_t)sizeof(ET);
    const int64_t rowb = (int64_t)a.S * (int64_t)sizeof(ET);
    ET ring[PF][N];
#pragma unroll
    for (int k = 0; k < PF; ++k)
#pragma unroll
        for (int s = 0; s < N; ++s)
            ring[k][s] = (k < T) ? *reinterpret_cast<const ET*>(nllb + k * rowb + sto[s]) : ET(0);
    // the carried column; a stream at column 0 (fresh or reset) starts like the one-shot sweep
    double* st = a.prev + ((int64_t)sl.stream * N) * 64 + lane;
    double prev[N];
#pragma unroll
    for (int s = 0; s < N; ++s) prev[s] = tb > 0 ? st[s * 64] : INF;
    // column ta of the stream: word index (ta % ring_cols) * 64 + lane of its history (no wrap: as in a whole utterance)
    uint32_t* bp = reinterpret_cast<uint32_t*>(a.hist + (int64_t)sl.stream * a.hist_stride) + lane;
    const int n_ring = a.ring_words;
    int rp = tb % n_ring;                                     // ring position of the next column (wave-uniform)
    auto column = [&](int t, const ET (&ev)[N]) {
        double e[N];
#pragma unroll
        for (int s = 0; s < N; ++s) e[s] = (double)ev[s];
        uint32_t word = 0;
        const double base0 = c0[0] + prev[0];
#pragma unroll
        for (int s = N - 1; s >= 1; --s) {
            const double v0 = c0[s] + prev[s];
            const double v1 = c1[s] + prev[s - 1];
            double best;
            if (SKIP && s >= 2) {                             // ascending origin order: s-2, s-1, s; strict '<'
                const double v2 = c2[s] + prev[s - 2];
                const bool b_a = v1 < v2;
                const double m = vmin(v1, v2);
                const bool b_b = v0 < m;
                best = vmin(v0, m);
                push_bit(word, __ballot(b_a));
                push_bit(word, __ballot(b_b));
            } else {
                const bool b = v0 < v1;
                best = vmin(v0, v1);
                push_bit(word, __ballot(b));
            }
            prev[s] = vmin(best + e[s], INF);                 // min(inf, nan) keeps inf (decode.py:124)
        }
        // the entry row of this lane's word: min over the words' last states of THIS column plus B's column
        const double x = prev[N - 1];
        double q0 = INF, q1 = INF, q2 = INF, q3 = INF;
        uint32_t i0 = 0, i1 = 16, i2 = 32, i3 = 48;
        // column w of B: s_bg[v 64 + w] = cost of word w after word v.  The lane's offset is made opaque once per column:
        // the image never changes, and the compiler would otherwise keep all of it in registers across the loop
        unsigned wo = (unsigned)w;
        asm volatile("" : "+v"(wo));
        // (the fences keep one group's 16 reads in flight, not all 64, and its compares and selects beside its minima)
#define GH_OBW_FENCE(ix) do { asm volatile("" : "+v"(ix)); __builtin_amdgcn_sched_barrier(0); } while (0)
        entry_group<0>(x, s_bg, wo, q0, i0);
        GH_OBW_FENCE(i0);
        entry_group<16>(x, s_bg, wo, q1, i1);                 // (more than 16 words: always)
        GH_OBW_FENCE(i1);
        if (W > 32) { entry_group<32>(x, s_bg, wo, q2, i2); GH_OBW_FENCE(i2); }   // wave-uniform; a skipped group stays +inf and never wins
        if (W > 48) { entry_group<48>(x, s_bg, wo, q3, i3); GH_OBW_FENCE(i3); }
#undef GH_OBW_FENCE
        GH_OBW_MERGE(q0, i0, q1, i1); GH_OBW_MERGE(q2, i2, q3, i3);
        GH_OBW_MERGE(q0, i0, q2, i2);
        word = (word << 6) | i0;
        // state 0: start row (row 0), entry row, self -- ascending origin, strict '<'; the start row exists in the stream's
        // column 0 only
        const double cs = ((tb + t == 0) ? 0.0 : INF) + cin0;
        const double cl = q0;                                 // (the arc entry row -> state 0 costs 0)
        const bool b_l = cl < cs;
        const double m2 = vmin(cl, cs);
        const bool b_s = base0 < m2;
        push_bit(word, __ballot(b_l));
        push_bit(word, __ballot(b_s));
        prev[0] = vmin(vmin(base0, m2) + e[0], INF);
        bp[(int64_t)rp * 64] = word;
        rp = rp + 1 == n_ring ? 0 : rp + 1;
    };
    int t0 = 0;
    for (; t0 + PF <= T; t0 += PF) {
#pragma unroll
        for (int k = 0; k < PF; ++k) {
            const int t = t0 + k;
            column(t, ring[k]);
            const int tn = (t + PF < T) ? t + PF : T - 1;     // the refill: unconditional, from a clamped column
            const char* colp = nllb + (int64_t)tn * rowb;
#pragma unroll
            for (int s = 0; s < N; ++s) ring[k][s] = *reinterpret_cast<const ET*>(colp + sto[s]);
        }
    }
#pragma unroll
    for (int k = 0; k < PF - 1; ++k)
        if (t0 + k < T) column(t0 + k, ring[k]);
#pragma unroll
    for (int s = 0; s < N; ++s) st[s * 64] = prev[s];
}

}  // namespace

int gh_launch_online_bigram_wide(gh_ctx* ctx, const gh_online* on, const gh_online_args& a, bool f64) {
    if (a.n_slots <= 0) return GH_OK;
    const gh_layerform& f = on->lat->h_layers;
    const gh_bigram_wide* wide = on->lat->d_bigram_wide;
    GH_REQUIRE(wide, "gh_online_push: internal: wide bigram form without its cost table");
    const dim3 grid((unsigned)((a.n_slots + OBW_WAVES - 1) / OBW_WAVES)), blk(64 * OBW_WAVES);
#define GH_OBW(ET, NN, SK) hipLaunchKernelGGL((viterbi_bigram_online_wide_kernel<ET, NN, SK>), grid, blk, 0, ctx->stream, a, wide)
    if (f64) { GH_NSKIP_SWITCH(f.N, f.skip, 8, GH_OBW, double, "gh_online_push: wide bigram form with %d states per word", f.N) }
    else { GH_NSKIP_SWITCH(f.N, f.skip, 8, GH_OBW, float, "gh_online_push: wide bigram form with %d states per word", f.N) }
#undef GH_OBW
    GH_HIP(hipGetLastError());
    return GH_OK;
}
