// ONLINE decode over the WIDE word-loop grammar (gh_layerform.loop == 1 with 17 .. 64 words): the wide loop sweep of
// gh_viterbi_layers_wide.hip (viterbi_loop_wide_kernel) CARRIED ACROSS CHUNKS of an utterance that is still arriving, as
// gh_viterbi_online.hip carries the narrow one.  A stream is fully described by
//   * the previous column: the N state costs of its 64 word lanes                [stream][N][64] doubles (512 N B),
//   * the number of frames it has taken (host side: the absolute column of the next frame),
// and its decision history: the wide kernel writes ONE COMPLETE 32-bit decision word per column and lane, [column][64 lanes],
// so the word of absolute column ta goes to hist[stream][ta % ring_cols][lane] -- 256 B per frame.  A session that keeps its
// full history passes a ring it never fills (ring_cols >= max_frames), and column ta then lies exactly where
// viterbi_loop_wide_kernel puts column ta of a whole utterance.  There is no open word to carry and a chunk never ends
// inside one.  The back-trace of the one-shot decode (gh_launch_lattice_backtrace hands a graph of more than GH_LAYERS_ROWW
// words to loop_backtrace_wide_kernel: path, labels, timed labels) therefore runs UNCHANGED on a full history, and "the
// result after k frames" is bitwise the whole decode of the first k frames.
//
// gfx950 mapping: as the wide loop kernel -- ONE STREAM PER WAVE, lane = word, the N states of the word in registers, no LDS,
// no barrier.  A stream owns its wave, so EXEC stays full and wave_min's v_readlane steps see every lane.  The column step is
// a copy of the one-shot kernel's (same candidate order, same strict '<', same wave_min, same decision bits in the same
// order); what differs is where `prev` comes from and goes to, and that the start-row term and the history address use the
// absolute column.  A chunk of t frames moves 512 N B of state in and out and t 256 B of decisions beside its emissions.
//
// THE RING.  A stream owns its wave, so the column, its ring position and the wrap are wave-uniform: the position starts from
// t0 % ring_cols once per launch and moves on by compare-and-subtract, no division per column and no lane arithmetic
// beyond the one-shot kernel's.  A session with a window (gh_online_create_wide_settle, window != 0) holds `window`
// unsettled frames and the column the anchor lies in; gh_online_wide_settle.hip has the settle walk over 64 word lanes
// that moves the anchor on.  A session from gh_online_create_wide keeps its full history and does not settle:
// gh_online_commit* / gh_online_tail* refuse it.  NOT OFFERED: a forced commit (a stream whose traces do not meet within
// the window can only be finished), the bigram grammar, and words of 12 or 16 states, beyond 16 words.
#include "gh_online.h"
#include "gh_viterbi.h"
#include "gh_wave.h"

namespace {

// minimum over the 64 lanes, left in every lane (viterbi_loop_wide_kernel's: row_ror:1,2,4,8 inside the 16-lane rows, across
// them through the scalar unit)
__device__ __forceinline__ double wave_min(double v) {
    v = vmin(v, row_rot<0x121>(v));
    v = vmin(v, row_rot<0x122>(v));
    v = vmin(v, row_rot<0x124>(v));
    v = vmin(v, row_rot<0x128>(v));
    auto at = [&](int l) { return __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(v), l), __builtin_amdgcn_readlane(__double2loint(v), l)); };
    return vmin(vmin(at(0), at(16)), vmin(at(32), at(48)));
}

template <typename ET, int N, bool SKIP>
__global__ __launch_bounds__(64) void viterbi_online_wide_kernel(gh_online_args a) {
    constexpr int PF = 4;
    const int lane = threadIdx.x, w = lane;
    const gh_layerform* __restrict__ lf = a.lf;
    const int W = lf->W;
    const gh_online_slot sl = a.slots[blockIdx.x];           // (grid = n_slots: wave-uniform)
    const int T = sl.count, tb = sl.t0;
    if (T <= 0) return;                                      // (gh_online_push drops such a slot on the host)
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
    const double cin = wact ? lf->cin[wc] : INF, cin0 = wact ? lf->cin0[wc] : INF, cout = wact ? lf->cout[wc] : INF;
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
    int rp = tb % n_ring;                                      // ring position of the next column (wave-uniform)
    __builtin_amdgcn_s_waitcnt(0x0F70);                        // (the ring's first fill drained: see viterbi_layers_kernel)
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
            if (SKIP && s >= 2) {
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
            prev[s] = vmin(best + e[s], INF);
        }
        // the loop row: minimum over the words' last states of THIS column
        const double cand = prev[N - 1] + cout;
        const double rm = wave_min(cand);
        push_bit(word, __ballot(cand == rm));
        // state 0: start row (row 0), loop row, self -- ascending origin, strict '<'; the start row exists in the stream's
        // column 0 only
        const double cs = ((tb + t == 0) ? 0.0 : INF) + cin0;
        const double cl = rm + cin;
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

int gh_launch_online_wide(gh_ctx* ctx, const gh_online* on, const gh_online_args& a, bool f64) {
    if (a.n_slots <= 0) return GH_OK;
    const gh_layerform& f = on->lat->h_layers;
    const dim3 grid((unsigned)a.n_slots), blk(64);
#define GH_ONW(ET, NN, SK) hipLaunchKernelGGL((viterbi_online_wide_kernel<ET, NN, SK>), grid, blk, 0, ctx->stream, a)
    if (f64) { GH_NSKIP_SWITCH(f.N, f.skip, 8, GH_ONW, double, "gh_online_push: wide loop form with %d states per word", f.N) }
    else { GH_NSKIP_SWITCH(f.N, f.skip, 8, GH_ONW, float, "gh_online_push: wide loop form with %d states per word", f.N) }
#undef GH_ONW
    GH_HIP(hipGetLastError());
    return GH_OK;
}
