// ONLINE decode over the BIGRAM form (gh_layerform.loop == 2, up to GH_LAYERS_ROWW words): the sweep of gh_viterbi_bigram.hip
// (viterbi_bigram_kernel, WANT_BP) CARRIED ACROSS CHUNKS, the way gh_viterbi_online.hip carries the loop form.  A bigram
// column reads the previous column and itself only, so a stream is again
//   * the previous column: the N state costs of its 16 word lanes               [stream][N][16] doubles,
//   * the decision word that is still open (pushed bits, right aligned)         [stream][16] uint32,
//   * the number of frames it has taken (host side: the absolute column of the next frame),
// and its decision history, in exactly the layout viterbi_bigram_kernel writes for a whole utterance of the same frames
// (gh_bigram_hb / gh_bigram_cpw, 16 lanes x 4 B per CPW columns, the last open word left aligned), record word index i at
// i % ring_words: in a session with full history the ring is as long as the last word index and nothing ever wraps.  bigram_backtrace_kernel reads nothing but those records, so gh_launch_bigram_backtrace runs UNCHANGED on the
// history (path, label and timed-label mode) and "the result after k frames" is bitwise the whole decode of the first k
// frames.
//
// gfx950 mapping: as viterbi_online_kernel -- FOUR STREAMS PER WAVE, DPP row = stream, lane = word, slot table
// {row0, stream, count, t0}, rows switched off by EXEC when their chunk ends, register ring with the clamped, unconditional
// refill.  The column step is a COPY of viterbi_bigram_kernel's (in-word candidates in ascending origin order with a strict
// '<', row_lane<v>(last) + bc[v] for v ascending, the GH_BG_MERGE tree whose left operand is always the lower word, the
// predecessor nibble, then the two state-0 bits); what differs is where `prev` and `word` come from and go to, and that the
// start-row term uses the absolute column and the record word goes to its ring position (carried beside the column and wrapped
// when a word fills, as in viterbi_online_kernel; a session with a window, gh_online_create_bigram_settle, makes it wrap).
#include "gh_online.h"
#include "gh_viterbi.h"
#include "gh_wave.h"

namespace {

// (a, ia) <- the smaller of (a, ia) and (b, ib); ia < ib always, so a tie keeps the lower word (gh_viterbi_bigram.hip)
#define GH_BG_MERGE(a, ia, b, ib) do { const bool lt_ = (b) < (a); a = vmin(a, b); ia = lt_ ? (ib) : (ia); } while (0)

template <typename ET, int N, bool SKIP>
__global__ __launch_bounds__(64) void viterbi_bigram_online_kernel(gh_online_args a) {
    constexpr int HB = gh_bigram_hb(N, SKIP), CPW = gh_bigram_cpw(N, SKIP);
    constexpr int PF = N > 8 ? 2 : 4;
    static_assert(CPW >= 1, "the decision bits of a column must fit one word");
    const int lane = threadIdx.x, kk = lane >> 4, w = lane & 15;
    const gh_layerform* __restrict__ lf = a.lf;
    const int W = lf->W;
    const int64_t slot = (int64_t)blockIdx.x * 4 + kk;
    const bool has = slot < a.n_slots;
    gh_online_slot sl;
    sl.row0 = 0; sl.stream = 0; sl.count = 0; sl.t0 = 0; sl.pad = 0;
    if (has) sl = a.slots[slot];
    const int T = sl.count, tb = sl.t0;
    const double INF = INFINITY;
    int Tmax = T;
    Tmax = max(Tmax, __shfl_xor(Tmax, 16));
    Tmax = max(Tmax, __shfl_xor(Tmax, 32));
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
    double bc[GH_LAYERS_ROWW];                                  // column w of B: bc[v] = cost of word w after word v
#pragma unroll
    for (int v = 0; v < GH_LAYERS_ROWW; ++v) bc[v] = (wact && v < W) ? lf->bg[v][wc] : INF;
    const char* nllb = static_cast<const char*>(a.nll) + (T > 0 ? sl.row0 : 0) * a.S * (int64_t)sizeof(ET);   // (no frames: frame 0)
    const int64_t rowb = (int64_t)a.S * (int64_t)sizeof(ET);
    ET ring[PF][N];
#pragma unroll
    for (int k = 0; k < PF; ++k)
#pragma unroll
        for (int s = 0; s < N; ++s)
            ring[k][s] = (k < T) ? *reinterpret_cast<const ET*>(nllb + k * rowb + sto[s]) : ET(0);
    // the carried column and the open record word; a stream at column 0 (fresh or reset) starts like the one-shot sweep
    double* st = a.prev + ((int64_t)sl.stream * N) * 16 + w;
    uint32_t* op = a.open + (int64_t)sl.stream * 16 + w;
    const bool carried = T > 0 && tb > 0;
    double prev[N];
#pragma unroll
    for (int s = 0; s < N; ++s) prev[s] = carried ? st[s * 16] : INF;
    uint32_t word = (carried && tb % CPW != 0) ? *op : 0u;
    uint32_t* bp = reinterpret_cast<uint32_t*>(a.hist + (int64_t)sl.stream * a.hist_stride) + w;
    const int n_ring = a.ring_words;
    int wr = (tb / CPW) % n_ring;                               // ring position of the open record word; it moves on as words fill

    for (int t0 = 0; t0 < Tmax; t0 += PF) {
#pragma unroll
        for (int k = 0; k < PF; ++k) {
            const int t = t0 + k;
            double e[N];
#pragma unroll
            for (int s = 0; s < N; ++s) e[s] = (double)ring[k][s];
            if (t < T) {                                       // row-uniform: the rows whose chunk has ended sit out
                const int ta = tb + t;                         // the absolute column
                const double base0 = c0[0] + prev[0];
#pragma unroll
                for (int s = N - 1; s >= 1; --s) {
                    const double v0 = c0[s] + prev[s];
                    const double v1 = c1[s] + prev[s - 1];
                    double best;
                    if (SKIP && s >= 2) {                      // ascending origin order: s-2, s-1, s; strict '<'
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
                    prev[s] = vmin(best + e[s], INF);          // min(inf, nan) keeps inf (decode.py:124)
                }
                // the entry row of this lane's word: min over the words' last states of THIS column plus B's column;
                // a tree whose left operand is always the lower word (first minimum = lowest origin row)
                const double x = prev[N - 1];
                double q0 = row_lane<0>(x) + bc[0], q1 = row_lane<1>(x) + bc[1], q2 = row_lane<2>(x) + bc[2], q3 = row_lane<3>(x) + bc[3];
                double q4 = row_lane<4>(x) + bc[4], q5 = row_lane<5>(x) + bc[5], q6 = row_lane<6>(x) + bc[6], q7 = row_lane<7>(x) + bc[7];
                double q8 = row_lane<8>(x) + bc[8], q9 = row_lane<9>(x) + bc[9], q10 = row_lane<10>(x) + bc[10], q11 = row_lane<11>(x) + bc[11];
                double q12 = row_lane<12>(x) + bc[12], q13 = row_lane<13>(x) + bc[13], q14 = row_lane<14>(x) + bc[14], q15 = row_lane<15>(x) + bc[15];
                uint32_t i0 = 0, i2 = 2, i4 = 4, i6 = 6, i8 = 8, i10 = 10, i12 = 12, i14 = 14;
                GH_BG_MERGE(q0, i0, q1, 1u); GH_BG_MERGE(q2, i2, q3, 3u); GH_BG_MERGE(q4, i4, q5, 5u); GH_BG_MERGE(q6, i6, q7, 7u);
                GH_BG_MERGE(q8, i8, q9, 9u); GH_BG_MERGE(q10, i10, q11, 11u); GH_BG_MERGE(q12, i12, q13, 13u); GH_BG_MERGE(q14, i14, q15, 15u);
                GH_BG_MERGE(q0, i0, q2, i2); GH_BG_MERGE(q4, i4, q6, i6); GH_BG_MERGE(q8, i8, q10, i10); GH_BG_MERGE(q12, i12, q14, i14);
                GH_BG_MERGE(q0, i0, q4, i4); GH_BG_MERGE(q8, i8, q12, i12);
                GH_BG_MERGE(q0, i0, q8, i8);
                word = (word << 4) | i0;
                // state 0: start row (row 0), entry row, self -- ascending origin, strict '<'
                const double cs = ((ta == 0) ? 0.0 : INF) + cin0;
                const double cl = q0;                          // (the arc entry row -> state 0 costs 0)
                const bool b_l = cl < cs;
                const double m2 = vmin(cl, cs);
                const bool b_s = base0 < m2;
                push_bit(word, __ballot(b_l));
                push_bit(word, __ballot(b_s));
                prev[0] = vmin(vmin(base0, m2) + e[0], INF);
                const int ci = ta % CPW;
                if (ci == CPW - 1) {
                    bp[(int64_t)wr * 16] = word;
                    word = 0;
                    wr = wr + 1 == n_ring ? 0 : wr + 1;
                } else if (t == T - 1) {
                    // the chunk ends inside a word: the history shows it left aligned (what the one-shot sweep leaves behind
                    // its last column), the state keeps the pushed bits for the next chunk
                    bp[(int64_t)wr * 16] = word << (HB * (CPW - 1 - ci));
                }
            }
            {   // the slot's refill: unconditional, from a clamped column, outside the divergent region (viterbi_bigram_kernel)
                const int tn = (t + PF < T) ? t + PF : (T > 0 ? T - 1 : 0);
                const char* colp = nllb + (int64_t)tn * rowb;
#pragma unroll
                for (int s = 0; s < N; ++s) ring[k][s] = *reinterpret_cast<const ET*>(colp + sto[s]);
            }
        }
    }
    if (T <= 0) return;                                        // (a stream that sat the tick out keeps its state)
#pragma unroll
    for (int s = 0; s < N; ++s) st[s * 16] = prev[s];
    *op = word;
}

}  // namespace

int gh_launch_online_bigram(gh_ctx* ctx, const gh_online* on, const gh_online_args& a, bool f64) {
    const gh_layerform& f = on->lat->h_layers;
    const dim3 grid((unsigned)((a.n_slots + 3) / 4)), blk(64);
#define GH_ONB(ET, NN, SK) hipLaunchKernelGGL((viterbi_bigram_online_kernel<ET, NN, SK>), grid, blk, 0, ctx->stream, a)
    if (f64) { GH_NSKIP_SWITCH(f.N, f.skip, 16_NO_SKIP16, GH_ONB, double, "gh_online_push: bigram form with %d states per word (skip arcs: %d)", f.N, f.skip) }
    else { GH_NSKIP_SWITCH(f.N, f.skip, 16_NO_SKIP16, GH_ONB, float, "gh_online_push: bigram form with %d states per word (skip arcs: %d)", f.N, f.skip) }
#undef GH_ONB
    GH_HIP(hipGetLastError());
    return GH_OK;
}
