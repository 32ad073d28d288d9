// ONLINE decode over the word-loop grammar (gh_layerform.loop == 1, up to GH_LAYERS_ROWW words): the loop-form sweep of
// gh_viterbi_layers.hip (viterbi_loop_kernel) CARRIED ACROSS CHUNKS of an utterance that is still arriving.  A column of
// decode_hmm_states (decode.py:80-146) depends on the previous column only, so a stream is fully described by
//   * the previous column: the N state costs of its 16 word lanes               [stream][N][16] doubles,
//   * the decision word that is still open (pushed bits, right aligned)         [stream][16] uint32,
//   * the number of frames it has taken (host side: the absolute column of the next frame),
// and its decision history: one region per stream, written at the ABSOLUTE word index in exactly the layout
// viterbi_loop_kernel writes for a whole utterance of the same frames (gh_loop_hb / gh_loop_cpw, 16 lanes x 4 B per CPW
// columns, the last open word left aligned).  The back-trace of the one-shot decode (gh_launch_lattice_backtrace, loop
// form, path and label mode) therefore runs UNCHANGED on the history, and "the result after k frames" is bitwise the
// whole decode of the first k frames: end costs, chosen end, path and labels (main.py:59-67).
//
// gfx950 mapping: as the loop kernel -- FOUR STREAMS PER WAVE, DPP row = stream, lane = word, the N states of the word in
// registers, rows switched off by EXEC when their chunk ends.  The column step is a copy of the loop kernel's (same
// candidate order, same strict '<', same decision bits); what differs is where `prev` and `word` come from and go to,
// and that the start-row term and the decision-word index use the absolute column.  A chunk moves 16 N 8 B of state in
// and out and 64 B of open word per stream beside its emissions and decisions.
//
// The history is addressed as a RING: decision word index i of a stream lives at i % ring_words.  A session created with a
// capacity (gh_online_create) has a ring as long as its last word index, so nothing ever wraps and it writes the bytes it
// always wrote; one created with a window (gh_online_create_window) holds `window` unsettled frames and one word of slack
// for the word the anchor lies in (gh_online_settle.hip: what is settled, and why the frames before it are dead).
#include "gh_online.h"
#include "gh_viterbi.h"
#include "gh_wave.h"

namespace {

__device__ __forceinline__ double row_min16(double v) {
    v = vmin(v, row_rot<0x121>(v));
    v = vmin(v, row_rot<0x122>(v));
    v = vmin(v, row_rot<0x124>(v));
    v = vmin(v, row_rot<0x128>(v));
    return v;
}

template <typename ET, int N, bool SKIP>
__global__ __launch_bounds__(64) void viterbi_online_kernel(gh_online_args a) {
    constexpr int HB = gh_loop_hb(N, SKIP), CPW = gh_loop_cpw(N, SKIP);
    constexpr int PF = N > 8 ? 2 : 4;
    static_assert(CPW >= 1, "decision bits of a column must fit one word");
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
    const double cin = wact ? lf->cin[wc] : INF, cin0 = wact ? lf->cin0[wc] : INF, cout = wact ? lf->cout[wc] : INF;
    const char* nllb = static_cast<const char*>(a.nll) + (T > 0 ? sl.row0 : 0) * a.S * (int64_t)sizeof(ET);   // (no frames: frame 0)
    const int64_t rowb = (int64_t)a.S * (int64_t)sizeof(ET);
    ET ring[PF][N];
#pragma unroll
    for (int k = 0; k < PF; ++k)
#pragma unroll
        for (int s = 0; s < N; ++s)
            ring[k][s] = (k < T) ? *reinterpret_cast<const ET*>(nllb + k * rowb + sto[s]) : ET(0);
    // the carried column and the open decision word; a stream at column 0 (fresh or reset) starts like the one-shot sweep
    double* st = a.prev + ((int64_t)sl.stream * N) * 16 + w;
    uint32_t* op = a.open + (int64_t)sl.stream * 16 + w;
    const bool carried = T > 0 && tb > 0;
    double prev[N];
#pragma unroll
    for (int s = 0; s < N; ++s) prev[s] = carried ? st[s * 16] : INF;
    uint32_t word = (carried && tb % CPW != 0) ? *op : 0u;
    uint32_t* bp = reinterpret_cast<uint32_t*>(a.hist + (int64_t)sl.stream * a.hist_stride) + w;
    const int n_ring = a.ring_words;
    int wr = (tb / CPW) % n_ring;                               // ring position of the open word; it moves on as words fill

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
                const double cand = prev[N - 1] + cout;
                const double rm = row_min16(cand);
                push_bit(word, __ballot(cand == rm));
                const double cs = ((ta == 0) ? 0.0 : INF) + cin0;
                const double cl = rm + cin;
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
            {   // the slot's refill: unconditional, from a clamped column, outside the divergent region (viterbi_loop_kernel)
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

int gh_launch_online_loop(gh_ctx* ctx, const gh_online* on, const gh_online_args& a, bool f64) {
    const gh_layerform& f = on->lat->h_layers;
    const dim3 grid((unsigned)((a.n_slots + 3) / 4)), blk(64);
#define GH_ON(ET, NN, SK) hipLaunchKernelGGL((viterbi_online_kernel<ET, NN, SK>), grid, blk, 0, ctx->stream, a)
    if (f64) { GH_NSKIP_SWITCH(f.N, f.skip, 16, GH_ON, double, "gh_online_push: loop form with %d states per word", f.N) }
    else { GH_NSKIP_SWITCH(f.N, f.skip, 16, GH_ON, float, "gh_online_push: loop form with %d states per word", f.N) }
#undef GH_ON
    GH_HIP(hipGetLastError());
    return GH_OK;
}
