// ONLINE decode over the K-layer word lattice (gh_layerform.loop == 0, up to GH_LAYERS_ROWW words per layer, up to 8 layers, words
// of 2 to 8 states): the layer-form sweep of gh_viterbi_layers.hip (viterbi_layers_kernel<ET, N, SKIP, true, 2>) CARRIED ACROSS
// CHUNKS of an utterance that is still arriving, as gh_viterbi_online.hip carries the loop sweep.  A column of decode_hmm_states
// (decode.py:80-146) depends on the previous column only, so a stream is fully described by
//   * the previous column: the N state costs of its 64 lanes in both register sets     [stream][2][N][64] doubles,
//   * the decision word that is still open (pushed bits, right aligned)                [stream][64] uint32,
//   * the number of frames it has taken (host side: the absolute column of the next frame),
// and its decision history: one region per stream, written at the ABSOLUTE word index in exactly the layout
// viterbi_layers_kernel writes for a whole utterance of the same frames (gh_layer_hb / gh_layer_cpw with two sets, 64 lanes x 4 B
// per CPW columns, the last open word left aligned).  The back-trace of the one-shot decode (gh_launch_lattice_backtrace, layer
// form, path and label mode) therefore runs UNCHANGED on the history, and "the result after k frames" is bitwise the whole
// layer-form decode of the first k frames: end costs, chosen end, path and labels (main.py:59-67).
//
// gfx950 mapping: as the layer kernel -- ONE WAVE PER STREAM, lane = (layer mod 4, word), two register sets (layers 0-3 and
// 4-7), the N states of a word in registers, no LDS, no barrier.  The column step is a copy of the layer kernel's (same candidate
// order, same strict '<', row_min16, row_bcast:15 and the v_readlane of lane 63 from layer 3 into layer 4, same decision bits);
// what differs is where `prev` and `word` come from and go to, and that the start-row term and the decision-word index use the
// absolute column.  A wave holds ONE stream, so everything that steers the column loop is wave-uniform and the DPP row
// operations and the readlane always run under the full EXEC mask.  The state is stored for all 64 lanes of both sets, live or
// not: dead lanes hold +inf, as they do in the one-shot sweep's registers.
//
// The history is addressed through gh_online_args::ring_words like the other sweeps'; a layer session keeps its full history
// (gh_online_create_layers), so ring_words is the last word index + 1 and nothing wraps.
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
__global__ __launch_bounds__(64) void viterbi_layers_online_kernel(gh_online_args a) {
    constexpr int H = 2;                                      // register sets: layers 0-3 and 4-7
    constexpr int BITS = H * gh_layer_hb(N, SKIP), CPW = gh_layer_cpw(N, SKIP, H);
    constexpr int PF = 4;                                     // columns of emissions in flight
    static_assert(gh_layer_word_bits(N, SKIP, H) == 32 && CPW >= 1, "the decision bits of a column must fit one 32-bit word");
    const int lane = threadIdx.x, kk = lane >> 4, w = lane & 15;
    const gh_layerform* __restrict__ lf = a.lf;
    const int K = lf->K, W = lf->W;
    const gh_online_slot sl = a.slots[blockIdx.x];            // grid = n_slots: wave-uniform
    const int T = sl.count, tb = sl.t0;
    if (T <= 0) return;                                       // (gh_online_push lists no stream that sits the tick out)
    const double INF = INFINITY;
    const bool wact = w < W;
    const int wc = wact ? w : 0;
    double c0[N], c1[N], c2[N];
    unsigned sto[N];                                          // byte offset of the state's emission inside a matrix row
#pragma unroll
    for (int s = 0; s < N; ++s) {
        c0[s] = wact ? lf->c0[wc][s] : INF;
        c1[s] = wact ? lf->c1[wc][s] : INF;
        c2[s] = (SKIP && wact) ? lf->c2[wc][s] : INF;
        sto[s] = (unsigned)lf->state[wc][s] * (unsigned)sizeof(ET);
    }
    double cin[H], cout[H];
#pragma unroll
    for (int h = 0; h < H; ++h) {
        const bool act = wact && (4 * h + kk) < K;            // unused layer slots / word lanes: everything stays +inf
        cin[h] = act ? lf->cin[wc] : INF;
        cout[h] = act ? lf->cout[wc] : INF;
    }
    const char* nllb = static_cast<const char*>(a.nll) + sl.row0 * a.S * (int64_t)sizeof(ET);   // wave-uniform
    const int64_t rowb = (int64_t)a.S * (int64_t)sizeof(ET);
    ET ring[PF][N];
#pragma unroll
    for (int k = 0; k < PF; ++k)
#pragma unroll
        for (int s = 0; s < N; ++s)
            ring[k][s] = (k < T) ? *reinterpret_cast<const ET*>(nllb + k * rowb + sto[s]) : ET(0);
    // the carried column and the open decision word; a stream at column 0 (fresh or reset) starts like the one-shot sweep
    double* st = a.prev + (int64_t)sl.stream * (H * N * 64) + lane;
    uint32_t* op = a.open + (int64_t)sl.stream * 64 + lane;
    const bool carried = tb > 0;
    double prev[H][N];
#pragma unroll
    for (int h = 0; h < H; ++h)
#pragma unroll
        for (int s = 0; s < N; ++s) prev[h][s] = carried ? st[(h * N + s) * 64] : INF;
    int cw = tb % CPW;                                        // columns already pushed into `word`
    uint32_t word = (carried && cw != 0) ? *op : 0u;
    uint32_t* bp = reinterpret_cast<uint32_t*>(a.hist + (int64_t)sl.stream * a.hist_stride) + lane;
    const int n_ring = a.ring_words;
    int wr = (tb / CPW) % n_ring;                             // position of the open word; it moves on as words fill

    // (the first fill and the state drained here, the refills below unconditional and clamped: see viterbi_layers_kernel)
    __builtin_amdgcn_s_waitcnt(0x0F70);
    auto column = [&](int t, const ET (&ev)[N]) {
        double e[N];
#pragma unroll
        for (int s = 0; s < N; ++s) e[s] = (double)ev[s];
        double carry = (tb + t == 0) ? 0.0 : INF;         // the start row: cost 0 in ABSOLUTE column 0 only (decode.py:99-101)
#pragma unroll
        for (int h = 0; h < H; ++h) {
            const double base0 = c0[0] + prev[h][0];      // state 0 from its own previous column
            // states N-1 .. 1 from the previous column (in place, descending: the neighbours are still old)
#pragma unroll
            for (int s = N - 1; s >= 1; --s) {
                const double v0 = c0[s] + prev[h][s];
                const double v1 = c1[s] + prev[h][s - 1];
                double best;
                if (SKIP && s >= 2) {                     // ascending origin order: s-2, s-1, s; strict '<'
                    const double v2 = c2[s] + prev[h][s - 2];
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
                prev[h][s] = vmin(best + e[s], INF);      // min(inf, nan) keeps inf (decode.py:124)
            }
            // the non-emitting row behind this layer: minimum over the words' last states, same column
            const double cand = prev[h][N - 1] + cout[h];
            const double rm = row_min16(cand);
            push_bit(word, __ballot(cand == rm));
            // ... handed to the next layer: rows 1-3 take the row above, row 0 the start row / layer 3
            const double nin = dpp_upd<0x142, 0xE>(carry, rm);
            carry = __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(rm), 63),
                                     __builtin_amdgcn_readlane(__double2loint(rm), 63));
            // state 0: the non-emitting row (lower row index: it wins ties) against the self arc
            const double cn = nin + cin[h];
            const bool b0 = base0 < cn;
            push_bit(word, __ballot(b0));
            prev[h][0] = vmin(vmin(base0, cn) + e[0], INF);
        }
        // (cw, t and T are wave-uniform: scalar branches, the EXEC mask stays full)
        if (++cw == CPW) {
            bp[(int64_t)wr * 64] = word;
            word = 0;
            cw = 0;
            wr = wr + 1 == n_ring ? 0 : wr + 1;
        } else if (t == T - 1) {
            // the chunk ends inside a word: the history shows it left aligned (what the one-shot sweep leaves behind its last
            // column), the state keeps the pushed bits for the next chunk
            bp[(int64_t)wr * 64] = word << (BITS * (CPW - cw));
        }
    };
    int t0 = 0;
    for (; t0 + PF <= T; t0 += PF) {
#pragma unroll
        for (int k = 0; k < PF; ++k) {
            const int t = t0 + k;
            column(t, ring[k]);
            const int tn = (t + PF < T) ? t + PF : T - 1;
            const char* colp = nllb + (int64_t)tn * rowb;
#pragma unroll
            for (int s = 0; s < N; ++s) ring[k][s] = *reinterpret_cast<const ET*>(colp + sto[s]);
        }
    }
#pragma unroll
    for (int k = 0; k < PF - 1; ++k)
        if (t0 + k < T) column(t0 + k, ring[k]);

#pragma unroll
    for (int h = 0; h < H; ++h)
#pragma unroll
        for (int s = 0; s < N; ++s) st[(h * N + s) * 64] = prev[h][s];
    *op = word;
}

}  // namespace

int gh_launch_online_layers(gh_ctx* ctx, const gh_online* on, const gh_online_args& a, bool f64) {
    const gh_layerform& f = on->lat->h_layers;
    const dim3 grid((unsigned)a.n_slots), blk(64);
#define GH_ON(ET, NN, SK) hipLaunchKernelGGL((viterbi_layers_online_kernel<ET, NN, SK>), grid, blk, 0, ctx->stream, a)
    if (f64) { GH_NSKIP_SWITCH(f.N, f.skip, 8, GH_ON, double, "gh_online_push: layer form with %d states per word", f.N) }
    else { GH_NSKIP_SWITCH(f.N, f.skip, 8, GH_ON, float, "gh_online_push: layer form with %d states per word", f.N) }
#undef GH_ON
    GH_HIP(hipGetLastError());
    return GH_OK;
}
