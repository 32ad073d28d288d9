// Viterbi over the WIDE BIGRAM form (gh_lattices::bigram_wide_ok, gh_internal.h): the bigram grammar of
// continuous_speech.build_bigram_grammar with 17 .. 64 words of 2 .. 8 states.  Same semantics as every other lattice kernel
// (decode_hmm_states, decode.py:80-146), as viterbi_bigram_kernel (gh_viterbi_bigram.hip) states them: candidates in
// ascending origin order with a strict '<', arcs that touch a non-emitting row read the SAME column, start only in cell
// (0, 0), vmin(x, INF) behind the emission, last of equal end points, path without the end cell; T == 1 is the router's.
//
// gfx950 mapping -- the organisation of viterbi_loop_wide_kernel (gh_viterbi_layers_wide.hip) with the column step of the
// narrow bigram kernel: ONE UTTERANCE PER WAVE, lane = word, the N state costs of the word, its arc costs and a four-deep
// ring of emissions in registers, refills unconditional from a clamped column.  Lanes behind the last word hold +inf, read
// word 0's tables and store nothing.  The step between the words' last states and their first states is
//     entry[w] = min_v ( last[v] + B[v][w] ),   v = 0 .. 63
//   * last[v] is wave-uniform for a given v: v_readlane with a constant lane, two 32-bit halves -- it is the scalar operand
//     of the v_add_f64;
//   * column w of B comes from LDS: an image [v][w] of 64 x 64 doubles (32 KB, +inf where there is no arc or no word),
//     SHARED BY THE FOUR WAVES OF A BLOCK (four utterances), filled once, one __syncthreads() in front of the column loop
//     and none inside.  Lane w reads 8 bytes at v 512 + w 8: consecutive lanes, consecutive banks.  (128 registers per
//     lane would hold the column too; the loop is bound by the vector unit, not by LDS, and the registers cost waves);
//   * v runs in ascending order inside four groups of 16, each keeping (best, arg) under a strict '<'; the groups are
//     merged with the lower group as the left operand: the reference's first minimum, no (value, index) pair compare.
//     A group that lies behind the last word is skipped (wave-uniform): 17 words pay for 32 candidates, not 64;
//   * when every candidate is +inf no '<' ever holds and the record says v = 0; the back-trace, which has the 64-bit arc
//     masks (gh_bigram_wide::bg_in), replaces a recorded v without arc by the lowest v with one.
// Decision record: one 32-bit word per column and lane at bp[t 64 + lane] (the wide loop form's layout) -- the in-word bits,
// 6 bits of predecessor word, the two bits of state 0: gh_bigram_wide_hb(N, skip) <= 32 bits.
// No scratch and no runtime-indexed private array for any instantiation (kernel-resource-usage remarks:
// profiles/bigram_wide_kernel_resources.txt).
#include "gh_internal.h"
#include "gh_viterbi.h"
#include "gh_wave.h"

namespace {

constexpr int BW_WAVES = 4;                // utterances (waves) per block: they share the LDS image of B

// (a, ia) <- the smaller of (a, ia) and (b, ib); ia < ib always, so a tie keeps the lower word
#define GH_BGW_MERGE(a, ia, b, ib) do { const bool lt_ = (b) < (a); a = vmin(a, b); ia = lt_ ? (ib) : (ia); } while (0)

// the value of lane L (a constant) as a wave-uniform double
template <int L> __device__ __forceinline__ double lane_value(double x) {
    return __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(x), L), __builtin_amdgcn_readlane(__double2loint(x), L));
}

// candidates v = V0 .. V0 + 15 in ascending order: (best, arg) <- first minimum of last[v] + B[v][w]
template <int V0, int I = 0> __device__ __forceinline__ void entry_group(double x, const double* s_bg, unsigned w, double& best, uint32_t& arg) {
    if constexpr (I < 16) {
        const double q = lane_value<V0 + I>(x) + s_bg[(V0 + I) * GH_LAYERS_MAXW + w];
        GH_BGW_MERGE(best, arg, q, (uint32_t)(V0 + I));
        entry_group<V0, I + 1>(x, s_bg, w, best, arg);
    }
}

template <typename ET, int N, bool SKIP, bool WANT_BP>
__global__ __launch_bounds__(64 * BW_WAVES) void viterbi_bigram_wide_kernel(gh_layers_args a, const gh_bigram_wide* __restrict__ bgw, int64_t slot_end) {
    constexpr int PF = 4;
    static_assert(gh_bigram_wide_hb(N, SKIP) <= 32, "the decision bits of a column must fit one word");
    __shared__ double s_bg[GH_LAYERS_MAXW * GH_LAYERS_MAXW];
    for (int i = threadIdx.x; i < GH_LAYERS_MAXW * GH_LAYERS_MAXW; i += 64 * BW_WAVES) s_bg[i] = (&bgw->bg[0][0])[i];
    __syncthreads();
    const int lane = threadIdx.x & 63, w = lane;
    const int64_t slot = a.slot0 + (int64_t)blockIdx.x * BW_WAVES + (threadIdx.x >> 6);
    if (slot >= slot_end) return;                             // (wave-uniform; no barrier behind this line)
    const gh_layerform* __restrict__ lf = a.lf;
    const int W = lf->W, Lr = lf->loop_row;
    const int64_t u = a.perm ? a.perm[slot] : slot;
    const int64_t f0 = a.utt_off[u];
    const int T = (int)(a.utt_off[u + 1] - f0);
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
    const char* nllb = static_cast<const char*>(a.nll) + (T > 0 ? f0 : 0) * a.S * (int64_t)sizeof(ET);
    const int64_t rowb = (int64_t)a.S * (int64_t)sizeof(ET);
    ET ring[PF][N];
#pragma unroll
    for (int k = 0; k < PF; ++k)
#pragma unroll
        for (int s = 0; s < N; ++s)
            ring[k][s] = (k < T) ? *reinterpret_cast<const ET*>(nllb + k * rowb + sto[s]) : ET(0);
    double prev[N];
#pragma unroll
    for (int s = 0; s < N; ++s) prev[s] = INF;
    uint32_t* bp = WANT_BP ? reinterpret_cast<uint32_t*>(a.bp + a.bp_off[slot]) + lane : nullptr;
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
                if (WANT_BP) { push_bit(word, __ballot(b_a)); push_bit(word, __ballot(b_b)); }
            } else {
                const bool b = v0 < v1;
                best = vmin(v0, v1);
                if (WANT_BP) push_bit(word, __ballot(b));
            }
            prev[s] = vmin(best + e[s], INF);                 // min(inf, nan) keeps inf (decode.py:124)
        }
        // the entry row of this lane's word: min over the words' last states of THIS column plus B's column
        const double x = prev[N - 1];
        double q0 = INF, q1 = INF, q2 = INF, q3 = INF;
        uint32_t i0 = 0, i1 = 16, i2 = 32, i3 = 48;
        // column w of B: s_bg[v 64 + w] = cost of word w after word v.  The lane's offset is made opaque once per column:
        // the image never changes, and the compiler would otherwise keep all of it in registers across the loop (128 per
        // lane, down to one wave per SIMD)
        unsigned wo = (unsigned)w;
        asm volatile("" : "+v"(wo));
        // (the fences keep one group's 16 reads in flight, not all 64, and its compares and selects beside its minima: left
        //  alone, the compiler sinks them behind the last group and keeps every intermediate minimum alive until then)
#define GH_BGW_FENCE(ix) do { if (WANT_BP) asm volatile("" : "+v"(ix)); __builtin_amdgcn_sched_barrier(0); } while (0)
        entry_group<0>(x, s_bg, wo, q0, i0);
        GH_BGW_FENCE(i0);
        entry_group<16>(x, s_bg, wo, q1, i1);                 // (more than 16 words: always)
        GH_BGW_FENCE(i1);
        if (W > 32) { entry_group<32>(x, s_bg, wo, q2, i2); GH_BGW_FENCE(i2); }   // wave-uniform; a skipped group stays +inf and never wins
        if (W > 48) { entry_group<48>(x, s_bg, wo, q3, i3); GH_BGW_FENCE(i3); }
#undef GH_BGW_FENCE
        GH_BGW_MERGE(q0, i0, q1, i1); GH_BGW_MERGE(q2, i2, q3, i3);
        GH_BGW_MERGE(q0, i0, q2, i2);
        if (WANT_BP) word = (word << 6) | i0;
        // state 0: start row (row 0), entry row, self -- ascending origin, strict '<'
        const double cs = ((t == 0) ? 0.0 : INF) + cin0;
        const double cl = q0;                                 // (the arc entry row -> state 0 costs 0)
        const bool b_l = cl < cs;
        const double m2 = vmin(cl, cs);
        const bool b_s = base0 < m2;
        if (WANT_BP) { push_bit(word, __ballot(b_l)); push_bit(word, __ballot(b_s)); }
        prev[0] = vmin(vmin(base0, m2) + e[0], INF);
        if (WANT_BP) bp[(int64_t)t * 64] = word;
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
    // ---- end costs + end selection ('>=': the last of equal minima) ----
    double best_v = INF;
    int best_slot = -1;
#pragma unroll
    for (int s = 0; s < N; ++s) {
        if (wact) {
            const int r = s == 0 ? Lr + W + w : 1 + w * (N - 1) + (s - 1);
            const int es = a.end_slot[r];
            if (es >= 0) {
                const double v = T > 0 ? prev[s] : INF;
                if (a.end_cost) a.end_cost[u * a.n_end + es] = v;
                if (v < best_v || (v == best_v && es > best_slot)) { best_v = v; best_slot = es; }
            }
        }
    }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
        const double ov = __shfl_xor(best_v, o);
        const int os = __shfl_xor(best_slot, o);
        if (ov < best_v || (ov == best_v && os > best_slot)) { best_v = ov; best_slot = os; }
    }
    if (lane == 0 && a.best_end) a.best_end[u] = T > 0 ? best_slot : -1;
}

// ---------------------------------------------------------------------------------------------------------------------
// Back-trace (decode.py:143-145), ONE LANE PER UTTERANCE like bigram_backtrace_kernel: the decision word of (column j, word
// bw) is bpu[j 64 + bw]; an entry row's predecessor is the 6-bit field of the SAME record, no scan of the column.  MODE 0:
// the (row, column) path as decode_hmm_states returns it, entry rows included; MODE 1: only the label sequence
// (gh_viterbi_labels), collected from the back of the utterance's slot and moved to its front at the end; MODE 2: the labels
// and, in a.path, the column of the first cell of every word's run (gh_viterbi_labels_timed).
template <int N, bool SKIP, int MODE>
__global__ __launch_bounds__(64) void bigram_backtrace_wide_kernel(gh_layers_args a, const gh_bigram_wide* __restrict__ bgw, int64_t slot_end) {
    constexpr int HB = gh_bigram_wide_hb(N, SKIP);
    __shared__ uint8_t s_arcs[GH_LAYERS_MAXW * GH_LAYERS_MAXN];
    __shared__ uint64_t s_in[GH_LAYERS_MAXW];
    const gh_layerform* __restrict__ lf = a.lf;
    for (int i = threadIdx.x; i < GH_LAYERS_MAXW * GH_LAYERS_MAXN; i += 64) s_arcs[i] = (&lf->arcs[0][0])[i];
    s_in[threadIdx.x] = bgw->bg_in[threadIdx.x];              // (64 lanes, GH_LAYERS_MAXW = 64 masks)
    static_assert(GH_LAYERS_MAXW == 64, "one arc mask per lane");
    __syncthreads();
    const int W = lf->W, Lr = lf->loop_row;
    const int64_t slot = a.slot0 + (int64_t)blockIdx.x * 64 + threadIdx.x;
    if (slot >= slot_end) return;
    const int64_t u = a.perm ? a.perm[slot] : slot;
    const int T = (int)(a.utt_off[u + 1] - a.utt_off[u]);
    const int be = a.best_end[u];
    int32_t* out_n = MODE == 0 ? a.path_len : a.n_labels;
    if (T <= 1 || be < 0) { out_n[u] = 0; return; }
    auto row_of = [&](int ww, int ss) { return ss == 0 ? Lr + W + ww : 1 + ww * (N - 1) + (ss - 1); };
    int bw, bs;
    {
        const int r = a.end_rows[be];
        if (r >= Lr + W) { bw = r - Lr - W; bs = 0; } else { bw = (r - 1) / (N - 1); bs = (r - 1) % (N - 1) + 1; }
    }
    const uint32_t* bpu = reinterpret_cast<const uint32_t*>(a.bp + a.bp_off[slot]);
    int32_t* path = MODE == 0 ? a.path + 2 * a.path_off[u] : nullptr;
    int32_t* labs = MODE >= 1 ? a.labels + a.label_off[u] : nullptr;
    int32_t* begs = MODE == 2 ? a.path + a.label_off[u] : nullptr;     // MODE 2: begin column of every label (a.path: see gh_layers_args)
    int prev_col = 0;                                         // MODE 2: column of the cell visited last
    const int64_t cap = MODE == 0 ? a.path_off[u + 1] - a.path_off[u] : a.label_off[u + 1] - a.label_off[u];
    int64_t len = 0;
    int prev_label = -1;                                      // MODE 1: label of the cell visited last
    int j = T - 1, kind = 0;                                  // kind 0: emitting (bw, bs); 1: entry row of word bw; 2: start row
    int flag = 0;
    auto visit = [&](int row, int col) {
        if (MODE == 0) {
            if (len >= cap) { flag |= 4; return; }
            reinterpret_cast<int2*>(path)[len] = make_int2(row, col);
            ++len;
        } else {
            const int l = a.row_label[row];
            if (prev_label >= 0 && l < 0) {
                if (len >= cap) { flag |= 8; return; }
                labs[cap - 1 - len] = prev_label;
                if (MODE == 2) begs[cap - 1 - len] = prev_col;
                ++len;
            }
            prev_label = l;
            if (MODE == 2) prev_col = col;
        }
    };
    while (j != 0 && !flag) {
        if (kind == 2) { flag |= 2; break; }                  // the start row, reached in a column > 0
        const uint32_t hb = bpu[(int64_t)j * 64 + bw] & (uint32_t)((1ull << HB) - 1ull);
        if (kind == 1) {                                      // entry row of word bw: the recorded predecessor word
            int v = (int)((hb >> 2) & 63u);
            const uint64_t in = s_in[bw];
            if (!((in >> v) & 1ull)) v = in ? __ffsll((unsigned long long)in) - 1 : -1;   // every candidate was +inf: the first existing arc
            if (v < 0 || v >= W) { flag |= 2; break; }
            bw = v;
            bs = N - 1;
            kind = 0;
            visit(row_of(bw, bs), j);
            continue;
        }
        const int arcs = s_arcs[bw * GH_LAYERS_MAXN + bs];
        if (bs >= 1) {
            int before = 0;
            for (int s2 = N - 1; s2 > bs; --s2) before += (SKIP && s2 >= 2) ? 2 : 1;
            int code;
            if (SKIP && bs >= 2) {
                const int b_a = (hb >> (HB - 1 - before)) & 1, b_b = (hb >> (HB - 2 - before)) & 1;
                code = b_b ? 0 : (b_a ? 1 : 2);
            } else {
                code = ((hb >> (HB - 1 - before)) & 1) ? 0 : 1;
            }
            // every candidate was +inf: the first existing arc (lowest origin) -- or none at all
            if (!((arcs >> code) & 1)) code = (arcs & 4) ? 2 : (arcs & 2) ? 1 : (arcs & 1) ? 0 : -1;
            if (code < 0) { flag |= 2; break; }
            bs -= code;
            --j;
            visit(row_of(bw, bs), j);
        } else {
            // candidates in ascending origin order: start row (arcs bit4), entry row (bit3), self (bit0)
            const int b_l = (hb >> 1) & 1, b_s = hb & 1;
            int pick = b_s ? 0 : (b_l ? 3 : 4);
            if (!((arcs >> pick) & 1)) pick = (arcs & 16) ? 4 : (arcs & 8) ? 3 : (arcs & 1) ? 0 : -1;
            if (pick < 0) { flag |= 2; break; }
            if (pick == 0) { --j; visit(row_of(bw, 0), j); }
            else if (pick == 3) { kind = 1; visit(Lr + bw, j); }
            else { kind = 2; visit(0, j); }
        }
    }
    if (flag) atomicOr(a.flag, flag);
    if (MODE >= 1) {
        if (!flag && prev_label >= 0) {
            if (len >= cap) atomicOr(a.flag, 8);
            else {
                labs[cap - 1 - len] = prev_label;
                if (MODE == 2) begs[cap - 1 - len] = prev_col;
                ++len;
            }
        }
        for (int64_t i = 0; i < len; ++i) labs[i] = labs[cap - len + i];       // to the front, start -> end order
        if (MODE == 2)
            for (int64_t i = 0; i < len; ++i) begs[i] = begs[cap - len + i];
    }
    out_n[u] = (int32_t)len;
}

}  // namespace

// decision words of one utterance of T frames in uint16 units: one 32-bit word per column and lane
size_t gh_bigram_wide_bp_entries(int64_t T) { return gh_bp_entries(T, 1, 64, 32); }

#define GH_BGW_CASES(ET, MACRO) \
    GH_NSKIP_SWITCH(f.N, f.skip, 8, MACRO, ET, "gh_viterbi: wide bigram form with %d states per word", f.N)

int gh_launch_viterbi_bigram_wide(gh_ctx* ctx, const gh_layers_args& a, const gh_layerform& f, const gh_bigram_wide* wide,
                                  int64_t u_begin, int64_t n_utts, bool f64, bool want_path) {
    if (n_utts <= 0) return GH_OK;
    GH_REQUIRE(wide, "gh_viterbi: internal: wide bigram form without its cost table");
    gh_layers_args b = a;
    b.slot0 = u_begin;
    const dim3 grid((unsigned)((n_utts + BW_WAVES - 1) / BW_WAVES)), blk(64 * BW_WAVES);
    const int64_t slot_end = u_begin + n_utts;
#define GH_BGW(ET, NN, SK)                                                                                                         \
    do {                                                                                                                           \
        if (want_path) hipLaunchKernelGGL((viterbi_bigram_wide_kernel<ET, NN, SK, true>), grid, blk, 0, ctx->stream, b, wide, slot_end);  \
        else hipLaunchKernelGGL((viterbi_bigram_wide_kernel<ET, NN, SK, false>), grid, blk, 0, ctx->stream, b, wide, slot_end);           \
    } while (0)
    if (f64) { GH_BGW_CASES(double, GH_BGW) } else { GH_BGW_CASES(float, GH_BGW) }
#undef GH_BGW
    GH_HIP(hipGetLastError());
    return GH_OK;
}

// the path (a.path) or the label sequences (a.labels) of the utterances [u_begin, u_begin + n_utts) from the decision words
int gh_launch_bigram_backtrace_wide(gh_ctx* ctx, const gh_layers_args& a, const gh_layerform& f, const gh_bigram_wide* wide,
                                    int64_t u_begin, int64_t n_utts, bool timed) {
    if (n_utts <= 0 || !(a.path || a.labels)) return GH_OK;
    GH_REQUIRE(wide, "gh_viterbi: internal: wide bigram form without its cost table");
    gh_layers_args b = a;
    b.slot0 = u_begin;
    const dim3 grid((unsigned)((n_utts + 63) / 64)), blk(64);
    const int64_t slot_end = u_begin + n_utts;
    const bool labels = a.labels != nullptr;
#define GH_BTW(ET, NN, SK)                                                                                                   \
    do {                                                                                                                     \
        if (timed) hipLaunchKernelGGL((bigram_backtrace_wide_kernel<NN, SK, 2>), grid, blk, 0, ctx->stream, b, wide, slot_end);  \
        else if (labels) hipLaunchKernelGGL((bigram_backtrace_wide_kernel<NN, SK, 1>), grid, blk, 0, ctx->stream, b, wide, slot_end); \
        else hipLaunchKernelGGL((bigram_backtrace_wide_kernel<NN, SK, 0>), grid, blk, 0, ctx->stream, b, wide, slot_end);        \
    } while (0)
    GH_BGW_CASES(double, GH_BTW)
#undef GH_BTW
    GH_HIP(hipGetLastError());
    return GH_OK;
}
