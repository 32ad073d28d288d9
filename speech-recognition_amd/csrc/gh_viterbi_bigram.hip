// Viterbi over the BIGRAM form (gh_layerform with loop = 2, gh_internal.h): the word-loop grammar with word-to-word costs
// (continuous_speech.build_bigram_grammar).  Same semantics as the generic kernel (decode_hmm_states, decode.py:80-146):
// candidates in ascending origin order with a strict '<', arcs that touch a non-emitting row read the SAME column, start
// only in cell (0, 0), last of equal end points, path without the end cell.
//
// gfx950 mapping -- the organisation of viterbi_loop_kernel (gh_viterbi_layers.hip): FOUR UTTERANCES PER WAVE, DPP row =
// utterance, lane = word, the N state costs of the word in registers, emissions read ahead through a register ring, the
// rows of finished utterances switched off by EXEC.  What differs is the step between the words' last states and their
// first states: the loop form takes ONE minimum over the row's 16 lanes; here every lane w takes its own
//     entry[w] = min_v ( last[v] + B[v][w] )        (the non-emitting entry row of word w, same column)
// with column w of B in 16 registers of lane w, statically indexed:
//   * last[v] reaches all 16 lanes of the row by the DPP row broadcast of lane v (row_newbcast:v, 0x150 + v; the one DPP
//     control gfx90a+ has for 64-bit operands too), v = 0 .. 15 IN ASCENDING ORDER.  Ascending v is ascending origin
//     row, so a strict '<' between neighbours of a reduction tree whose left operand is always the lower v is the
//     reference's first minimum; no (value, v) pair has to be compared, as a reduction over row ROTATIONS would need
//     (there lane w meets v = w, w+1, .., 15, 0, .., w-1).  16 broadcast + add, then 15 x (compare, vmin, select v);
//   * the arg-min v (4 bits) is shifted into the lane's decision word behind the in-word decision bits of the column:
//     N + 5 (+ N - 2 with skip arcs) bits per column and lane -- ONE stream of wider records at fewer columns per
//     32-bit word (N = 5: 3 columns instead of the loop form's 4) rather than a second stream of nibbles: the forward
//     sweep keeps one store per CPW columns and the back-trace one load per change of word, and the record of a
//     column stays in one place;
//   * a forbidden pair is a +inf in B: it never wins against a finite candidate.  When EVERY candidate of an entry row is
//     +inf the reference keeps the first EXISTING arc; the sweep then records v = 0, and the back-trace, which has the
//     arc masks (gh_layerform::bg_in), replaces a recorded v without arc by the lowest v with one.
// Word sizes: 2 .. 8, 12 and 16 states like the loop form, except 16 states WITH skip arcs (35 decision bits per column:
// left to the row-per-lane kernels).  No scratch in the column loop for any of them (kernel-resource-usage remarks).
#include "gh_internal.h"
#include "gh_viterbi.h"
#include "gh_wave.h"

namespace {

template <int N, bool SKIP> struct BigramBits {
    static constexpr int HB = gh_bigram_hb(N, SKIP), CPW = gh_bigram_cpw(N, SKIP);
    static_assert(CPW >= 1, "the decision bits of a column must fit one word");
};

// (a, ia) <- the smaller of (a, ia) and (b, ib); ia < ib always, so a tie keeps the lower word
#define GH_BG_MERGE(a, ia, b, ib) do { const bool lt_ = (b) < (a); a = vmin(a, b); ia = lt_ ? (ib) : (ia); } while (0)

template <typename ET, int N, bool SKIP, bool WANT_BP>
__global__ __launch_bounds__(64) void viterbi_bigram_kernel(gh_layers_args a, int64_t slot_end) {
    constexpr int HB = BigramBits<N, SKIP>::HB, CPW = BigramBits<N, SKIP>::CPW;
    constexpr int PF = N > 8 ? 2 : 4;
    const int lane = threadIdx.x, kk = lane >> 4, w = lane & 15;
    const gh_layerform* __restrict__ lf = a.lf;
    const int W = lf->W, Lr = lf->loop_row;
    const int64_t slot = a.slot0 + (int64_t)blockIdx.x * 4 + kk;
    const bool has_utt = slot < slot_end;
    const int64_t u = has_utt ? (a.perm ? a.perm[slot] : slot) : 0;
    const int64_t f0 = has_utt ? a.utt_off[u] : 0;
    const int T = has_utt ? (int)(a.utt_off[u + 1] - f0) : 0;
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
    const char* nllb = static_cast<const char*>(a.nll) + (T > 0 ? f0 : 0) * a.S * (int64_t)sizeof(ET);   // per row (no frames: frame 0)
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
    uint32_t word = 0;
    uint32_t* bp = (WANT_BP && has_utt) ? reinterpret_cast<uint32_t*>(a.bp + a.bp_off[slot]) + w : nullptr;

    for (int t0 = 0; t0 < Tmax; t0 += PF) {                    // (the columns behind Tmax in the last group: no row is in them)
#pragma unroll
        for (int k = 0; k < PF; ++k) {
            const int t = t0 + k;
            double e[N];
#pragma unroll
            for (int s = 0; s < N; ++s) e[s] = (double)ring[k][s];
            if (t < T) {                                       // row-uniform: the rows of finished utterances sit out
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
                        if (WANT_BP) { push_bit(word, __ballot(b_a)); push_bit(word, __ballot(b_b)); }
                    } else {
                        const bool b = v0 < v1;
                        best = vmin(v0, v1);
                        if (WANT_BP) push_bit(word, __ballot(b));
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
                if (WANT_BP) word = (word << 4) | i0;
                // state 0: start row (row 0), entry row, self -- ascending origin, strict '<'
                const double cs = ((t == 0) ? 0.0 : INF) + cin0;
                const double cl = q0;                          // (the arc entry row -> state 0 costs 0)
                const bool b_l = cl < cs;
                const double m2 = vmin(cl, cs);
                const bool b_s = base0 < m2;
                if (WANT_BP) { push_bit(word, __ballot(b_l)); push_bit(word, __ballot(b_s)); }
                prev[0] = vmin(vmin(base0, m2) + e[0], INF);
                if (WANT_BP) {
                    const int ci = t % CPW;
                    if (ci == CPW - 1 || t == T - 1) {
                        if (CPW > 1 && ci < CPW - 1) word <<= HB * (CPW - 1 - ci);   // last, partly filled word: left aligned
                        bp[(int64_t)(t / CPW) * 16] = word;
                        word = 0;
                    }
                }
            }
            {   // the slot's refill: unconditional, from a clamped column, OUTSIDE the divergent region and behind the last
                // use of the old value (see viterbi_layers_kernel); rows without frames read frame 0 of the matrix
                const int tn = (t + PF < T) ? t + PF : (T > 0 ? T - 1 : 0);
                const char* colp = nllb + (int64_t)tn * rowb;
#pragma unroll
                for (int s = 0; s < N; ++s) ring[k][s] = *reinterpret_cast<const ET*>(colp + sto[s]);
            }
        }
    }
    if (!has_utt) return;
    // ---- end costs + end selection inside the row ('>=': the last of equal minima) ----
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
    for (int o = 8; o >= 1; o >>= 1) {
        const double ov = __shfl_xor(best_v, o);
        const int os = __shfl_xor(best_slot, o);
        if (ov < best_v || (ov == best_v && os > best_slot)) { best_v = ov; best_slot = os; }
    }
    if (w == 0 && a.best_end) a.best_end[u] = T > 0 ? best_slot : -1;
}

// ---------------------------------------------------------------------------------------------------------------------
// Back-trace (decode.py:143-145), ONE LANE PER UTTERANCE like lattice_backtrace_kernel: the lane keeps the decision word
// of its current (word index, word) in a register and the one below it prefetched.  An entry row's predecessor is the
// nibble of the SAME lane's record (the loop form scans 16 lanes' equality bits instead).  MODE 0: the (row, column) path
// as decode_hmm_states returns it, entry rows included; MODE 1: only the label sequence of main.py:59-67
// (gh_viterbi_labels), collected from the back of the utterance's slot and moved to its front at the end; MODE 2: the labels
// and, in a.path, the column of the first cell of every word's run (gh_viterbi_labels_timed).
template <int N, bool SKIP, int MODE>
__global__ __launch_bounds__(64) void bigram_backtrace_kernel(gh_layers_args a, int64_t slot_end) {
    constexpr int HB = BigramBits<N, SKIP>::HB, CPW = BigramBits<N, SKIP>::CPW;
    __shared__ uint8_t s_arcs[GH_LAYERS_ROWW * GH_LAYERS_MAXN];
    __shared__ uint16_t s_in[GH_LAYERS_ROWW];
    const gh_layerform* __restrict__ lf = a.lf;
    for (int i = threadIdx.x; i < GH_LAYERS_ROWW * GH_LAYERS_MAXN; i += 64) s_arcs[i] = (&lf->arcs[0][0])[i];
    if (threadIdx.x < GH_LAYERS_ROWW) s_in[threadIdx.x] = lf->bg_in[threadIdx.x];
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
    int64_t key = -1;                                         // index of the decision word held in `cw`
    uint32_t cw = 0, pw = 0;                                  // current word, and the one 16 words below it
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
        const int wi = j / CPW;
        const int shift = (CPW - 1 - j % CPW) * HB;
        const int64_t want = (int64_t)wi * 16 + bw;
        if (want != key) {
            if (want == key - 16) cw = pw; else cw = bpu[want];
            key = want;
            pw = (wi > 0) ? bpu[want - 16] : 0u;
        }
        const uint32_t hb = (cw >> shift) & (uint32_t)((1ull << HB) - 1ull);
        if (kind == 1) {                                      // entry row of word bw: the recorded predecessor word
            int v = (int)((hb >> 2) & 15u);
            const int in = s_in[bw];
            if (!((in >> v) & 1)) v = in ? __ffs(in) - 1 : -1;                 // every candidate was +inf: the first existing arc
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

// word sizes the kernels above are instantiated for (16 states with skip arcs: 35 decision bits per column)
bool gh_bigram_n_ok(int N, int skip) { return gh_seq_n_ok(N) && !(N == 16 && skip); }

// back-pointer scratch of one utterance of T frames, in uint16 units (the lattice kernels' common unit)
size_t gh_bigram_bp_entries(const gh_layerform& f, int64_t T) {
    if (f.W > GH_LAYERS_ROWW) return gh_bigram_wide_bp_entries(T);
    return gh_bp_entries(T, gh_bigram_cpw(f.N, f.skip), 16, 32);
}

#define GH_BG_CASES(ET, MACRO) \
    GH_NSKIP_SWITCH(f.N, f.skip, 16_NO_SKIP16, MACRO, ET, "gh_viterbi: bigram form with %d states per word (skip arcs: %d)", f.N, f.skip)

int gh_launch_viterbi_bigram(gh_ctx* ctx, const gh_layers_args& a, const gh_layerform& f, int64_t u_begin, int64_t n_utts,
                             bool f64, bool want_path, const gh_bigram_wide* wide) {
    if (f.W > GH_LAYERS_ROWW) return gh_launch_viterbi_bigram_wide(ctx, a, f, wide, u_begin, n_utts, f64, want_path);
    if (n_utts <= 0) return GH_OK;
    gh_layers_args b = a;
    b.slot0 = u_begin;
    const dim3 grid((unsigned)((n_utts + 3) / 4)), blk(64);
    const int64_t slot_end = u_begin + n_utts;
#define GH_BG(ET, NN, SK)                                                                                                    \
    do {                                                                                                                     \
        if (want_path) hipLaunchKernelGGL((viterbi_bigram_kernel<ET, NN, SK, true>), grid, blk, 0, ctx->stream, b, slot_end);  \
        else hipLaunchKernelGGL((viterbi_bigram_kernel<ET, NN, SK, false>), grid, blk, 0, ctx->stream, b, slot_end);           \
    } while (0)
    if (f64) { GH_BG_CASES(double, GH_BG) } else { GH_BG_CASES(float, GH_BG) }
#undef GH_BG
    GH_HIP(hipGetLastError());
    return GH_OK;
}

// the path (a.path) or the label sequences (a.labels) of the utterances [u_begin, u_begin + n_utts) from the decision words
int gh_launch_bigram_backtrace(gh_ctx* ctx, const gh_layers_args& a, const gh_layerform& f, int64_t u_begin, int64_t n_utts, bool timed,
                               const gh_bigram_wide* wide) {
    if (f.W > GH_LAYERS_ROWW) return gh_launch_bigram_backtrace_wide(ctx, a, f, wide, u_begin, n_utts, timed);
    if (n_utts <= 0 || !(a.path || a.labels)) return GH_OK;
    gh_layers_args b = a;
    b.slot0 = u_begin;
    const dim3 grid((unsigned)((n_utts + 63) / 64)), blk(64);
    const int64_t slot_end = u_begin + n_utts;
    const bool labels = a.labels != nullptr;
#define GH_BT(ET, NN, SK)                                                                                             \
    do {                                                                                                              \
        if (timed) hipLaunchKernelGGL((bigram_backtrace_kernel<NN, SK, 2>), grid, blk, 0, ctx->stream, b, slot_end); \
        else if (labels) hipLaunchKernelGGL((bigram_backtrace_kernel<NN, SK, 1>), grid, blk, 0, ctx->stream, b, slot_end); \
        else hipLaunchKernelGGL((bigram_backtrace_kernel<NN, SK, 0>), grid, blk, 0, ctx->stream, b, slot_end);          \
    } while (0)
    GH_BG_CASES(double, GH_BT)
#undef GH_BT
    GH_HIP(hipGetLastError());
    return GH_OK;
}
