// The SETTLED PREFIX of an online stream (gh_online_commit, gh_online_tail): the part of the running hypothesis that no
// later audio can change, and with it the part of the decision history that is dead.
//
// Every hypothesis a stream can still end in is the back-trace of some cell of its newest column that is alive (finite
// carried cost).  Trace back from ALL of them at once: where the traces meet in one cell -- the ANCHOR -- everything at and
// before that cell is common to every future result.  A trace is a function of the decision bits alone, so the set of cells
// the traces occupy can only shrink going back, the first column (from the newest) in which it has one member is the latest
// such column, and below it nothing has to be looked at.  The cell a trace occupies "in column c" is the one in which it
// ARRIVES there from column c + 1: a first state that was entered from the loop row is followed through the loop row to the
// last state that fed it (same column) before the step to the column below.
//
// online_settle_kernel -- the mapping of the loop kernels: FOUR STREAMS PER WAVE, DPP row = stream, lane = word.  A lane
// holds the live states of its word as a bit mask and maps it through its OWN decision word (64 contiguous bytes per row and
// CPW columns), so a column step is one load per lane and a few bit operations however many cells are alive; lane = stream
// would walk every live cell's trace on its own, 16 N of them with scattered loads.  The loop-row hop is the only thing
// that crosses lanes: a row ballot of the lanes that take it, and the lowest lane of the column's `cand == rm` bits gets
// bit N - 1.  The size of the set is a DPP row sum of popcounts.  Cost: O(unsettled tail) per stream.
// online_segment_kernel -- ONE path from a cell down to an anchor (or to column 0), lane = stream as in
// lattice_backtrace_kernel, with the label rule of that kernel's MODE 1: the newly settled words (new anchor -> old anchor)
// and the words of the unsettled tail (best end -> anchor).
// online_bigram_settle_kernel, online_bigram_segment_kernel -- the same two walks over the records of a bigram session that
// settles (gh_online_create_bigram_settle), further down.
// The wide forms (17 .. 64 words, a wave per stream) have their two walks in gh_online_wide_settle.hip and
// gh_online_bigram_wide_settle.hip; the host side -- every check, the task table, the flags -- is gh_online.hip's and the same
// for all four (gh_online_form::walk).
// Bit layout: gh_loop_hb / gh_loop_cpw (gh_viterbi.h); tie rules: the LOOP branch of lattice_backtrace_kernel.  A finite
// cell has only finite predecessors, so the "+inf: first existing arc" fallback is never taken by the settle walk; the
// segment walk keeps it, because the chosen end of a stream may be a +inf cell (the one-shot decode's rule for it).
#include "gh_online.h"
#include "gh_viterbi.h"
#include "gh_wave.h"

namespace {

__device__ __forceinline__ int row_sum16(int v) {
    v += dpp_mov<0x121>(v);
    v += dpp_mov<0x122>(v);
    v += dpp_mov<0x124>(v);
    v += dpp_mov<0x128>(v);
    return v;
}

template <int N, bool SKIP>
__global__ __launch_bounds__(64) void online_settle_kernel(gh_settle_args a) {
    constexpr int HB = gh_loop_hb(N, SKIP), CPW = gh_loop_cpw(N, SKIP);
    constexpr uint32_t HBM = (uint32_t)((1ull << HB) - 1ull);
    static_assert(CPW >= 1 && N <= 16, "decision bits of a column must fit one word, the states of a word one mask");
    const int lane = threadIdx.x, kk = lane >> 4, w = lane & 15;
    const int W = a.lf->W;
    const int64_t i = (int64_t)blockIdx.x * 4 + kk;
    const bool has = i < a.n;
    gh_settle_task tk;
    tk.stream = 0; tk.T = 0; tk.has_anchor = 0; tk.pad = 0;
    if (has) tk = a.tasks[i];
    gh_online_anchor old;
    old.col = -1; old.word = 0; old.state = 0; old.pad = 0;
    if (has && tk.has_anchor) old = a.anchor[tk.stream];
    const int lo = old.col >= 0 ? old.col : 0;                  // every trace passes the old anchor: the walk ends there
    const int ring = a.ring_words;
    const double INF = INFINITY;
    // the start set: the emitting cells of the newest column that are alive
    uint32_t mask = 0;
    if (has && tk.T >= 2 && w < W) {
        const double* st = a.prev + ((int64_t)tk.stream * N) * 16 + w;
#pragma unroll
        for (int s = 0; s < N; ++s) mask |= (uint32_t)(st[s * 16] < INF) << s;
    }
    int j = tk.T - 1;
    bool active = row_sum16(__popc(mask)) > 0 && j > lo;        // row-uniform
    const uint32_t* hp = reinterpret_cast<const uint32_t*>(a.hist + (int64_t)tk.stream * a.hist_stride) + w;
    int ci = active ? j % CPW : 0, wr = active ? (j / CPW) % ring : 0, held = -1;
    uint32_t word = 0;
    int flag = 0;
    bool mine = false;                                          // this lane holds the anchor: (j, w, lowest bit of mask)
    while (__ballot(active)) {
        // ---- one column step back, j -> j - 1, through the decisions of column j ----
        if (active && wr != held) { word = hp[(int64_t)wr * 16]; held = wr; }
        const uint32_t hb = (word >> ((CPW - 1 - ci) * HB)) & HBM;
        // first states: self keeps the bit; the loop row hands it to the last state of the column's best word (same column)
        const bool b0 = mask & 1u, b_l = (hb >> 1) & 1u, b_s = hb & 1u;
        const uint32_t hops = (uint32_t)(__ballot(active && b0 && !b_s && b_l) >> (kk * 16)) & 0xffffu;
        const uint32_t eq = (uint32_t)(__ballot(active && w < W && ((hb >> 2) & 1u)) >> (kk * 16)) & 0xffffu;
        if (active && b0 && !b_s) {
            mask &= ~1u;
            if (!b_l) flag |= 2;                                // the start row, in a column > 0
        }
        if (hops) {
            if (!eq) flag |= 2;
            else if (w == __ffs(eq) - 1) mask |= 1u << (N - 1); // lowest word = lowest origin row (np.argmin)
        }
        uint32_t nm = mask & 1u;
        int before = 0;
#pragma unroll
        for (int s = N - 1; s >= 1; --s) {
            int code;
            if (SKIP && s >= 2) {
                const int b_a = (hb >> (HB - 1 - before)) & 1, b_b = (hb >> (HB - 2 - before)) & 1;
                code = b_b ? 0 : (b_a ? 1 : 2);
                before += 2;
            } else {
                code = ((hb >> (HB - 1 - before)) & 1) ? 0 : 1;
                before += 1;
            }
            if ((mask >> s) & 1u) nm |= 1u << (s - code);
        }
        if (active) {
            mask = nm;
            --j;
            if (ci == 0) { ci = CPW - 1; wr = wr == 0 ? ring - 1 : wr - 1; } else --ci;
        }
        const int size = row_sum16(__popc(mask));
        if (active && size == 1) {
            mine = mask != 0;
            active = false;
        } else if (active && j <= lo) {
            if (old.col >= 0) flag |= 2;                        // the traces did not meet in the old anchor
            active = false;
        }
    }
    if (flag) atomicOr(a.flag, flag);
    const uint32_t found = (uint32_t)(__ballot(mine) >> (kk * 16)) & 0xffffu;
    if (has && (found ? mine : w == 0)) {
        gh_online_anchor c = old;                               // nothing new: the anchor stays
        if (mine) { c.col = j; c.word = w; c.state = __ffs(mask) - 1; c.pad = 0; }
        a.cand[i] = c;
    }
}

// One path, lane = stream.  Commit mode (a.cand): from the new anchor (visited) down to the old one; tail mode: from the
// chosen end of the newest column (not visited, as in the one-shot back-trace) down to the anchor.  Without an anchor the
// walk ends in column 0 like the one-shot back-trace.  Labels: MODE 1 of lattice_backtrace_kernel; the run of labelled rows
// the anchor lies in belongs to the settled side, so the label pending on arrival is dropped.  TIMED (MODE 2 of that kernel):
// every label also stores the column of the cell visited last -- the first cell of the word's run (main.py:59-67), an
// absolute column of the stream whatever the ring has overwritten -- and the pending column is dropped with the pending label.
template <int N, bool SKIP, bool TIMED>
__global__ __launch_bounds__(64) void online_segment_kernel(gh_settle_args a) {
    constexpr int HB = gh_loop_hb(N, SKIP), CPW = gh_loop_cpw(N, SKIP);
    constexpr uint32_t HBM = (uint32_t)((1ull << HB) - 1ull);
    __shared__ uint8_t s_arcs[GH_LAYERS_ROWW * GH_LAYERS_MAXN];
    const gh_layerform* __restrict__ lf = a.lf;
    for (int k = threadIdx.x; k < GH_LAYERS_ROWW * GH_LAYERS_MAXN; k += 64) s_arcs[k] = (&lf->arcs[0][0])[k];
    __syncthreads();
    const int W = lf->W, Lr = lf->loop_row;
    const int64_t i = (int64_t)blockIdx.x * 64 + threadIdx.x;
    if (i >= a.n) return;
    const gh_settle_task tk = a.tasks[i];
    const bool commit = a.cand != nullptr;
    gh_online_anchor stop;
    stop.col = -1; stop.word = 0; stop.state = 0; stop.pad = 0;
    if (tk.has_anchor) stop = a.anchor[tk.stream];
    auto row_of = [&](int ww, int ss) { return ss == 0 ? Lr + 1 + ww : 1 + ww * (N - 1) + (ss - 1); };
    int j, bw, bs;
    bool strict = true;                                         // a walk that misses the anchor is an internal error
    if (commit) {
        const gh_online_anchor c = a.cand[i];
        a.settled_frames[i] = c.col + 1;
        if (c.col < 0 || c.col == stop.col) { if (a.n_labels) a.n_labels[i] = 0; return; }
        a.anchor[tk.stream] = c;
        if (!a.labels) return;
        j = c.col; bw = c.word; bs = c.state;
    } else {
        const int be = a.best_end[i];
        if (tk.T <= 1 || be < 0) { a.n_labels[i] = 0; return; }
        const int r = a.end_rows[be];
        if (r > Lr) { bw = r - Lr - 1; bs = 0; } else { bw = (r - 1) / (N - 1); bs = (r - 1) % (N - 1) + 1; }
        j = tk.T - 1;
        // (a +inf end is traced on the fallback arcs, which need not lead to the anchor: outside the contract, not an error)
        strict = a.prev[((int64_t)tk.stream * N + bs) * 16 + bw] < INFINITY;
    }
    const int lo = stop.col >= 0 ? stop.col : 0;
    const uint32_t* bpu = reinterpret_cast<const uint32_t*>(a.hist + (int64_t)tk.stream * a.hist_stride);
    int32_t* labs = a.labels + a.label_off[i];
    int32_t* begs = TIMED ? a.begins + a.label_off[i] : nullptr;
    int prev_col = 0;                                           // TIMED: column of the cell visited last
    const int64_t cap = a.label_off[i + 1] - a.label_off[i];
    const int ring = a.ring_words;
    int64_t len = 0;
    int prev_label = -1, kind = 0, flag = 0;
    int hwi = -1, hwr = 0;                                      // word index whose ring position is held
    int64_t key = -1;
    uint32_t cw = 0;
    auto visit = [&](int row, int col) {
        const int l = a.row_label[row];
        if (prev_label >= 0 && l < 0) {
            if (len >= cap) { flag |= 8; return; }
            labs[cap - 1 - len] = prev_label;
            if (TIMED) begs[cap - 1 - len] = prev_col;
            ++len;
        }
        prev_label = l;
        if (TIMED) prev_col = col;
    };
    if (commit) visit(row_of(bw, bs), j);
    while (j > lo && !flag) {
        const int wi = j / CPW;
        const int shift = (CPW - 1 - j % CPW) * HB;
        if (wi != hwi) { hwr = wi % ring; hwi = wi; }
        if (kind == 0) {
            const int64_t want = (int64_t)hwr * 16 + bw;
            if (want != key) { cw = bpu[want]; key = want; }
            const uint32_t hb = (cw >> shift) & HBM;
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
                if (!((arcs >> code) & 1)) code = (arcs & 4) ? 2 : (arcs & 2) ? 1 : (arcs & 1) ? 0 : -1;
                if (code < 0) { flag |= 2; break; }
                bs -= code;
                --j;
                visit(row_of(bw, bs), j);
            } else {
                const int b_l = (hb >> 1) & 1, b_s = hb & 1;
                int pick = b_s ? 0 : (b_l ? 3 : 4);
                if (!((arcs >> pick) & 1)) pick = (arcs & 16) ? 4 : (arcs & 8) ? 3 : (arcs & 1) ? 0 : -1;
                if (pick == 0) { --j; visit(row_of(bw, 0), j); }
                else if (pick == 3) { kind = 1; visit(Lr, j); }
                else { flag |= 2; break; }                      // no origin, or the start row in a column > 0
            }
        } else {
            const uint4* rowp = reinterpret_cast<const uint4*>(bpu + (int64_t)hwr * 16);
            int found = -1;
#pragma unroll
            for (int q4 = 3; q4 >= 0; --q4) {
                const uint4 v = rowp[q4];
                if ((v.w >> (shift + 2)) & 1u) found = 4 * q4 + 3;
                if ((v.z >> (shift + 2)) & 1u) found = 4 * q4 + 2;
                if ((v.y >> (shift + 2)) & 1u) found = 4 * q4 + 1;
                if ((v.x >> (shift + 2)) & 1u) found = 4 * q4;
            }
            if (found < 0 || found >= W) { flag |= 2; break; }
            bw = found;
            bs = N - 1;
            kind = 0;
            visit(row_of(bw, bs), j);
        }
    }
    if (!flag && stop.col >= 0) {
        if (bw != stop.word || bs != stop.state) { if (strict) flag |= 2; }
        prev_label = -1;                                        // the anchor's own run is settled already
    }
    if (flag) atomicOr(a.flag, flag);
    if (!flag && prev_label >= 0) {
        if (len >= cap) atomicOr(a.flag, 8);
        else {
            labs[cap - 1 - len] = prev_label;
            if (TIMED) begs[cap - 1 - len] = prev_col;
            ++len;
        }
    }
    for (int64_t k = 0; k < len; ++k) labs[k] = labs[cap - len + k];
    if (TIMED)
        for (int64_t k = 0; k < len; ++k) begs[k] = begs[cap - len + k];
    a.n_labels[i] = (int32_t)len;
}

// ------------------------------------------------------------------------------------------------- the BIGRAM records
// The same two walks over the records of viterbi_bigram_online_kernel (gh_bigram_hb / gh_bigram_cpw: the in-word bits from
// the top, then the 4-bit predecessor word v, b_l, b_s).  Copies of the kernels above, not a shared template: what differs
// is the hop out of a first state.  The loop form has ONE non-emitting row, so all hopping lanes of a column land in the
// same word (the lowest `cand == rm` bit); here every word has its own entry row and a hopping lane names ITS predecessor
// word in its own record.

// OR over the 16 lanes of a DPP row, in all of them (the rotations of row_sum16)
__device__ __forceinline__ uint32_t row_or16(uint32_t v) {
    v |= (uint32_t)dpp_mov<0x121>((int)v);
    v |= (uint32_t)dpp_mov<0x122>((int)v);
    v |= (uint32_t)dpp_mov<0x124>((int)v);
    v |= (uint32_t)dpp_mov<0x128>((int)v);
    return v;
}

// online_settle_kernel for the bigram records.  The hop: a lane whose first state is live and was entered through its entry
// row (b0 && !b_s && b_l) contributes 1 << v, the row ORs the contributions, and lane w gets bit N - 1 where bit w of the
// OR is set -- before the in-word decisions of the same column are applied, because the entry row read the last states
// of THIS column.  A finite cell has only finite predecessors, so the recorded nibble is an existing arc (bigram_backtrace_kernel's
// bg_in fallback is for +inf cells) and v < W; anything else is flag 2.
template <int N, bool SKIP>
__global__ __launch_bounds__(64) void online_bigram_settle_kernel(gh_settle_args a) {
    constexpr int HB = gh_bigram_hb(N, SKIP), CPW = gh_bigram_cpw(N, SKIP);
    constexpr uint32_t HBM = (uint32_t)((1ull << HB) - 1ull);
    static_assert(CPW >= 1 && N <= 16, "the record of a column must fit one word, the states of a word one mask");
    const int lane = threadIdx.x, kk = lane >> 4, w = lane & 15;
    const int W = a.lf->W;
    const int64_t i = (int64_t)blockIdx.x * 4 + kk;
    const bool has = i < a.n;
    gh_settle_task tk;
    tk.stream = 0; tk.T = 0; tk.has_anchor = 0; tk.pad = 0;
    if (has) tk = a.tasks[i];
    gh_online_anchor old;
    old.col = -1; old.word = 0; old.state = 0; old.pad = 0;
    if (has && tk.has_anchor) old = a.anchor[tk.stream];
    const int lo = old.col >= 0 ? old.col : 0;                  // every trace passes the old anchor: the walk ends there
    const int ring = a.ring_words;
    const double INF = INFINITY;
    // the start set: the emitting cells of the newest column that are alive
    uint32_t mask = 0;
    if (has && tk.T >= 2 && w < W) {
        const double* st = a.prev + ((int64_t)tk.stream * N) * 16 + w;
#pragma unroll
        for (int s = 0; s < N; ++s) mask |= (uint32_t)(st[s * 16] < INF) << s;
    }
    int j = tk.T - 1;
    bool active = row_sum16(__popc(mask)) > 0 && j > lo;        // row-uniform
    const uint32_t* hp = reinterpret_cast<const uint32_t*>(a.hist + (int64_t)tk.stream * a.hist_stride) + w;
    int ci = active ? j % CPW : 0, wr = active ? (j / CPW) % ring : 0, held = -1;
    uint32_t word = 0;
    int flag = 0;
    bool mine = false;                                          // this lane holds the anchor: (j, w, lowest bit of mask)
    while (__ballot(active)) {
        // ---- one column step back, j -> j - 1, through the records of column j ----
        if (active && wr != held) { word = hp[(int64_t)wr * 16]; held = wr; }
        const uint32_t hb = (word >> ((CPW - 1 - ci) * HB)) & HBM;
        // first states: self keeps the bit; the entry row hands it to the last state of the word this lane's record names
        const bool b0 = mask & 1u, b_l = (hb >> 1) & 1u, b_s = hb & 1u;
        const uint32_t v = (hb >> 2) & 15u;
        const bool hop = active && b0 && !b_s && b_l;
        if (active && b0 && !b_s) {
            mask &= ~1u;
            if (!b_l || (int)v >= W) flag |= 2;                 // the start row in a column > 0, or a word the graph has not
        }
        const uint32_t hops = row_or16((hop && (int)v < W) ? 1u << v : 0u);
        if ((hops >> w) & 1u) mask |= 1u << (N - 1);
        uint32_t nm = mask & 1u;
        int before = 0;
#pragma unroll
        for (int s = N - 1; s >= 1; --s) {
            int code;
            if (SKIP && s >= 2) {
                const int b_a = (hb >> (HB - 1 - before)) & 1, b_b = (hb >> (HB - 2 - before)) & 1;
                code = b_b ? 0 : (b_a ? 1 : 2);
                before += 2;
            } else {
                code = ((hb >> (HB - 1 - before)) & 1) ? 0 : 1;
                before += 1;
            }
            if ((mask >> s) & 1u) nm |= 1u << (s - code);
        }
        if (active) {
            mask = nm;
            --j;
            if (ci == 0) { ci = CPW - 1; wr = wr == 0 ? ring - 1 : wr - 1; } else --ci;
        }
        const int size = row_sum16(__popc(mask));
        if (active && size == 1) {
            mine = mask != 0;
            active = false;
        } else if (active && j <= lo) {
            if (old.col >= 0) flag |= 2;                        // the traces did not meet in the old anchor
            active = false;
        }
    }
    if (flag) atomicOr(a.flag, flag);
    const uint32_t found = (uint32_t)(__ballot(mine) >> (kk * 16)) & 0xffffu;
    if (has && (found ? mine : w == 0)) {
        gh_online_anchor c = old;                               // nothing new: the anchor stays
        if (mine) { c.col = j; c.word = w; c.state = __ffs(mask) - 1; c.pad = 0; }
        a.cand[i] = c;
    }
}

// online_segment_kernel for the bigram records: bigram_backtrace_kernel's step (rows: state 0 of word w is loop_row + W + w,
// its entry row loop_row + w; the predecessor nibble with the bg_in fallback; the arc-mask fallbacks; label MODE 1 / 2)
// with the stop conditions above -- commit: new anchor -> old anchor, tail: chosen end -> anchor, the label pending at the
// anchor dropped, reads through the ring, a +inf end not strict.
template <int N, bool SKIP, bool TIMED>
__global__ __launch_bounds__(64) void online_bigram_segment_kernel(gh_settle_args a) {
    constexpr int HB = gh_bigram_hb(N, SKIP), CPW = gh_bigram_cpw(N, SKIP);
    constexpr uint32_t HBM = (uint32_t)((1ull << HB) - 1ull);
    __shared__ uint8_t s_arcs[GH_LAYERS_ROWW * GH_LAYERS_MAXN];
    __shared__ uint16_t s_in[GH_LAYERS_ROWW];
    const gh_layerform* __restrict__ lf = a.lf;
    for (int k = threadIdx.x; k < GH_LAYERS_ROWW * GH_LAYERS_MAXN; k += 64) s_arcs[k] = (&lf->arcs[0][0])[k];
    if (threadIdx.x < GH_LAYERS_ROWW) s_in[threadIdx.x] = lf->bg_in[threadIdx.x];
    __syncthreads();
    const int W = lf->W, Lr = lf->loop_row;
    const int64_t i = (int64_t)blockIdx.x * 64 + threadIdx.x;
    if (i >= a.n) return;
    const gh_settle_task tk = a.tasks[i];
    const bool commit = a.cand != nullptr;
    gh_online_anchor stop;
    stop.col = -1; stop.word = 0; stop.state = 0; stop.pad = 0;
    if (tk.has_anchor) stop = a.anchor[tk.stream];
    auto row_of = [&](int ww, int ss) { return ss == 0 ? Lr + W + ww : 1 + ww * (N - 1) + (ss - 1); };
    int j, bw, bs;
    bool strict = true;                                         // a walk that misses the anchor is an internal error
    if (commit) {
        const gh_online_anchor c = a.cand[i];
        a.settled_frames[i] = c.col + 1;
        if (c.col < 0 || c.col == stop.col) { if (a.n_labels) a.n_labels[i] = 0; return; }
        a.anchor[tk.stream] = c;
        if (!a.labels) return;
        j = c.col; bw = c.word; bs = c.state;
    } else {
        const int be = a.best_end[i];
        if (tk.T <= 1 || be < 0) { a.n_labels[i] = 0; return; }
        const int r = a.end_rows[be];
        if (r >= Lr + W) { bw = r - Lr - W; bs = 0; } else { bw = (r - 1) / (N - 1); bs = (r - 1) % (N - 1) + 1; }
        j = tk.T - 1;
        // (a +inf end is traced on the fallback arcs, which need not lead to the anchor: outside the contract, not an error)
        strict = a.prev[((int64_t)tk.stream * N + bs) * 16 + bw] < INFINITY;
    }
    const int lo = stop.col >= 0 ? stop.col : 0;
    const uint32_t* bpu = reinterpret_cast<const uint32_t*>(a.hist + (int64_t)tk.stream * a.hist_stride);
    int32_t* labs = a.labels + a.label_off[i];
    int32_t* begs = TIMED ? a.begins + a.label_off[i] : nullptr;
    int prev_col = 0;                                           // TIMED: column of the cell visited last
    const int64_t cap = a.label_off[i + 1] - a.label_off[i];
    const int ring = a.ring_words;
    int64_t len = 0;
    int prev_label = -1, kind = 0, flag = 0;                    // kind 0: emitting (bw, bs); 1: entry row of word bw
    int hwi = -1, hwr = 0;                                      // word index whose ring position is held
    int64_t key = -1;
    uint32_t cw = 0;
    auto visit = [&](int row, int col) {
        const int l = a.row_label[row];
        if (prev_label >= 0 && l < 0) {
            if (len >= cap) { flag |= 8; return; }
            labs[cap - 1 - len] = prev_label;
            if (TIMED) begs[cap - 1 - len] = prev_col;
            ++len;
        }
        prev_label = l;
        if (TIMED) prev_col = col;
    };
    if (commit) visit(row_of(bw, bs), j);
    while (j > lo && !flag) {
        const int wi = j / CPW;
        const int shift = (CPW - 1 - j % CPW) * HB;
        if (wi != hwi) { hwr = wi % ring; hwi = wi; }
        const int64_t want = (int64_t)hwr * 16 + bw;
        if (want != key) { cw = bpu[want]; key = want; }
        const uint32_t hb = (cw >> shift) & HBM;
        if (kind == 1) {                                        // entry row of word bw: the recorded predecessor word
            int v = (int)((hb >> 2) & 15u);
            const int in = s_in[bw];
            if (!((in >> v) & 1)) v = in ? __ffs(in) - 1 : -1;  // every candidate was +inf: the first existing arc
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
            if (pick == 0) { --j; visit(row_of(bw, 0), j); }
            else if (pick == 3) { kind = 1; visit(Lr + bw, j); }
            else { flag |= 2; break; }                          // no origin, or the start row in a column > 0
        }
    }
    if (!flag && stop.col >= 0) {
        if (bw != stop.word || bs != stop.state) { if (strict) flag |= 2; }
        prev_label = -1;                                        // the anchor's own run is settled already
    }
    if (flag) atomicOr(a.flag, flag);
    if (!flag && prev_label >= 0) {
        if (len >= cap) atomicOr(a.flag, 8);
        else {
            labs[cap - 1 - len] = prev_label;
            if (TIMED) begs[cap - 1 - len] = prev_col;
            ++len;
        }
    }
    for (int64_t k = 0; k < len; ++k) labs[k] = labs[cap - len + k];
    if (TIMED)
        for (int64_t k = 0; k < len; ++k) begs[k] = begs[cap - len + k];
    a.n_labels[i] = (int32_t)len;
}

}  // namespace

int gh_launch_online_bigram_settle(gh_ctx* ctx, const gh_online* on, const gh_settle_args& a, bool settle, const char* who) {
    const gh_layerform& f = on->lat->h_layers;
    const dim3 blk(64);
    const dim3 grid((unsigned)(settle ? (a.n + 3) / 4 : (a.n + 63) / 64));
#define GH_STB(ET, NN, SK)                                                                                          \
    do {                                                                                                            \
        if (settle) hipLaunchKernelGGL((online_bigram_settle_kernel<NN, SK>), grid, blk, 0, ctx->stream, a);        \
        else if (a.begins) hipLaunchKernelGGL((online_bigram_segment_kernel<NN, SK, true>), grid, blk, 0, ctx->stream, a); \
        else hipLaunchKernelGGL((online_bigram_segment_kernel<NN, SK, false>), grid, blk, 0, ctx->stream, a);       \
    } while (0)
    GH_NSKIP_SWITCH(f.N, f.skip, 16_NO_SKIP16, GH_STB, , "%s: bigram form with %d states per word (skip arcs: %d)", who, f.N, f.skip)
#undef GH_STB
    GH_HIP(hipGetLastError());
    return GH_OK;
}

int gh_launch_online_loop_settle(gh_ctx* ctx, const gh_online* on, const gh_settle_args& a, bool settle, const char* who) {
    const gh_layerform& f = on->lat->h_layers;
    const dim3 blk(64);
    const dim3 grid((unsigned)(settle ? (a.n + 3) / 4 : (a.n + 63) / 64));
#define GH_ST(ET, NN, SK)                                                                                    \
    do {                                                                                                     \
        if (settle) hipLaunchKernelGGL((online_settle_kernel<NN, SK>), grid, blk, 0, ctx->stream, a);        \
        else if (a.begins) hipLaunchKernelGGL((online_segment_kernel<NN, SK, true>), grid, blk, 0, ctx->stream, a); \
        else hipLaunchKernelGGL((online_segment_kernel<NN, SK, false>), grid, blk, 0, ctx->stream, a);       \
    } while (0)
    GH_NSKIP_SWITCH(f.N, f.skip, 16, GH_ST, , "%s: loop form with %d states per word", who, f.N)
#undef GH_ST
    GH_HIP(hipGetLastError());
    return GH_OK;
}
