// The SETTLED PREFIX of a WIDE online stream (gh_online_create_wide_settle: the word loop with 17 .. 64 words): the two walks
// of gh_online_commit and gh_online_tail over the history viterbi_online_wide_kernel writes -- ONE complete 32-bit decision
// word per column and lane (CPW = 1), column j of a stream at word index (j % ring_words) * 64 + lane.  What the anchor is,
// why the set of cells only shrinks going back and what the flags mean: the header of gh_online_settle.hip, whose
// online_settle_kernel / online_segment_kernel these two restate for 64 word lanes; the host side (checks, task table,
// flags) is gh_online.hip's, which launches these for a session of the wide loop form (gh_online_form::walk).
//
// online_wide_settle_kernel -- the mapping of the wide sweep: ONE STREAM PER WAVE, lane = word.  A lane holds the live states
// of its word as an N-bit mask and maps it through its OWN decision word, so a column step is one coalesced 256 B row for
// the wave and a few bit operations however many cells are alive.  The row's address depends on the column alone, never on
// the masks: the rows of the next PF columns are in flight while a column is processed, where the walk would otherwise be
// a chain of dependent global loads.  The loop-row hop is the only step that crosses lanes, and with the whole wave on one
// stream it is a plain 64-bit ballot: of the lanes whose first state leaves through the loop row, and of the column's
// `cand == rm` bits, whose lowest lane (lowest word = lowest origin row, np.argmin) gets bit N - 1.  The size of the set
// needs no sum either: it has one member iff one lane has a mask and no lane has two bits.  Cost: O(unsettled tail) rows.
// online_wide_segment_kernel -- ONE path from a cell down to an anchor (or to column 0), lane = stream: online_segment_kernel
// with the addressing of loop_backtrace_wide_kernel (the decision word of (column j, word bw), the loop row's search over
// the column's (W + 3) / 4 uint4s), reads through the ring, the same label rules (MODE 1, timed MODE 2 with absolute
// columns), `strict`, the +inf-end fallback and flags 2 / 8.
#include "gh_online.h"
#include "gh_viterbi.h"
#include "gh_wave.h"

namespace {

template <int N, bool SKIP>
__global__ __launch_bounds__(64) void online_wide_settle_kernel(gh_settle_args a) {
    constexpr int HB = gh_loop_hb(N, SKIP), PF = 4;
    constexpr uint32_t HBM = (uint32_t)((1ull << HB) - 1ull);
    static_assert(HB <= 32 && N <= 8, "decision bits of a column must fit one word, the states of a word one mask");
    const int lane = threadIdx.x, w = lane;
    const int W = a.lf->W;
    const int64_t i = blockIdx.x;                               // (grid = n: wave-uniform, like everything but the masks)
    const gh_settle_task tk = a.tasks[i];
    gh_online_anchor old;
    old.col = -1; old.word = 0; old.state = 0; old.pad = 0;
    if (tk.has_anchor) old = a.anchor[tk.stream];
    const int lo = old.col >= 0 ? old.col : 0;                  // every trace passes the old anchor: the walk ends there
    const int ring = a.ring_words;
    const double INF = INFINITY;
    // the start set: the emitting cells of the newest column that are alive (lanes past the last word hold no bit, ever)
    uint32_t mask = 0;
    if (tk.T >= 2 && w < W) {
        const double* st = a.prev + ((int64_t)tk.stream * N) * 64 + w;
#pragma unroll
        for (int s = 0; s < N; ++s) mask |= (uint32_t)(st[s * 64] < INF) << s;
    }
    int j = tk.T - 1;
    bool active = __ballot(mask != 0) != 0 && j > lo;
    const uint32_t* hp = reinterpret_cast<const uint32_t*>(a.hist + (int64_t)tk.stream * a.hist_stride) + lane;
    // the rows of columns j, j - 1, .. in flight: jq / rq is the column / ring position the next load takes, held at column
    // lo + 1 (the last one a step reads) once the walk's end is in sight
    int jq = active ? j : 0, rq = active ? j % ring : 0;
    uint32_t pf[PF];
#pragma unroll
    for (int k = 0; k < PF; ++k) {
        pf[k] = active ? hp[(int64_t)rq * 64] : 0u;
        if (jq > lo + 1) { --jq; rq = rq == 0 ? ring - 1 : rq - 1; }
    }
    int flag = 0;
    bool mine = false;                                          // this lane holds the anchor: (j, w, lowest bit of mask)
    while (active) {
#pragma unroll
        for (int k = 0; k < PF; ++k) {
            if (!active) break;
            // ---- one column step back, j -> j - 1, through the decisions of column j ----
            const uint32_t hb = pf[k] & HBM;
            pf[k] = hp[(int64_t)rq * 64];
            if (jq > lo + 1) { --jq; rq = rq == 0 ? ring - 1 : rq - 1; }
            // first states: self keeps the bit; the loop row hands it to the last state of the column's best word (same column)
            const bool b0 = mask & 1u, b_l = (hb >> 1) & 1u, b_s = hb & 1u;
            const uint64_t hops = __ballot(b0 && !b_s && b_l);
            const uint64_t eq = __ballot(w < W && ((hb >> 2) & 1u));
            if (b0 && !b_s) {
                mask &= ~1u;
                if (!b_l) flag |= 2;                            // the start row, in a column > 0
            }
            if (hops) {
                if (!eq) flag |= 2;
                else if (w == __ffsll((unsigned long long)eq) - 1) mask |= 1u << (N - 1);   // lowest word = lowest origin row (np.argmin)
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
            mask = nm;
            --j;
            // the size of the set: one member iff one lane holds a mask and no lane holds two bits
            const uint64_t some = __ballot(mask != 0), many = __ballot(__popc(mask) > 1);
            if (some != 0 && (some & (some - 1)) == 0 && many == 0) {
                mine = mask != 0;
                active = false;
            } else if (some == 0 || j <= lo) {
                if (old.col >= 0) flag |= 2;                    // the traces did not meet in the old anchor (an empty set: a
                active = false;                                 // trace without predecessor, flagged above, left none to follow)
            }
        }
    }
    if (flag) atomicOr(a.flag, flag);
    const uint64_t found = __ballot(mine);
    if (found ? mine : lane == 0) {
        gh_online_anchor c = old;                               // nothing new: the anchor stays
        if (mine) { c.col = j; c.word = w; c.state = __ffs(mask) - 1; c.pad = 0; }
        a.cand[i] = c;
    }
}

// One path, lane = stream: online_segment_kernel over the wide layout.  Commit mode (a.cand): from the new anchor (visited)
// down to the old one; tail mode: from the chosen end of the newest column (not visited) down to the anchor; without an
// anchor the walk ends in column 0.  The run of labelled rows the anchor lies in belongs to the settled side, so the label
// pending on arrival is dropped, and with TIMED its column with it.  rp is the ring position of column j and follows it down.
template <int N, bool SKIP, bool TIMED>
__global__ __launch_bounds__(64) void online_wide_segment_kernel(gh_settle_args a) {
    constexpr int HB = gh_loop_hb(N, SKIP);
    constexpr uint32_t HBM = (uint32_t)((1ull << HB) - 1ull);
    __shared__ uint8_t s_arcs[GH_LAYERS_MAXW * GH_LAYERS_MAXN];
    const gh_layerform* __restrict__ lf = a.lf;
    for (int k = threadIdx.x; k < GH_LAYERS_MAXW * GH_LAYERS_MAXN; k += 64) s_arcs[k] = (&lf->arcs[0][0])[k];
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
        strict = a.prev[((int64_t)tk.stream * N + bs) * 64 + bw] < INFINITY;
    }
    const int lo = stop.col >= 0 ? stop.col : 0;
    const uint32_t* bpu = reinterpret_cast<const uint32_t*>(a.hist + (int64_t)tk.stream * a.hist_stride);
    int32_t* labs = a.labels + a.label_off[i];
    int32_t* begs = TIMED ? a.begins + a.label_off[i] : nullptr;
    int prev_col = 0;                                           // TIMED: column of the cell visited last
    const int64_t cap = a.label_off[i + 1] - a.label_off[i];
    const int ring = a.ring_words;
    int rp = j % ring;
    int64_t len = 0;
    int prev_label = -1, kind = 0, flag = 0;
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
    auto down = [&]() { --j; rp = rp == 0 ? ring - 1 : rp - 1; };
    if (commit) visit(row_of(bw, bs), j);
    while (j > lo && !flag) {
        if (kind == 0) {
            const uint32_t hb = bpu[(int64_t)rp * 64 + bw] & HBM;
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
                down();
                visit(row_of(bw, bs), j);
            } else {
                // candidates in ascending origin order: start row (arcs bit4), loop row (bit3), self (bit0)
                const int b_l = (hb >> 1) & 1, b_s = hb & 1;
                int pick = b_s ? 0 : (b_l ? 3 : 4);
                if (!((arcs >> pick) & 1)) pick = (arcs & 16) ? 4 : (arcs & 8) ? 3 : (arcs & 1) ? 0 : -1;
                if (pick == 0) { down(); visit(row_of(bw, 0), j); }
                else if (pick == 3) { kind = 1; visit(Lr, j); }
                else { flag |= 2; break; }                      // no origin, or the start row in a column > 0
            }
        } else {
            const uint4* rowp = reinterpret_cast<const uint4*>(bpu + (int64_t)rp * 64);
            int found = -1;
            for (int q4 = (W + 3) / 4 - 1; q4 >= 0; --q4) {     // the words' decision words of this column
                const uint4 v = rowp[q4];
                if ((v.w >> 2) & 1u) found = 4 * q4 + 3;
                if ((v.z >> 2) & 1u) found = 4 * q4 + 2;
                if ((v.y >> 2) & 1u) found = 4 * q4 + 1;
                if ((v.x >> 2) & 1u) found = 4 * q4;
            }
            if (found < 0 || found >= W) { flag |= 2; break; }  // lowest word = lowest origin row (np.argmin)
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

}  // namespace

int gh_launch_online_wide_settle(gh_ctx* ctx, const gh_online* on, const gh_settle_args& a, bool settle, const char* who) {
    if (a.n <= 0) return GH_OK;
    const gh_layerform& f = on->lat->h_layers;
    const dim3 blk(64);
    const dim3 grid((unsigned)(settle ? a.n : (a.n + 63) / 64));
#define GH_STW(ET, NN, SK)                                                                                        \
    do {                                                                                                          \
        if (settle) hipLaunchKernelGGL((online_wide_settle_kernel<NN, SK>), grid, blk, 0, ctx->stream, a);        \
        else if (a.begins) hipLaunchKernelGGL((online_wide_segment_kernel<NN, SK, true>), grid, blk, 0, ctx->stream, a); \
        else hipLaunchKernelGGL((online_wide_segment_kernel<NN, SK, false>), grid, blk, 0, ctx->stream, a);       \
    } while (0)
    GH_NSKIP_SWITCH(f.N, f.skip, 8, GH_STW, , "%s: wide loop form with %d states per word", who, f.N)
#undef GH_STW
    GH_HIP(hipGetLastError());
    return GH_OK;
}
