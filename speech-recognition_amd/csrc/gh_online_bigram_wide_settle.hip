// The SETTLED PREFIX of a WIDE BIGRAM online stream (gh_online_create_bigram_wide_settle: the bigram grammar with 17 .. 64
// words): the two walks of gh_online_commit and gh_online_tail over the history viterbi_bigram_online_wide_kernel writes --
// ONE complete 32-bit record per column and lane (gh_bigram_wide_hb: the in-word bits from the top, 6 bits of predecessor word
// v, b_l, b_s), column j of a stream at word index (j % ring_words) * 64 + lane.  What the anchor is, why the set of cells only
// shrinks going back and what the flags mean: the header of gh_online_settle.hip.  The host side (checks, task table, flags) is
// gh_online.hip's, which launches these for a session of the wide bigram form (gh_online_form::walk).
//
// online_bigram_wide_settle_kernel -- online_wide_settle_kernel's structure (gh_online_wide_settle.hip): ONE STREAM PER WAVE,
// lane = word, a lane holds the live states of its word as an N-bit mask and maps it through its OWN record; the row address
// depends on the column alone, so the rows of the next PF columns are in flight, held at column lo + 1; the set has one member
// iff one lane has a mask and no lane has two bits (two ballots); the walk ends in the old anchor.  What differs is THE HOP out
// of a first state, which is online_bigram_settle_kernel's stretched from a 16-lane DPP row to the wave: a lane whose first
// state is live and was entered through its entry row (b0 && !b_s && b_l) names ITS predecessor word v in its own record, and
// lane w gets bit N - 1 iff some hopper names v == w -- before the in-word decisions of the same column are applied, because
// the entry row read the last states of THIS column.  Several hoppers per column that name different words, across the 16-lane
// groups, are the normal case.  The 64-lane OR of "1 << v" is a 64-byte LDS HIT TABLE per wave: every lane zeroes its own slot,
// the hoppers store 1 at [v], every lane reads its own slot.  The block is one wave and the LDS serves a wave's accesses in
// issue order, so there is no barrier; the cost is the same few instructions for 1 hopper or 64 (a loop over the set bits of
// the hop ballot with v_readlane costs that much per hopper: DESIGN.md 4.20), and a column without a hopper skips it
// (wave-uniform).  A finite cell has only finite predecessors, so the recorded v is an existing arc and v < W; anything else
// is flag 2, and so is !b_l on a first state that leaves in a column > 0.
// online_bigram_wide_segment_kernel -- ONE path from a cell down to an anchor (or to column 0), lane = stream:
// online_bigram_segment_kernel with the addressing and the rules of bigram_backtrace_wide_kernel (rows: state 0 of word w is
// loop_row + W + w, its entry row loop_row + w; the record of (column j, word bw) read through the ring; an entry row's
// predecessor from the 6-bit field of the same record with the 64-bit gh_bigram_wide::bg_in fallback; the arc-mask fallbacks),
// the same label rules (MODE 1, timed MODE 2 with absolute columns), `strict`, the +inf-end fallback and flags 2 / 8.  The cost
// table reaches it as a second kernel argument: gh_settle_args keeps its size, and no older kernel its descriptor.
// No scratch and no runtime-indexed private array for any instantiation (profiles/online_bigram_wide_settle_kernel_resources.txt).
#include "gh_online.h"
#include "gh_viterbi.h"
#include "gh_wave.h"

namespace {

template <int N, bool SKIP>
__global__ __launch_bounds__(64) void online_bigram_wide_settle_kernel(gh_settle_args a) {
    constexpr int HB = gh_bigram_wide_hb(N, SKIP), PF = 4;
    constexpr uint32_t HBM = (uint32_t)((1ull << HB) - 1ull);
    static_assert(HB <= 32 && N <= 8, "the record of a column must fit one word, the states of a word one mask");
    static_assert(GH_LAYERS_MAXW == 64, "one hit slot per lane");
    __shared__ uint8_t hit[GH_LAYERS_MAXW];                     // the hit table of the hop (one wave: fences of wavefront scope)
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
            // ---- one column step back, j -> j - 1, through the records of column j ----
            const uint32_t hb = pf[k] & HBM;
            pf[k] = hp[(int64_t)rq * 64];
            if (jq > lo + 1) { --jq; rq = rq == 0 ? ring - 1 : rq - 1; }
            // first states: self keeps the bit; the entry row hands it to the last state of the word this lane's record names
            const bool b0 = mask & 1u, b_l = (hb >> 1) & 1u, b_s = hb & 1u;
            const int v = (int)((hb >> 2) & 63u);
            const bool hop = b0 && !b_s && b_l && v < W;
            if (b0 && !b_s) {
                mask &= ~1u;
                if (!b_l || v >= W) flag |= 2;                  // the start row in a column > 0, or a word the graph has not
            }
            if (__ballot(hop)) {                                // (wave-uniform) the hit table: lane w learns whether some hopper names w
                // (relaxed atomics and fences of wavefront scope: ds_write_b8, ds_write_b8, ds_read_u8 in this order, no
                //  barrier and no wait on the rows in flight)
                __hip_atomic_store(&hit[lane], (uint8_t)0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT);
                __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
                if (hop) __hip_atomic_store(&hit[v], (uint8_t)1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT);   // (v < W <= 64: inside the table)
                __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
                if (__hip_atomic_load(&hit[lane], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT)) mask |= 1u << (N - 1);
                __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
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

// One path, lane = stream: online_bigram_segment_kernel over the wide layout.  Commit mode (a.cand): from the new anchor
// (visited) down to the old one; tail mode: from the chosen end of the newest column (not visited) down to the anchor; without
// an anchor the walk ends in column 0.  The run of labelled rows the anchor lies in belongs to the settled side, so the label
// pending on arrival is dropped, and with TIMED its column with it.  rp is the ring position of column j and follows it down.
template <int N, bool SKIP, bool TIMED>
__global__ __launch_bounds__(64) void online_bigram_wide_segment_kernel(gh_settle_args a, const gh_bigram_wide* __restrict__ bgw) {
    constexpr int HB = gh_bigram_wide_hb(N, SKIP);
    constexpr uint32_t HBM = (uint32_t)((1ull << HB) - 1ull);
    __shared__ uint8_t s_arcs[GH_LAYERS_MAXW * GH_LAYERS_MAXN];
    __shared__ uint64_t s_in[GH_LAYERS_MAXW];
    const gh_layerform* __restrict__ lf = a.lf;
    for (int k = threadIdx.x; k < GH_LAYERS_MAXW * GH_LAYERS_MAXN; k += 64) s_arcs[k] = (&lf->arcs[0][0])[k];
    s_in[threadIdx.x] = bgw->bg_in[threadIdx.x];                // (64 lanes, GH_LAYERS_MAXW = 64 masks)
    static_assert(GH_LAYERS_MAXW == 64, "one arc mask per lane");
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
    int prev_label = -1, kind = 0, flag = 0;                    // kind 0: emitting (bw, bs); 1: entry row of word bw
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
        const uint32_t hb = bpu[(int64_t)rp * 64 + bw] & HBM;
        if (kind == 1) {                                        // entry row of word bw: the recorded predecessor word
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
            if (!((arcs >> code) & 1)) code = (arcs & 4) ? 2 : (arcs & 2) ? 1 : (arcs & 1) ? 0 : -1;
            if (code < 0) { flag |= 2; break; }
            bs -= code;
            down();
            visit(row_of(bw, bs), j);
        } else {
            // candidates in ascending origin order: start row (arcs bit4), entry row (bit3), self (bit0)
            const int b_l = (hb >> 1) & 1, b_s = hb & 1;
            int pick = b_s ? 0 : (b_l ? 3 : 4);
            if (!((arcs >> pick) & 1)) pick = (arcs & 16) ? 4 : (arcs & 8) ? 3 : (arcs & 1) ? 0 : -1;
            if (pick == 0) { down(); visit(row_of(bw, 0), j); }
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

int gh_launch_online_bigram_wide_settle(gh_ctx* ctx, const gh_online* on, const gh_settle_args& a, bool settle, const char* who) {
    if (a.n <= 0) return GH_OK;
    const gh_layerform& f = on->lat->h_layers;
    const gh_bigram_wide* wide = on->lat->d_bigram_wide;
    GH_REQUIRE(wide, "%s: internal: wide bigram form without its cost table", who);
    const dim3 blk(64);
    const dim3 grid((unsigned)(settle ? a.n : (a.n + 63) / 64));
#define GH_STBW(ET, NN, SK)                                                                                                      \
    do {                                                                                                                         \
        if (settle) hipLaunchKernelGGL((online_bigram_wide_settle_kernel<NN, SK>), grid, blk, 0, ctx->stream, a);                \
        else if (a.begins) hipLaunchKernelGGL((online_bigram_wide_segment_kernel<NN, SK, true>), grid, blk, 0, ctx->stream, a, wide); \
        else hipLaunchKernelGGL((online_bigram_wide_segment_kernel<NN, SK, false>), grid, blk, 0, ctx->stream, a, wide);         \
    } while (0)
    GH_NSKIP_SWITCH(f.N, f.skip, 8, GH_STBW, , "%s: wide bigram form with %d states per word", who, f.N)
#undef GH_STBW
    GH_HIP(hipGetLastError());
    return GH_OK;
}
