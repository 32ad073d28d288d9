// The FORCED COMMIT of an online stream (gh_online_force): bound the unsettled tail of a narrow loop session to M frames.
//
// gh_online_commit settles a prefix only where the traces of all live cells of the newest column happen to meet
// (gh_online_settle.hip).  A stream whose traces do not meet within its window can take no more frames.  Forcing makes them
// meet: with T frames taken and c* = T - 1 - M, let A be the cell in which the trace of the CHOSEN END (the end gh_online_tail
// reports: online_end_kernel's rule) arrives in column c*.  Every live cell of the newest column whose trace does not pass A
// is set to +inf in the carried column.  After that every live trace passes A, so the ordinary commit called next finds an
// anchor in a column >= c* and hands out the words by its own segment walk: the anchor logic stays in one place, and this
// kernel writes the carried column and nothing else -- no anchor, no history, no open word.  The chosen end passes A by
// construction, so the words of the same tick do not change; from the forced tick on the decode is the carried decode
// with those cells removed, no longer the one-shot decode of the prefix.
//
// online_force_kernel -- the mapping of online_settle_kernel: FOUR STREAMS PER WAVE, DPP row = stream, lane = word, the
// states of a word as a bit mask that is mapped through the lane's OWN decision word of a column.  Three phases, one launch:
//   1. BACK WALK, T - 1 -> c*: the settle walk's column step on a set of one cell, the chosen end.  "Arrives" and the tie rules
//      are that walk's (the LOOP branch of lattice_backtrace_kernel: the lowest word of the `cand == rm` bits).
//   2. FORWARD MARKING, c* + 1 -> T - 1: from {A}, the cells of column j whose trace arrives in a marked cell of column j - 1.
//      Non-first states: bit s is set iff bit s - code_s of the old mask is.  First state: self takes the old bit 0; the loop
//      row takes the NEW bit N - 1 of the lowest `cand == rm` lane (the same-column hop: the non-first states are mapped
//      first); the start row is never a descendant.
//   3. PRUNE: finite and not marked -> +inf, plain vector stores; the count per stream goes to `pruned`.
// Both loops take T - 1 - c* = M steps.  A trace that reaches the start row in a column > 0, or a loop hop without a
// `cand == rm` lane, sets flag 2 and ends that stream's walk without pruning it.  Every ballot and row reduction sits under
// wave-uniform control flow (the loops run while any row is active, and all lanes take every step); what a row does with the
// result depends on values that are the same in its 16 lanes.
// Nothing happens (pruned = 0) where T < 2, c* < 0, c* <= the old anchor's column, or the chosen end is +inf.
// Cost: a forced stream reads its unsettled decision words twice more, once down and once up, and writes at most 16 N doubles.
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

// the lanes of DPP row kk for which p holds, as bits 0 .. 15
__device__ __forceinline__ uint32_t row_ballot16(bool p, int kk) { return (uint32_t)(__ballot(p) >> (kk * 16)) & 0xffffu; }

// the decision code of state s >= 1 in the column bits hb: 0 self, 1 from s - 1, 2 from s - 2; `before`: bits consumed so far
template <int N, bool SKIP>
__device__ __forceinline__ int in_word_code(uint32_t hb, int s, int& before) {
    constexpr int HB = gh_loop_hb(N, SKIP);
    int code;
    if (SKIP && s >= 2) {
        const int b_a = (hb >> (HB - 1 - before)) & 1, b_b = (hb >> (HB - 2 - before)) & 1;
        code = b_b ? 0 : (b_a ? 1 : 2);
        before += 2;
    } else {
        code = ((hb >> (HB - 1 - before)) & 1) ? 0 : 1;
        before += 1;
    }
    return code;
}

template <int N, bool SKIP>
__global__ __launch_bounds__(64) void online_force_kernel(gh_force_args a) {
    constexpr int HB = gh_loop_hb(N, SKIP), CPW = gh_loop_cpw(N, SKIP);
    constexpr uint32_t HBM = (uint32_t)((1ull << HB) - 1ull);
    static_assert(CPW >= 1 && N <= 16, "decision bits of a column must fit one word, the states of a word one mask");
    const int lane = threadIdx.x, kk = lane >> 4, w = lane & 15;
    const int W = a.lf->W, Lr = a.lf->loop_row;
    const int64_t i = (int64_t)blockIdx.x * 4 + kk;
    const bool has = i < a.n;
    gh_settle_task tk;
    tk.stream = 0; tk.T = 0; tk.has_anchor = 0; tk.pad = 0;
    if (has) tk = a.tasks[i];
    int lo = -1;
    if (has && tk.has_anchor) lo = a.anchor[tk.stream].col;
    const int T = tk.T, cstar = T - 1 - a.max_tail;
    const int ring = a.ring_words;
    const double INF = INFINITY;
    const bool wact = has && T >= 2 && w < W;
    double* st = a.prev + ((int64_t)tk.stream * N) * 16 + w;
    // the newest column: the live cells of this word, and its best end (online_end_kernel: '>=', the last of equal minima)
    uint32_t live = 0;
    double best_v = INF;
    int best_slot = -1, best_s = 0;
    if (wact) {
#pragma unroll
        for (int s = 0; s < N; ++s) {
            const double v = st[s * 16];
            live |= (uint32_t)(v < INF) << s;
            const int es = a.end_slot[s == 0 ? Lr + 1 + w : 1 + w * (N - 1) + (s - 1)];
            if (es >= 0 && (v < best_v || (v == best_v && es > best_slot))) { best_v = v; best_slot = es; best_s = s; }
        }
    }
    const int own_slot = best_slot;
#pragma unroll
    for (int o = 8; o >= 1; o >>= 1) {
        const double ov = __shfl_xor(best_v, o);
        const int os = __shfl_xor(best_slot, o);
        if (ov < best_v || (ov == best_v && os > best_slot)) { best_v = ov; best_slot = os; }
    }
    // row-uniform from here: the task, and the row's best end in all its lanes
    const bool go = has && T >= 2 && cstar >= 0 && cstar > lo && best_slot >= 0 && best_v < INF;
    uint32_t mask = (go && wact && own_slot == best_slot) ? 1u << best_s : 0u;
    const uint32_t* hp = reinterpret_cast<const uint32_t*>(a.hist + (int64_t)tk.stream * a.hist_stride) + w;
    int j = T - 1;
    bool active = go && j > cstar;
    int ci = active ? j % CPW : 0, wr = active ? (j / CPW) % ring : 0, held = -1;
    uint32_t word = 0;
    bool bad = false;
    // ---- 1. the back walk: one column step j -> j - 1 through the decisions of column j (online_settle_kernel's step) ----
    while (__ballot(active)) {
        if (active && wr != held) { word = hp[(int64_t)wr * 16]; held = wr; }
        const uint32_t hb = (word >> ((CPW - 1 - ci) * HB)) & HBM;
        const bool b0 = mask & 1u, b_l = (hb >> 1) & 1u, b_s = hb & 1u;
        const uint32_t hops = row_ballot16(active && b0 && !b_s && b_l, kk);
        const uint32_t lost = row_ballot16(active && b0 && !b_s && !b_l, kk);      // the start row, in a column > 0
        const uint32_t eq = row_ballot16(active && w < W && ((hb >> 2) & 1u), kk);
        if (active && b0 && !b_s) mask &= ~1u;
        if (hops && eq && w == __ffs(eq) - 1) mask |= 1u << (N - 1);               // lowest word = lowest origin row (np.argmin)
        uint32_t nm = mask & 1u;
        int before = 0;
#pragma unroll
        for (int s = N - 1; s >= 1; --s) {
            const int code = in_word_code<N, SKIP>(hb, s, before);
            if ((mask >> s) & 1u) nm |= 1u << (s - code);
        }
        if (active) {
            mask = nm;
            --j;
            if (ci == 0) { ci = CPW - 1; wr = wr == 0 ? ring - 1 : wr - 1; } else --ci;
        }
        if (active && (lost || (hops && !eq))) { bad = true; active = false; }
        else if (active && j <= cstar) active = false;
    }
    // ---- 2. forward marking from {A}: column j - 1 -> j through the decisions of column j ----
    active = go && !bad && j < T - 1;
    while (__ballot(active)) {
        if (active) {
            ++j;
            if (ci == CPW - 1) { ci = 0; wr = wr + 1 == ring ? 0 : wr + 1; } else ++ci;
            if (wr != held) { word = hp[(int64_t)wr * 16]; held = wr; }
        }
        const uint32_t hb = (word >> ((CPW - 1 - ci) * HB)) & HBM;
        const bool b_l = (hb >> 1) & 1u, b_s = hb & 1u;
        uint32_t nm = 0;
        int before = 0;
#pragma unroll
        for (int s = N - 1; s >= 1; --s) {
            const int code = in_word_code<N, SKIP>(hb, s, before);
            nm |= ((mask >> (s - code)) & 1u) << s;
        }
        const uint32_t eq = row_ballot16(active && w < W && ((hb >> 2) & 1u), kk);
        const uint32_t last = row_ballot16(active && ((nm >> (N - 1)) & 1u), kk);
        const bool hop = eq && ((last >> (__ffs(eq) - 1)) & 1u);                   // the loop row's origin is marked
        if (b_s ? (mask & 1u) : (b_l && hop)) nm |= 1u;
        if (active && w < W) mask = nm;
        if (active && j >= T - 1) active = false;
    }
    // ---- 3. prune: alive and not a descendant of A ----
    int cnt = 0;
    if (go && !bad && wact) {
        const uint32_t kill = live & ~mask;
#pragma unroll
        for (int s = 0; s < N; ++s)
            if ((kill >> s) & 1u) st[s * 16] = INF;
        cnt = __popc(kill);
    }
    cnt = row_sum16(cnt);
    if (has && w == 0) a.pruned[i] = cnt;
    if (bad && w == 0) atomicOr(a.flag, 2);
}

}  // namespace

int gh_launch_online_loop_force(gh_ctx* ctx, const gh_online* on, const gh_force_args& a) {
    const gh_layerform& f = on->lat->h_layers;
    const dim3 blk(64);
    const dim3 grid((unsigned)((a.n + 3) / 4));
#define GH_FC(ET, NN, SK) hipLaunchKernelGGL((online_force_kernel<NN, SK>), grid, blk, 0, ctx->stream, a)
    GH_NSKIP_SWITCH(f.N, f.skip, 16, GH_FC, , "gh_online_force: loop form with %d states per word", f.N)
#undef GH_FC
    GH_HIP(hipGetLastError());
    return GH_OK;
}
