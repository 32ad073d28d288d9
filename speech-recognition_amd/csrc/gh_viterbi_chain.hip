// Viterbi for left-to-right chains (isolated word models, stacked side by side): every arc of
// row r comes from r, r-1 or r-2, no non-emitting rows.  Same semantics as the generic kernel
// (reference: decode_hmm_states, sr/recognition/decode.py:80-146, as HMM.evaluate uses it,
// hmm.py:126-135): candidates in ascending origin order (r-2, r-1, r) with a strict '<', start
// cells only in column 0, +inf elsewhere in column 0.
//
// gfx950 mapping: ONE WAVE per (utterance, group of <= 64 consecutive rows holding whole chains).
// The cost column lives in one VGPR pair per lane; the neighbour's previous cost arrives by a
// DPP wave shift (no LDS, no barrier); the lane's emission stream nll[t, state(row)] is a
// strided walk through the resident [N,S] matrix, prefetched PF columns ahead in a register
// ring.  A column is ~15 VALU instructions, so the kernel runs at the rate HBM delivers the
// likelihood matrix.  Back-pointers are 1 byte per cell (which of the three arcs won).
#include <stdlib.h>
#include <string.h>
#include "gh_internal.h"
#include "gh_viterbi.h"
#include "gh_wave.h"

namespace {

constexpr int PF = 8;  // emission prefetch depth (columns)
// The lane = chain form exists with two ring depths (template parameter LPF): PF, and the shallow ring LANE_PF with which
// the headline instantiation is allocated 80 registers and fits beside two likelihood waves (see the kernel).
#ifndef GH_VL_PF
#define GH_VL_PF 2
#endif
constexpr int LANE_PF = GH_VL_PF;

template <typename ET, bool WANT_BP, bool WANT_COSTS, bool SKIP>
__global__ __launch_bounds__(64) void viterbi_chain_kernel(gh_chain_args a) {
    const int lane = threadIdx.x;
    const int64_t slot = a.slot0 + blockIdx.x / a.n_groups;
    const int g = blockIdx.x % a.n_groups;
    const int64_t u = a.perm ? a.perm[slot] : slot;
    const int r0 = a.group_row0[g];
    const int nrows = a.group_row0[g + 1] - r0;
    const int r = r0 + lane;
    const bool act = lane < nrows;
    const int64_t f0 = a.utt_off[u];
    const int T = (int)(a.utt_off[u + 1] - f0);
    const int S = a.S, R = a.R;
    const double INF = INFINITY;
    if (T <= 0) return;

    // per-lane row constants
    const int rr = act ? r : r0;
    const double c0 = act ? a.cost0[rr] : INF;   // self arc        (+inf = absent)
    const double c1 = act ? a.cost1[rr] : INF;   // arc from r-1
    const double c2 = (SKIP && act) ? a.cost2[rr] : INF;  // arc from r-2
    const uint8_t info = act ? a.row_info[rr] : 0x0F;     // bits 0-1 first arc code (3 = none), bit 2 start row
    const uint8_t first_code = info & 3;
    const bool is_start = (info & 4) != 0;
    const ET* ep = static_cast<const ET*>(a.nll) + f0 * S + (act ? a.row_state[rr] : 0);

    ET ring[PF];
#pragma unroll
    for (int k = 0; k < PF; ++k) ring[k] = (k < T) ? ep[(int64_t)k * S] : ET(0);
    ep += (int64_t)PF * S;

    double prev = INF;
    uint8_t* bp = WANT_BP ? a.bp + a.bp_off[slot] + rr : nullptr;
    double* co = WANT_COSTS ? a.costs + a.costs_off[u] + (int64_t)rr * T : nullptr;

    auto column = [&](int t, ET ev) {
        const double e = (double)ev;
        const double p1 = wave_shr1(prev, INF);
        double best = INF;
        uint8_t code = first_code;
        if (SKIP) {
            const double p2 = wave_shr1(p1, INF);
            const double v2 = c2 + p2;
            if (v2 < best) { best = v2; code = 2; }
        }
        const double v1 = c1 + p1;
        if (v1 < best) { best = v1; code = 1; }
        const double v0 = c0 + prev;
        if (v0 < best) { best = v0; code = 0; }
        double c = best + e;
        c = (c != c) ? INF : c;                      // min(inf, nan) keeps inf (decode.py:124)
        if (first_code == 3) c = INF;                // row without arcs stays +inf (decode.py:116-117)
        if (t == 0 && is_start) { c = e; code = 3; } // decode.py:99-101
        prev = c;
        if (WANT_BP && act) { *bp = code; bp += R; }
        if (WANT_COSTS && act) { *co = c; co += 1; }
    };

    int t = 0;
    for (; t + PF <= T; t += PF) {
#pragma unroll
        for (int k = 0; k < PF; ++k) {
            const ET ev = ring[k];
            ring[k] = (t + k + PF < T) ? ep[(int64_t)k * S] : ET(0);
            column(t + k, ev);
        }
        ep += (int64_t)PF * S;
    }
#pragma unroll
    for (int k = 0; k < PF; ++k)
        if (t + k < T) column(t + k, ring[k]);

    // end costs: every end row knows its slot in the graph's end list
    if (act) {
        const int es = a.end_slot[rr];
        if (es >= 0) a.end_cost[u * a.n_end + es] = prev;
    }
}

// ---- lane = chain form: graphs whose chains all have N rows (gh_lattices::chain_unit; stacked word models) ----
// ONE LANE walks one chain: its N previous costs, arc costs and row flags live in registers, the predecessors of a row
// are the lane's own registers (no DPP shift, no idle lanes inside an utterance).  A wave holds floor(64 / chains per
// utterance) whole utterances from consecutive launch slots (perm sorts by length: nearly equal); a lane whose utterance
// has ended stops updating.  More than 64 chains per utterance: several waves per utterance.  The lane reads its N
// consecutive emissions nll[t, state(row0) .. +N-1] of a column into the same prefetch ring as above.
//
// Same results bit for bit as viterbi_chain_kernel.  With back-pointers the candidates are tried in the same order with
// the same strict '<'.  Without them the cell is min(min(c2+p2, c1+p1), c0+p0) + e in v_min_f64: the value of a minimum
// does not depend on the order of equal candidates, minNum drops a NaN candidate exactly as `v < best` does, and the
// `c != c -> +inf` rule is one more minimum against +inf.  A row without arcs has three +inf arc costs, so its cell is
// +inf (or NaN -> +inf) without a test of its own; an arc that would cross a chain boundary has cost +inf by the
// definition of a chain and is left out.  Column 0 (start rows take e, the others +inf) is peeled.
// SELECT (no back-pointers and the whole utterance in one wave): the end selection of chain_end_select_kernel happens
// here, on the end costs parked in LDS.
// chain_lanes_wave: what one wave does for position `wv` of the one-wave-per-group grid (s_end: 64 * N doubles of LDS when
// SELECT).  The kernel below calls it once (grid = every position) or in a strided loop (a capped grid).
template <typename ET, int N, bool WANT_BP, bool WANT_COSTS, bool SKIP, int LPF>
__device__ __forceinline__ void chain_lanes_wave(const gh_chain_args& a, const int64_t wv, double* s_end) {
    constexpr bool SELECT = !WANT_BP;
    const int lane = threadIdx.x;
    const int C = a.unit_chains;               // chains per utterance
    const bool one_wave = C <= 64;             // (then SELECT applies)
    int ul = 0, chain;
    int64_t slot;
    bool act;
    if (one_wave) {
        const int upw = 64 / C;
        ul = lane / C;
        chain = lane - ul * C;
        slot = a.slot0 + wv * upw + ul;
        act = ul < upw && slot < a.slot0 + a.n_slots;
        if (!act) { ul = 0; chain = 0; slot = a.slot0 + wv * upw; }   // an idle lane shadows lane 0: same loads, no stores
    } else {
        const int wpu = (C + 63) >> 6;
        slot = a.slot0 + wv / wpu;
        chain = (int)(wv % wpu) * 64 + lane;
        act = chain < C;
        if (!act) chain = 0;
    }
    const int64_t u = a.perm ? a.perm[slot] : slot;
    const int64_t f0 = a.utt_off[u];
    const int T = (int)(a.utt_off[u + 1] - f0);
    const int S = a.S, R = a.R;
    const int row0 = chain * N;
    const double INF = INFINITY;

    // the lane's row constants
    double c0[N], c1[N], c2[N];
    uint32_t info = 0;      // 3 bits per row: bits 0-1 code of the first arc (3 = none), bit 2 start row
#pragma unroll
    for (int i = 0; i < N; ++i) {
        c0[i] = a.cost0[row0 + i];
        c1[i] = i >= 1 ? a.cost1[row0 + i] : INF;
        c2[i] = (SKIP && i >= 2) ? a.cost2[row0 + i] : INF;
        info |= (uint32_t)(a.row_info[row0 + i] & 7) << (3 * i);
    }
    const ET* ep = static_cast<const ET*>(a.nll) + f0 * S + a.row_state[row0];

    // wave-uniform bounds of the lanes' lengths: the loop without guards runs while every lane is inside its utterance
    int tmin = T, tmax = T;
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
        tmin = min(tmin, __shfl_xor(tmin, m, 64));
        tmax = max(tmax, __shfl_xor(tmax, m, 64));
    }
    tmin = __builtin_amdgcn_readfirstlane(tmin);
    tmax = __builtin_amdgcn_readfirstlane(tmax);

    double prev[N];
    uint8_t* bp = WANT_BP ? a.bp + a.bp_off[slot] + row0 : nullptr;
    double* co = WANT_COSTS ? a.costs + a.costs_off[u] + (int64_t)row0 * T : nullptr;

    // column 0
    if (T > 0) {
#pragma unroll
        for (int i = 0; i < N; ++i) {
            const bool is_start = (info >> (3 * i + 2)) & 1;
            prev[i] = is_start ? (double)ep[i] : INF;      // decode.py:99-101
            if (WANT_BP && act) bp[i] = is_start ? 3 : (info >> (3 * i)) & 3;
            if (WANT_COSTS && act) co[(int64_t)i * T] = prev[i];
        }
        if (WANT_BP) bp += R;
        if (WANT_COSTS) co += 1;
    } else {
#pragma unroll
        for (int i = 0; i < N; ++i) prev[i] = INF;
    }

    ET ring[LPF][N];
    const ET* lp = ep + S;

    auto column = [&](const ET (&ev)[N]) {
#pragma unroll
        for (int i = N - 1; i >= 0; --i) {          // descending: prev[i-1], prev[i-2] are still the previous column's
            const double e = (double)ev[i];
            double c;
            if (WANT_BP) {
                double best = INF;
                uint32_t code = (info >> (3 * i)) & 3;
                if (SKIP && i >= 2) {
                    const double v2 = c2[i] + prev[i - 2];
                    if (v2 < best) { best = v2; code = 2; }
                }
                if (i >= 1) {
                    const double v1 = c1[i] + prev[i - 1];
                    if (v1 < best) { best = v1; code = 1; }
                }
                const double v0 = c0[i] + prev[i];
                if (v0 < best) { best = v0; code = 0; }
                c = best + e;
                c = (c != c) ? INF : c;                  // min(inf, nan) keeps inf (decode.py:124)
                if (act) bp[i] = (uint8_t)code;
            } else {
                double m = c0[i] + prev[i];
                if (i >= 1) {
                    double m1 = c1[i] + prev[i - 1];
                    if (SKIP && i >= 2) m1 = vmin(c2[i] + prev[i - 2], m1);
                    m = vmin(m1, m);
                }
                c = vmin(m + e, INF);
            }
            prev[i] = c;
            if (WANT_COSTS && act) co[(int64_t)i * T] = c;
        }
        if (WANT_BP) bp += R;
        if (WANT_COSTS) co += 1;
    };

    // The loop without guards has its own ring fill in front of it: reached over the guarded fill, the wait for a ring slot
    // at the top of the loop becomes a wait for every load in flight (the compiler cannot count loads behind branches).
    int t = 1;
#ifdef GH_VL_PRIO
    __builtin_amdgcn_s_setprio(3);
#endif
    if (1 + 2 * LPF <= tmin) {
#pragma unroll
        for (int k = 0; k < LPF; ++k) {
#pragma unroll
            for (int i = 0; i < N; ++i) ring[k][i] = lp[i];
            lp += S;
        }
        do {                                        // every lane: columns t .. t+LPF-1 exist, loads t+LPF .. t+2LPF-1 are inside
#pragma unroll
            for (int k = 0; k < LPF; ++k) {
                column(ring[k]);      // (consumed before the slot's refill is issued: the ring stays in its registers)
#pragma unroll
                for (int i = 0; i < N; ++i) ring[k][i] = lp[i];
                lp += S;
            }
            t += LPF;
        } while (t + 2 * LPF <= tmin);
    } else {
#pragma unroll
        for (int k = 0; k < LPF; ++k) {
#pragma unroll
            for (int i = 0; i < N; ++i) ring[k][i] = (1 + k < T) ? lp[i] : ET(0);
            lp += S;
        }
    }
    for (; t < tmax; t += LPF) {
#pragma unroll
        for (int k = 0; k < LPF; ++k) {
            if (t + k < T) column(ring[k]);
#pragma unroll
            for (int i = 0; i < N; ++i) ring[k][i] = (t + k + LPF < T) ? lp[i] : ET(0);
            lp += S;
        }
    }
#ifdef GH_VL_PRIO
    __builtin_amdgcn_s_setprio(0);
#endif

    // end costs: every end row knows its slot in the graph's end list
    if (T > 0) {
#pragma unroll
        for (int i = 0; i < N; ++i) {
            const int es = a.end_slot[row0 + i];
            if (act && es >= 0) {
                a.end_cost[u * a.n_end + es] = prev[i];
                if (SELECT && one_wave) s_end[ul * a.n_end + es] = prev[i];
            }
        }
    }
    if (SELECT && one_wave) {
        __syncthreads();
        if (act && chain == 0) {
            double best = INF;
            int bi = -1;
            if (T > 0)
                for (int k = 0; k < a.n_end; ++k) {
                    const double c = s_end[ul * a.n_end + k];
                    if (best >= c) { best = c; bi = k; }          // '>=': the last of equal minima (decode.py:129-134)
                }
            a.best_end[u] = bi;
            if (a.path_len) a.path_len[u] = 0;
        }
    }
}

// Registers of the headline instantiation (fp64, n = 5, no back-pointers, no skip arcs) with the shallow ring: a SIMD has
// 512, two waves of loglik_mfma_kernel<double,20,8> hold 2 x 216, so a decode wave of at most 80 starts beside them
// instead of waiting for one of them to retire and then keeping its successor out.  waves_per_eu(6) is that
// budget (512 / 6 -> 80); tools/headline_registers.py checks the sum and that nothing spills.  1 = the default.
template <typename ET, int N, bool WANT_BP, bool WANT_COSTS, bool SKIP, int LPF>
__global__ __launch_bounds__(64)
__attribute__((amdgpu_waves_per_eu((LPF == LANE_PF && sizeof(ET) == 8 && N == 5 && !WANT_BP && !SKIP) ? 6 : 1)))
void viterbi_chain_lanes_kernel(gh_chain_args a) {
    constexpr bool SELECT = !WANT_BP;
    __shared__ double s_end[SELECT ? 64 * N : 1];
    if (LPF != LANE_PF) {                   // "alone": the grid is every position (the walk below costs ~25 registers)
        chain_lanes_wave<ET, N, WANT_BP, WANT_COSTS, SKIP, LPF>(a, blockIdx.x, s_end);
        return;
    }
    for (int64_t wv = blockIdx.x; wv < a.n_lane_waves; wv += gridDim.x) {
        chain_lanes_wave<ET, N, WANT_BP, WANT_COSTS, SKIP, LPF>(a, wv, s_end);
        if (SELECT) __syncthreads();        // (the end selection has read s_end before the next position writes it)
    }
}

// End selection ('>=': the last of equal minima, decode.py:129-134) + back-trace of one utterance
// per wave; lane 0 walks the 1-byte back-pointers, the pairs are parked in LDS and flushed by
// the wave.
__global__ __launch_bounds__(64) void chain_backtrace_kernel(gh_chain_args a, int64_t u_begin) {
    __shared__ int32_t pbuf[2 * 256];
    __shared__ int s_n, s_i, s_j, s_len;
    const int lane = threadIdx.x;
    const int64_t slot = u_begin + blockIdx.x;
    const int64_t u = a.perm ? a.perm[slot] : slot;
    const int T = (int)(a.utt_off[u + 1] - a.utt_off[u]);
    const int R = a.R;
    if (lane == 0) {
        double best = INFINITY;
        int bi = -1;
        for (int k = 0; k < a.n_end; ++k) {
            const double c = a.end_cost[u * a.n_end + k];
            if (best >= c) { best = c; bi = k; }
        }
        if (T <= 0) bi = -1;
        a.best_end[u] = bi;
        s_i = bi >= 0 ? a.end_rows[bi] : 0;
        s_j = T - 1;
        s_len = 0;
        s_n = 0;
    }
    __syncthreads();
    if (!a.path || T <= 1 || a.best_end[u] < 0) {
        if (lane == 0 && a.path_len) a.path_len[u] = 0;
        return;
    }
    const uint8_t* bp = a.bp + a.bp_off[slot];
    int32_t* path = a.path + 2 * a.path_off[u];
    while (s_j != 0) {
        if (lane == 0) {
            int i = s_i, j = s_j, n = 0;
            while (j != 0 && n < 256) {
                const int code = bp[(int64_t)j * R + i];
                if (code == 3) { atomicOr(a.flag, 2); j = 0; break; }
                i -= code;
                --j;
                pbuf[2 * n] = i;
                pbuf[2 * n + 1] = j;
                ++n;
            }
            s_i = i; s_j = j; s_n = n;
        }
        __syncthreads();
        const int n = s_n, len = s_len;
        for (int k = lane; k < 2 * n; k += 64) path[2 * (int64_t)len + k] = pbuf[k];
        __syncthreads();
        if (lane == 0) s_len = len + n;
        __syncthreads();
    }
    if (lane == 0) a.path_len[u] = s_len;
}

}  // namespace

int gh_launch_viterbi_chain(gh_ctx* ctx, const gh_chain_args& a, int64_t u_begin, int64_t n_utts, bool f64,
                            bool want_bp, bool want_costs, bool skip) {
    if (n_utts <= 0) return GH_OK;
    gh_chain_args b = a;
    dim3 grid((unsigned)(n_utts * a.n_groups)), blk(64);
    b.slot0 = u_begin;  // perm[] and bp_off[] are indexed by absolute launch slot
#define GH_VC(ET, BP, CO, SK) hipLaunchKernelGGL((viterbi_chain_kernel<ET, BP, CO, SK>), grid, blk, 0, ctx->stream, b)
#define GH_VC_S(ET, BP, CO) do { if (skip) GH_VC(ET, BP, CO, true); else GH_VC(ET, BP, CO, false); } while (0)
#define GH_VC_T(ET) do { if (want_costs) GH_VC_S(ET, true, true); else if (want_bp) GH_VC_S(ET, true, false); else GH_VC_S(ET, false, false); } while (0)
    if (f64) GH_VC_T(double); else GH_VC_T(float);
#undef GH_VC_T
#undef GH_VC_S
#undef GH_VC
    GH_HIP(hipGetLastError());
    return GH_OK;
}

// Lane = chain form for chains of `unit` rows each (1 .. 8).  *selected: the kernel has written best_end itself (no
// back-pointers wanted and every utterance inside one wave), the end selection need not be launched.
bool gh_chain_lanes_ok(int unit) { return unit >= 1 && unit <= 8; }
int gh_launch_viterbi_chain_lanes(gh_ctx* ctx, const gh_chain_args& a, int unit, int64_t u_begin, int64_t n_utts, bool f64,
                                  bool want_bp, bool want_costs, bool skip, bool* selected) {
    if (selected) *selected = false;
    if (n_utts <= 0) return GH_OK;
    GH_REQUIRE(gh_chain_lanes_ok(unit) && a.R % unit == 0, "gh_viterbi: internal: chains of %d rows in the lane form", unit);
    gh_chain_args b = a;
    b.slot0 = u_begin;  // perm[] and bp_off[] are indexed by absolute launch slot
    b.n_slots = n_utts;
    b.unit_chains = a.R / unit;
    const int C = b.unit_chains;
    const int64_t n_waves = C <= 64 ? (n_utts + 64 / C - 1) / (64 / C) : n_utts * ((C + 63) / 64);
    b.n_lane_waves = n_waves;
    // Two forms of the launch.  "alone": the ring of PF columns and one wave per position.  "beside": the shallow ring and
    // at most one wave per SIMD, the waves walking the positions in a strided loop -- the form for a decode that runs
    // under another stream's likelihood kernel (two batches in flight): it starts in the registers two likelihood waves
    // leave free and never puts a second decode wave on a SIMD.  Measured at the headline's 1.5 waves per SIMD (DESIGN
    // section 6); taken from half a wave to two waves per SIMD, outside of that the launch stays as it was.
    // GMMHMM_CHAIN_FORM=alone|beside and GMMHMM_CHAIN_WAVES=n (the cap of "beside") override, both read at every call.
    const int64_t simds = 4 * (int64_t)(ctx->n_cu > 0 ? ctx->n_cu : 256);
    bool beside = 2 * n_waves > simds && n_waves <= 2 * simds;
    if (const char* e = getenv("GMMHMM_CHAIN_FORM")) beside = !strcmp(e, "beside") ? true : !strcmp(e, "alone") ? false : beside;
    int64_t cap = beside ? simds : n_waves;
    if (const char* e = getenv("GMMHMM_CHAIN_WAVES")) { const long v = atol(e); if (v > 0 && beside) cap = v; }
    dim3 grid((unsigned)(n_waves < cap ? n_waves : cap)), blk(64);
    if (const char* e = getenv("GMMHMM_HOST_TRACE"))
        if (atoi(e)) fprintf(stderr, "[gh_viterbi chain lanes] %s grid %u of %lld positions\n", beside ? "beside" : "alone", grid.x, (long long)n_waves);
    if (unit < 3) skip = false;   // (no r-2 arc inside a chain of two rows)
#define GH_VL_L(ET, NN, BP, CO, SK, LPF) hipLaunchKernelGGL((viterbi_chain_lanes_kernel<ET, NN, BP, CO, SK, LPF>), grid, blk, 0, ctx->stream, b)
#define GH_VL(ET, NN, BP, CO, SK) do { if (beside) GH_VL_L(ET, NN, BP, CO, SK, LANE_PF); else GH_VL_L(ET, NN, BP, CO, SK, PF); } while (0)
#define GH_VL_S(ET, NN, BP, CO) do { if (NN >= 3 && skip) GH_VL(ET, NN, BP, CO, (NN >= 3)); else GH_VL(ET, NN, BP, CO, false); } while (0)
#define GH_VL_T(ET, NN) do { if (want_costs) GH_VL_S(ET, NN, true, true); else if (want_bp) GH_VL_S(ET, NN, true, false); else GH_VL_S(ET, NN, false, false); } while (0)
#define GH_VL_N(ET) switch (unit) { case 1: GH_VL_T(ET, 1); break; case 2: GH_VL_T(ET, 2); break; case 3: GH_VL_T(ET, 3); break; \
                                    case 4: GH_VL_T(ET, 4); break; case 5: GH_VL_T(ET, 5); break; case 6: GH_VL_T(ET, 6); break; \
                                    case 7: GH_VL_T(ET, 7); break; default: GH_VL_T(ET, 8); break; }
    if (f64) GH_VL_N(double) else GH_VL_N(float)
#undef GH_VL_N
#undef GH_VL_T
#undef GH_VL_S
#undef GH_VL
#undef GH_VL_L
    GH_HIP(hipGetLastError());
    if (selected) *selected = !want_bp && !want_costs && C <= 64;
    return GH_OK;
}

// No path wanted: the end selection alone, one LANE per utterance (chain_backtrace_kernel spends a workgroup per utterance on
// it: 45 us per 10 000 utterances of the headline step, all of it workgroup starts)
__global__ void chain_end_select_kernel(gh_chain_args a, int64_t u_begin, int64_t n_utts) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_utts) return;
    const int64_t slot = u_begin + i;
    const int64_t u = a.perm ? a.perm[slot] : slot;
    const int T = (int)(a.utt_off[u + 1] - a.utt_off[u]);
    double best = INFINITY;
    int bi = -1;
    for (int k = 0; k < a.n_end; ++k) {
        const double c = a.end_cost[u * a.n_end + k];
        if (best >= c) { best = c; bi = k; }                  // '>=': the last of equal minima (decode.py:129-134)
    }
    a.best_end[u] = T <= 0 ? -1 : bi;
    if (a.path_len) a.path_len[u] = 0;
}

int gh_launch_chain_backtrace(gh_ctx* ctx, const gh_chain_args& a, int64_t u_begin, int64_t n_utts) {
    if (n_utts <= 0) return GH_OK;
    if (!a.path) {
        hipLaunchKernelGGL(chain_end_select_kernel, dim3((unsigned)((n_utts + 255) / 256)), dim3(256), 0, ctx->stream, a, u_begin, n_utts);
        GH_HIP(hipGetLastError());
        return GH_OK;
    }
    hipLaunchKernelGGL(chain_backtrace_kernel, dim3((unsigned)n_utts), dim3(64), 0, ctx->stream, a, u_begin);
    GH_HIP(hipGetLastError());
    return GH_OK;
}
