// FORWARD SCORES of stacked word chains (gh_chain_forward, gh_wordstream_create_soft / _result_soft): soft[u, w] = -log P(x_u | w)
// summed over ALL paths of word w's chain, the sum-product twin of the carried lane = chain Viterbi sweep
// (viterbi_chain_online_kernel, gh_viterbi_chain_online.hip).  NOT IN THE REFERENCE; the CPU restatement's forward_backward on one
// chain with its end row is the statement.  A word chain needs no backward sweep for its log P, and a forward column depends on
// the previous column only: a stream is described by ONE more column, [stream][N][C] log-alphas (fp64 for fp32 likelihoods too).
//
// Log domain, fp64, the file compiled without contraction; a[] = the previous column:
//   column 0:                       a[s] = start row ? -e[s][0] : -inf
//   column t, s descending, in place: a[s] = LSE(a[s-2] - c2[s], a[s-1] - c1[s], a[s] - c0[s]) - e[s][t]
//   LSE(x..) = m + log(sum exp(x - m)), m = max, the sum in the order written; m = -inf gives -inf, never NaN
// An arc that does not exist costs +inf: its term is -inf and adds exp(-inf) = 0.  The log P of a chain is the cell of its end
// row in the last column; no path gives -inf, i.e. soft = +inf.
//
// gfx950 mapping: that of viterbi_chain_online_kernel -- lane = chain, its N log-alphas and arc costs in registers; C <= 64:
// 64 / C consecutive slots per wave, C > 64: ceil(C / 64) waves per slot; idle lanes shadow lane 0 (same loads, no stores); every
// load outside the unguarded run is guarded by the lane's own count; a lane whose chunk has ended stops updating; a slot whose
// ABSOLUTE column is 0 does not read the state buffer.  No LDS, no atomics.  Every log-sum-exp is per lane and written
// select-style (no branch on its maximum); the only cross-lane step is the wave-uniform bound of the column counts in front of
// the loops.  Per column and lane at N = 5 without skip arcs: 8 exp and 4 log of the device library (11 and 4 with skip arcs;
// state 0 has one term and needs neither) against 15 add / min of the Viterbi sweep: instruction bound, not HBM bound.
//
// ONE KERNEL serves both hosts: gh_chain_forward pushes every whole utterance onto a fresh slot (absolute column 0, count = T)
// of a temporary [U][N][C] buffer, a soft session pushes chunks onto its own column.  Carried == one-shot therefore holds
// bitwise.  NOT BUILT: a fused sweep that computes the cost column and the log-alpha column from one read of the emissions; the
// extended-exponent arithmetic of fb_seq_kernel (gh_seq.hip) in place of exp / log per term.
#include "gh_wordstream.h"
#include "gh_viterbi.h"
#include "gh_wave.h"

namespace {

constexpr int PF = 8;  // emission prefetch depth (columns), as the Viterbi sweep

// log-sum-exp inside a lane, terms in ascending origin (the order of the host statement).  Select-style: with m = -inf the
// terms are compared against 0 instead, every exp() is 0, log(0) = -inf and 0 + -inf = -inf (never -inf - -inf)
__device__ __forceinline__ double lse_ref(double m) { return (m == -INFINITY) ? 0.0 : m; }
__device__ __forceinline__ double lse2(double x, double y) {
    const double m = lse_ref(vmax(x, y));
    return m + log(exp(x - m) + exp(y - m));
}
__device__ __forceinline__ double lse3(double x, double y, double z) {
    const double m = lse_ref(vmax(vmax(x, y), z));
    return m + log((exp(x - m) + exp(y - m)) + exp(z - m));
}

template <typename ET, int N, bool SKIP>
__global__ __launch_bounds__(64) void forward_chain_kernel(gh_wordstream_args a) {
    const int lane = threadIdx.x;
    const int C = a.C;
    int chain;
    int64_t slot;
    bool act;
    if (C <= 64) {
        const int spw = 64 / C;
        const int k = lane / C;
        chain = lane - k * C;
        slot = (int64_t)blockIdx.x * spw + k;
        act = k < spw && slot < a.n_slots;
        if (!act) { chain = 0; slot = (int64_t)blockIdx.x * spw; }   // an idle lane shadows lane 0: same loads, no stores
    } else {
        const int wps = (C + 63) >> 6;
        slot = blockIdx.x / wps;
        chain = (blockIdx.x % wps) * 64 + lane;
        act = chain < C;
        if (!act) chain = 0;
    }
    const gh_online_slot sl = a.slots[slot];
    const int S = a.S;
    const int row0 = chain * N;
    const double INF = INFINITY, NEG = -INFINITY;
    const bool fresh = sl.t0 == 0;              // the chunk starts at absolute column 0: column 0 is peeled below
    const int T = sl.count;
    const int Tl = T - ((fresh && T > 0) ? 1 : 0);   // columns of the chunk that take the ordinary step

    // the lane's row constants
    double c0[N], c1[N], c2[N];
    uint32_t start = 0;     // bit i: row i of the chain is a start row
#pragma unroll
    for (int i = 0; i < N; ++i) {
        c0[i] = a.cost0[row0 + i];
        c1[i] = i >= 1 ? a.cost1[row0 + i] : INF;
        c2[i] = (SKIP && i >= 2) ? a.cost2[row0 + i] : INF;
        start |= (uint32_t)((a.row_info[row0 + i] >> 2) & 1) << i;
    }
    // first row of the slot ([row0, row0 + count) of the matrix are the only rows this lane reads)
    const ET* ep = static_cast<const ET*>(a.nll) + sl.row0 * (int64_t)S + a.row_state[row0];

    // wave-uniform bounds of the lanes' column counts: the loop without guards runs while every lane is inside its chunk
    // (EXEC is full here: the one cross-lane step of the kernel)
    int tmin = Tl, tmax = Tl;
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
        tmin = min(tmin, __shfl_xor(tmin, m, 64));
        tmax = max(tmax, __shfl_xor(tmax, m, 64));
    }
    tmin = __builtin_amdgcn_readfirstlane(tmin);
    tmax = __builtin_amdgcn_readfirstlane(tmax);

    // the carried column; a stream at column 0 (fresh or reset) starts like the one-shot call and reads no state
    double* st = a.state + ((int64_t)sl.stream * N) * C + chain;
    double al[N];
    const ET* lp = ep;
    if (fresh) {
        if (T > 0) {
#pragma unroll
            for (int i = 0; i < N; ++i) al[i] = ((start >> i) & 1) ? -(double)ep[i] : NEG;
            lp = ep + S;
        } else {
#pragma unroll
            for (int i = 0; i < N; ++i) al[i] = NEG;
        }
    } else {
#pragma unroll
        for (int i = 0; i < N; ++i) al[i] = st[(int64_t)i * C];
    }

    ET ring[PF][N];

    auto column = [&](const ET (&ev)[N]) {
#pragma unroll
        for (int i = N - 1; i >= 0; --i) {          // descending: al[i-1], al[i-2] are still the previous column's
            const double e = (double)ev[i];
            const double t0 = al[i] - c0[i];
            double r = t0;                          // (the log-sum-exp of one term is the term)
            if (i >= 1) {
                const double t1 = al[i - 1] - c1[i];
                if (SKIP && i >= 2) r = lse3(al[i - 2] - c2[i], t1, t0);
                else r = lse2(t1, t0);
            }
            al[i] = r - e;
        }
    };

    // As in the Viterbi sweep the loop without guards has its own ring fill in front of it.  `t` counts the columns of
    // the lane's own run lp[0 .. Tl): every load below is at a column < Tl of that run, i.e. inside the slot's rows.
    int t = 0;
    if (2 * PF <= tmin) {
#pragma unroll
        for (int k = 0; k < PF; ++k) {
#pragma unroll
            for (int i = 0; i < N; ++i) ring[k][i] = lp[i];
            lp += S;
        }
        do {                                        // every lane: columns t .. t+PF-1 exist, loads t+PF .. t+2PF-1 are inside
#pragma unroll
            for (int k = 0; k < PF; ++k) {
                column(ring[k]);
#pragma unroll
                for (int i = 0; i < N; ++i) ring[k][i] = lp[i];
                lp += S;
            }
            t += PF;
        } while (t + 2 * PF <= tmin);
    } else {
#pragma unroll
        for (int k = 0; k < PF; ++k) {
#pragma unroll
            for (int i = 0; i < N; ++i) ring[k][i] = (k < Tl) ? lp[i] : ET(0);
            lp += S;
        }
    }
    for (; t < tmax; t += PF) {
#pragma unroll
        for (int k = 0; k < PF; ++k) {
            if (t + k < Tl) column(ring[k]);        // (a lane whose chunk has ended stops updating)
#pragma unroll
            for (int i = 0; i < N; ++i) ring[k][i] = (t + k + PF < Tl) ? lp[i] : ET(0);
            lp += S;
        }
    }

    if (!act || T <= 0) return;                     // (a stream that sat the tick out keeps its state)
#pragma unroll
    for (int i = 0; i < N; ++i) st[(int64_t)i * C] = al[i];
}

// soft[i, end] = -(the log-alpha of the end's row in the carried column of stream ids[i]) (ids null: stream i), gathered
// through the chain form's end slots like wordstream_result_kernel gathers costs.  No frames: +inf.  One lane per stream.
__global__ __launch_bounds__(64) void chain_soft_result_kernel(const int32_t* __restrict__ end_slot, int n_end, int N, int C,
                                                               const double* __restrict__ alpha, const int64_t* __restrict__ ids,
                                                               const int64_t* __restrict__ frames, int64_t n,
                                                               double* __restrict__ soft) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int64_t stream = ids ? ids[i] : i;
    const bool any = frames[i] > 0;
    double* out = soft + i * n_end;
    for (int c = 0; c < C; ++c)
        for (int s = 0; s < N; ++s) {
            const int es = end_slot[c * N + s];
            if (es >= 0) out[es] = any ? -alpha[(stream * N + s) * C + c] : INFINITY;
        }
}

}  // namespace

int gh_launch_forward_chain(gh_ctx* ctx, const gh_wordstream_args& a, int N, bool skip, bool f64) {
    const int C = a.C;
    const int64_t n_waves = C <= 64 ? (a.n_slots + 64 / C - 1) / (64 / C) : a.n_slots * ((C + 63) / 64);
    const dim3 grid((unsigned)n_waves), blk(64);
    if (N < 3) skip = false;   // (no r-2 arc inside a chain of two rows)
#define GH_FC(ET, NN, SK) hipLaunchKernelGGL((forward_chain_kernel<ET, NN, SK>), grid, blk, 0, ctx->stream, a)
#define GH_FC_S(ET, NN) do { if (NN >= 3 && skip) GH_FC(ET, NN, (NN >= 3)); else GH_FC(ET, NN, false); } while (0)
#define GH_FC_N(ET) switch (N) { case 1: GH_FC_S(ET, 1); break; case 2: GH_FC_S(ET, 2); break; case 3: GH_FC_S(ET, 3); break; \
                                 case 4: GH_FC_S(ET, 4); break; case 5: GH_FC_S(ET, 5); break; case 6: GH_FC_S(ET, 6); break; \
                                 case 7: GH_FC_S(ET, 7); break; default: GH_FC_S(ET, 8); break; }
    if (f64) GH_FC_N(double) else GH_FC_N(float)
#undef GH_FC_N
#undef GH_FC_S
#undef GH_FC
    GH_HIP(hipGetLastError());
    return GH_OK;
}

// The gather of n streams into host `soft` [n, n_end]: ids [n] (null: 0 .. n - 1) and frames [n] travel in one upload to d_ids
// [2 n], the result comes back through d_soft [n, n_end] (both carved by the caller, with everything else of its call: the
// context's scratch moves when it grows).  Synchronises.
static int soft_gather(gh_ctx* ctx, const gh_lattices* lat, int N, int C, const double* d_alpha, int64_t n, const int64_t* ids,
                       const int64_t* frames, int64_t* d_ids, double* d_soft, double* soft) {
    const int n_end = lat->lat[0].n_end;
    hipStream_t st = ctx->stream;
    std::vector<int64_t> h((size_t)2 * n);
    for (int64_t i = 0; i < n; ++i) {
        h[(size_t)i] = ids ? ids[i] : i;
        h[(size_t)(n + i)] = frames[i];
    }
    if (n_end > 0) {
        GH_HIP(hipMemcpyAsync(d_ids, h.data(), (size_t)2 * n * 8, hipMemcpyHostToDevice, st));
        hipLaunchKernelGGL(chain_soft_result_kernel, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, st, lat->d_ch_end_slot, n_end, N, C,
                           d_alpha, d_ids, d_ids + n, n, d_soft);
        GH_HIP(hipGetLastError());
        GH_HIP(hipMemcpyAsync(soft, d_soft, (size_t)n * n_end * 8, hipMemcpyDeviceToHost, st));
    }
    GH_HIP(hipStreamSynchronize(st));
    return GH_OK;
}

// --------------------------------------------------------------------------------------------------------------- C ABI
extern "C" int gh_chain_forward(gh_ctx* ctx, const gh_lattices* lat, const gh_batch* b, double* out_soft) {
    GH_REQUIRE(ctx && lat && b, "gh_chain_forward: NULL argument");
    char why[96];
    gh_wordchain_refusal(lat, why, sizeof why);
    if (why[0]) {
        gh_set_error("gh_chain_forward: the forward scores take one graph of word chains of equal length (1 .. 8 consecutive "
                     "states each), not %s", why);
        return GH_ERR_UNSUPPORTED;
    }
    const int64_t U = b->U;
    if (U == 0) return GH_OK;
    GH_REQUIRE(out_soft, "gh_chain_forward: out_soft is NULL");
    GH_REQUIRE(b->nll, "gh_chain_forward: gh_loglik has not been run on this batch");
    GH_REQUIRE(lat->lat[0].max_state < b->nll_S, "gh_chain_forward: the graph uses state %d but the model has %d", lat->lat[0].max_state,
               b->nll_S);
    const int N = lat->chain_unit, C = lat->lat[0].R / N;
    // every whole utterance is a push onto a fresh slot: absolute column 0, count = T, its column in a temporary buffer
    std::vector<gh_online_slot> slots;
    std::vector<int64_t> frames((size_t)U);
    slots.reserve((size_t)U);
    for (int64_t u = 0; u < U; ++u) {
        const int64_t Tu = b->offsets[u + 1] - b->offsets[u];
        GH_REQUIRE(Tu <= 0x7fffffff, "gh_chain_forward: an utterance of %lld frames", (long long)Tu);
        frames[(size_t)u] = Tu;
        if (Tu == 0) continue;
        gh_online_slot s;
        s.row0 = b->offsets[u]; s.stream = (int32_t)u; s.count = (int32_t)Tu; s.t0 = 0; s.pad = 0;
        slots.push_back(s);
    }
    GH_REQUIRE(U <= 0x7fffffff, "gh_chain_forward: %lld utterances", (long long)U);
    GH_HIP(hipSetDevice(ctx->device));
    // longest first: the slots of a wave then end close to each other
    std::stable_sort(slots.begin(), slots.end(), [](const gh_online_slot& x, const gh_online_slot& y) { return x.count > y.count; });
    // the gather's pieces lie behind the column buffer in ONE carve: the scratch must not move between the two kernels
    const int n_end = lat->lat[0].n_end;
    double* d_alpha;
    gh_online_slot* d_slots;
    int64_t* d_ids;
    double* d_soft;
    Carver cv;
    cv.add(&d_alpha, (size_t)U * N * C); cv.add(&d_slots, slots.size() + 1); cv.add(&d_ids, (size_t)2 * U);
    cv.add(&d_soft, (size_t)U * std::max(n_end, 1));
    const int rc0 = cv.commit(ctx);
    if (rc0) return rc0;
    hipStream_t st = ctx->stream;
    if (!slots.empty()) {
        GH_HIP(hipMemcpyAsync(d_slots, slots.data(), slots.size() * sizeof(gh_online_slot), hipMemcpyHostToDevice, st));
        gh_wordstream_args a = gh_wordchain_args(lat, b);
        a.slots = d_slots; a.n_slots = (int64_t)slots.size(); a.state = d_alpha;
        const int rc = gh_launch_forward_chain(ctx, a, N, lat->chain_skip, b->dtype == GH_F64);
        if (rc) return rc;
    }
    return soft_gather(ctx, lat, N, C, d_alpha, U, nullptr, frames.data(), d_ids, d_soft, out_soft);   // (`slots` is pageable: synchronised)
}

extern "C" int gh_wordstream_result_soft(gh_ctx* ctx, gh_wordstream* ws, int64_t n, const int64_t* ids, double* soft) {
    GH_REQUIRE(ctx && ws, "gh_wordstream_result_soft: NULL argument");
    GH_REQUIRE(ctx == ws->ctx, "gh_wordstream_result_soft: the session belongs to another context");
    GH_REQUIRE(ws->d_alpha, "gh_wordstream_result_soft: the session carries no forward column (it was not made by gh_wordstream_create_soft)");
    if (!ids) n = ws->n_streams;
    if (n <= 0) return GH_OK;
    GH_REQUIRE(soft, "gh_wordstream_result_soft: soft is NULL");
    std::vector<int64_t> fr((size_t)n);
    for (int64_t i = 0; i < n; ++i) {
        const int64_t id = ids ? ids[i] : i;
        GH_REQUIRE(id >= 0 && id < ws->n_streams, "gh_wordstream_result_soft: stream %lld out of range [0, %lld)", (long long)id,
                   (long long)ws->n_streams);
        fr[(size_t)i] = ws->frames[(size_t)id];
    }
    GH_HIP(hipSetDevice(ctx->device));
    int64_t* d_ids;
    double* d_soft;
    Carver cv;
    cv.add(&d_ids, (size_t)2 * n); cv.add(&d_soft, (size_t)n * std::max(ws->lat->lat[0].n_end, 1));
    const int rc = cv.commit(ctx);
    if (rc) return rc;
    return soft_gather(ctx, ws->lat, ws->N, ws->C, ws->d_alpha, n, ids, fr.data(), d_ids, d_soft, soft);
}
