// ONLINE isolated-word recognition (gh_wordstream_*): the lane = chain sweep of gh_viterbi_chain.hip
// (viterbi_chain_lanes_kernel, in its form without back-pointers) CARRIED ACROSS CHUNKS of utterances that are still
// arriving.  HMM.evaluate (hmm.py:126-135) needs the cost of the last state in the last column only, and a column of
// decode_hmm_states (decode.py:80-146) depends on the previous column only, so a stream is fully described by
//   * the previous column of its C word chains of N states                       [stream][N][C] doubles (always fp64),
//   * the number of frames it has taken (host side: the absolute column of the next frame).
// There is no decision history: nothing grows with the length of a stream, which is why a session has no capacity.
//
// gfx950 mapping: as the lanes kernel -- lane = chain, its N costs and arc costs in registers; C <= 64: 64 / C consecutive
// slots of the push per wave, C > 64: ceil(C / 64) waves per slot; idle lanes shadow lane 0 (same loads, no stores); a
// lane whose chunk has ended stops updating.  The column step is a copy of the lanes kernel's !WANT_BP branch (same
// v_min_f64 tree, states in descending order), so the carried column is bitwise the one-shot column.  What differs is
// where `prev` comes from and goes to, and that the column-0 rule (start rows take their emission, all others +inf)
// applies where the ABSOLUTE column is 0: such a stream does not read the state buffer, so a reset clears nothing on
// the device.  A chunk moves 8 N C B of state in and out per stream beside its t N C emissions.
//
// ONE FRAME: a stream that holds exactly one frame shows column 0 of every longer decode.  The reference's one-frame
// decode is something else (its column wrap, decode.py:109-114, lets a row read the row above it in the same column)
// and is not reproduced; from two frames on the result is the whole decode of the frames so far.
#include "gh_wordstream.h"
#include "gh_viterbi.h"
#include "gh_wave.h"

namespace {

constexpr int PF = 8;  // emission prefetch depth (columns), as the one-shot sweep

template <typename ET, int N, bool SKIP>
__global__ __launch_bounds__(64) void viterbi_chain_online_kernel(gh_wordstream_args a) {
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
    const double INF = INFINITY;
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
    int tmin = Tl, tmax = Tl;
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
        tmin = min(tmin, __shfl_xor(tmin, m, 64));
        tmax = max(tmax, __shfl_xor(tmax, m, 64));
    }
    tmin = __builtin_amdgcn_readfirstlane(tmin);
    tmax = __builtin_amdgcn_readfirstlane(tmax);

    // the carried column; a stream at column 0 (fresh or reset) starts like the one-shot sweep and reads no state
    double* st = a.state + ((int64_t)sl.stream * N) * C + chain;
    double prev[N];
    const ET* lp = ep;
    if (fresh) {
        if (T > 0) {
#pragma unroll
            for (int i = 0; i < N; ++i) prev[i] = ((start >> i) & 1) ? (double)ep[i] : INF;      // decode.py:99-101
            lp = ep + S;
        } else {
#pragma unroll
            for (int i = 0; i < N; ++i) prev[i] = INF;
        }
    } else {
#pragma unroll
        for (int i = 0; i < N; ++i) prev[i] = st[(int64_t)i * C];
    }

    ET ring[PF][N];

    auto column = [&](const ET (&ev)[N]) {
#pragma unroll
        for (int i = N - 1; i >= 0; --i) {          // descending: prev[i-1], prev[i-2] are still the previous column's
            const double e = (double)ev[i];
            double m = c0[i] + prev[i];
            if (i >= 1) {
                double m1 = c1[i] + prev[i - 1];
                if (SKIP && i >= 2) m1 = vmin(c2[i] + prev[i - 2], m1);
                m = vmin(m1, m);
            }
            prev[i] = vmin(m + e, INF);
        }
    };

    // As in the one-shot sweep the loop without guards has its own ring fill in front of it.  `t` counts the columns of
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
    for (int i = 0; i < N; ++i) st[(int64_t)i * C] = prev[i];
}

// End costs of n named streams from their carried columns, gathered through the chain form's end slots into [n, n_end],
// and the cheapest end as the FIRST of equal minima: the recogniser's rule (np.argmin; core.py `if cost < c`), not the
// "last of equal" rule of decode_hmm_states' end points.  No frames: +inf / -1.  One lane per stream.
__global__ __launch_bounds__(64) void wordstream_result_kernel(const int32_t* __restrict__ end_slot, int n_end, int N, int C,
                                                               const double* __restrict__ state, const int64_t* __restrict__ ids,
                                                               const int64_t* __restrict__ frames, int64_t n,
                                                               double* __restrict__ end_cost, int32_t* __restrict__ best) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int64_t stream = ids[i];
    const bool any = frames[i] > 0;
    double* out = end_cost + i * n_end;
    for (int c = 0; c < C; ++c)
        for (int s = 0; s < N; ++s) {
            const int es = end_slot[c * N + s];
            if (es >= 0) out[es] = any ? state[(stream * N + s) * C + c] : INFINITY;
        }
    int bi = -1;
    if (any && n_end > 0) {
        double bv = out[0];                         // (this lane's own stores)
        bi = 0;
        for (int k = 1; k < n_end; ++k) {
            const double v = out[k];
            if (v < bv) { bv = v; bi = k; }
        }
    }
    best[i] = bi;
}

int launch_wordstream(gh_ctx* ctx, const gh_wordstream_args& a, int N, bool skip, bool f64) {
    const int C = a.C;
    const int64_t n_waves = C <= 64 ? (a.n_slots + 64 / C - 1) / (64 / C) : a.n_slots * ((C + 63) / 64);
    const dim3 grid((unsigned)n_waves), blk(64);
    if (N < 3) skip = false;   // (no r-2 arc inside a chain of two rows)
#define GH_WS(ET, NN, SK) hipLaunchKernelGGL((viterbi_chain_online_kernel<ET, NN, SK>), grid, blk, 0, ctx->stream, a)
#define GH_WS_S(ET, NN) do { if (NN >= 3 && skip) GH_WS(ET, NN, (NN >= 3)); else GH_WS(ET, NN, false); } while (0)
#define GH_WS_N(ET) switch (N) { case 1: GH_WS_S(ET, 1); break; case 2: GH_WS_S(ET, 2); break; case 3: GH_WS_S(ET, 3); break; \
                                 case 4: GH_WS_S(ET, 4); break; case 5: GH_WS_S(ET, 5); break; case 6: GH_WS_S(ET, 6); break; \
                                 case 7: GH_WS_S(ET, 7); break; default: GH_WS_S(ET, 8); break; }
    if (f64) GH_WS_N(double) else GH_WS_N(float)
#undef GH_WS_N
#undef GH_WS_S
#undef GH_WS
    GH_HIP(hipGetLastError());
    return GH_OK;
}

}  // namespace

// --------------------------------------------------------------------------------------------------------------- C ABI
void gh_wordchain_refusal(const gh_lattices* lat, char* why, size_t n) {
    why[0] = 0;
    if (lat->deferred_src) snprintf(why, n, "a handle made from transcripts");
    else if (lat->L != 1) snprintf(why, n, "several graphs (one graph of stacked word chains serves all streams)");
    else if (lat->beam > 0) snprintf(why, n, "a rank beam is set on the graph");
    else if (lat->bigram_ok || lat->bigram_wide_ok) snprintf(why, n, "a bigram grammar");
    else if (lat->layers_ok && lat->h_layers.loop) snprintf(why, n, "a word-loop grammar");
    else if (lat->layers_ok) snprintf(why, n, "a K-layer word lattice");
    else if (!lat->chain_ok) snprintf(why, n, "a graph that is not made of left-to-right chains");
    else if (lat->chain_unit <= 0) snprintf(why, n, "chains of unequal length");
    else if (!gh_chain_lanes_ok(lat->chain_unit)) snprintf(why, n, "chains of %d states", lat->chain_unit);
    else if (!lat->chain_consecutive) snprintf(why, n, "chains whose states are not consecutive");
}

gh_wordstream_args gh_wordchain_args(const gh_lattices* lat, const gh_batch* b) {
    gh_wordstream_args a;
    memset(&a, 0, sizeof a);
    a.cost0 = lat->d_ch_cost0; a.cost1 = lat->d_ch_cost1; a.cost2 = lat->d_ch_cost2; a.row_info = lat->d_ch_info;
    a.row_state = lat->d_row_state; a.nll = b->nll; a.S = b->nll_S; a.C = lat->lat[0].R / lat->chain_unit;
    return a;
}

// gh_wordstream_create and gh_wordstream_create_soft: a soft session carries a second column of the same size
static int wordstream_create(gh_ctx* ctx, const gh_lattices* lat, int64_t n_streams, gh_wordstream** out, bool soft, const char* who) {
    GH_REQUIRE(ctx && lat && out, "%s: NULL argument", who);
    *out = nullptr;
    GH_REQUIRE(n_streams >= 1 && n_streams <= 0x7fffffff, "%s: n_streams=%lld", who, (long long)n_streams);
    char why[96];
    gh_wordchain_refusal(lat, why, sizeof why);
    if (why[0]) {
        gh_set_error("%s: online word recognition takes one graph of word chains of equal length (1 .. 8 consecutive "
                     "states each), not %s", who, why);
        return GH_ERR_UNSUPPORTED;
    }
    GH_HIP(hipSetDevice(ctx->device));
    gh_wordstream* ws = new gh_wordstream();
    ws->ctx = ctx; ws->lat = lat; ws->n_streams = n_streams;
    ws->N = lat->chain_unit; ws->C = lat->lat[0].R / lat->chain_unit;
    ws->d_arena = nullptr; ws->h_slots = nullptr; ws->copied = nullptr; ws->copy_pending = false;
    ws->frames.assign((size_t)n_streams, 0);
    ws->seen.assign((size_t)n_streams, 0);
    auto pad = [](size_t b) { return (b + 255) & ~size_t(255); };
    const size_t b_col = pad((size_t)n_streams * ws->N * ws->C * sizeof(double)), b_state = (soft ? 2 : 1) * b_col;
    const size_t b_slots = pad((size_t)n_streams * sizeof(gh_online_slot));
    hipError_t e = hipMalloc(&ws->d_arena, b_state + b_slots);
    if (e == hipSuccess) e = hipHostMalloc((void**)&ws->h_slots, b_slots, hipHostMallocDefault);
    if (e == hipSuccess) e = hipEventCreateWithFlags(&ws->copied, hipEventDisableTiming);
    if (e != hipSuccess) {
        gh_set_error("%s: %lld streams (%zu bytes): %s", who, (long long)n_streams, b_state + b_slots, hipGetErrorString(e));
        gh_wordstream_destroy(ws);
        return e == hipErrorOutOfMemory ? GH_ERR_NOMEM : GH_ERR_HIP;
    }
    char* p = static_cast<char*>(ws->d_arena);
    ws->d_state = reinterpret_cast<double*>(p);
    ws->d_alpha = soft ? reinterpret_cast<double*>(p + b_col) : nullptr;
    p += b_state;
    ws->d_slots = reinterpret_cast<gh_online_slot*>(p);
    *out = ws;
    return GH_OK;
}

extern "C" int gh_wordstream_create(gh_ctx* ctx, const gh_lattices* lat, int64_t n_streams, gh_wordstream** out) {
    return wordstream_create(ctx, lat, n_streams, out, false, "gh_wordstream_create");
}

extern "C" int gh_wordstream_create_soft(gh_ctx* ctx, const gh_lattices* lat, int64_t n_streams, gh_wordstream** out) {
    return wordstream_create(ctx, lat, n_streams, out, true, "gh_wordstream_create_soft");
}

extern "C" void gh_wordstream_destroy(gh_wordstream* ws) {
    if (!ws) return;
    hipSetDevice(ws->ctx->device);
    hipStreamSynchronize(ws->ctx->stream);
    if (ws->copied) hipEventDestroy(ws->copied);
    if (ws->h_slots) hipHostFree(ws->h_slots);
    if (ws->d_arena) hipFree(ws->d_arena);
    delete ws;
}

extern "C" int gh_wordstream_reset(gh_ctx* ctx, gh_wordstream* ws, int64_t n, const int64_t* ids) {
    GH_REQUIRE(ctx && ws, "gh_wordstream_reset: NULL argument");
    if (!ids) {
        std::fill(ws->frames.begin(), ws->frames.end(), 0);
        return GH_OK;
    }
    for (int64_t k = 0; k < n; ++k)
        GH_REQUIRE(ids[k] >= 0 && ids[k] < ws->n_streams, "gh_wordstream_reset: stream %lld out of range [0, %lld)", (long long)ids[k],
                   (long long)ws->n_streams);
    // (a stream at column 0 does not read its carried column: nothing on the device has to be cleared)
    for (int64_t k = 0; k < n; ++k) ws->frames[(size_t)ids[k]] = 0;
    return GH_OK;
}

extern "C" int gh_wordstream_frames(const gh_wordstream* ws, int64_t* out) {
    GH_REQUIRE(ws && out, "gh_wordstream_frames: NULL argument");
    memcpy(out, ws->frames.data(), ws->frames.size() * sizeof(int64_t));
    return GH_OK;
}

extern "C" int gh_wordstream_push(gh_ctx* ctx, gh_wordstream* ws, const gh_batch* b, const int64_t* ids, const int64_t* first,
                                  const int64_t* count) {
    GH_REQUIRE(ctx && ws && b, "gh_wordstream_push: NULL argument");
    GH_REQUIRE(ctx == ws->ctx, "gh_wordstream_push: the session belongs to another context");
    const int64_t U = b->U;
    if (U == 0) return GH_OK;
    GH_REQUIRE(ids, "gh_wordstream_push: ids is NULL");
    GH_REQUIRE(U <= ws->n_streams, "gh_wordstream_push: %lld utterances for %lld streams", (long long)U, (long long)ws->n_streams);
    // everything is checked before anything is enqueued: a refused push moves no stream
    struct Seen {
        std::vector<uint8_t>& v; const int64_t* ids; int64_t n = 0;
        ~Seen() { for (int64_t k = 0; k < n; ++k) v[(size_t)ids[k]] = 0; }
    } seen{ws->seen, ids};
    std::vector<gh_online_slot> slots;
    slots.reserve((size_t)U);
    for (int64_t u = 0; u < U; ++u) {
        const int64_t id = ids[u];
        GH_REQUIRE(id >= 0 && id < ws->n_streams, "gh_wordstream_push: stream %lld out of range [0, %lld)", (long long)id,
                   (long long)ws->n_streams);
        GH_REQUIRE(!ws->seen[(size_t)id], "gh_wordstream_push: stream %lld is named twice", (long long)id);
        ws->seen[(size_t)id] = 1;
        seen.n = u + 1;
        const int64_t Tu = b->offsets[u + 1] - b->offsets[u];
        const int64_t fr = first ? first[u] : 0, cn = count ? count[u] : Tu - fr;
        GH_REQUIRE(fr >= 0 && cn >= 0 && fr + cn <= Tu, "gh_wordstream_push: columns [%lld, %lld) of utterance %lld, which has %lld",
                   (long long)fr, (long long)(fr + cn), (long long)u, (long long)Tu);
        GH_REQUIRE(cn <= 0x7fffffff, "gh_wordstream_push: a chunk of %lld frames", (long long)cn);
        if (cn == 0) continue;
        gh_online_slot s;
        // (the sweep only asks whether the absolute column is 0: a stream past 2^31 frames stays at the largest value)
        s.row0 = b->offsets[u] + fr; s.stream = (int32_t)id; s.count = (int32_t)cn;
        s.t0 = (int32_t)std::min<int64_t>(ws->frames[(size_t)id], 0x7fffffff); s.pad = 0;
        slots.push_back(s);
    }
    if (slots.empty()) return GH_OK;
    GH_REQUIRE(b->nll, "gh_wordstream_push: gh_loglik has not been run on this batch");
    GH_REQUIRE(ws->lat->lat[0].max_state < b->nll_S, "gh_wordstream_push: the graph uses state %d but the model has %d",
               ws->lat->lat[0].max_state, b->nll_S);
    GH_HIP(hipSetDevice(ctx->device));
    // longest chunks first: the slots of a wave then end close to each other
    std::stable_sort(slots.begin(), slots.end(), [](const gh_online_slot& x, const gh_online_slot& y) { return x.count > y.count; });
    if (ws->copy_pending) GH_HIP(hipEventSynchronize(ws->copied));          // (the staging buffer is free again)
    memcpy(ws->h_slots, slots.data(), slots.size() * sizeof(gh_online_slot));
    GH_HIP(hipMemcpyAsync(ws->d_slots, ws->h_slots, slots.size() * sizeof(gh_online_slot), hipMemcpyHostToDevice, ctx->stream));
    GH_HIP(hipEventRecord(ws->copied, ctx->stream));
    ws->copy_pending = true;
    const gh_lattices* lat = ws->lat;
    gh_wordstream_args a = gh_wordchain_args(lat, b);
    a.slots = ws->d_slots; a.n_slots = (int64_t)slots.size(); a.state = ws->d_state;
    int rc = launch_wordstream(ctx, a, ws->N, lat->chain_skip, b->dtype == GH_F64);
    if (rc) return rc;
    if (ws->d_alpha) {                              // a soft session: the log-alpha column on the same slot table
        a.state = ws->d_alpha;
        rc = gh_launch_forward_chain(ctx, a, ws->N, lat->chain_skip, b->dtype == GH_F64);
        if (rc) return rc;
    }
    for (const gh_online_slot& s : slots) ws->frames[(size_t)s.stream] += s.count;
    return GH_OK;
}

extern "C" int gh_wordstream_result(gh_ctx* ctx, gh_wordstream* ws, int64_t n, const int64_t* ids, double* end_cost, int32_t* best) {
    GH_REQUIRE(ctx && ws, "gh_wordstream_result: NULL argument");
    GH_REQUIRE(ctx == ws->ctx, "gh_wordstream_result: the session belongs to another context");
    if (!ids) n = ws->n_streams;
    if (n <= 0) return GH_OK;
    const int n_end = ws->lat->lat[0].n_end;
    std::vector<int64_t> h((size_t)2 * n);          // ids, then the frames of every named stream
    for (int64_t i = 0; i < n; ++i) {
        const int64_t id = ids ? ids[i] : i;
        GH_REQUIRE(id >= 0 && id < ws->n_streams, "gh_wordstream_result: stream %lld out of range [0, %lld)", (long long)id,
                   (long long)ws->n_streams);
        h[(size_t)i] = id;
        h[(size_t)(n + i)] = ws->frames[(size_t)id];
    }
    GH_HIP(hipSetDevice(ctx->device));
    int64_t* d_ids;
    double* d_endcost;
    int32_t* d_best;
    Carver cv;
    cv.add(&d_ids, (size_t)2 * n); cv.add(&d_endcost, (size_t)n * n_end); cv.add(&d_best, (size_t)n);
    const int rc = cv.commit(ctx);
    if (rc) return rc;
    hipStream_t st = ctx->stream;
    GH_HIP(hipMemcpyAsync(d_ids, h.data(), (size_t)2 * n * 8, hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(wordstream_result_kernel, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, st, ws->lat->d_ch_end_slot, n_end, ws->N, ws->C,
                       ws->d_state, d_ids, d_ids + n, n, d_endcost, d_best);
    GH_HIP(hipGetLastError());
    if (best) GH_HIP(hipMemcpyAsync(best, d_best, (size_t)n * 4, hipMemcpyDeviceToHost, st));
    if (end_cost && n_end > 0) GH_HIP(hipMemcpyAsync(end_cost, d_endcost, (size_t)n * n_end * 8, hipMemcpyDeviceToHost, st));
    GH_HIP(hipStreamSynchronize(st));
    return GH_OK;
}
