// ONLINE decode over the word-loop grammar (gh_layerform.loop == 1, up to GH_LAYERS_ROWW words): the loop-form sweep of
// gh_viterbi_layers.hip (viterbi_loop_kernel) CARRIED ACROSS CHUNKS of an utterance that is still arriving.  A column of
// decode_hmm_states (decode.py:80-146) depends on the previous column only, so a stream is fully described by
//   * the previous column: the N state costs of its 16 word lanes               [stream][N][16] doubles,
//   * the decision word that is still open (pushed bits, right aligned)         [stream][16] uint32,
//   * the number of frames it has taken (host side: the absolute column of the next frame),
// and its decision history: one region per stream, written at the ABSOLUTE word index in exactly the layout
// viterbi_loop_kernel writes for a whole utterance of the same frames (gh_loop_hb / gh_loop_cpw, 16 lanes x 4 B per CPW
// columns, the last open word left aligned).  The back-trace of the one-shot decode (gh_launch_lattice_backtrace, loop
// form, path and label mode) therefore runs UNCHANGED on the history, and "the result after k frames" is bitwise the
// whole decode of the first k frames: end costs, chosen end, path and labels (main.py:59-67).
//
// gfx950 mapping: as the loop kernel -- FOUR STREAMS PER WAVE, DPP row = stream, lane = word, the N states of the word in
// registers, rows switched off by EXEC when their chunk ends.  The column step is a copy of the loop kernel's (same
// candidate order, same strict '<', same decision bits); what differs is where `prev` and `word` come from and go to,
// and that the start-row term and the decision-word index use the absolute column.  A chunk moves 16 N 8 B of state in
// and out and 64 B of open word per stream beside its emissions and decisions.
//
// The history is addressed as a RING: decision word index i of a stream lives at i % ring_words.  A session created with a
// capacity (gh_online_create) has a ring as long as its last word index, so nothing ever wraps and it writes the bytes it
// always wrote; one created with a window (gh_online_create_window) holds `window` unsettled frames and one word of slack
// for the word the anchor lies in (gh_online_settle.hip: what is settled, and why the frames before it are dead).
//
// The same session object serves the BIGRAM form (gh_online_create_bigram, on->bigram): push, result, reset, frames and
// destroy below dispatch on it -- the carried sweep and the end kernel of gh_viterbi_bigram_online.hip, the back-trace of
// gh_viterbi_bigram.hip -- with every host-side check unchanged.  One made by gh_online_create_bigram keeps its full history
// and has no commit; gh_online_create_bigram_settle makes one that settles (gh_online_settle.hip: the walk over the bigram
// records) and, with a window, keeps the unsettled tail in the same ring.
//
// ... and the WIDE loop form (gh_online_create_wide, on->wide: 17 .. 64 words): the carried sweep and the end kernel of
// gh_viterbi_online_wide.hip, a wave per stream, the history in the one-shot wide kernel's layout -- the back-trace hands
// over to the wide one by itself.  One made by gh_online_create_wide keeps its full history and has no commit;
// gh_online_create_wide_settle makes one that settles (gh_online_wide_settle.hip: the settle walk over 64 word lanes) and,
// with a window, keeps the unsettled tail in a ring of columns.
//
// ... and the WIDE BIGRAM form (gh_online_create_bigram_wide, on->wide && on->bigram: the bigram grammar with 17 .. 64 words):
// the carried sweep and the end kernel of gh_viterbi_bigram_online_wide.hip, the history in the one-shot wide bigram kernel's
// layout, the back-trace of gh_viterbi_bigram_wide.hip.  One made by gh_online_create_bigram_wide keeps its full history and
// has no commit; gh_online_create_bigram_wide_settle makes one that settles (gh_online_bigram_wide_settle.hip: the settle walk
// over 64 word lanes with the hop through the predecessor word a record names) and, with a window, keeps the unsettled tail in
// a ring of columns.
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
__global__ __launch_bounds__(64) void viterbi_online_kernel(gh_online_args a) {
    constexpr int HB = gh_loop_hb(N, SKIP), CPW = gh_loop_cpw(N, SKIP);
    constexpr int PF = N > 8 ? 2 : 4;
    static_assert(CPW >= 1, "decision bits of a column must fit one word");
    const int lane = threadIdx.x, kk = lane >> 4, w = lane & 15;
    const gh_layerform* __restrict__ lf = a.lf;
    const int W = lf->W;
    const int64_t slot = (int64_t)blockIdx.x * 4 + kk;
    const bool has = slot < a.n_slots;
    gh_online_slot sl;
    sl.row0 = 0; sl.stream = 0; sl.count = 0; sl.t0 = 0; sl.pad = 0;
    if (has) sl = a.slots[slot];
    const int T = sl.count, tb = sl.t0;
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
    const double cin = wact ? lf->cin[wc] : INF, cin0 = wact ? lf->cin0[wc] : INF, cout = wact ? lf->cout[wc] : INF;
    const char* nllb = static_cast<const char*>(a.nll) + (T > 0 ? sl.row0 : 0) * a.S * (int64_t)sizeof(ET);   // (no frames: frame 0)
    const int64_t rowb = (int64_t)a.S * (int64_t)sizeof(ET);
    ET ring[PF][N];
#pragma unroll
    for (int k = 0; k < PF; ++k)
#pragma unroll
        for (int s = 0; s < N; ++s)
            ring[k][s] = (k < T) ? *reinterpret_cast<const ET*>(nllb + k * rowb + sto[s]) : ET(0);
    // the carried column and the open decision word; a stream at column 0 (fresh or reset) starts like the one-shot sweep
    double* st = a.prev + ((int64_t)sl.stream * N) * 16 + w;
    uint32_t* op = a.open + (int64_t)sl.stream * 16 + w;
    const bool carried = T > 0 && tb > 0;
    double prev[N];
#pragma unroll
    for (int s = 0; s < N; ++s) prev[s] = carried ? st[s * 16] : INF;
    uint32_t word = (carried && tb % CPW != 0) ? *op : 0u;
    uint32_t* bp = reinterpret_cast<uint32_t*>(a.hist + (int64_t)sl.stream * a.hist_stride) + w;
    const int n_ring = a.ring_words;
    int wr = (tb / CPW) % n_ring;                               // ring position of the open word; it moves on as words fill

    for (int t0 = 0; t0 < Tmax; t0 += PF) {
#pragma unroll
        for (int k = 0; k < PF; ++k) {
            const int t = t0 + k;
            double e[N];
#pragma unroll
            for (int s = 0; s < N; ++s) e[s] = (double)ring[k][s];
            if (t < T) {                                       // row-uniform: the rows whose chunk has ended sit out
                const int ta = tb + t;                         // the absolute column
                const double base0 = c0[0] + prev[0];
#pragma unroll
                for (int s = N - 1; s >= 1; --s) {
                    const double v0 = c0[s] + prev[s];
                    const double v1 = c1[s] + prev[s - 1];
                    double best;
                    if (SKIP && s >= 2) {
                        const double v2 = c2[s] + prev[s - 2];
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
                    prev[s] = vmin(best + e[s], INF);
                }
                const double cand = prev[N - 1] + cout;
                const double rm = row_min16(cand);
                push_bit(word, __ballot(cand == rm));
                const double cs = ((ta == 0) ? 0.0 : INF) + cin0;
                const double cl = rm + cin;
                const bool b_l = cl < cs;
                const double m2 = vmin(cl, cs);
                const bool b_s = base0 < m2;
                push_bit(word, __ballot(b_l));
                push_bit(word, __ballot(b_s));
                prev[0] = vmin(vmin(base0, m2) + e[0], INF);
                const int ci = ta % CPW;
                if (ci == CPW - 1) {
                    bp[(int64_t)wr * 16] = word;
                    word = 0;
                    wr = wr + 1 == n_ring ? 0 : wr + 1;
                } else if (t == T - 1) {
                    // the chunk ends inside a word: the history shows it left aligned (what the one-shot sweep leaves behind
                    // its last column), the state keeps the pushed bits for the next chunk
                    bp[(int64_t)wr * 16] = word << (HB * (CPW - 1 - ci));
                }
            }
            {   // the slot's refill: unconditional, from a clamped column, outside the divergent region (viterbi_loop_kernel)
                const int tn = (t + PF < T) ? t + PF : (T > 0 ? T - 1 : 0);
                const char* colp = nllb + (int64_t)tn * rowb;
#pragma unroll
                for (int s = 0; s < N; ++s) ring[k][s] = *reinterpret_cast<const ET*>(colp + sto[s]);
            }
        }
    }
    if (T <= 0) return;                                        // (a stream that sat the tick out keeps its state)
#pragma unroll
    for (int s = 0; s < N; ++s) st[s * 16] = prev[s];
    *op = word;
}

// End costs and end selection of n streams from their carried columns: the tail of viterbi_loop_kernel ('>=': the last of
// equal minima, decode.py:129-134; no frames: +inf / -1).  DPP row = stream, lane = word.
__global__ __launch_bounds__(64) void online_end_kernel(const gh_layerform* __restrict__ lf, const int32_t* __restrict__ end_slot,
                                                        int n_end, const double* __restrict__ prev, const int64_t* __restrict__ ids,
                                                        const int64_t* __restrict__ utt_off, int64_t n, double* __restrict__ end_cost,
                                                        int32_t* __restrict__ best_end) {
    const int lane = threadIdx.x, kk = lane >> 4, w = lane & 15;
    const int64_t i = (int64_t)blockIdx.x * 4 + kk;
    if (i >= n) return;
    const int W = lf->W, N = lf->N, Lr = lf->loop_row;
    const int64_t stream = ids[i];
    const int64_t T = utt_off[i + 1] - utt_off[i];
    const double INF = INFINITY;
    double best_v = INF;
    int best_slot = -1;
    if (w < W)
        for (int s = 0; s < N; ++s) {
            const int r = s == 0 ? Lr + 1 + w : 1 + w * (N - 1) + (s - 1);
            const int es = end_slot[r];
            if (es >= 0) {
                const double v = T > 0 ? prev[(stream * N + s) * 16 + w] : INF;
                end_cost[i * n_end + es] = v;
                if (v < best_v || (v == best_v && es > best_slot)) { best_v = v; best_slot = es; }
            }
        }
#pragma unroll
    for (int o = 8; o >= 1; o >>= 1) {
        const double ov = __shfl_xor(best_v, o);
        const int os = __shfl_xor(best_slot, o);
        if (ov < best_v || (ov == best_v && os > best_slot)) { best_v = ov; best_slot = os; }
    }
    if (w == 0) best_end[i] = T > 0 ? best_slot : -1;
}

int launch_online(gh_ctx* ctx, const gh_online_args& a, const gh_layerform& f, bool f64) {
    const dim3 grid((unsigned)((a.n_slots + 3) / 4)), blk(64);
#define GH_ON(ET, NN, SK) hipLaunchKernelGGL((viterbi_online_kernel<ET, NN, SK>), grid, blk, 0, ctx->stream, a)
    if (f64) { GH_NSKIP_SWITCH(f.N, f.skip, 16, GH_ON, double, "gh_online_push: loop form with %d states per word", f.N) }
    else { GH_NSKIP_SWITCH(f.N, f.skip, 16, GH_ON, float, "gh_online_push: loop form with %d states per word", f.N) }
#undef GH_ON
    GH_HIP(hipGetLastError());
    return GH_OK;
}

// a session with history for `frames` frames per stream: all a stream will ever take, or (window) its unsettled tail
// (bigram: the graph must be in bigram form instead; settles: commit and tail serve the session -- a loop session always, a
//  bigram one from gh_online_create_bigram_settle only, and only such a bigram session may have a window)
int online_create(gh_ctx* ctx, const gh_lattices* lat, int64_t n_streams, int64_t frames, bool window, bool bigram, bool settles,
                  gh_online** out) {
    const char* const who = bigram ? (settles ? "gh_online_create_bigram_settle" : "gh_online_create_bigram")
                                   : window ? "gh_online_create_window" : "gh_online_create";
    GH_REQUIRE(ctx && lat && out, "%s: NULL argument", who);
    *out = nullptr;
    GH_REQUIRE(n_streams >= 1 && n_streams <= 0x7fffffff, "%s: n_streams=%lld", who, (long long)n_streams);
    GH_REQUIRE(frames >= 1 && frames <= 0x7fffffff, "%s: %s=%lld", who, window ? "window_frames" : "max_frames", (long long)frames);
    const char* why = nullptr;
    if (lat->L != 1 || lat->deferred_src) why = "several graphs (one graph serves all streams)";
    else if (lat->beam > 0) why = "a rank beam is set on the graph";
    else if (bigram) {
        if (lat->layers_ok && lat->h_layers.loop) why = "a word-loop graph (gh_online_create takes it)";
        else if (lat->layers_ok) why = "a K-layer word lattice";
        else if (!lat->bigram_ok) why = "a graph that is not in bigram form (more than 16 words, and 16 states with skip arcs, are not)";
        else if (!gh_bigram_n_ok(lat->h_layers.N, lat->h_layers.skip)) why = "a word size the bigram sweep is not built for";
    }
    else if (lat->bigram_ok) why = "a bigram grammar (gh_online_create_bigram takes it, with full history)";
    else if (lat->layers_ok && !lat->h_layers.loop) why = "a K-layer word lattice";
    else if (!lat->layers_ok || lat->h_layers.loop != 1) why = "a graph that is not in loop form";
    else if (lat->h_layers.W > GH_LAYERS_ROWW) why = "more than 16 words";
    if (why) {
        gh_set_error("%s: online decoding takes the %s grammar with up to %d words, not %s", who, bigram ? "bigram" : "word-loop",
                     GH_LAYERS_ROWW, why);
        return GH_ERR_UNSUPPORTED;
    }
    GH_HIP(hipSetDevice(ctx->device));
    const gh_layerform& f = lat->h_layers;
    gh_online* on = new gh_online();
    on->ctx = ctx; on->lat = lat; on->bigram = bigram; on->settles = settles; on->n_streams = n_streams;
    // a window: whole decision words, one more for the word the anchor lies in; the stream itself ends with the 32-bit column
    const int cpw = bigram ? gh_bigram_cpw(f.N, f.skip != 0) : gh_loop_cpw(f.N, f.skip != 0);
    on->max_frames = window ? 0x7fffffff : frames;
    on->window = window ? frames : 0;
    on->ring_words = (int32_t)((frames + cpw - 1) / cpw + (window ? 1 : 0));
    on->hist_stride = (int64_t)on->ring_words * 16 * 2;
    on->d_arena = nullptr; on->h_slots = nullptr; on->copied = nullptr; on->copy_pending = false;
    on->frames.assign((size_t)n_streams, 0);
    on->settled.assign((size_t)n_streams, 0);
    on->seen.assign((size_t)n_streams, 0);
    auto pad = [](size_t b) { return (b + 255) & ~size_t(255); };
    const size_t b_prev = pad((size_t)n_streams * f.N * 16 * sizeof(double)), b_open = pad((size_t)n_streams * 16 * 4);
    const size_t b_hist = pad((size_t)n_streams * (size_t)on->hist_stride * 2), b_slots = pad((size_t)n_streams * sizeof(gh_online_slot));
    const size_t b_anchor = pad((size_t)n_streams * sizeof(gh_online_anchor));
    hipError_t e = hipMalloc(&on->d_arena, b_prev + b_open + b_hist + b_slots + b_anchor);
    if (e == hipSuccess) e = hipHostMalloc((void**)&on->h_slots, b_slots, hipHostMallocDefault);
    if (e == hipSuccess) e = hipEventCreateWithFlags(&on->copied, hipEventDisableTiming);
    if (e != hipSuccess) {
        gh_set_error("%s: %lld streams x %lld frames (%zu bytes): %s", who, (long long)n_streams, (long long)frames,
                     b_prev + b_open + b_hist + b_slots + b_anchor, hipGetErrorString(e));
        gh_online_destroy(on);
        return e == hipErrorOutOfMemory ? GH_ERR_NOMEM : GH_ERR_HIP;
    }
    char* p = static_cast<char*>(on->d_arena);
    on->d_prev = reinterpret_cast<double*>(p); p += b_prev;
    on->d_open = reinterpret_cast<uint32_t*>(p); p += b_open;
    on->d_hist = reinterpret_cast<uint16_t*>(p); p += b_hist;
    on->d_slots = reinterpret_cast<gh_online_slot*>(p); p += b_slots;
    on->d_anchor = reinterpret_cast<gh_online_anchor*>(p);   // (read only where `settled` says a stream has one)
    *out = on;
    return GH_OK;
}

// a WIDE session (gh_viterbi_online_wide.hip): the word loop with 17 .. 64 words, a wave per stream.  State [stream][N][64]
// doubles, no open word, and the full history in the one-shot wide kernel's layout -- gh_loop_wide_bp_entries(max_frames)
// uint16 units, 256 B per frame, per stream; no ring, no anchors.
// settles (gh_online_create_wide_settle): commit and tail serve the session, which has its anchors; `frames` is then its
// capacity (full history, the same layout) or, with `window`, the unsettled frames its ring of columns holds -- frames + 1
// columns (online_create's formula at one column per word: the column the anchor lies in is kept), 128 uint16 units each
int online_create_wide(gh_ctx* ctx, const gh_lattices* lat, int64_t n_streams, int64_t max_frames, bool settles, bool window,
                       gh_online** out) {
    const char* const who = settles ? "gh_online_create_wide_settle" : "gh_online_create_wide";
    GH_REQUIRE(ctx && lat && out, "%s: NULL argument", who);
    *out = nullptr;
    GH_REQUIRE(n_streams >= 1 && n_streams <= 0x7fffffff, "%s: n_streams=%lld", who, (long long)n_streams);
    GH_REQUIRE(max_frames >= 1 && max_frames <= 0x7fffffff, "%s: %s=%lld", who, window ? "window_frames" : "max_frames", (long long)max_frames);
    const char* why = nullptr;
    if (lat->L != 1 || lat->deferred_src) why = "several graphs (one graph serves all streams)";
    else if (lat->beam > 0) why = "a rank beam is set on the graph";
    else if (lat->bigram_ok) why = "a bigram grammar (gh_online_create_bigram takes it)";
    else if (lat->layers_ok && !lat->h_layers.loop) why = "a K-layer word lattice";
    else if (!lat->layers_ok || lat->h_layers.loop != 1) why = "a graph that is not in loop form";
    else if (lat->h_layers.W <= GH_LAYERS_ROWW) why = "16 words or fewer (gh_online_create takes it)";
    else if (lat->h_layers.W > GH_LAYERS_MAXW) why = "more than 64 words";
    else if (lat->h_layers.N > 8) why = "more than 8 states per word";
    if (why) {
        gh_set_error("%s: wide online decoding takes the word-loop grammar with %d to %d words of up to 8 states, not %s", who,
                     GH_LAYERS_ROWW + 1, GH_LAYERS_MAXW, why);
        return GH_ERR_UNSUPPORTED;
    }
    const gh_layerform& f = lat->h_layers;
    auto pad = [](size_t b) { return (b + 255) & ~size_t(255); };
    // max_frames < 2^31: the stride (128 uint16 units per frame) fits gh_layers_args::bp_off with room to spare; streams x
    // stride is checked before anything is allocated
    const int64_t stride = (int64_t)gh_loop_wide_bp_entries(max_frames + (window ? 1 : 0));
    const size_t stream_bytes = (size_t)stride * 2 + (size_t)f.N * 64 * sizeof(double) + sizeof(gh_online_slot) + sizeof(gh_online_anchor);
    if ((size_t)n_streams > (SIZE_MAX / 2 - 1024) / stream_bytes) {
        gh_set_error("%s: %lld streams x %lld frames (%.0f bytes): the size does not fit a size_t", who, (long long)n_streams,
                     (long long)max_frames, (double)n_streams * (double)stream_bytes);
        return GH_ERR_NOMEM;
    }
    GH_HIP(hipSetDevice(ctx->device));
    gh_online* on = new gh_online();
    on->ctx = ctx; on->lat = lat; on->bigram = false; on->settles = settles; on->wide = true; on->n_streams = n_streams;
    on->max_frames = window ? 0x7fffffff : max_frames;
    on->window = window ? max_frames : 0;
    on->ring_words = window ? (int32_t)std::min<int64_t>(max_frames + 1, 0x7fffffff) : 0x7fffffff;   // (columns; full history: never filled)
    on->hist_stride = stride;
    on->d_arena = nullptr; on->h_slots = nullptr; on->copied = nullptr; on->copy_pending = false;
    on->d_open = nullptr; on->d_anchor = nullptr;
    on->frames.assign((size_t)n_streams, 0);
    on->settled.assign((size_t)n_streams, 0);
    on->seen.assign((size_t)n_streams, 0);
    const size_t b_prev = pad((size_t)n_streams * f.N * 64 * sizeof(double));
    const size_t b_hist = pad((size_t)n_streams * (size_t)stride * 2), b_slots = pad((size_t)n_streams * sizeof(gh_online_slot));
    const size_t b_anchor = settles ? pad((size_t)n_streams * sizeof(gh_online_anchor)) : 0;
    hipError_t e = hipMalloc(&on->d_arena, b_prev + b_hist + b_slots + b_anchor);
    if (e == hipSuccess) e = hipHostMalloc((void**)&on->h_slots, b_slots, hipHostMallocDefault);
    if (e == hipSuccess) e = hipEventCreateWithFlags(&on->copied, hipEventDisableTiming);
    if (e != hipSuccess) {
        gh_set_error("%s: %lld streams x %lld frames (%zu bytes): %s", who, (long long)n_streams, (long long)max_frames,
                     b_prev + b_hist + b_slots + b_anchor, hipGetErrorString(e));
        gh_online_destroy(on);
        return e == hipErrorOutOfMemory ? GH_ERR_NOMEM : GH_ERR_HIP;
    }
    char* p = static_cast<char*>(on->d_arena);
    on->d_prev = reinterpret_cast<double*>(p); p += b_prev;
    on->d_hist = reinterpret_cast<uint16_t*>(p); p += b_hist;
    on->d_slots = reinterpret_cast<gh_online_slot*>(p); p += b_slots;
    if (settles) on->d_anchor = reinterpret_cast<gh_online_anchor*>(p);   // (read only where `settled` says a stream has one)
    *out = on;
    return GH_OK;
}

// a WIDE BIGRAM session (gh_viterbi_bigram_online_wide.hip): the bigram grammar with 17 .. 64 words of 2 .. 8 states, a wave
// per stream.  State [stream][N][64] doubles, no open word, and the full history in the one-shot wide bigram kernel's layout
// -- gh_bigram_wide_bp_entries(max_frames) uint16 units, 256 B per frame, per stream; a ring that is never filled, no anchors:
// the session does not settle.
// settles (gh_online_create_bigram_wide_settle): commit and tail serve the session, which has its anchors; `max_frames` is then
// its capacity (full history, the same layout) or, with `window`, the unsettled frames its ring of columns holds -- frames + 1
// columns as in online_create_wide (the column the anchor lies in is kept), 128 uint16 units each
int online_create_bigram_wide(gh_ctx* ctx, const gh_lattices* lat, int64_t n_streams, int64_t max_frames, bool settles, bool window,
                              gh_online** out) {
    const char* const who = settles ? "gh_online_create_bigram_wide_settle" : "gh_online_create_bigram_wide";
    GH_REQUIRE(ctx && lat && out, "%s: NULL argument", who);
    *out = nullptr;
    GH_REQUIRE(n_streams >= 1 && n_streams <= 0x7fffffff, "%s: n_streams=%lld", who, (long long)n_streams);
    GH_REQUIRE(max_frames >= 1 && max_frames <= 0x7fffffff, "%s: %s=%lld", who, window ? "window_frames" : "max_frames", (long long)max_frames);
    const char* why = nullptr;
    if (lat->L != 1 || lat->deferred_src) why = "several graphs (one graph serves all streams)";
    else if (lat->beam > 0) why = "a rank beam is set on the graph";
    else if (lat->bigram_ok) why = "a bigram grammar of 16 words or fewer (gh_online_create_bigram takes it)";
    else if (lat->layers_ok && lat->h_layers.loop)
        why = lat->h_layers.W > GH_LAYERS_ROWW ? "a word-loop graph (gh_online_create_wide takes it)" : "a word-loop graph (gh_online_create takes it)";
    else if (lat->layers_ok) why = "a K-layer word lattice";
    else if (!lat->bigram_wide_ok) why = "a graph that is not in wide bigram form (more than 64 words, and more than 8 states per word, are not)";
    if (why) {
        gh_set_error("%s: wide online bigram decoding takes the bigram grammar with %d to %d words of 2 to 8 states, not %s", who,
                     GH_LAYERS_ROWW + 1, GH_LAYERS_MAXW, why);
        return GH_ERR_UNSUPPORTED;
    }
    GH_REQUIRE(lat->d_bigram_wide, "%s: internal: wide bigram form without its cost table", who);
    const gh_layerform& f = lat->h_layers;
    auto pad = [](size_t b) { return (b + 255) & ~size_t(255); };
    // max_frames < 2^31: the stride (128 uint16 units per frame) fits gh_layers_args::bp_off with room to spare; streams x
    // stride is checked before anything is allocated
    const int64_t stride = (int64_t)gh_bigram_wide_bp_entries(max_frames + (window ? 1 : 0));
    const size_t stream_bytes = (size_t)stride * 2 + (size_t)f.N * 64 * sizeof(double) + sizeof(gh_online_slot) +
                                (settles ? sizeof(gh_online_anchor) : 0);
    if ((size_t)n_streams > (SIZE_MAX / 2 - 1024) / stream_bytes) {
        gh_set_error("%s: %lld streams x %lld frames (%.0f bytes): the size does not fit a size_t", who, (long long)n_streams,
                     (long long)max_frames, (double)n_streams * (double)stream_bytes);
        return GH_ERR_NOMEM;
    }
    GH_HIP(hipSetDevice(ctx->device));
    gh_online* on = new gh_online();
    on->ctx = ctx; on->lat = lat; on->bigram = true; on->settles = settles; on->wide = true; on->n_streams = n_streams;
    on->max_frames = window ? 0x7fffffff : max_frames;
    on->window = window ? max_frames : 0;
    on->ring_words = window ? (int32_t)std::min<int64_t>(max_frames + 1, 0x7fffffff) : 0x7fffffff;   // (columns; full history: never filled)
    on->hist_stride = stride;
    on->d_arena = nullptr; on->h_slots = nullptr; on->copied = nullptr; on->copy_pending = false;
    on->d_open = nullptr; on->d_anchor = nullptr;
    on->frames.assign((size_t)n_streams, 0);
    on->settled.assign((size_t)n_streams, 0);
    on->seen.assign((size_t)n_streams, 0);
    const size_t b_prev = pad((size_t)n_streams * f.N * 64 * sizeof(double));
    const size_t b_hist = pad((size_t)n_streams * (size_t)stride * 2), b_slots = pad((size_t)n_streams * sizeof(gh_online_slot));
    const size_t b_anchor = settles ? pad((size_t)n_streams * sizeof(gh_online_anchor)) : 0;
    hipError_t e = hipMalloc(&on->d_arena, b_prev + b_hist + b_slots + b_anchor);
    if (e == hipSuccess) e = hipHostMalloc((void**)&on->h_slots, b_slots, hipHostMallocDefault);
    if (e == hipSuccess) e = hipEventCreateWithFlags(&on->copied, hipEventDisableTiming);
    if (e != hipSuccess) {
        gh_set_error("%s: %lld streams x %lld frames (%zu bytes): %s", who, (long long)n_streams, (long long)max_frames,
                     b_prev + b_hist + b_slots + b_anchor, hipGetErrorString(e));
        gh_online_destroy(on);
        return e == hipErrorOutOfMemory ? GH_ERR_NOMEM : GH_ERR_HIP;
    }
    char* p = static_cast<char*>(on->d_arena);
    on->d_prev = reinterpret_cast<double*>(p); p += b_prev;
    on->d_hist = reinterpret_cast<uint16_t*>(p); p += b_hist;
    on->d_slots = reinterpret_cast<gh_online_slot*>(p); p += b_slots;
    if (settles) on->d_anchor = reinterpret_cast<gh_online_anchor*>(p);   // (read only where `settled` says a stream has one)
    *out = on;
    return GH_OK;
}

}  // namespace

int gh_launch_online_end(gh_ctx* ctx, const gh_online* on, const int64_t* d_ids, const int64_t* d_utt_off, int64_t n, double* d_end_cost,
                         int32_t* d_best_end) {
    hipLaunchKernelGGL(online_end_kernel, dim3((unsigned)((n + 3) / 4)), dim3(64), 0, ctx->stream, on->lat->d_layers, on->lat->d_lf_end_slot,
                       on->lat->lat[0].n_end, on->d_prev, d_ids, d_utt_off, n, d_end_cost, d_best_end);
    GH_HIP(hipGetLastError());
    return GH_OK;
}

// --------------------------------------------------------------------------------------------------------------- C ABI
extern "C" int gh_online_create(gh_ctx* ctx, const gh_lattices* lat, int64_t n_streams, int64_t max_frames, gh_online** out) {
    return online_create(ctx, lat, n_streams, max_frames, false, false, true, out);
}

extern "C" int gh_online_create_bigram(gh_ctx* ctx, const gh_lattices* lat, int64_t n_streams, int64_t max_frames, gh_online** out) {
    return online_create(ctx, lat, n_streams, max_frames, false, true, false, out);
}

extern "C" int gh_online_create_wide(gh_ctx* ctx, const gh_lattices* lat, int64_t n_streams, int64_t max_frames, gh_online** out) {
    return online_create_wide(ctx, lat, n_streams, max_frames, false, false, out);
}

extern "C" int gh_online_create_wide_settle(gh_ctx* ctx, const gh_lattices* lat, int64_t n_streams, int64_t frames, int window,
                                            gh_online** out) {
    return online_create_wide(ctx, lat, n_streams, frames, true, window != 0, out);
}

extern "C" int gh_online_create_bigram_wide(gh_ctx* ctx, const gh_lattices* lat, int64_t n_streams, int64_t max_frames, gh_online** out) {
    return online_create_bigram_wide(ctx, lat, n_streams, max_frames, false, false, out);
}

extern "C" int gh_online_create_bigram_wide_settle(gh_ctx* ctx, const gh_lattices* lat, int64_t n_streams, int64_t frames, int window,
                                                   gh_online** out) {
    return online_create_bigram_wide(ctx, lat, n_streams, frames, true, window != 0, out);
}

extern "C" int gh_online_create_window(gh_ctx* ctx, const gh_lattices* lat, int64_t n_streams, int64_t window_frames, gh_online** out) {
    return online_create(ctx, lat, n_streams, window_frames, true, false, true, out);
}

extern "C" int gh_online_create_bigram_settle(gh_ctx* ctx, const gh_lattices* lat, int64_t n_streams, int64_t frames, int window,
                                              gh_online** out) {
    return online_create(ctx, lat, n_streams, frames, window != 0, true, true, out);
}

extern "C" void gh_online_destroy(gh_online* on) {
    if (!on) return;
    hipSetDevice(on->ctx->device);
    hipStreamSynchronize(on->ctx->stream);
    if (on->copied) hipEventDestroy(on->copied);
    if (on->h_slots) hipHostFree(on->h_slots);
    if (on->d_arena) hipFree(on->d_arena);
    delete on;
}

extern "C" int gh_online_reset(gh_ctx* ctx, gh_online* on, int64_t n, const int64_t* ids) {
    GH_REQUIRE(ctx && on, "gh_online_reset: NULL argument");
    if (!ids) {
        std::fill(on->frames.begin(), on->frames.end(), 0);
        std::fill(on->settled.begin(), on->settled.end(), 0);
        return GH_OK;
    }
    for (int64_t k = 0; k < n; ++k)
        GH_REQUIRE(ids[k] >= 0 && ids[k] < on->n_streams, "gh_online_reset: stream %lld out of range [0, %lld)", (long long)ids[k],
                   (long long)on->n_streams);
    // (a stream at column 0 starts from +inf and an empty word, and its anchor is read only once `settled` says it has one:
    //  nothing on the device has to be cleared)
    for (int64_t k = 0; k < n; ++k) on->frames[(size_t)ids[k]] = on->settled[(size_t)ids[k]] = 0;
    return GH_OK;
}

extern "C" int gh_online_frames(const gh_online* on, int64_t* out) {
    GH_REQUIRE(on && out, "gh_online_frames: NULL argument");
    memcpy(out, on->frames.data(), on->frames.size() * sizeof(int64_t));
    return GH_OK;
}

extern "C" int gh_online_push(gh_ctx* ctx, gh_online* on, const gh_batch* b, const int64_t* ids, const int64_t* first,
                              const int64_t* count) {
    GH_REQUIRE(ctx && on && b, "gh_online_push: NULL argument");
    GH_REQUIRE(ctx == on->ctx, "gh_online_push: the session belongs to another context");
    const int64_t U = b->U;
    if (U == 0) return GH_OK;
    GH_REQUIRE(ids, "gh_online_push: ids is NULL");
    GH_REQUIRE(U <= on->n_streams, "gh_online_push: %lld utterances for %lld streams", (long long)U, (long long)on->n_streams);
    const gh_layerform& f = on->lat->h_layers;
    // everything is checked before anything is enqueued: a refused push moves no stream
    struct Seen {
        std::vector<uint8_t>& v; const int64_t* ids; int64_t n = 0;
        ~Seen() { for (int64_t k = 0; k < n; ++k) v[(size_t)ids[k]] = 0; }
    } seen{on->seen, ids};
    std::vector<gh_online_slot> slots;
    slots.reserve((size_t)U);
    for (int64_t u = 0; u < U; ++u) {
        const int64_t id = ids[u];
        GH_REQUIRE(id >= 0 && id < on->n_streams, "gh_online_push: stream %lld out of range [0, %lld)", (long long)id, (long long)on->n_streams);
        GH_REQUIRE(!on->seen[(size_t)id], "gh_online_push: stream %lld is named twice", (long long)id);
        on->seen[(size_t)id] = 1;
        seen.n = u + 1;
        const int64_t Tu = b->offsets[u + 1] - b->offsets[u];
        const int64_t fr = first ? first[u] : 0, cn = count ? count[u] : Tu - fr;
        GH_REQUIRE(fr >= 0 && cn >= 0 && fr + cn <= Tu, "gh_online_push: columns [%lld, %lld) of utterance %lld, which has %lld", (long long)fr,
                   (long long)(fr + cn), (long long)u, (long long)Tu);
        GH_REQUIRE(on->frames[(size_t)id] + cn <= on->max_frames, "gh_online_push: stream %lld would hold %lld frames, capacity %lld",
                   (long long)id, (long long)(on->frames[(size_t)id] + cn), (long long)on->max_frames);
        GH_REQUIRE(!on->window || on->frames[(size_t)id] + cn - on->settled[(size_t)id] <= on->window,
                   "gh_online_push: stream %lld would hold %lld unsettled frames, window %lld (gh_online_commit moves the window on; a "
                   "stream whose traces have not met within it can only be finished)", (long long)id,
                   (long long)(on->frames[(size_t)id] + cn - on->settled[(size_t)id]), (long long)on->window);
        if (cn == 0) continue;
        gh_online_slot s;
        s.row0 = b->offsets[u] + fr; s.stream = (int32_t)id; s.count = (int32_t)cn; s.t0 = (int32_t)on->frames[(size_t)id]; s.pad = 0;
        slots.push_back(s);
    }
    if (slots.empty()) return GH_OK;
    GH_REQUIRE(b->nll, "gh_online_push: gh_loglik has not been run on this batch");
    GH_REQUIRE(on->lat->lat[0].max_state < b->nll_S, "gh_online_push: the graph uses state %d but the model has %d", on->lat->lat[0].max_state,
               b->nll_S);
    GH_REQUIRE(gh_seq_n_ok(f.N), "gh_online_push: %s form with %d states per word", on->bigram ? "bigram" : "loop", f.N);
    GH_HIP(hipSetDevice(ctx->device));
    // longest chunks first: the four rows of a wave then end close to each other (a wide session: the long waves start first)
    std::stable_sort(slots.begin(), slots.end(), [](const gh_online_slot& x, const gh_online_slot& y) { return x.count > y.count; });
    if (on->copy_pending) GH_HIP(hipEventSynchronize(on->copied));          // (the staging buffer is free again)
    memcpy(on->h_slots, slots.data(), slots.size() * sizeof(gh_online_slot));
    GH_HIP(hipMemcpyAsync(on->d_slots, on->h_slots, slots.size() * sizeof(gh_online_slot), hipMemcpyHostToDevice, ctx->stream));
    GH_HIP(hipEventRecord(on->copied, ctx->stream));
    on->copy_pending = true;
    gh_online_args a;
    memset(&a, 0, sizeof a);
    a.lf = on->lat->d_layers; a.nll = b->nll; a.S = b->nll_S; a.slots = on->d_slots; a.n_slots = (int64_t)slots.size();
    a.prev = on->d_prev; a.open = on->d_open; a.hist = on->d_hist; a.hist_stride = on->hist_stride; a.ring_words = on->ring_words;
    const int rc = on->wide && on->bigram ? gh_launch_online_bigram_wide(ctx, a, f, on->lat->d_bigram_wide, b->dtype == GH_F64)
                 : on->wide ? gh_launch_online_wide(ctx, a, f, b->dtype == GH_F64)
                 : on->bigram ? gh_launch_online_bigram(ctx, a, f, b->dtype == GH_F64) : launch_online(ctx, a, f, b->dtype == GH_F64);
    if (rc) return rc;
    for (const gh_online_slot& s : slots) on->frames[(size_t)s.stream] += s.count;
    return GH_OK;
}

extern "C" int gh_online_result_timed(gh_ctx* ctx, gh_online* on, int64_t n, const int64_t* ids, double* end_cost, int32_t* best_end,
                                      const int32_t* row_label, int32_t* labels, const int64_t* label_off, int32_t* n_labels,
                                      int32_t* path, const int64_t* path_off, int32_t* path_len, int32_t* out_begin) {
    GH_REQUIRE(ctx && on, "gh_online_result: NULL argument");
    GH_REQUIRE(!out_begin || labels, "gh_online_result_timed: out_begin needs labels");
    GH_REQUIRE(ctx == on->ctx, "gh_online_result: the session belongs to another context");
    GH_REQUIRE(!labels || (row_label && label_off && n_labels), "gh_online_result: labels need row_label, label_off and n_labels");
    GH_REQUIRE(!path || (path_off && path_len), "gh_online_result: path needs path_off and path_len");
    if (on->window) {
        gh_set_error("gh_online_result: a session with a window keeps the unsettled tail of the history only; gh_online_commit gives the "
                     "settled words and gh_online_tail the rest (paths are not offered)");
        return GH_ERR_UNSUPPORTED;
    }
    if (!ids) n = on->n_streams;
    if (n <= 0) return GH_OK;
    const gh_lattices* lat = on->lat;
    const gh_layerform& f = lat->h_layers;
    const int n_end = lat->lat[0].n_end, nlev = lat->lat[0].nlev, R = lat->lat[0].R;
    std::vector<int64_t> h_ids((size_t)n), utt_off((size_t)n + 1, 0), bp_off((size_t)n);
    for (int64_t i = 0; i < n; ++i) {
        const int64_t id = ids ? ids[i] : i;
        GH_REQUIRE(id >= 0 && id < on->n_streams, "gh_online_result: stream %lld out of range [0, %lld)", (long long)id, (long long)on->n_streams);
        const int64_t T = on->frames[(size_t)id];
        h_ids[(size_t)i] = id;
        utt_off[(size_t)i + 1] = utt_off[(size_t)i] + T;
        bp_off[(size_t)i] = id * on->hist_stride;
        if (path) GH_REQUIRE(path_off[i + 1] - path_off[i] >= (T > 1 ? T * nlev : 0), "gh_online_result: path capacity of stream %lld too small", (long long)id);
    }
    GH_HIP(hipSetDevice(ctx->device));
    int* d_flag;
    int32_t *d_best, *d_rowlabel = nullptr, *d_nlabels = nullptr, *d_labels = nullptr, *d_begins = nullptr, *d_path = nullptr, *d_pathlen = nullptr;
    double* d_endcost;
    int64_t *d_ids, *d_uttoff, *d_bpoff, *d_labeloff = nullptr, *d_pathoff = nullptr;
    Carver cv;
    cv.add(&d_flag, 64); cv.add(&d_best, (size_t)n); cv.add(&d_endcost, (size_t)n * n_end);
    cv.add(&d_ids, (size_t)n); cv.add(&d_uttoff, (size_t)n + 1); cv.add(&d_bpoff, (size_t)n);
    if (labels) { cv.add(&d_rowlabel, (size_t)R); cv.add(&d_labeloff, (size_t)n + 1); cv.add(&d_nlabels, (size_t)n); cv.add(&d_labels, (size_t)label_off[n]); }
    if (out_begin) cv.add(&d_begins, (size_t)label_off[n]);
    if (path) { cv.add(&d_pathoff, (size_t)n + 1); cv.add(&d_pathlen, (size_t)n); cv.add(&d_path, (size_t)2 * path_off[n]); }
    int rc = cv.commit(ctx);
    if (rc) return rc;
    hipStream_t st = ctx->stream;
    GH_HIP(hipMemsetAsync(d_flag, 0, sizeof(int), st));
    GH_HIP(hipMemcpyAsync(d_ids, h_ids.data(), (size_t)n * 8, hipMemcpyHostToDevice, st));
    GH_HIP(hipMemcpyAsync(d_uttoff, utt_off.data(), (size_t)(n + 1) * 8, hipMemcpyHostToDevice, st));
    GH_HIP(hipMemcpyAsync(d_bpoff, bp_off.data(), (size_t)n * 8, hipMemcpyHostToDevice, st));
    if (labels) {
        GH_HIP(hipMemcpyAsync(d_rowlabel, row_label, (size_t)R * 4, hipMemcpyHostToDevice, st));
        GH_HIP(hipMemcpyAsync(d_labeloff, label_off, (size_t)(n + 1) * 8, hipMemcpyHostToDevice, st));
    }
    if (path) GH_HIP(hipMemcpyAsync(d_pathoff, path_off, (size_t)(n + 1) * 8, hipMemcpyHostToDevice, st));
    rc = on->wide && on->bigram ? gh_launch_online_bigram_wide_end(ctx, on, d_ids, d_uttoff, n, d_endcost, d_best)
       : on->wide ? gh_launch_online_wide_end(ctx, on, d_ids, d_uttoff, n, d_endcost, d_best)
       : on->bigram ? gh_launch_online_bigram_end(ctx, on, d_ids, d_uttoff, n, d_endcost, d_best)
                    : gh_launch_online_end(ctx, on, d_ids, d_uttoff, n, d_endcost, d_best);
    if (rc) return rc;
    // the one-shot decode's own back-trace on the history: utterance i = stream ids[i], its decision words at bp_off[i]
    // (a wide session: gh_launch_lattice_backtrace hands over to the wide loop back-trace, f.W > GH_LAYERS_ROWW, and
    //  gh_launch_bigram_backtrace, given the cost table of the wide bigram form, to the wide bigram one; a narrow bigram
    //  session has no such table: null)
    gh_layers_args c;
    memset(&c, 0, sizeof c);
    c.lf = lat->d_layers; c.end_slot = lat->d_lf_end_slot; c.end_rows = lat->d_end_rows; c.n_end = n_end; c.S = 0;
    c.utt_off = d_uttoff; c.bp = on->d_hist; c.bp_off = d_bpoff; c.best_end = d_best; c.flag = d_flag;
    if (path) {
        c.path = d_path; c.path_off = d_pathoff; c.path_len = d_pathlen;
        rc = on->bigram ? gh_launch_bigram_backtrace(ctx, c, f, 0, n, false, lat->d_bigram_wide) : gh_launch_lattice_backtrace(ctx, c, f, 0, n);
        if (rc) return rc;
    }
    if (labels) {
        c.row_label = d_rowlabel; c.labels = d_labels; c.label_off = d_labeloff; c.n_labels = d_nlabels;
        if (d_begins) c.path = d_begins;                    // timed label mode: the begins go where a path launch has its path
        rc = on->bigram ? gh_launch_bigram_backtrace(ctx, c, f, 0, n, d_begins != nullptr, lat->d_bigram_wide)
                        : gh_launch_lattice_backtrace(ctx, c, f, 0, n, d_begins != nullptr);
        if (rc) return rc;
    }
    int flag = 0;
    GH_HIP(hipMemcpyAsync(&flag, d_flag, sizeof(int), hipMemcpyDeviceToHost, st));
    if (best_end) GH_HIP(hipMemcpyAsync(best_end, d_best, (size_t)n * 4, hipMemcpyDeviceToHost, st));
    if (end_cost) GH_HIP(hipMemcpyAsync(end_cost, d_endcost, (size_t)n * n_end * 8, hipMemcpyDeviceToHost, st));
    if (labels) {
        GH_HIP(hipMemcpyAsync(n_labels, d_nlabels, (size_t)n * 4, hipMemcpyDeviceToHost, st));
        if (label_off[n] > 0) GH_HIP(hipMemcpyAsync(labels, d_labels, (size_t)label_off[n] * 4, hipMemcpyDeviceToHost, st));
        if (out_begin && label_off[n] > 0) GH_HIP(hipMemcpyAsync(out_begin, d_begins, (size_t)label_off[n] * 4, hipMemcpyDeviceToHost, st));
    }
    if (path) {
        GH_HIP(hipMemcpyAsync(path_len, d_pathlen, (size_t)n * 4, hipMemcpyDeviceToHost, st));
        if (path_off[n] > 0) GH_HIP(hipMemcpyAsync(path, d_path, (size_t)2 * path_off[n] * 4, hipMemcpyDeviceToHost, st));
    }
    GH_HIP(hipStreamSynchronize(st));
    if (flag & 4) {
        gh_set_error("gh_online_result: path capacity of a stream too small");
        return GH_ERR_INVALID;
    }
    if (flag & 2) {
        gh_set_error("gh_online_result: back-trace reached a cell without predecessor");
        return GH_ERR_INVALID;
    }
    if (flag & 8) {
        gh_set_error("gh_online_result: label capacity of a stream too small");
        return GH_ERR_INVALID;
    }
    return GH_OK;
}

extern "C" int gh_online_result(gh_ctx* ctx, gh_online* on, int64_t n, const int64_t* ids, double* end_cost, int32_t* best_end,
                                const int32_t* row_label, int32_t* labels, const int64_t* label_off, int32_t* n_labels,
                                int32_t* path, const int64_t* path_off, int32_t* path_len) {
    return gh_online_result_timed(ctx, on, n, ids, end_cost, best_end, row_label, labels, label_off, n_labels, path, path_off, path_len,
                                  nullptr);
}
