// THE ONLINE SESSION (gh_online_*): Viterbi decode CARRIED ACROSS CHUNKS of utterances that are still arriving.  A column of
// decode_hmm_states (decode.py:80-146) depends on the previous column only, so a stream is fully described by
//   * the previous column: the N state costs of its word lanes,
//   * in a form with an open word, the decision word that is still open (pushed bits, right aligned),
//   * the number of frames it has taken (host side: the absolute column of the next frame),
// and its decision history: one region per stream, written at the ABSOLUTE word index in exactly the layout the one-shot sweep
// of the same form writes for a whole utterance of the same frames.  The back-trace of the one-shot decode therefore runs
// UNCHANGED on the history, and "the result after k frames" is bitwise the whole decode of the first k frames: end costs,
// chosen end, path and labels (main.py:59-67).
//
// The FORM of a session -- narrow or wide, loop or bigram rows, or the K-layer lattice: gh_online_forms in gh_online.h -- is fixed
// by the entry point that made it and says how many lanes a stream has, how its history is sized, and which sweep, walks and
// back-trace serve it.
// Independent of the form, a session either keeps its FULL HISTORY (max_frames is its capacity, nothing ever wraps) or has a
// WINDOW: the history is addressed as a ring, decision word index i of a stream at i % ring_words, and holds `window`
// unsettled frames and the word the anchor lies in.  A session that SETTLES has anchors: gh_online_commit moves them on and
// returns what it settled, gh_online_tail gives the rest (gh_online_settle.hip: what is settled, and why the frames before
// the anchor are dead); a window needs one that settles, and gh_online_result is refused with a window.
#include "gh_online.h"

namespace {

// End costs and end selection of n streams from their carried columns: the tail of the form's one-shot sweep ('>=': the last of
// equal minima, decode.py:129-134; no frames: +inf / -1).  Lane = word; LANES 16: four streams to the block, DPP row = stream;
// 64: a block per stream.  BIGRAM_ROWS: state 0 of word w is row loop_row + W + w, else loop_row + 1 + w.
template <int LANES, bool BIGRAM_ROWS>
__global__ __launch_bounds__(64) void online_end_kernel(const gh_layerform* __restrict__ lf, const int32_t* __restrict__ end_slot,
                                                        int n_end, const double* __restrict__ prev, const int64_t* __restrict__ ids,
                                                        const int64_t* __restrict__ utt_off, int64_t n, double* __restrict__ end_cost,
                                                        int32_t* __restrict__ best_end) {
    const int lane = threadIdx.x, w = lane % LANES;
    const int64_t i = (int64_t)blockIdx.x * (64 / LANES) + lane / LANES;
    if (LANES < 64 && i >= n) return;                          // (64: grid = n)
    const int W = lf->W, N = lf->N, Lr = lf->loop_row;
    const int64_t stream = ids[i];
    const int64_t T = utt_off[i + 1] - utt_off[i];
    const double INF = INFINITY;
    double best_v = INF;
    int best_slot = -1;
    if (w < W)
        for (int s = 0; s < N; ++s) {
            const int r = s == 0 ? Lr + (BIGRAM_ROWS ? W : 1) + w : 1 + w * (N - 1) + (s - 1);
            const int es = end_slot[r];
            if (es >= 0) {
                const double v = T > 0 ? prev[(stream * N + s) * LANES + w] : INF;
                end_cost[i * n_end + es] = v;
                if (v < best_v || (v == best_v && es > best_slot)) { best_v = v; best_slot = es; }
            }
        }
#pragma unroll
    for (int o = LANES / 2; o >= 1; o >>= 1) {
        const double ov = __shfl_xor(best_v, o);
        const int os = __shfl_xor(best_slot, o);
        if (ov < best_v || (ov == best_v && os > best_slot)) { best_v = ov; best_slot = os; }
    }
    if (w == 0) best_end[i] = T > 0 ? best_slot : -1;
}

// The same for the K-layer lattice (two register sets): the tail of viterbi_layers_kernel.  A block per stream, lane = (layer mod 4,
// word); state s of word w in layer 4 h + kk is row layer * (P + 1) + 1 + w * N + s and lives in set h of the lane.
__global__ __launch_bounds__(64) void online_layers_end_kernel(const gh_layerform* __restrict__ lf, const int32_t* __restrict__ end_slot,
                                                               int n_end, const double* __restrict__ prev, const int64_t* __restrict__ ids,
                                                               const int64_t* __restrict__ utt_off, int64_t n, double* __restrict__ end_cost,
                                                               int32_t* __restrict__ best_end) {
    const int lane = threadIdx.x, kk = lane >> 4, w = lane & 15;
    const int64_t i = blockIdx.x;                              // (grid = n)
    const int W = lf->W, N = lf->N, K = lf->K, P = lf->P;
    const int64_t stream = ids[i];
    const int64_t T = utt_off[i + 1] - utt_off[i];
    const double INF = INFINITY;
    double best_v = INF;
    int best_slot = -1;
    if (w < W)
        for (int h = 0; h < 2; ++h) {
            const int layer = 4 * h + kk;
            if (layer >= K) continue;
            for (int s = 0; s < N; ++s) {
                const int es = end_slot[layer * (P + 1) + 1 + w * N + s];
                if (es >= 0) {
                    const double v = T > 0 ? prev[((stream * 2 + h) * N + s) * 64 + lane] : INF;
                    end_cost[i * n_end + es] = v;
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
    if (lane == 0) best_end[i] = T > 0 ? best_slot : -1;
}

int launch_online_end(gh_ctx* ctx, const gh_online* on, const int64_t* d_ids, const int64_t* d_utt_off, int64_t n, double* d_end_cost,
                      int32_t* d_best_end) {
    if (n <= 0) return GH_OK;
    const gh_online_form& fm = *on->form;
    const int per_block = 64 / fm.lanes;
    const auto kernel = fm.sets == 2   ? online_layers_end_kernel
                        : fm.lanes == 16 ? (fm.bigram_rows ? online_end_kernel<16, true> : online_end_kernel<16, false>)
                                         : (fm.bigram_rows ? online_end_kernel<64, true> : online_end_kernel<64, false>);
    hipLaunchKernelGGL(kernel, dim3((unsigned)((n + per_block - 1) / per_block)), dim3(64), 0, ctx->stream, on->lat->d_layers,
                       on->lat->d_lf_end_slot, on->lat->lat[0].n_end, on->d_prev, d_ids, d_utt_off, n, d_end_cost, d_best_end);
    GH_HIP(hipGetLastError());
    return GH_OK;
}

// ------------------------------------------------------------------------------------------------------------- create
// What a form takes for a graph: null, or what the graph is instead.  One graph, no beam: all forms.
const char* not_one_plain_graph(const gh_lattices* lat) {
    if (lat->L != 1 || lat->deferred_src) return "several graphs (one graph serves all streams)";
    if (lat->beam > 0) return "a rank beam is set on the graph";
    return nullptr;
}

int refuse(const char* who, const char* takes, const char* why) {
    gh_set_error("%s: %s, not %s", who, takes, why);
    return GH_ERR_UNSUPPORTED;
}

int check_loop(const char* who, const gh_lattices* lat) {
    const char* why = not_one_plain_graph(lat);
    if (why) {}
    else if (lat->bigram_ok) why = "a bigram grammar (gh_online_create_bigram takes it, with full history)";
    else if (lat->layers_ok && !lat->h_layers.loop) why = "a K-layer word lattice (gh_online_create_layers takes it)";
    else if (!lat->layers_ok || lat->h_layers.loop != 1) why = "a graph that is not in loop form";
    else if (lat->h_layers.W > GH_LAYERS_ROWW) why = "more than 16 words";
    return why ? refuse(who, "online decoding takes the word-loop grammar with up to 16 words", why) : GH_OK;
}

int check_bigram(const char* who, const gh_lattices* lat) {
    const char* why = not_one_plain_graph(lat);
    if (why) {}
    else if (lat->layers_ok && lat->h_layers.loop) why = "a word-loop graph (gh_online_create takes it)";
    else if (lat->layers_ok) why = "a K-layer word lattice (gh_online_create_layers takes it)";
    else if (!lat->bigram_ok) why = "a graph that is not in bigram form (more than 16 words, and 16 states with skip arcs, are not)";
    else if (!gh_bigram_n_ok(lat->h_layers.N, lat->h_layers.skip)) why = "a word size the bigram sweep is not built for";
    return why ? refuse(who, "online decoding takes the bigram grammar with up to 16 words", why) : GH_OK;
}

int check_wide(const char* who, const gh_lattices* lat) {
    const char* why = not_one_plain_graph(lat);
    if (why) {}
    else if (lat->bigram_ok) why = "a bigram grammar (gh_online_create_bigram takes it)";
    else if (lat->layers_ok && !lat->h_layers.loop) why = "a K-layer word lattice (gh_online_create_layers takes it)";
    else if (!lat->layers_ok || lat->h_layers.loop != 1) why = "a graph that is not in loop form";
    else if (lat->h_layers.W <= GH_LAYERS_ROWW) why = "16 words or fewer (gh_online_create takes it)";
    else if (lat->h_layers.W > GH_LAYERS_MAXW) why = "more than 64 words";
    else if (lat->h_layers.N > 8) why = "more than 8 states per word";
    return why ? refuse(who, "wide online decoding takes the word-loop grammar with 17 to 64 words of up to 8 states", why) : GH_OK;
}

int check_bigram_wide(const char* who, const gh_lattices* lat) {
    const char* why = not_one_plain_graph(lat);
    if (why) {}
    else if (lat->bigram_ok) why = "a bigram grammar of 16 words or fewer (gh_online_create_bigram takes it)";
    else if (lat->layers_ok && lat->h_layers.loop)
        why = lat->h_layers.W > GH_LAYERS_ROWW ? "a word-loop graph (gh_online_create_wide takes it)" : "a word-loop graph (gh_online_create takes it)";
    else if (lat->layers_ok) why = "a K-layer word lattice (gh_online_create_layers takes it)";
    else if (!lat->bigram_wide_ok) why = "a graph that is not in wide bigram form (more than 64 words, and more than 8 states per word, are not)";
    if (why) return refuse(who, "wide online bigram decoding takes the bigram grammar with 17 to 64 words of 2 to 8 states", why);
    GH_REQUIRE(lat->d_bigram_wide, "%s: internal: wide bigram form without its cost table", who);
    return GH_OK;
}
// (two register sets and 32-bit decision words: up to 8 layers of words of up to 8 states -- gh_viterbi_layers_online.hip)
int check_layers(const char* who, const gh_lattices* lat) {
    const char* why = not_one_plain_graph(lat);
    if (why) {}
    else if (lat->bigram_ok || lat->bigram_wide_ok) why = "a bigram grammar (gh_online_create_bigram and gh_online_create_bigram_wide take it)";
    else if (lat->layers_ok && lat->h_layers.loop) why = "a word-loop graph (gh_online_create and gh_online_create_wide take it)";
    else if (!lat->layers_ok) why = "a graph that is not in layer form";
    else if (lat->h_layers.W > GH_LAYERS_ROWW) why = "more than 16 words per layer (not offered yet)";
    else if (lat->h_layers.K > 8) why = "more than 8 layers (not offered yet)";
    else if (lat->h_layers.N > 8) why = "more than 8 states per word (not offered yet)";
    return why ? refuse(who, "online decoding of a K-layer word lattice takes 1 to 8 layers of up to 16 words of 2 to 8 states", why) : GH_OK;
}
static_assert(GH_LAYERS_ROWW == 16 && GH_LAYERS_MAXW == 64, "the word counts the messages above name");

// a session of form `id` with history for `frames` frames per stream: all a stream will ever take, or (window) its unsettled
// tail.  settles: it has anchors, and commit and tail serve it; `who` is the entry point, for the messages
int online_create(const char* who, gh_online_form_id id, bool settles, bool window, gh_ctx* ctx, const gh_lattices* lat, int64_t n_streams,
                  int64_t frames, gh_online** out) {
    GH_REQUIRE(ctx && lat && out, "%s: NULL argument", who);
    *out = nullptr;
    GH_REQUIRE(n_streams >= 1 && n_streams <= 0x7fffffff, "%s: n_streams=%lld", who, (long long)n_streams);
    GH_REQUIRE(frames >= 1 && frames <= 0x7fffffff, "%s: %s=%lld", who, window ? "window_frames" : "max_frames", (long long)frames);
    int rc = GH_OK;
    switch (id) {
        case GH_ONLINE_LOOP: rc = check_loop(who, lat); break;
        case GH_ONLINE_BIGRAM: rc = check_bigram(who, lat); break;
        case GH_ONLINE_WIDE: rc = check_wide(who, lat); break;
        case GH_ONLINE_BIGRAM_WIDE: rc = check_bigram_wide(who, lat); break;
        case GH_ONLINE_LAYERS: rc = check_layers(who, lat); break;
    }
    if (rc) return rc;
    const gh_online_form& fm = gh_online_forms[id];
    const gh_layerform& f = lat->h_layers;
    // the history (gh_online_form::cpw): frames <= 2^31 - 1, so the stride fits gh_layers_args::bp_off with room to spare;
    // streams x stride is checked before anything is allocated
    const int cpw = fm.cpw(f.N, f.skip != 0);
    const int64_t words = (frames + cpw - 1) / cpw + (window ? 1 : 0), stride = words * fm.lanes * 2;
    const size_t stream_bytes = (size_t)stride * 2 + (size_t)fm.sets * f.N * fm.lanes * sizeof(double) + (fm.open_word ? fm.lanes * 4 : 0) +
                                sizeof(gh_online_slot) + (settles ? sizeof(gh_online_anchor) : 0);
    if ((size_t)n_streams > (SIZE_MAX / 2 - 2048) / stream_bytes) {
        gh_set_error("%s: %lld streams x %lld frames (%.0f bytes): the size does not fit a size_t", who, (long long)n_streams,
                     (long long)frames, (double)n_streams * (double)stream_bytes);
        return GH_ERR_NOMEM;
    }
    GH_HIP(hipSetDevice(ctx->device));
    gh_online* on = new gh_online();
    on->ctx = ctx; on->lat = lat; on->form = &fm; on->settles = settles; on->n_streams = n_streams;
    on->max_frames = window ? 0x7fffffff : frames;
    on->window = window ? frames : 0;
    on->ring_words = (int32_t)std::min<int64_t>(words, 0x7fffffff);
    on->hist_stride = stride;
    on->frames.assign((size_t)n_streams, 0);
    on->settled.assign((size_t)n_streams, 0);
    on->seen.assign((size_t)n_streams, 0);
    auto pad = [](size_t b) { return (b + 255) & ~size_t(255); };
    const size_t b_prev = pad((size_t)n_streams * fm.sets * f.N * fm.lanes * sizeof(double)), b_open = fm.open_word ? pad((size_t)n_streams * fm.lanes * 4) : 0;
    const size_t b_hist = pad((size_t)n_streams * (size_t)stride * 2), b_slots = pad((size_t)n_streams * sizeof(gh_online_slot));
    const size_t b_anchor = settles ? pad((size_t)n_streams * sizeof(gh_online_anchor)) : 0;
    const size_t total = b_prev + b_open + b_hist + b_slots + b_anchor;
    hipError_t e = hipMalloc(&on->d_arena, total);
    if (e == hipSuccess) e = hipHostMalloc((void**)&on->h_slots, b_slots, hipHostMallocDefault);
    if (e == hipSuccess) e = hipEventCreateWithFlags(&on->copied, hipEventDisableTiming);
    if (e != hipSuccess) {
        gh_set_error("%s: %lld streams x %lld frames (%zu bytes): %s", who, (long long)n_streams, (long long)frames, total, hipGetErrorString(e));
        gh_online_destroy(on);
        return e == hipErrorOutOfMemory ? GH_ERR_NOMEM : GH_ERR_HIP;
    }
    char* p = static_cast<char*>(on->d_arena);
    on->d_prev = reinterpret_cast<double*>(p); p += b_prev;
    if (fm.open_word) on->d_open = reinterpret_cast<uint32_t*>(p);
    p += b_open;
    on->d_hist = reinterpret_cast<uint16_t*>(p); p += b_hist;
    on->d_slots = reinterpret_cast<gh_online_slot*>(p); p += b_slots;
    if (settles) on->d_anchor = reinterpret_cast<gh_online_anchor*>(p);   // (read only where `settled` says a stream has one)
    *out = on;
    return GH_OK;
}

// a wide session that does not settle is refused with its own sentence, whatever its rows; then a narrow bigram one
int refuse_unsettled(const gh_online* on, const char* who) {
    if (on->settles) return GH_OK;
    if (on->form->sets == 2)
        gh_set_error("%s: a session on a K-layer word lattice keeps its full history and does not settle (an utterance of exactly K "
                     "words is bounded in length); gh_online_result gives the running hypothesis", who);
    else if (on->form->lanes == 64)
        gh_set_error("%s: a wide session (more than 16 words) keeps its full history and does not settle; gh_online_result "
                     "gives the running hypothesis", who);
    else
        gh_set_error("%s: a bigram session has no settled prefix (its records need their own settle walk); gh_online_result gives the "
                     "running hypothesis", who);
    return GH_ERR_UNSUPPORTED;
}

// the streams a call names (NULL: all), checked; `distinct`: a stream may be named once
int tasks_of(gh_online* on, const char* who, int64_t& n, const int64_t* ids, bool distinct, std::vector<gh_settle_task>& tasks) {
    if (!ids) n = on->n_streams;
    tasks.resize((size_t)std::max<int64_t>(n, 0));
    for (int64_t i = 0; i < n; ++i) {
        const int64_t id = ids ? ids[i] : i;
        GH_REQUIRE(id >= 0 && id < on->n_streams, "%s: stream %lld out of range [0, %lld)", who, (long long)id, (long long)on->n_streams);
        gh_settle_task& t = tasks[(size_t)i];
        t.stream = (int32_t)id; t.T = (int32_t)on->frames[(size_t)id]; t.has_anchor = on->settled[(size_t)id] > 0; t.pad = 0;
    }
    if (distinct && ids) {
        int64_t twice = -1, k = 0;
        for (; k < n && twice < 0; ++k) {
            if (on->seen[(size_t)ids[k]]) twice = ids[k];
            on->seen[(size_t)ids[k]] = 1;
        }
        for (int64_t q = 0; q < k; ++q) on->seen[(size_t)ids[q]] = 0;
        GH_REQUIRE(twice < 0, "%s: stream %lld is named twice", who, (long long)twice);
    }
    return GH_OK;
}

// The label buffers of a result, commit or tail call: the caller's arrays (labels null: none wanted; begins: the timed twin)
// and their device side.  `slack`: labels the device buffers hold beyond label_off[n] (commit and tail: one).
struct LabelStage {
    const int32_t* row_label; int32_t* labels; const int64_t* label_off; int32_t* n_labels; int32_t* begins;
    int64_t n; int R; size_t slack;
    int32_t *d_rowlabel = nullptr, *d_nlabels = nullptr, *d_labels = nullptr, *d_begins = nullptr;
    int64_t* d_labeloff = nullptr;
    void carve(Carver& cv) {
        if (labels) { cv.add(&d_rowlabel, (size_t)R); cv.add(&d_labeloff, (size_t)n + 1); cv.add(&d_nlabels, (size_t)n); cv.add(&d_labels, (size_t)label_off[n] + slack); }
        if (begins) cv.add(&d_begins, (size_t)label_off[n] + slack);
    }
    int upload(hipStream_t st) const {
        if (!labels) return GH_OK;
        GH_HIP(hipMemcpyAsync(d_rowlabel, row_label, (size_t)R * 4, hipMemcpyHostToDevice, st));
        GH_HIP(hipMemcpyAsync(d_labeloff, label_off, (size_t)(n + 1) * 8, hipMemcpyHostToDevice, st));
        return GH_OK;
    }
    int fetch(hipStream_t st) const {
        if (!labels) return GH_OK;
        GH_HIP(hipMemcpyAsync(n_labels, d_nlabels, (size_t)n * 4, hipMemcpyDeviceToHost, st));
        if (label_off[n] > 0) GH_HIP(hipMemcpyAsync(labels, d_labels, (size_t)label_off[n] * 4, hipMemcpyDeviceToHost, st));
        if (begins && label_off[n] > 0) GH_HIP(hipMemcpyAsync(begins, d_begins, (size_t)label_off[n] * 4, hipMemcpyDeviceToHost, st));
        return GH_OK;
    }
};

// what the flag word of the walks and back-traces says (4: result with paths only); `lost`: the sentence of flag 2
int flag_error(const char* who, int flag, const char* lost) {
    if (flag & 4) gh_set_error("%s: path capacity of a stream too small", who);
    else if (flag & 2) gh_set_error("%s: %s", who, lost);
    else if (flag & 8) gh_set_error("%s: label capacity of a stream too small", who);
    return flag & 14 ? GH_ERR_INVALID : GH_OK;
}

// the walk arguments every commit and tail call fills alike
gh_settle_args settle_args(const gh_online* on, const gh_settle_task* d_tasks, int64_t n, const LabelStage& ls, int* d_flag) {
    gh_settle_args a;
    memset(&a, 0, sizeof a);
    a.lf = on->lat->d_layers; a.end_rows = on->lat->d_end_rows; a.tasks = d_tasks; a.n = n; a.prev = on->d_prev; a.hist = on->d_hist;
    a.hist_stride = on->hist_stride; a.ring_words = on->ring_words; a.anchor = on->d_anchor;
    a.row_label = ls.d_rowlabel; a.labels = ls.d_labels; a.label_off = ls.d_labeloff; a.n_labels = ls.d_nlabels; a.flag = d_flag;
    a.begins = ls.d_begins;
    return a;
}

}  // namespace

int gh_online_loop_trace(gh_ctx* ctx, const gh_online* on, const gh_layers_args& a, int64_t n, bool timed) {
    return gh_launch_lattice_backtrace(ctx, a, on->lat->h_layers, 0, n, timed);
}

// (the wide bigram back-trace reads the graph's cost table; a narrow bigram graph has none: null)
int gh_online_bigram_trace(gh_ctx* ctx, const gh_online* on, const gh_layers_args& a, int64_t n, bool timed) {
    return gh_launch_bigram_backtrace(ctx, a, on->lat->h_layers, 0, n, timed, on->lat->d_bigram_wide);
}

// --------------------------------------------------------------------------------------------------------------- C ABI
extern "C" int gh_online_create(gh_ctx* ctx, const gh_lattices* lat, int64_t n_streams, int64_t max_frames, gh_online** out) {
    return online_create("gh_online_create", GH_ONLINE_LOOP, true, false, ctx, lat, n_streams, max_frames, out);
}

extern "C" int gh_online_create_window(gh_ctx* ctx, const gh_lattices* lat, int64_t n_streams, int64_t window_frames, gh_online** out) {
    return online_create("gh_online_create_window", GH_ONLINE_LOOP, true, true, ctx, lat, n_streams, window_frames, out);
}

extern "C" int gh_online_create_bigram(gh_ctx* ctx, const gh_lattices* lat, int64_t n_streams, int64_t max_frames, gh_online** out) {
    return online_create("gh_online_create_bigram", GH_ONLINE_BIGRAM, false, false, ctx, lat, n_streams, max_frames, out);
}

extern "C" int gh_online_create_bigram_settle(gh_ctx* ctx, const gh_lattices* lat, int64_t n_streams, int64_t frames, int window,
                                              gh_online** out) {
    return online_create("gh_online_create_bigram_settle", GH_ONLINE_BIGRAM, true, window != 0, ctx, lat, n_streams, frames, out);
}

extern "C" int gh_online_create_wide(gh_ctx* ctx, const gh_lattices* lat, int64_t n_streams, int64_t max_frames, gh_online** out) {
    return online_create("gh_online_create_wide", GH_ONLINE_WIDE, false, false, ctx, lat, n_streams, max_frames, out);
}

extern "C" int gh_online_create_wide_settle(gh_ctx* ctx, const gh_lattices* lat, int64_t n_streams, int64_t frames, int window,
                                            gh_online** out) {
    return online_create("gh_online_create_wide_settle", GH_ONLINE_WIDE, true, window != 0, ctx, lat, n_streams, frames, out);
}

extern "C" int gh_online_create_bigram_wide(gh_ctx* ctx, const gh_lattices* lat, int64_t n_streams, int64_t max_frames, gh_online** out) {
    return online_create("gh_online_create_bigram_wide", GH_ONLINE_BIGRAM_WIDE, false, false, ctx, lat, n_streams, max_frames, out);
}

extern "C" int gh_online_create_bigram_wide_settle(gh_ctx* ctx, const gh_lattices* lat, int64_t n_streams, int64_t frames, int window,
                                                   gh_online** out) {
    return online_create("gh_online_create_bigram_wide_settle", GH_ONLINE_BIGRAM_WIDE, true, window != 0, ctx, lat, n_streams, frames, out);
}

extern "C" int gh_online_create_layers(gh_ctx* ctx, const gh_lattices* lat, int64_t n_streams, int64_t max_frames, gh_online** out) {
    return online_create("gh_online_create_layers", GH_ONLINE_LAYERS, false, false, ctx, lat, n_streams, max_frames, out);
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
    GH_REQUIRE(gh_seq_n_ok(f.N), "gh_online_push: %s form with %d states per word", on->form->grammar, f.N);
    GH_HIP(hipSetDevice(ctx->device));
    // longest chunks first: the four rows of a wave then end close to each other (a wave per stream: the long waves start first)
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
    const int rc = on->form->sweep(ctx, on, a, b->dtype == GH_F64);
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
    const int n_end = lat->lat[0].n_end, nlev = lat->lat[0].nlev;
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
    int32_t *d_best, *d_path = nullptr, *d_pathlen = nullptr;
    double* d_endcost;
    int64_t *d_ids, *d_uttoff, *d_bpoff, *d_pathoff = nullptr;
    LabelStage ls{row_label, labels, label_off, n_labels, out_begin, n, lat->lat[0].R, 0};
    Carver cv;
    cv.add(&d_flag, 64); cv.add(&d_best, (size_t)n); cv.add(&d_endcost, (size_t)n * n_end);
    cv.add(&d_ids, (size_t)n); cv.add(&d_uttoff, (size_t)n + 1); cv.add(&d_bpoff, (size_t)n);
    ls.carve(cv);
    if (path) { cv.add(&d_pathoff, (size_t)n + 1); cv.add(&d_pathlen, (size_t)n); cv.add(&d_path, (size_t)2 * path_off[n]); }
    int rc = cv.commit(ctx);
    if (rc) return rc;
    hipStream_t st = ctx->stream;
    GH_HIP(hipMemsetAsync(d_flag, 0, sizeof(int), st));
    GH_HIP(hipMemcpyAsync(d_ids, h_ids.data(), (size_t)n * 8, hipMemcpyHostToDevice, st));
    GH_HIP(hipMemcpyAsync(d_uttoff, utt_off.data(), (size_t)(n + 1) * 8, hipMemcpyHostToDevice, st));
    GH_HIP(hipMemcpyAsync(d_bpoff, bp_off.data(), (size_t)n * 8, hipMemcpyHostToDevice, st));
    if ((rc = ls.upload(st))) return rc;
    if (path) GH_HIP(hipMemcpyAsync(d_pathoff, path_off, (size_t)(n + 1) * 8, hipMemcpyHostToDevice, st));
    rc = launch_online_end(ctx, on, d_ids, d_uttoff, n, d_endcost, d_best);
    if (rc) return rc;
    // the one-shot decode's own back-trace on the history: utterance i = stream ids[i], its decision words at bp_off[i]
    gh_layers_args c;
    memset(&c, 0, sizeof c);
    c.lf = lat->d_layers; c.end_slot = lat->d_lf_end_slot; c.end_rows = lat->d_end_rows; c.n_end = n_end; c.S = 0;
    c.utt_off = d_uttoff; c.bp = on->d_hist; c.bp_off = d_bpoff; c.best_end = d_best; c.flag = d_flag;
    if (path) {
        c.path = d_path; c.path_off = d_pathoff; c.path_len = d_pathlen;
        rc = on->form->trace(ctx, on, c, n, false);
        if (rc) return rc;
    }
    if (labels) {
        c.row_label = ls.d_rowlabel; c.labels = ls.d_labels; c.label_off = ls.d_labeloff; c.n_labels = ls.d_nlabels;
        if (ls.d_begins) c.path = ls.d_begins;              // timed label mode: the begins go where a path launch has its path
        rc = on->form->trace(ctx, on, c, n, ls.d_begins != nullptr);
        if (rc) return rc;
    }
    int flag = 0;
    GH_HIP(hipMemcpyAsync(&flag, d_flag, sizeof(int), hipMemcpyDeviceToHost, st));
    if (best_end) GH_HIP(hipMemcpyAsync(best_end, d_best, (size_t)n * 4, hipMemcpyDeviceToHost, st));
    if (end_cost) GH_HIP(hipMemcpyAsync(end_cost, d_endcost, (size_t)n * n_end * 8, hipMemcpyDeviceToHost, st));
    if ((rc = ls.fetch(st))) return rc;
    if (path) {
        GH_HIP(hipMemcpyAsync(path_len, d_pathlen, (size_t)n * 4, hipMemcpyDeviceToHost, st));
        if (path_off[n] > 0) GH_HIP(hipMemcpyAsync(path, d_path, (size_t)2 * path_off[n] * 4, hipMemcpyDeviceToHost, st));
    }
    GH_HIP(hipStreamSynchronize(st));
    return flag_error("gh_online_result", flag, "back-trace reached a cell without predecessor");
}

extern "C" int gh_online_result(gh_ctx* ctx, gh_online* on, int64_t n, const int64_t* ids, double* end_cost, int32_t* best_end,
                                const int32_t* row_label, int32_t* labels, const int64_t* label_off, int32_t* n_labels,
                                int32_t* path, const int64_t* path_off, int32_t* path_len) {
    return gh_online_result_timed(ctx, on, n, ids, end_cost, best_end, row_label, labels, label_off, n_labels, path, path_off, path_len,
                                  nullptr);
}

extern "C" int gh_online_commit_timed(gh_ctx* ctx, gh_online* on, int64_t n, const int64_t* ids, int64_t* settled_frames,
                                      const int32_t* row_label, int32_t* labels, const int64_t* label_off, int32_t* n_new_labels,
                                      int32_t* out_begin) {
    GH_REQUIRE(ctx && on, "gh_online_commit: NULL argument");
    GH_REQUIRE(!out_begin || labels, "gh_online_commit_timed: out_begin needs labels");
    GH_REQUIRE(ctx == on->ctx, "gh_online_commit: the session belongs to another context");
    int rc = refuse_unsettled(on, "gh_online_commit");
    if (rc) return rc;
    GH_REQUIRE(!labels || (row_label && label_off && n_new_labels), "gh_online_commit: labels need row_label, label_off and n_new_labels");
    std::vector<gh_settle_task> tasks;
    rc = tasks_of(on, "gh_online_commit", n, ids, true, tasks);
    if (rc) return rc;
    if (n <= 0) return GH_OK;
    GH_HIP(hipSetDevice(ctx->device));
    int* d_flag;
    gh_settle_task* d_tasks;
    gh_online_anchor* d_cand;
    int64_t* d_settled;
    LabelStage ls{row_label, labels, label_off, n_new_labels, out_begin, n, on->lat->lat[0].R, 1};
    Carver cv;
    cv.add(&d_flag, 64); cv.add(&d_tasks, (size_t)n); cv.add(&d_cand, (size_t)n); cv.add(&d_settled, (size_t)n);
    ls.carve(cv);
    rc = cv.commit(ctx);
    if (rc) return rc;
    hipStream_t st = ctx->stream;
    GH_HIP(hipMemsetAsync(d_flag, 0, sizeof(int), st));
    GH_HIP(hipMemcpyAsync(d_tasks, tasks.data(), (size_t)n * sizeof(gh_settle_task), hipMemcpyHostToDevice, st));
    if ((rc = ls.upload(st))) return rc;
    gh_settle_args a = settle_args(on, d_tasks, n, ls, d_flag);
    a.cand = d_cand; a.settled_frames = d_settled;
    rc = on->form->walk(ctx, on, a, true, "gh_online_commit");
    if (rc) return rc;
    rc = on->form->walk(ctx, on, a, false, "gh_online_commit");
    if (rc) return rc;
    int flag = 0;
    std::vector<int64_t> h_settled((size_t)n);
    GH_HIP(hipMemcpyAsync(&flag, d_flag, sizeof(int), hipMemcpyDeviceToHost, st));
    GH_HIP(hipMemcpyAsync(h_settled.data(), d_settled, (size_t)n * 8, hipMemcpyDeviceToHost, st));
    if ((rc = ls.fetch(st))) return rc;
    GH_HIP(hipStreamSynchronize(st));
    // (the anchors on the device have moved whatever the flag says: the mirror follows them)
    for (int64_t i = 0; i < n; ++i) on->settled[(size_t)tasks[(size_t)i].stream] = h_settled[(size_t)i];
    if (settled_frames) memcpy(settled_frames, h_settled.data(), (size_t)n * 8);
    return flag_error("gh_online_commit", flag, "a trace reached a cell without predecessor or missed the anchor");
}

extern "C" int gh_online_commit(gh_ctx* ctx, gh_online* on, int64_t n, const int64_t* ids, int64_t* settled_frames,
                                const int32_t* row_label, int32_t* labels, const int64_t* label_off, int32_t* n_new_labels) {
    return gh_online_commit_timed(ctx, on, n, ids, settled_frames, row_label, labels, label_off, n_new_labels, nullptr);
}

extern "C" int gh_online_tail_timed(gh_ctx* ctx, gh_online* on, int64_t n, const int64_t* ids, double* end_cost, int32_t* best_end,
                                    const int32_t* row_label, int32_t* labels, const int64_t* label_off, int32_t* n_labels,
                                    int32_t* out_begin) {
    GH_REQUIRE(ctx && on, "gh_online_tail: NULL argument");
    GH_REQUIRE(!out_begin || labels, "gh_online_tail_timed: out_begin needs labels");
    GH_REQUIRE(ctx == on->ctx, "gh_online_tail: the session belongs to another context");
    int rc = refuse_unsettled(on, "gh_online_tail");
    if (rc) return rc;
    GH_REQUIRE(!labels || (row_label && label_off && n_labels), "gh_online_tail: labels need row_label, label_off and n_labels");
    std::vector<gh_settle_task> tasks;
    rc = tasks_of(on, "gh_online_tail", n, ids, false, tasks);
    if (rc) return rc;
    if (n <= 0) return GH_OK;
    const int n_end = on->lat->lat[0].n_end;
    std::vector<int64_t> h_ids((size_t)n), utt_off((size_t)n + 1, 0);
    for (int64_t i = 0; i < n; ++i) {
        h_ids[(size_t)i] = tasks[(size_t)i].stream;
        utt_off[(size_t)i + 1] = utt_off[(size_t)i] + tasks[(size_t)i].T;
    }
    GH_HIP(hipSetDevice(ctx->device));
    int* d_flag;
    gh_settle_task* d_tasks;
    double* d_endcost;
    int64_t *d_ids, *d_uttoff;
    int32_t* d_best;
    LabelStage ls{row_label, labels, label_off, n_labels, out_begin, n, on->lat->lat[0].R, 1};
    Carver cv;
    cv.add(&d_flag, 64); cv.add(&d_tasks, (size_t)n); cv.add(&d_best, (size_t)n); cv.add(&d_endcost, (size_t)n * n_end);
    cv.add(&d_ids, (size_t)n); cv.add(&d_uttoff, (size_t)n + 1);
    ls.carve(cv);
    rc = cv.commit(ctx);
    if (rc) return rc;
    hipStream_t st = ctx->stream;
    GH_HIP(hipMemsetAsync(d_flag, 0, sizeof(int), st));
    GH_HIP(hipMemcpyAsync(d_tasks, tasks.data(), (size_t)n * sizeof(gh_settle_task), hipMemcpyHostToDevice, st));
    GH_HIP(hipMemcpyAsync(d_ids, h_ids.data(), (size_t)n * 8, hipMemcpyHostToDevice, st));
    GH_HIP(hipMemcpyAsync(d_uttoff, utt_off.data(), (size_t)(n + 1) * 8, hipMemcpyHostToDevice, st));
    if ((rc = ls.upload(st))) return rc;
    rc = launch_online_end(ctx, on, d_ids, d_uttoff, n, d_endcost, d_best);
    if (rc) return rc;
    if (labels) {
        gh_settle_args a = settle_args(on, d_tasks, n, ls, d_flag);
        a.best_end = d_best;
        rc = on->form->walk(ctx, on, a, false, "gh_online_tail");
        if (rc) return rc;
    }
    int flag = 0;
    GH_HIP(hipMemcpyAsync(&flag, d_flag, sizeof(int), hipMemcpyDeviceToHost, st));
    if (best_end) GH_HIP(hipMemcpyAsync(best_end, d_best, (size_t)n * 4, hipMemcpyDeviceToHost, st));
    if (end_cost) GH_HIP(hipMemcpyAsync(end_cost, d_endcost, (size_t)n * n_end * 8, hipMemcpyDeviceToHost, st));
    if ((rc = ls.fetch(st))) return rc;
    GH_HIP(hipStreamSynchronize(st));
    return flag_error("gh_online_tail", flag, "back-trace reached a cell without predecessor or missed the anchor");
}

extern "C" int gh_online_tail(gh_ctx* ctx, gh_online* on, int64_t n, const int64_t* ids, double* end_cost, int32_t* best_end,
                              const int32_t* row_label, int32_t* labels, const int64_t* label_off, int32_t* n_labels) {
    return gh_online_tail_timed(ctx, on, n, ids, end_cost, best_end, row_label, labels, label_off, n_labels, nullptr);
}

// The forced commit: prunes, in the carried column of the named streams, the live cells whose trace does not pass the cell in
// which the chosen end's trace arrives in column T - 1 - max_tail (gh_online_force.hip).  The anchors do not move here: the
// gh_online_commit called next finds them.  Everything is checked before anything is enqueued.
extern "C" int gh_online_force(gh_ctx* ctx, gh_online* on, int64_t n, const int64_t* ids, int64_t max_tail, int32_t* pruned) {
    GH_REQUIRE(ctx && on, "gh_online_force: NULL argument");
    GH_REQUIRE(ctx == on->ctx, "gh_online_force: the session belongs to another context");
    GH_REQUIRE(max_tail >= 1, "gh_online_force: max_tail=%lld (at least one frame stays unsettled)", (long long)max_tail);
    std::vector<gh_settle_task> tasks;
    int rc = tasks_of(on, "gh_online_force", n, ids, true, tasks);
    if (rc) return rc;
    const gh_online_form& fm = *on->form;
    const char* why = nullptr;
    if (fm.sets == 2) why = "a session on a K-layer word lattice does not settle, and a forced commit for it is not built yet";
    else if (fm.lanes == 64 && fm.bigram_rows) why = "the forced commit of a wide bigram session (17 to 64 words) is not built yet";
    else if (fm.lanes == 64) why = "the forced commit of a wide session (17 to 64 words) is not built yet";
    else if (fm.bigram_rows) why = "the forced commit of a bigram session is not built yet (its records need their own marking)";
    if (why) {
        gh_set_error("gh_online_force: %s; the narrow loop session (gh_online_create, gh_online_create_window) has it", why);
        return GH_ERR_UNSUPPORTED;
    }
    rc = refuse_unsettled(on, "gh_online_force");
    if (rc) return rc;
    if (n <= 0) return GH_OK;
    GH_REQUIRE(pruned, "gh_online_force: pruned is NULL");
    GH_HIP(hipSetDevice(ctx->device));
    int* d_flag;
    gh_settle_task* d_tasks;
    int32_t* d_pruned;
    Carver cv;
    cv.add(&d_flag, 64); cv.add(&d_tasks, (size_t)n); cv.add(&d_pruned, (size_t)n);
    rc = cv.commit(ctx);
    if (rc) return rc;
    hipStream_t st = ctx->stream;
    GH_HIP(hipMemsetAsync(d_flag, 0, sizeof(int), st));
    GH_HIP(hipMemcpyAsync(d_tasks, tasks.data(), (size_t)n * sizeof(gh_settle_task), hipMemcpyHostToDevice, st));
    gh_force_args a;
    memset(&a, 0, sizeof a);
    a.lf = on->lat->d_layers; a.end_slot = on->lat->d_lf_end_slot; a.tasks = d_tasks; a.n = n; a.prev = on->d_prev; a.hist = on->d_hist;
    a.hist_stride = on->hist_stride; a.ring_words = on->ring_words; a.max_tail = (int)std::min<int64_t>(max_tail, 0x7fffffff);
    a.anchor = on->d_anchor; a.pruned = d_pruned; a.flag = d_flag;
    rc = gh_launch_online_loop_force(ctx, on, a);
    if (rc) return rc;
    int flag = 0;
    GH_HIP(hipMemcpyAsync(&flag, d_flag, sizeof(int), hipMemcpyDeviceToHost, st));
    GH_HIP(hipMemcpyAsync(pruned, d_pruned, (size_t)n * 4, hipMemcpyDeviceToHost, st));
    GH_HIP(hipStreamSynchronize(st));
    return flag_error("gh_online_force", flag, "the trace of the chosen end reached a cell without predecessor");
}
