// Streaming MFCC / delta front-end: int16 PCM arrives per stream in chunks of any size, and every push returns exactly
// the feature frames [ceps | delta | delta-delta] that have become final, as a resident batch.  CONTRACT: a stream's
// concatenated output is bitwise gh_batch_create_from_pcm(mode 1) of that utterance ALONE, however the audio was cut.
//   * cepstral frame t is complete when t * step + flen <= n (n = samples so far); mfcc_kernel sends two frames through one
//     complex FFT, so a frame's bits depend on its partner: frames are paired (2m, 2m + 1) by ABSOLUTE index and a pair is
//     computed when both frames are complete; a trailing odd frame at the end pairs with a dead slot (live[1] == false);
//   * feature frame t is final when cepstra t + 2 exist (delta needs t + 1, delta-delta t + 2); at the end of the
//     utterance all ceil(n / step) frames come out, zero-extended like `segment`, with delta_feature's one-sided rules;
//   * carried per stream on the device: the samples from one before the first uncomputed pair (pre-emphasis) to the
//     newest, fewer than flen + 2 step + 1 of them, in two buffers written in turn; the last 4 cepstral rows (416 B).
//     A stream at sample 0 reads no carry: a reset touches nothing on the device.
// Normalisation is a FIXED affine map (per-utterance `standardize` is not causal): the raw value is rounded to the batch
// dtype, (x - mean) / std is evaluated in fp64 on that and rounded to the dtype; gh_batch_affine is the same map on any
// resident batch.  A front-end made by gh_stream_create_running applies the causal running mean / variance normalisation
// instead (gh_norm_running.hip): the stack kernel writes the raw rows, as it does without a map, and the
// running pass follows it in place; per stream it carries two fp64 sums per coefficient on the device (624 B) and the
// count of the frames they hold on the host.  A stream whose count is 0 reads no carried sums.
// The kernel body from the FFT to the DCT, the tables and build_tables are gh_mfcc_core.h's, the ones gh_mfcc.hip uses, and
// the delta rules are gh_delta.h's, the ones gh_frontend.hip uses: one text each, compiled here under the same flags.
#include "gh_mfcc_core.h"
#include "gh_delta.h"
#include "gh_norm_running.h"
#include <climits>

namespace {

// one stream of one push (host-built, uploaded with the chunk)
struct StreamSlot {
    int64_t chunk_off;            // first sample of its chunk in the uploaded samples
    int64_t n_before, n_after;    // samples it held before the push / holds now
    int64_t cbase, cnew;          // absolute index of sample 0 of the carry it reads / of the carry this push leaves behind
    int64_t c_first, c_end;       // cepstral frames [c_first, c_end) are computed by this push (c_first is even)
    int64_t f_first, f_end;       // feature frames [f_first, f_end) become final
    int64_t T;                    // frames of the whole utterance when it ends here, INT64_MAX while it is open
    int64_t out_off, ceps_off;    // first row in the output batch / in the scratch cepstra
    int64_t pair_off;             // first frame pair in the launch
    int32_t id, rd;               // stream; carry buffer to read (the other one is written)
};

struct StreamMfccArgs {
    const int16_t* chunk;         // the chunks of this push, back to back
    const int16_t* carry;         // [2][n_streams][cap]
    const StreamSlot* slot;
    const int32_t* pair_slot;     // slot of every frame pair (host-built table)
    int64_t n_pairs, n_streams;
    int cap, flen, fstep, pad_left;
    MfccTables t;
    double* ceps;                 // [new cepstral rows][NCEPS]
};

// One wave per frame pair, four pairs per workgroup: mfcc_kernel with samples addressed by ABSOLUTE index in the stream
// -- below n_before they sit in the carry, from there on in the chunk -- and the carried previous sample in front of a
// frame's first one (only absolute sample 0 is taken as it is).  A frame that is computed before the end is complete, so
// the zero extension (s0 + js < n_after) only ever acts at the end.
__global__ __launch_bounds__(256) void stream_mfcc_kernel(StreamMfccArgs a) {
    constexpr int S1 = MFCC_S1;
    __shared__ double s_x[4][8 * S1];
    __shared__ double s_lfb[4][2][NFILT];
    __shared__ double s_wup[NBIN], s_wdn[NBIN];          // per-bin filter weights, shared by the block
    for (int k = threadIdx.x; k < NBIN; k += 256) { s_wup[k] = a.t.wup[k]; s_wdn[k] = a.t.wdn[k]; }
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    double* ex = s_x[wv];
    const int64_t pr = (int64_t)blockIdx.x * 4 + wv;
    const bool have = pr < a.n_pairs;                    // a wave past the last pair walks the last pair's addresses, stores nothing
    const int64_t prc = have ? pr : a.n_pairs - 1;
    const StreamSlot s = a.slot[a.pair_slot[prc]];
    const int64_t fA = s.c_first + 2 * (prc - s.pair_off);   // frames fA (A) and fA + 1 (B) of the stream
    const int16_t* carry = a.carry + ((int64_t)s.rd * a.n_streams + s.id) * a.cap;
    const int16_t* chunk = a.chunk + s.chunk_off;
    int64_t s0[2];
    bool live[2];
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        live[h] = have && fA + h < s.c_end;
        s0[h] = (fA + h) * a.fstep;
    }
    auto sample_at = [&](int64_t i) {                    // cbase <= i < n_after
        const int16_t* p = i < s.n_before ? carry + (i - s.cbase) : chunk + (i - s.n_before);
        return (double)*p;
    };
    // ---- windowed, zero padded frames: lane l holds z[l + 64 j], j = 0..7 (loads unconditional on clamped addresses) ----
    c2 v[8];
    double cur[2][8], prv[2][8];
    const int64_t last = s.n_after - 1;                  // (a slot with a pair has n_after > c_first * step > cbase)
#pragma unroll
    for (int h = 0; h < 2; ++h) {
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            int64_t p = s0[h] + (lane + 64 * j - a.pad_left);
            p = p < s.cbase ? s.cbase : (p > last ? last : p);
            cur[h][j] = sample_at(p);
            prv[h][j] = sample_at(p > s.cbase ? p - 1 : p);
        }
    }
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const int js = lane + 64 * j - a.pad_left;
        const double w = a.t.window[lane + 64 * j];
        double xs[2];
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const bool in = live[h] && js >= 0 && js < a.flen && s0[h] + js < s.n_after;
            const double x = (s0[h] + js == 0) ? cur[h][j] : __dsub_rn(cur[h][j], __dmul_rn(0.97, prv[h][j]));
            xs[h] = in ? x * w : 0.0;
        }
        v[j] = (c2){xs[0], xs[1]};
    }
    double* o = a.ceps + (s.ceps_off + (fA - s.c_first)) * NCEPS;
    mfcc_pair_tail(a.t, v, ex, s_lfb[wv], s_wup, s_wdn, lane, [](double, double) {}, [&](double acc0, double acc1) {
        if (lane < NCEPS) {
            if (live[0]) o[lane] = acc0;
            if (live[1]) o[NCEPS + lane] = acc1;
        }
    });
}

// the affine map of the header comment
template <typename OT> __device__ __forceinline__ OT affine(double raw, const double* mean, const double* sd, int k) {
    const OT r = (OT)raw;
    return mean ? (OT)(((double)r - mean[k]) / sd[k]) : r;
}

// One workgroup per stream of the push: stack_kernel's delta_stack (t == 0; t == T - 1 only at the end) on cepstral
// rows t - 2 .. t + 2, of which those below c_first are carried (row r at r & 3) and the rest are new; then the affine
// map, straight into the output batch.
template <typename OT>
__global__ __launch_bounds__(256) void stream_stack_kernel(const StreamSlot* __restrict__ slot, const double* __restrict__ ceps,
                                                           const double* __restrict__ cc /*[n_streams][4][NCEPS]*/,
                                                           const double* __restrict__ mean, const double* __restrict__ sd,
                                                           OT* __restrict__ out) {
    const StreamSlot s = slot[blockIdx.x];
    const int nf = (int)(s.f_end - s.f_first);
    const double* old = cc + (int64_t)s.id * 4 * NCEPS;
    const double* fresh = ceps + s.ceps_off * NCEPS;
    auto f = [&](int64_t r, int c) { return r >= s.c_first ? fresh[(r - s.c_first) * NCEPS + c] : old[(r & 3) * NCEPS + c]; };
    for (int i = threadIdx.x; i < nf * NCEPS; i += blockDim.x) {
        const int64_t t = s.f_first + i / NCEPS;
        const int c = i % NCEPS;
        double x, d, dd;
        delta_stack(f, t, s.T, c, x, d, dd);
        OT* o = out + (s.out_off + i / NCEPS) * (3 * NCEPS);
        o[c] = affine<OT>(x, mean, sd, c);
        o[NCEPS + c] = affine<OT>(d, mean, sd, NCEPS + c);
        o[2 * NCEPS + c] = affine<OT>(dd, mean, sd, 2 * NCEPS + c);
    }
}

// One wave per stream of the push, after the two kernels above: the samples from cnew on go to the stream's other carry
// buffer (never the one being read), the newest of the last 4 cepstral rows to their places r & 3.
__global__ __launch_bounds__(64) void stream_carry_kernel(const StreamSlot* __restrict__ slot, const int16_t* __restrict__ chunk,
                                                          int16_t* carry, int64_t n_streams, int cap,
                                                          const double* __restrict__ ceps, double* __restrict__ cc) {
    const StreamSlot s = slot[blockIdx.x];
    const int16_t* rd = carry + ((int64_t)s.rd * n_streams + s.id) * cap;
    int16_t* wr = carry + ((int64_t)(s.rd ^ 1) * n_streams + s.id) * cap;
    const int len = (int)(s.n_after - s.cnew);           // <= cap (checked on the host); 0 for a stream that ended
    for (int k = threadIdx.x; k < len; k += 64) {
        const int64_t i = s.cnew + k;
        wr[k] = i < s.n_before ? rd[i - s.cbase] : chunk[s.chunk_off + (i - s.n_before)];
    }
    const int64_t r0 = s.c_end - 4 > s.c_first ? s.c_end - 4 : s.c_first;
    double* keep = cc + (int64_t)s.id * 4 * NCEPS;
    for (int k = threadIdx.x; k < (int)(s.c_end - r0) * NCEPS; k += 64) {
        const int64_t r = r0 + k / NCEPS;
        keep[(r & 3) * NCEPS + k % NCEPS] = ceps[(s.ceps_off + (r - s.c_first)) * NCEPS + k % NCEPS];
    }
}

template <typename OT>
__global__ __launch_bounds__(256) void affine_kernel(OT* __restrict__ x, int64_t n, int D, const double* __restrict__ mean,
                                                     const double* __restrict__ sd) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) x[i] = affine<OT>((double)x[i], mean, sd, (int)(i % D));
}

int check_affine(const char* who, const double* mean, const double* sd, int D) {
    for (int k = 0; k < D; ++k)
        GH_REQUIRE(std::isfinite(mean[k]) && std::isfinite(sd[k]) && sd[k] != 0.0, "%s: mean[%d]=%g std[%d]=%g", who, k, mean[k], k, sd[k]);
    return GH_OK;
}

}  // namespace

struct gh_stream {
    gh_ctx* ctx;
    gh_dtype dtype;
    int64_t n_streams, max_chunk;
    int flen, fstep, pad_left, cap;
    bool normalise;
    void* d_arena;                 // the one device allocation the pointers below point into
    MfccTables t;
    double *d_mean, *d_sd;         // [3 NCEPS] (unused without a map)
    int16_t* d_carry;              // [2][n_streams][cap]
    double* d_cc;                  // [n_streams][4][NCEPS]
    bool running = false, keep = false;    // the running normalisation; whether its statistics survive gh_stream_reset
    double prior_frames = 0.0;
    double *d_prior = nullptr, *d_norm = nullptr;   // [3][3 NCEPS] constants of the rule; [n_streams][2][3 NCEPS] carried sums
    std::vector<int64_t> norm_c;   // per stream: frames its carried sums hold (empty without the rule)
    std::vector<int64_t> samples;  // per stream: samples taken since its last reset
    std::vector<uint8_t> ended, rd;    // ... whether it has ended; which carry buffer holds its samples
    hipEvent_t ev[5] = {};         // gh_stream_profile: around upload, MFCC, stack, carry of a push
    bool profile = false;
    double phase_ms[4] = {0, 0, 0, 0};
    // first cepstral frame that is not computed after n samples of an open stream, and where its carry begins
    int64_t pairs_done(int64_t n) const { return n < flen ? 0 : (((n - flen) / fstep + 1) & ~int64_t(1)); }
    int64_t carry_base(int64_t n) const { return std::min(std::max<int64_t>(pairs_done(n) * fstep - 1, 0), n); }
};

// the rule of a front-end with the running normalisation (mean / std are then its prior)
struct RunningRule { double prior_frames, min_std; bool keep; };

static int stream_create(const char* who, gh_ctx* ctx, int64_t n_streams, int sample_rate, double frame_size, double frame_stride,
                         double low_freq, double high_freq, int64_t max_chunk_samples, gh_dtype dtype, const double* mean,
                         const double* std_, const RunningRule* run, gh_stream** out) {
    GH_REQUIRE(ctx && out, "%s: NULL argument", who);
    GH_REQUIRE(dtype == GH_F32 || dtype == GH_F64, "%s: bad dtype %d", who, (int)dtype);
    GH_REQUIRE(n_streams >= 1 && max_chunk_samples >= 1, "%s: n_streams=%lld max_chunk_samples=%lld", who,
               (long long)n_streams, (long long)max_chunk_samples);
    GH_REQUIRE((mean == nullptr) == (std_ == nullptr), "%s: mean and std come together", who);
    HostTables h;
    int rc = build_tables("gh_stream", sample_rate, frame_size, frame_stride, low_freq, high_freq, h);
    if (rc) return rc;
    if (run) {
        if ((rc = gh_norm_check(who, mean, std_, 3 * NCEPS, run->prior_frames, run->min_std))) return rc;
    } else if (mean && (rc = check_affine(who, mean, std_, 3 * NCEPS))) return rc;
    GH_HIP(hipSetDevice(ctx->device));
    gh_stream* fe = new gh_stream();
    fe->ctx = ctx; fe->dtype = dtype; fe->n_streams = n_streams; fe->max_chunk = max_chunk_samples;
    fe->flen = h.flen; fe->fstep = h.fstep; fe->pad_left = h.pad_left;
    fe->cap = h.flen + 2 * h.fstep + 2;
    fe->normalise = mean != nullptr && !run;
    fe->samples.assign((size_t)n_streams, 0);
    fe->ended.assign((size_t)n_streams, 0);
    fe->rd.assign((size_t)n_streams, 0);
    UploadArena ar;
    std::vector<double> vm(mean ? mean : h.window.data(), (mean ? mean : h.window.data()) + 3 * NCEPS);
    std::vector<double> vs(std_ ? std_ : h.window.data(), (std_ ? std_ : h.window.data()) + 3 * NCEPS);
    std::vector<int16_t> carry((size_t)2 * n_streams * fe->cap, 0);
    std::vector<double> cc((size_t)n_streams * 4 * NCEPS, 0.0);
    double *d_window, *d_tw, *d_wup, *d_wdn, *d_dct;
    int* d_seg;
    ar.add(&d_window, h.window); ar.add(&d_tw, h.tw); ar.add(&d_wup, h.wup); ar.add(&d_wdn, h.wdn);
    ar.add(&d_seg, h.seg); ar.add(&d_dct, h.dct);
    ar.add(&fe->d_mean, vm); ar.add(&fe->d_sd, vs);
    ar.add(&fe->d_carry, carry); ar.add(&fe->d_cc, cc);
    if (run) {
        fe->running = true; fe->keep = run->keep; fe->prior_frames = run->prior_frames;
        fe->norm_c.assign((size_t)n_streams, 0);
        ar.add(&fe->d_prior, gh_norm_prior(mean, std_, 3 * NCEPS, run->prior_frames, run->min_std));
        ar.add(&fe->d_norm, std::vector<double>((size_t)n_streams * 2 * 3 * NCEPS, 0.0));
    }
    rc = ar.commit(&fe->d_arena);
    if (rc) { if (fe->d_arena) (void)hipFree(fe->d_arena); delete fe; return rc; }
    fe->t.window = d_window; fe->t.tw = d_tw; fe->t.wup = d_wup; fe->t.wdn = d_wdn; fe->t.seg = d_seg; fe->t.dct = d_dct;
    *out = fe;
    return GH_OK;
}

extern "C" int gh_stream_create(gh_ctx* ctx, int64_t n_streams, int sample_rate, double frame_size, double frame_stride,
                                double low_freq, double high_freq, int64_t max_chunk_samples, gh_dtype dtype,
                                const double* mean, const double* std_, gh_stream** out) {
    return stream_create("gh_stream_create", ctx, n_streams, sample_rate, frame_size, frame_stride, low_freq, high_freq,
                         max_chunk_samples, dtype, mean, std_, nullptr, out);
}

extern "C" int gh_stream_create_running(gh_ctx* ctx, int64_t n_streams, int sample_rate, double frame_size, double frame_stride,
                                        double low_freq, double high_freq, int64_t max_chunk_samples, gh_dtype dtype,
                                        const double* mean, const double* std_, double prior_frames, double min_std,
                                        int keep_across_resets, gh_stream** out) {
    const RunningRule run{prior_frames, min_std, keep_across_resets != 0};
    return stream_create("gh_stream_create_running", ctx, n_streams, sample_rate, frame_size, frame_stride, low_freq, high_freq,
                         max_chunk_samples, dtype, mean, std_, &run, out);
}

extern "C" void gh_stream_destroy(gh_stream* fe) {
    if (!fe) return;
    if (fe->d_arena) (void)hipFree(fe->d_arena);
    for (hipEvent_t e : fe->ev) if (e) (void)hipEventDestroy(e);
    delete fe;
}

extern "C" int gh_stream_profile(gh_stream* fe, int on) {
    GH_REQUIRE(fe, "gh_stream_profile: NULL argument");
    if (on) {
        GH_HIP(hipSetDevice(fe->ctx->device));
        for (hipEvent_t& e : fe->ev) if (!e) GH_HIP(hipEventCreate(&e));
    }
    fe->profile = on != 0;
    return GH_OK;
}

extern "C" int gh_stream_phase_ms(const gh_stream* fe, double* out) {
    GH_REQUIRE(fe && out, "gh_stream_phase_ms: NULL argument");
    memcpy(out, fe->phase_ms, sizeof(fe->phase_ms));
    return GH_OK;
}

extern "C" int gh_stream_reset(gh_stream* fe, int64_t n, const int64_t* ids) {
    GH_REQUIRE(fe && n >= 0, "gh_stream_reset: NULL argument");
    const bool stats = fe->running && !fe->keep;           // every utterance is normalised alone
    if (!ids) {
        std::fill(fe->samples.begin(), fe->samples.end(), 0);
        std::fill(fe->ended.begin(), fe->ended.end(), 0);
        if (stats) std::fill(fe->norm_c.begin(), fe->norm_c.end(), 0);
        return GH_OK;
    }
    for (int64_t i = 0; i < n; ++i)
        GH_REQUIRE(ids[i] >= 0 && ids[i] < fe->n_streams, "gh_stream_reset: stream %lld of %lld", (long long)ids[i], (long long)fe->n_streams);
    for (int64_t i = 0; i < n; ++i) {
        fe->samples[(size_t)ids[i]] = 0; fe->ended[(size_t)ids[i]] = 0;
        if (stats) fe->norm_c[(size_t)ids[i]] = 0;
    }
    return GH_OK;
}

extern "C" int gh_stream_reset_stats(gh_stream* fe, int64_t n, const int64_t* ids) {
    GH_REQUIRE(fe && n >= 0, "gh_stream_reset_stats: NULL argument");
    for (int64_t i = 0; ids && i < n; ++i)
        GH_REQUIRE(ids[i] >= 0 && ids[i] < fe->n_streams, "gh_stream_reset_stats: stream %lld of %lld", (long long)ids[i], (long long)fe->n_streams);
    if (!fe->running) return GH_OK;                        // nothing to clear
    if (!ids) std::fill(fe->norm_c.begin(), fe->norm_c.end(), 0);
    else for (int64_t i = 0; i < n; ++i) fe->norm_c[(size_t)ids[i]] = 0;
    return GH_OK;
}

extern "C" int gh_stream_norm_frames(const gh_stream* fe, int64_t* out) {
    GH_REQUIRE(fe && out, "gh_stream_norm_frames: NULL argument");
    if (fe->running) memcpy(out, fe->norm_c.data(), (size_t)fe->n_streams * 8);
    else memset(out, 0, (size_t)fe->n_streams * 8);
    return GH_OK;
}

extern "C" int gh_stream_samples(const gh_stream* fe, int64_t* out) {
    GH_REQUIRE(fe && out, "gh_stream_samples: NULL argument");
    memcpy(out, fe->samples.data(), (size_t)fe->n_streams * 8);
    return GH_OK;
}

extern "C" int gh_stream_push(gh_ctx* ctx, gh_stream* fe, int64_t n, const int64_t* ids, const int16_t* samples,
                              const int64_t* sample_off, const uint8_t* end, gh_batch** out) {
    const char* who = "gh_stream_push";
    GH_REQUIRE(ctx && fe && out && n >= 0 && (n == 0 || (ids && sample_off)), "%s: NULL argument", who);
    GH_REQUIRE(ctx == fe->ctx, "%s: the front-end belongs to another context", who);
    // ---- every check before anything is enqueued: a refused push moves no stream ----
    static const int64_t zero = 0;
    if (n == 0) sample_off = &zero;
    GH_REQUIRE(sample_off[0] == 0, "%s: sample_off must start at 0", who);
    std::vector<uint8_t> seen((size_t)fe->n_streams, 0);
    std::vector<StreamSlot> slot((size_t)n);
    std::vector<int64_t> f_off((size_t)n + 1, 0);
    std::vector<int32_t> pair_slot;
    std::vector<NormSlot> nslot(fe->running ? (size_t)n : 0);
    int64_t n_ceps = 0;
    for (int64_t u = 0; u < n; ++u) {
        const int64_t id = ids[u], len = sample_off[u + 1] - sample_off[u];
        GH_REQUIRE(id >= 0 && id < fe->n_streams, "%s: stream %lld of %lld", who, (long long)id, (long long)fe->n_streams);
        GH_REQUIRE(!seen[(size_t)id], "%s: stream %lld is named twice", who, (long long)id);
        seen[(size_t)id] = 1;
        GH_REQUIRE(len >= 0 && len <= fe->max_chunk, "%s: stream %lld gets %lld samples, max_chunk_samples %lld", who, (long long)id,
                   (long long)len, (long long)fe->max_chunk);
        GH_REQUIRE(!fe->ended[(size_t)id], "%s: stream %lld has ended (reset it first)", who, (long long)id);
        StreamSlot& s = slot[(size_t)u];
        s.id = (int32_t)id;
        s.rd = fe->rd[(size_t)id];
        s.chunk_off = sample_off[u];
        s.n_before = fe->samples[(size_t)id];
        s.n_after = s.n_before + len;
        s.cbase = fe->carry_base(s.n_before);
        s.c_first = fe->pairs_done(s.n_before);
        s.f_first = std::max<int64_t>(s.c_first - 2, 0);
        if (end && end[u]) {
            const int64_t T = (s.n_after + fe->fstep - 1) / fe->fstep;
            GH_REQUIRE(s.n_after >= 1 && T >= 2, "%s: stream %lld ends with %lld samples, fewer than 2 frames (delta_feature indexes feat[i + 1])",
                       who, (long long)id, (long long)s.n_after);
            s.T = s.c_end = s.f_end = T;
            s.cnew = s.n_after;
        } else {
            s.T = INT64_MAX;
            s.c_end = fe->pairs_done(s.n_after);
            s.f_end = std::max<int64_t>(s.c_end - 2, 0);
            s.cnew = fe->carry_base(s.n_after);
        }
        GH_REQUIRE(s.cnew >= s.cbase && s.n_after - s.cnew <= fe->cap && s.n_before - s.cbase <= fe->cap,
                   "%s: internal: stream %lld would carry %lld samples, room for %d", who, (long long)id, (long long)(s.n_after - s.cnew), fe->cap);
        s.out_off = f_off[(size_t)u];
        f_off[(size_t)u + 1] = s.out_off + (s.f_end - s.f_first);
        if (fe->running) nslot[(size_t)u] = NormSlot{s.out_off, s.f_end - s.f_first, fe->norm_c[(size_t)id], id};
        s.ceps_off = n_ceps;
        n_ceps += s.c_end - s.c_first;
        s.pair_off = (int64_t)pair_slot.size();
        pair_slot.insert(pair_slot.end(), (size_t)((s.c_end - s.c_first + 1) / 2), (int32_t)u);
    }
    const int64_t total = sample_off[n], N = f_off[(size_t)n], n_pairs = (int64_t)pair_slot.size();
    GH_REQUIRE(samples || total == 0, "%s: samples is NULL", who);
    GH_HIP(hipSetDevice(ctx->device));
    const size_t esz = fe->dtype == GH_F64 ? 8 : 4;
    void* feats = nullptr;
    if (N > 0) GH_HIP(hipMalloc(&feats, (size_t)N * 3 * NCEPS * esz));
    gh_batch* b = nullptr;
    int rc = gh_batch_wrap(ctx, fe->dtype, 3 * NCEPS, N, n, feats, f_off.data(), &b);
    if (rc) { if (feats) (void)hipFree(feats); return rc; }
    b->feats = feats;
    b->owns_feats = true;
    if (n > 0) {
        int16_t* d_chunk;
        StreamSlot* d_slot;
        int32_t* d_pair;
        double* d_ceps;
        NormSlot* d_nslot = nullptr;
        Carver cv;
        cv.add(&d_chunk, (size_t)total + 1);
        cv.add(&d_slot, (size_t)n);
        cv.add(&d_pair, (size_t)n_pairs + 1);
        cv.add(&d_ceps, (size_t)(n_ceps + 1) * NCEPS);
        if (fe->running) cv.add(&d_nslot, (size_t)n);
        if ((rc = cv.commit(ctx))) { gh_batch_destroy(b); return rc; }
        hipStream_t st = ctx->stream;
        hipError_t e = hipSuccess;
        int mark = 0;
        auto tick = [&] { if (fe->profile && e == hipSuccess) e = hipEventRecord(fe->ev[mark++], st); };
        tick();
        if (total && e == hipSuccess) e = hipMemcpyAsync(d_chunk, samples, (size_t)total * 2, hipMemcpyHostToDevice, st);
        if (e == hipSuccess) e = hipMemcpyAsync(d_slot, slot.data(), (size_t)n * sizeof(StreamSlot), hipMemcpyHostToDevice, st);
        if (e == hipSuccess && n_pairs) e = hipMemcpyAsync(d_pair, pair_slot.data(), (size_t)n_pairs * 4, hipMemcpyHostToDevice, st);
        if (e == hipSuccess && fe->running) e = hipMemcpyAsync(d_nslot, nslot.data(), (size_t)n * sizeof(NormSlot), hipMemcpyHostToDevice, st);
        tick();
        if (e == hipSuccess && n_pairs) {
            StreamMfccArgs a;
            a.chunk = d_chunk; a.carry = fe->d_carry; a.slot = d_slot; a.pair_slot = d_pair;
            a.n_pairs = n_pairs; a.n_streams = fe->n_streams;
            a.cap = fe->cap; a.flen = fe->flen; a.fstep = fe->fstep; a.pad_left = fe->pad_left;
            a.t = fe->t; a.ceps = d_ceps;
            hipLaunchKernelGGL(stream_mfcc_kernel, dim3((unsigned)((n_pairs + 3) / 4)), dim3(256), 0, st, a);
            e = hipGetLastError();
        }
        tick();
        if (e == hipSuccess && N > 0) {
            const double* m = fe->normalise ? fe->d_mean : nullptr;
            if (fe->dtype == GH_F64)
                hipLaunchKernelGGL((stream_stack_kernel<double>), dim3((unsigned)n), dim3(256), 0, st, d_slot, d_ceps, fe->d_cc, m, fe->d_sd, (double*)feats);
            else
                hipLaunchKernelGGL((stream_stack_kernel<float>), dim3((unsigned)n), dim3(256), 0, st, d_slot, d_ceps, fe->d_cc, m, fe->d_sd, (float*)feats);
            e = hipGetLastError();
            // the running normalisation, in place on the raw rows (counted in this phase)
            if (e == hipSuccess && fe->running)
                e = gh_norm_launch(st, fe->dtype, feats, 3 * NCEPS, d_nslot, n, fe->d_prior, fe->prior_frames, fe->d_norm);
        }
        tick();
        if (e == hipSuccess) {
            hipLaunchKernelGGL(stream_carry_kernel, dim3((unsigned)n), dim3(64), 0, st, d_slot, d_chunk, fe->d_carry, fe->n_streams, fe->cap,
                               d_ceps, fe->d_cc);
            e = hipGetLastError();
        }
        tick();
        if (e == hipSuccess) e = hipStreamSynchronize(st);   // (the uploads come from the caller's and this call's host memory)
        for (int k = 0; k < 4 && fe->profile && e == hipSuccess; ++k) {
            float ms = 0;
            e = hipEventElapsedTime(&ms, fe->ev[k], fe->ev[k + 1]);
            fe->phase_ms[k] = ms;
        }
        if (e != hipSuccess) {
            gh_set_error("%s: %s", who, hipGetErrorString(e));
            gh_batch_destroy(b);
            return e == hipErrorOutOfMemory ? GH_ERR_NOMEM : GH_ERR_HIP;
        }
    }
    for (int64_t u = 0; u < n; ++u) {
        const size_t id = (size_t)ids[u];
        fe->samples[id] = slot[(size_t)u].n_after;
        fe->rd[id] ^= 1;
        if (fe->running) fe->norm_c[id] += nslot[(size_t)u].nf;
        if (end && end[u]) fe->ended[id] = 1;
    }
    *out = b;
    return GH_OK;
}

extern "C" int gh_batch_affine(gh_ctx* ctx, gh_batch* b, const double* mean, const double* std_) {
    GH_REQUIRE(ctx && b && mean && std_, "gh_batch_affine: NULL argument");
    int rc = check_affine("gh_batch_affine", mean, std_, b->D);
    if (rc) return rc;
    const int64_t n = b->N * b->D;
    if (n == 0) return GH_OK;
    GH_HIP(hipSetDevice(ctx->device));
    double *d_mean, *d_sd;
    Carver cv;
    cv.add(&d_mean, (size_t)b->D);
    cv.add(&d_sd, (size_t)b->D);
    if ((rc = cv.commit(ctx))) return rc;
    hipStream_t st = ctx->stream;
    GH_HIP(hipMemcpyAsync(d_mean, mean, (size_t)b->D * 8, hipMemcpyHostToDevice, st));
    GH_HIP(hipMemcpyAsync(d_sd, std_, (size_t)b->D * 8, hipMemcpyHostToDevice, st));
    const dim3 grid((unsigned)((n + 255) / 256)), block(256);
    if (b->dtype == GH_F64) hipLaunchKernelGGL((affine_kernel<double>), grid, block, 0, st, (double*)b->feats, n, b->D, d_mean, d_sd);
    else hipLaunchKernelGGL((affine_kernel<float>), grid, block, 0, st, (float*)b->feats, n, b->D, d_mean, d_sd);
    GH_HIP(hipGetLastError());
    GH_HIP(hipStreamSynchronize(st));
    b->nll_serial = 0;             // likelihoods the batch may hold belong to the features it had
    return GH_OK;
}
