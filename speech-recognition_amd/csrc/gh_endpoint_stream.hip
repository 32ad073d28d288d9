// Streaming endpoint detection: record_callback (sr/audio_capture/record.py:116-174) as the reference runs it -- once per
// chunk of audio, its state carried between calls -- for n_streams live recordings whose int16 audio arrives in pieces of
// any size.  CONTRACT: however a recording is cut, the events, frames_done and per-frame values of its stream are exactly
// gh_endpoints(max_segments = large) of the whole recording: the same integer sums, the same fp64 operations in the same
// order (this file is compiled with -ffp-contract=off like gh_endpoint.hip).
//   * after n samples a stream has classified gh_endpoint_frames(n) frames; frame i >= 1 is samples [i stride, i stride +
//     width), frame 0 keeps energy 0 and is never classified;
//   * carried per stream on the device: the classifier's registers (level, bg, attr, started, speech, silence: 32 B) and
//     the samples from the first sample of the next frame to classify up to the newest -- with width % stride == 0 fewer
//     than 2 width - stride of them -- in two buffers written in turn.  A stream at frame 0 starts from the initial
//     registers and a stream at sample 0 reads no carry: a reset touches nothing on the device.
// A push is three kernels, the one-shot split:
//   eps_energy_kernel    one wave per tile of up to 64 NEW frames of one stream; samples are addressed by absolute index
//                        (below n_before in the carry, from there on in the chunk), summed in units of Q samples as exact
//                        64-bit integers in LDS, then lane f adds the units of frame f.  Integer sums: the order is free.
//   eps_classify_kernel  one LANE per stream of the push: the recurrence continued from the carried registers over the new
//                        energies, stored back; emits events (start / end, and the closing event of a recording that ends
//                        while speech is open).
//   eps_carry_kernel     one wave per stream, behind the two above: the samples from the next frame's first one on go to
//                        the stream's OTHER carry buffer (never the one the energy waves read).
// The classifier step and the unit sums are COPIES of gh_endpoint.hip's: moving them into a shared header moved the machine
// code of all five one-shot kernels (register allocation; profiles/stream_endpoints_isa_fingerprint.txt), so the
// one-shot file stays as it is, as the online column step does beside gh_viterbi_layers.hip.
#include "gh_internal.h"
#include "gh_host.h"
#include <climits>

namespace {

constexpr int EPS_WAVES = 4;                 // tiles (waves) per workgroup of the energy kernel
constexpr size_t EPS_LDS_MAX = 40960;        // LDS per workgroup: four workgroups per CU stay resident

// the registers ep_classify_kernel holds between two frames
struct EpsState { double level, bg; int32_t speech, silence; uint8_t attr, started, pad[6]; };

// one stream of one push (host-built, uploaded with the chunk)
struct EpsSlot {
    int64_t chunk_off;            // first sample of its chunk in the uploaded samples
    int64_t n_before, n_after;    // samples it held before the push / holds now
    int64_t cbase, cnew;          // absolute index of sample 0 of the carry it reads / of the carry this push leaves behind
    int64_t f_first, f_end;       // frames [f_first, f_end) are newly complete (absolute indices)
    int64_t e_off;                // first energy (and per-frame output) of the push
    int64_t ev_off;               // first event slot of the push
    int32_t ev_cap;               // event slots it owns
    int32_t id, rd, end;          // stream; carry buffer to read (the other one is written); the recording ends here
};

struct EpsTile { int32_t slot, f0; };       // frames f_first + [f0, f0 + FT) of slot

template <int Q> struct eps_vec;
template <> struct eps_vec<8> { typedef short t __attribute__((ext_vector_type(8))); };
template <> struct eps_vec<4> { typedef short t __attribute__((ext_vector_type(4))); };
template <> struct eps_vec<2> { typedef short t __attribute__((ext_vector_type(2))); };
template <> struct eps_vec<1> { typedef short t; };

template <int Q> __device__ __forceinline__ unsigned long long eps_squares(const int16_t* p) {   // p: 2-byte aligned
    typename eps_vec<Q>::t v;
    __builtin_memcpy(&v, p, sizeof(v));
    if constexpr (Q == 1) {
        return (unsigned long long)((int)v * (int)v);
    } else {
        unsigned long long s = 0;
#pragma unroll
        for (int j = 0; j < Q; j += 2)      // two squares fit 32 bits (2 * 2^30), eight do not
            s += (unsigned)((int)v[j] * (int)v[j]) + (unsigned)((int)v[j + 1] * (int)v[j + 1]);
        return s;
    }
}

struct EpsEnergyArgs {
    const int16_t* chunk;         // the chunks of this push, back to back
    const int16_t* carry;         // [2][n_streams][cap]
    const EpsSlot* slot;
    const EpsTile* tiles; int64_t n_tiles;
    int64_t n_streams;
    int cap, width, stride, FT, units;            // units: LDS slots per wave, >= ((FT - 1) stride + width) / Q
    double* E;                                    // [new frames of the push]
};

template <int Q>
__global__ __launch_bounds__(64 * EPS_WAVES) void eps_energy_kernel(EpsEnergyArgs a) {
    extern __shared__ unsigned long long eps_lds[];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    unsigned long long* mine = eps_lds + (size_t)wv * a.units;
    const int64_t tile = (int64_t)blockIdx.x * EPS_WAVES + wv;
    int nF = 0, f0 = 0;
    int64_t fa = 0, e_off = 0, n_before = 0, cbase = 0;
    const int16_t *carry = a.carry, *chunk = a.chunk;
    if (tile < a.n_tiles) {
        const EpsTile t = a.tiles[tile];
        const EpsSlot s = a.slot[t.slot];
        const int64_t nf = s.f_end - s.f_first;
        f0 = t.f0;
        nF = (int)(nf - f0 < a.FT ? nf - f0 : a.FT);
        fa = s.f_first + f0;
        e_off = s.e_off;
        n_before = s.n_before;
        cbase = s.cbase;
        carry = a.carry + ((int64_t)s.rd * a.n_streams + s.id) * a.cap;
        chunk = a.chunk + s.chunk_off;
    }
    // every new frame is complete: it ends at or before n_after, and the first one begins at or behind cbase
    const int nu = nF > 0 ? ((nF - 1) * a.stride + a.width) / Q : 0;
    const int64_t p0 = fa * a.stride;
    for (int v = lane; v < nu; v += 64) {
        const int64_t p = p0 + (int64_t)v * Q;           // absolute index of the unit's first sample
        unsigned long long s;
        if (p + Q <= n_before) s = eps_squares<Q>(carry + (p - cbase));
        else if (p >= n_before) s = eps_squares<Q>(chunk + (p - n_before));
        else {                                           // the one unit that lies across the seam
            s = 0;
#pragma unroll
            for (int j = 0; j < Q; ++j) {
                const int64_t q = p + j;
                const int x = q < n_before ? carry[q - cbase] : chunk[q - n_before];
                s += (unsigned)(x * x);
            }
        }
        mine[v] = s;
    }
    __syncthreads();
    if (lane < nF) {
        const int first = lane * (a.stride / Q), cnt = a.width / Q;
        unsigned long long s = 0;
        for (int j = 0; j < cnt; ++j) s += mine[first + j];
        // calc_energy (:26-30); frame 0 is never classified and keeps energy 0 (:132-135)
        a.E[e_off + f0 + lane] = (s <= 1 || fa + lane == 0) ? 0.0 : 10 * log10((double)s);
    }
}

struct EpsClassifyArgs {
    const EpsSlot* slot; int64_t n;
    gh_endpoint_params p;
    const double* E;
    EpsState* state;                             // [n_streams]
    int64_t* ev_sample; uint8_t* ev_kind;        // [event slots]: sample; kind (0 start, 1 end) | open << 1
    int32_t* ev_n; uint8_t* started;             // [n] x 2
    int* flag;                                   // bit 0: a stream ran out of event slots
    uint8_t* o_attr; double *o_level, *o_bg;     // [new frames] zero filled, or all null
};

__global__ __launch_bounds__(64) void eps_classify_kernel(EpsClassifyArgs a) {
    const int64_t u = (int64_t)blockIdx.x * 64 + threadIdx.x;
    if (u >= a.n) return;
    const EpsSlot s = a.slot[u];
    const double* e = a.E + s.e_off - s.f_first;            // indexed by absolute frame
    const int64_t ob = s.e_off - s.f_first;
    const double ff = a.p.forget, ff1 = a.p.forget + 1, adj = a.p.adjustment, onset = a.p.onset, offset = a.p.offset;
    const int64_t stride = a.p.stride, width = a.p.width;
    double level = 0, bg = 0;
    bool attr = false, started = false;                     // attr: the previous frame's is_speech ATTRIBUTE (:188)
    int speech = 0, silence = 0, nev = 0;
    bool full = false;
    if (s.f_first > 0) {                                    // (a stream at frame 0 starts from the initial registers)
        const EpsState st = a.state[s.id];
        level = st.level; bg = st.bg; attr = st.attr != 0; started = st.started != 0; speech = st.speech; silence = st.silence;
    }
    auto emit = [&](int kind, int64_t sample) {
        if (nev < s.ev_cap) { a.ev_sample[s.ev_off + nev] = sample; a.ev_kind[s.ev_off + nev] = (uint8_t)kind; ++nev; }
        else full = true;
    };
    for (int64_t i = s.f_first > 1 ? s.f_first : 1; i < s.f_end; ++i) {
        // ---- the step of ep_classify_kernel (gh_endpoint.hip), a copy: see the header comment
        const double en = e[i];
        bool is_speech = false;                        // the RETURNED decision: drives the counters
        bool now = false;                              // this frame's attribute: what the next frame carries
        if (i <= 10) level = en;                       // (:182-183)
        else { level = (level + ff * en) / ff1; is_speech = attr; }   // (:186-188)
        if (i <= 10) bg = bg + en;                     // (:195-196) sum of E[0..10] in frame order, E[0] = 0
        if (i >= 10) {
            if (i == 10) bg = bg / 10;                 // (:197) eleven terms over ten
            else bg = bg + (en - bg) * adj;            // (:199-200)
            if (level < bg) level = bg;                // (:202-203) attribute stays False, the carried decision is returned
            else if (level - bg > onset) now = is_speech = true;
            else if (level - bg < offset) now = is_speech = false;
            else now = is_speech;
            if (a.o_attr) { a.o_attr[ob + i] = now; a.o_bg[ob + i] = bg; }
        }
        if (a.o_level) a.o_level[ob + i] = level;
        attr = now;
        if (is_speech) { ++speech; silence = 0; } else { ++silence; speech = 0; }     // (:152-157)
        if (speech > a.p.speech_frames && !started) {                                  // (:159-162)
            silence = 0;
            started = true;
            emit(0, i * stride);
        } else if (silence > a.p.silence_frames && started) {                          // (:164-169): re-arms, nothing else changes
            started = false;
            emit(1, i * stride + width);
        }
    }
    if (s.end && started) emit(1 | 2, s.n_after - 1);       // speech never ended: the open segment runs to the last sample
    if (s.f_end > 0) {
        EpsState st;
        st.level = level; st.bg = bg; st.speech = speech; st.silence = silence; st.attr = attr; st.started = started;
#pragma unroll
        for (int k = 0; k < 6; ++k) st.pad[k] = 0;
        a.state[s.id] = st;
    }
    a.ev_n[u] = nev;
    a.started[u] = started;
    if (full) atomicOr(a.flag, 1);
}

// One wave per stream of the push, behind the two kernels above: the samples from cnew on go to the stream's other carry
// buffer (never the one being read).
__global__ __launch_bounds__(64) void eps_carry_kernel(const EpsSlot* __restrict__ slot, const int16_t* __restrict__ chunk, int16_t* carry,
                                                       int64_t n_streams, int cap) {
    const EpsSlot s = slot[blockIdx.x];
    const int16_t* rd = carry + ((int64_t)s.rd * n_streams + s.id) * cap;
    int16_t* wr = carry + ((int64_t)(s.rd ^ 1) * n_streams + s.id) * cap;
    const int len = (int)(s.n_after - s.cnew);           // <= cap (checked on the host); 0 for a recording that ended
    for (int k = threadIdx.x; k < len; k += 64) {
        const int64_t i = s.cnew + k;
        wr[k] = i < s.n_before ? rd[i - s.cbase] : chunk[s.chunk_off + (i - s.n_before)];
    }
}

int eps_pick_q(int g) { return g % 8 == 0 ? 8 : (g % 4 == 0 ? 4 : (g % 2 == 0 ? 2 : 1)); }

}  // namespace

struct gh_epstream {
    gh_ctx* ctx;
    gh_endpoint_params prm;
    int64_t n_streams, max_chunk;
    int cap, Q, FT, units, ev_gap;     // carry samples per stream; unit width; frames per tile; LDS units per wave; frames between two events
    void* d_arena = nullptr;           // the one device allocation the two pointers below point into
    EpsState* d_state = nullptr;       // [n_streams]
    int16_t* d_carry = nullptr;        // [2][n_streams][cap]
    char* h_stage = nullptr;           // page-locked: a push's slots, tiles and samples on their way up
    size_t stage_bytes = 0;
    hipEvent_t copied = nullptr;       // the last upload from h_stage
    bool copy_pending = false;
    std::vector<int64_t> samples, frames;   // per stream: samples taken / frames classified since its last reset
    std::vector<uint8_t> ended, rd, seen;   // ... whether its recording has ended; which carry buffer holds its samples
    hipEvent_t ev[5] = {};             // gh_epstream_profile: around upload, energies, classifier, carry of a push
    bool profile = false;
    double phase_ms[4] = {0, 0, 0, 0};
    int64_t carry_base(int64_t n) const { return gh_endpoint_frames(n, prm.width, prm.stride) * prm.stride; }
};

extern "C" void gh_epstream_destroy(gh_epstream* ep) {
    if (!ep) return;
    (void)hipSetDevice(ep->ctx->device);
    (void)hipStreamSynchronize(ep->ctx->stream);
    if (ep->copied) (void)hipEventDestroy(ep->copied);
    if (ep->h_stage) (void)hipHostFree(ep->h_stage);
    if (ep->d_arena) (void)hipFree(ep->d_arena);
    for (hipEvent_t e : ep->ev) if (e) (void)hipEventDestroy(e);
    delete ep;
}

extern "C" int gh_epstream_create(gh_ctx* ctx, int64_t n_streams, const gh_endpoint_params* prm, int64_t max_chunk_samples,
                                  gh_epstream** out) {
    const char* who = "gh_epstream_create";
    GH_REQUIRE(ctx && prm && out, "%s: NULL argument", who);
    *out = nullptr;
    GH_REQUIRE(n_streams >= 1 && n_streams <= 0x7fffffff && max_chunk_samples >= 1 && max_chunk_samples <= ((int64_t)1 << 30),
               "%s: n_streams=%lld max_chunk_samples=%lld", who, (long long)n_streams, (long long)max_chunk_samples);
    const int width = prm->width, stride = prm->stride;
    GH_REQUIRE(width >= 1 && stride >= 1 && stride <= width && width <= (1 << 22), "%s: width=%d stride=%d (1 <= stride <= width <= 2^22)", who,
               width, stride);
    GH_REQUIRE(width % stride == 0,
               "%s: frames of %d samples every %d: a stream needs width %% stride == 0 -- otherwise the reference's frames fall behind the audio "
               "by %d samples per chunk, without bound; such recordings are for gh_endpoints", who, width, stride,
               width - (width / stride) * stride);
    const int Q = eps_pick_q(stride);                    // (gcd(width, stride) = stride)
    int FT = 64;
    auto units_of = [&](int ft) { return (size_t)((int64_t)(ft - 1) * stride + width) / Q; };
    while (FT > 1 && EPS_WAVES * units_of(FT) * 8 > EPS_LDS_MAX) FT >>= 1;
    if (EPS_WAVES * units_of(FT) * 8 > EPS_LDS_MAX) {
        gh_set_error("%s: frames of %d samples every %d are %d units of %d samples, more than the %d that fit LDS", who, width, stride, width / Q, Q,
                     (int)(EPS_LDS_MAX / (EPS_WAVES * 8)));
        return GH_ERR_UNSUPPORTED;
    }
    GH_HIP(hipSetDevice(ctx->device));
    gh_epstream* ep = new gh_epstream();
    ep->ctx = ctx; ep->prm = *prm; ep->n_streams = n_streams; ep->max_chunk = max_chunk_samples;
    ep->cap = 2 * width - stride;                        // the carry is SHORTER than this: see the header comment
    ep->Q = Q; ep->FT = FT; ep->units = (int)units_of(FT);
    // two events of a stream are at least min(speech_frames, silence_frames) + 1 frames apart: a start needs more than
    // speech_frames speech frames behind an end (which left speech = 0), an end more than silence_frames behind a start
    ep->ev_gap = std::max(1, std::min(prm->speech_frames, prm->silence_frames) + 1);
    ep->samples.assign((size_t)n_streams, 0);
    ep->frames.assign((size_t)n_streams, 0);
    ep->ended.assign((size_t)n_streams, 0);
    ep->rd.assign((size_t)n_streams, 0);
    ep->seen.assign((size_t)n_streams, 0);
    auto pad = [](size_t b) { return (b + 255) & ~size_t(255); };
    const size_t b_state = pad((size_t)n_streams * sizeof(EpsState)), b_carry = pad((size_t)2 * n_streams * ep->cap * 2);
    hipError_t e = hipMalloc(&ep->d_arena, b_state + b_carry);
    if (e == hipSuccess) e = hipEventCreateWithFlags(&ep->copied, hipEventDisableTiming);
    if (e != hipSuccess) {
        gh_set_error("%s: %lld streams (%zu bytes): %s", who, (long long)n_streams, b_state + b_carry, hipGetErrorString(e));
        gh_epstream_destroy(ep);
        return e == hipErrorOutOfMemory ? GH_ERR_NOMEM : GH_ERR_HIP;
    }
    ep->d_state = reinterpret_cast<EpsState*>(ep->d_arena);
    ep->d_carry = reinterpret_cast<int16_t*>(static_cast<char*>(ep->d_arena) + b_state);
    *out = ep;
    return GH_OK;
}

extern "C" int gh_epstream_profile(gh_epstream* ep, int on) {
    GH_REQUIRE(ep, "gh_epstream_profile: NULL argument");
    if (on) {
        GH_HIP(hipSetDevice(ep->ctx->device));
        for (hipEvent_t& e : ep->ev) if (!e) GH_HIP(hipEventCreate(&e));
    }
    ep->profile = on != 0;
    return GH_OK;
}

extern "C" int gh_epstream_phase_ms(const gh_epstream* ep, double* out) {
    GH_REQUIRE(ep && out, "gh_epstream_phase_ms: NULL argument");
    memcpy(out, ep->phase_ms, sizeof(ep->phase_ms));
    return GH_OK;
}

extern "C" int gh_epstream_reset(gh_epstream* ep, int64_t n, const int64_t* ids) {
    GH_REQUIRE(ep && n >= 0, "gh_epstream_reset: NULL argument");
    if (!ids) {
        std::fill(ep->samples.begin(), ep->samples.end(), 0);
        std::fill(ep->frames.begin(), ep->frames.end(), 0);
        std::fill(ep->ended.begin(), ep->ended.end(), 0);
        return GH_OK;
    }
    for (int64_t i = 0; i < n; ++i)
        GH_REQUIRE(ids[i] >= 0 && ids[i] < ep->n_streams, "gh_epstream_reset: stream %lld of %lld", (long long)ids[i], (long long)ep->n_streams);
    // (a stream at frame 0 starts from the initial registers and reads no carry: nothing on the device has to be cleared)
    for (int64_t i = 0; i < n; ++i) ep->samples[(size_t)ids[i]] = ep->frames[(size_t)ids[i]] = ep->ended[(size_t)ids[i]] = 0;
    return GH_OK;
}

extern "C" int gh_epstream_samples(const gh_epstream* ep, int64_t* out) {
    GH_REQUIRE(ep && out, "gh_epstream_samples: NULL argument");
    memcpy(out, ep->samples.data(), (size_t)ep->n_streams * 8);
    return GH_OK;
}

extern "C" int gh_epstream_push(gh_ctx* ctx, gh_epstream* ep, int64_t n, const int64_t* ids, const int16_t* samples,
                                const int64_t* sample_off, const uint8_t* end, int64_t ev_cap, int64_t* n_events, int64_t* ev_stream,
                                uint8_t* ev_kind, int64_t* ev_sample, uint8_t* ev_open, int64_t* frames_done, uint8_t* started,
                                const int64_t* frame_off, uint8_t* out_is_speech, double* out_level, double* out_background,
                                double* out_energy) {
    const char* who = "gh_epstream_push";
    GH_REQUIRE(ctx && ep && n_events && n >= 0 && (n == 0 || (ids && sample_off && frames_done && started)), "%s: NULL argument", who);
    GH_REQUIRE(ctx == ep->ctx, "%s: the session belongs to another context", who);
    GH_REQUIRE(ev_cap >= 0 && (ev_cap == 0 || (ev_stream && ev_kind && ev_sample && ev_open)), "%s: ev_cap=%lld without event arrays", who,
               (long long)ev_cap);
    const bool want_frames = out_is_speech || out_level || out_background || out_energy;
    GH_REQUIRE(!want_frames || (frame_off && out_is_speech && out_level && out_background && out_energy && frame_off[0] == 0),
               "%s: the per-frame outputs come together, with frame_off", who);
    *n_events = 0;
    if (n == 0) return GH_OK;
    GH_REQUIRE(sample_off[0] == 0, "%s: sample_off must start at 0", who);
    GH_REQUIRE(n <= ep->n_streams, "%s: %lld chunks for %lld streams", who, (long long)n, (long long)ep->n_streams);
    // ---- every check before anything is enqueued: a refused push moves no stream ----
    struct Seen {
        std::vector<uint8_t>& v; const int64_t* ids; int64_t n = 0;
        ~Seen() { for (int64_t k = 0; k < n; ++k) v[(size_t)ids[k]] = 0; }
    } seen{ep->seen, ids};
    const int width = ep->prm.width, stride = ep->prm.stride;
    std::vector<EpsSlot> slot((size_t)n);
    std::vector<EpsTile> tiles;
    int64_t NF = 0, NE = 0;
    for (int64_t u = 0; u < n; ++u) {
        const int64_t id = ids[u], len = sample_off[u + 1] - sample_off[u];
        GH_REQUIRE(id >= 0 && id < ep->n_streams, "%s: stream %lld of %lld", who, (long long)id, (long long)ep->n_streams);
        GH_REQUIRE(!ep->seen[(size_t)id], "%s: stream %lld is named twice", who, (long long)id);
        ep->seen[(size_t)id] = 1;
        seen.n = u + 1;
        GH_REQUIRE(len >= 0 && len <= ep->max_chunk, "%s: stream %lld gets %lld samples, max_chunk_samples %lld", who, (long long)id,
                   (long long)len, (long long)ep->max_chunk);
        GH_REQUIRE(!ep->ended[(size_t)id], "%s: stream %lld has ended (reset it first)", who, (long long)id);
        EpsSlot& s = slot[(size_t)u];
        s.id = (int32_t)id;
        s.rd = ep->rd[(size_t)id];
        s.end = end && end[u] ? 1 : 0;
        s.chunk_off = sample_off[u];
        s.n_before = ep->samples[(size_t)id];
        s.n_after = s.n_before + len;
        s.f_first = ep->frames[(size_t)id];
        s.f_end = gh_endpoint_frames(s.n_after, width, stride);
        s.cbase = s.f_first * stride;
        s.cnew = s.end ? s.n_after : s.f_end * stride;
        GH_REQUIRE(s.f_end < ((int64_t)1 << 31), "%s: stream %lld would hold %lld frames", who, (long long)id, (long long)s.f_end);
        GH_REQUIRE(s.f_end >= s.f_first && s.cnew >= s.cbase && s.cnew <= s.n_after && s.n_after - s.cnew < ep->cap &&
                   s.n_before - s.cbase < ep->cap && s.cbase <= s.n_before,
                   "%s: internal: stream %lld would carry %lld samples, room for %d", who, (long long)id, (long long)(s.n_after - s.cnew), ep->cap);
        const int64_t nf = s.f_end - s.f_first;
        GH_REQUIRE(!want_frames || frame_off[u + 1] - frame_off[u] == nf, "%s: frame_off gives stream %lld %lld new frames, it has %lld", who,
                   (long long)id, (long long)(frame_off[u + 1] - frame_off[u]), (long long)nf);
        s.e_off = NF;
        NF += nf;
        s.ev_off = NE;
        s.ev_cap = (int32_t)((nf + ep->ev_gap - 1) / ep->ev_gap + 1);      // ... plus one for the closing event
        NE += s.ev_cap;
        for (int64_t f0 = 0; f0 < nf; f0 += ep->FT) tiles.push_back({(int32_t)u, (int32_t)f0});
    }
    const int64_t total = sample_off[n], NT = (int64_t)tiles.size();
    GH_REQUIRE(samples || total == 0, "%s: samples is NULL", who);
    GH_REQUIRE(ev_cap >= NE, "%s: room for %lld events, this push can emit %lld ((new frames + %d) / %d + 1 per stream)", who, (long long)ev_cap,
               (long long)NE, ep->ev_gap - 1, ep->ev_gap);
    GH_HIP(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    // ---- the upload: slots, tiles and samples through the page-locked staging buffer, one copy ----
    auto pad = [](size_t b) { return (b + 255) & ~size_t(255); };
    const size_t b_slot = pad((size_t)n * sizeof(EpsSlot)), b_tile = pad((size_t)NT * sizeof(EpsTile)), b_pcm = pad((size_t)total * 2);
    const size_t b_up = b_slot + b_tile + b_pcm;
    if (ep->copy_pending) { GH_HIP(hipEventSynchronize(ep->copied)); ep->copy_pending = false; }   // (the staging buffer is free again)
    if (ep->stage_bytes < b_up) {
        if (ep->h_stage) (void)hipHostFree(ep->h_stage);
        ep->h_stage = nullptr; ep->stage_bytes = 0;
        const size_t want = b_up + b_up / 2;
        GH_HIP(hipHostMalloc((void**)&ep->h_stage, want, hipHostMallocDefault));
        ep->stage_bytes = want;
    }
    char* d_up; double *d_E, *d_level = nullptr, *d_bg = nullptr; int64_t* d_evs; uint8_t *d_evk, *d_started, *d_attr = nullptr;
    int32_t* d_evn; int* d_flag;
    Carver cv;
    cv.add(&d_up, b_up);
    cv.add(&d_E, (size_t)NF);
    cv.add(&d_evs, (size_t)NE);
    cv.add(&d_evn, (size_t)n);
    cv.add(&d_evk, (size_t)NE);
    cv.add(&d_started, (size_t)n);
    cv.add(&d_flag, 64);
    if (want_frames) { cv.add(&d_level, (size_t)NF); cv.add(&d_bg, (size_t)NF); cv.add(&d_attr, (size_t)NF); }
    int rc = cv.commit(ctx);
    if (rc) return rc;
    const EpsSlot* d_slot = reinterpret_cast<const EpsSlot*>(d_up);
    const EpsTile* d_tiles = reinterpret_cast<const EpsTile*>(d_up + b_slot);
    const int16_t* d_chunk = reinterpret_cast<const int16_t*>(d_up + b_slot + b_tile);
    memcpy(ep->h_stage, slot.data(), (size_t)n * sizeof(EpsSlot));
    if (NT) memcpy(ep->h_stage + b_slot, tiles.data(), (size_t)NT * sizeof(EpsTile));
    if (total) memcpy(ep->h_stage + b_slot + b_tile, samples, (size_t)total * 2);
    std::vector<int64_t> h_evs((size_t)NE);
    std::vector<uint8_t> h_evk((size_t)NE);
    std::vector<int32_t> h_evn((size_t)n);
    int flag = 0;
    hipError_t e = hipSuccess;
    int mark = 0;
    auto tick = [&] { if (ep->profile && e == hipSuccess) e = hipEventRecord(ep->ev[mark++], st); };
    tick();
    e = e == hipSuccess ? hipMemcpyAsync(d_up, ep->h_stage, b_slot + b_tile + (size_t)total * 2, hipMemcpyHostToDevice, st) : e;
    if (e == hipSuccess) e = hipEventRecord(ep->copied, st);
    if (e == hipSuccess) ep->copy_pending = true;
    if (e == hipSuccess) e = hipMemsetAsync(d_flag, 0, sizeof(int), st);
    if (e == hipSuccess && want_frames && NF) {
        e = hipMemsetAsync(d_level, 0, (size_t)NF * 8, st);
        if (e == hipSuccess) e = hipMemsetAsync(d_bg, 0, (size_t)NF * 8, st);
        if (e == hipSuccess) e = hipMemsetAsync(d_attr, 0, (size_t)NF, st);
    }
    tick();
    if (e == hipSuccess && NT) {
        EpsEnergyArgs ea;
        ea.chunk = d_chunk; ea.carry = ep->d_carry; ea.slot = d_slot; ea.tiles = d_tiles; ea.n_tiles = NT; ea.n_streams = ep->n_streams;
        ea.cap = ep->cap; ea.width = width; ea.stride = stride; ea.FT = ep->FT; ea.units = ep->units; ea.E = d_E;
        const dim3 grid((unsigned)((NT + EPS_WAVES - 1) / EPS_WAVES)), block(64 * EPS_WAVES);
        const size_t lds = (size_t)EPS_WAVES * ep->units * 8;
        if (ep->Q == 8) hipLaunchKernelGGL(eps_energy_kernel<8>, grid, block, lds, st, ea);
        else if (ep->Q == 4) hipLaunchKernelGGL(eps_energy_kernel<4>, grid, block, lds, st, ea);
        else if (ep->Q == 2) hipLaunchKernelGGL(eps_energy_kernel<2>, grid, block, lds, st, ea);
        else hipLaunchKernelGGL(eps_energy_kernel<1>, grid, block, lds, st, ea);
        e = hipGetLastError();
    }
    tick();
    if (e == hipSuccess) {
        EpsClassifyArgs ca;
        ca.slot = d_slot; ca.n = n; ca.p = ep->prm; ca.E = d_E; ca.state = ep->d_state; ca.ev_sample = d_evs; ca.ev_kind = d_evk;
        ca.ev_n = d_evn; ca.started = d_started; ca.flag = d_flag;
        ca.o_attr = d_attr; ca.o_level = d_level; ca.o_bg = d_bg;
        hipLaunchKernelGGL(eps_classify_kernel, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, st, ca);
        e = hipGetLastError();
    }
    tick();
    if (e == hipSuccess) {
        hipLaunchKernelGGL(eps_carry_kernel, dim3((unsigned)n), dim3(64), 0, st, d_slot, d_chunk, ep->d_carry, ep->n_streams, ep->cap);
        e = hipGetLastError();
    }
    tick();
    if (e == hipSuccess) e = hipMemcpyAsync(&flag, d_flag, sizeof(int), hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipMemcpyAsync(h_evn.data(), d_evn, (size_t)n * 4, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipMemcpyAsync(started, d_started, (size_t)n, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess && NE) e = hipMemcpyAsync(h_evs.data(), d_evs, (size_t)NE * 8, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess && NE) e = hipMemcpyAsync(h_evk.data(), d_evk, (size_t)NE, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess && want_frames && NF) {
        e = hipMemcpyAsync(out_is_speech, d_attr, (size_t)NF, hipMemcpyDeviceToHost, st);
        if (e == hipSuccess) e = hipMemcpyAsync(out_level, d_level, (size_t)NF * 8, hipMemcpyDeviceToHost, st);
        if (e == hipSuccess) e = hipMemcpyAsync(out_background, d_bg, (size_t)NF * 8, hipMemcpyDeviceToHost, st);
        if (e == hipSuccess) e = hipMemcpyAsync(out_energy, d_E, (size_t)NF * 8, hipMemcpyDeviceToHost, st);
    }
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e == hipSuccess) ep->copy_pending = false;
    for (int k = 0; k < 4 && ep->profile && e == hipSuccess; ++k) {
        float ms = 0;
        e = hipEventElapsedTime(&ms, ep->ev[k], ep->ev[k + 1]);
        ep->phase_ms[k] = ms;
    }
    if (e != hipSuccess) {
        gh_set_error("%s: %s", who, hipGetErrorString(e));
        return e == hipErrorOutOfMemory ? GH_ERR_NOMEM : GH_ERR_HIP;
    }
    // the kernels have run: the streams have moved, whatever the flag says
    for (int64_t u = 0; u < n; ++u) {
        const size_t id = (size_t)ids[u];
        ep->samples[id] = slot[(size_t)u].n_after;
        ep->frames[id] = slot[(size_t)u].f_end;
        ep->rd[id] ^= 1;
        if (slot[(size_t)u].end) ep->ended[id] = 1;
        frames_done[u] = slot[(size_t)u].f_end;
    }
    if (flag & 1) {
        gh_set_error("%s: internal: a stream emitted more events than the bound allows (%d frames between two events)", who, ep->ev_gap);
        return GH_ERR_HIP;
    }
    int64_t k = 0;
    for (int64_t u = 0; u < n; ++u)
        for (int32_t j = 0; j < h_evn[(size_t)u]; ++j, ++k) {
            const size_t at = (size_t)(slot[(size_t)u].ev_off + j);
            ev_stream[k] = ids[u];
            ev_kind[k] = h_evk[at] & 1;
            ev_open[k] = (h_evk[at] >> 1) & 1;
            ev_sample[k] = h_evs[at];
        }
    *n_events = k;
    return GH_OK;
}
