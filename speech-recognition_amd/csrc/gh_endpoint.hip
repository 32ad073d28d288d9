// Endpoint detection of AudioRecorder (sr/audio_capture/record.py:116-217) for a batch of int16 recordings.
// The reference runs inside a PyAudio callback, one chunk of `samples per frame` samples at a time: frame 0 is the first
// chunk, every later chunk appends int(width / stride) frames of `width` samples every `stride` (:132-147), each new
// frame goes through classify_frame (:176-217) and the speech / silence counters (:152-169).  Here:
//   ep_energy_kernel   calc_energy (:23-31) of every frame.  One wave per tile of up to 64 consecutive frames of one
//                      recording: the tile's samples are read once, 16 bytes per lane and 1 KiB per wave instruction,
//                      as sums of squares over units of Q = 8 samples (the widest power of two that divides
//                      gcd(width, stride), at most one 16-byte load) kept in LDS as exact 64-bit integers; lane f then
//                      adds the width / Q units of frame f, applies the `<= 1` rule and 10 log10 in fp64.
//   ep_classify_kernel the classifier and the counters, one LANE per recording over the energies above, in the
//                      reference's order of operations in fp64 (this file is compiled with -ffp-contract=off: log10 is
//                      the only operation whose rounding can differ from numpy's).  The recurrence is sequential by
//                      design: level and background are clamped affine maps that would compose, but not with the
//                      reference's roundings.  A lane stops at its recording's last segment.
// max_segments > 1 re-arms the detector after an end with every piece of state left as it is.
#include "gh_internal.h"
#include "gh_host.h"

namespace {

constexpr int EP_WAVES = 4;                 // tiles (waves) per workgroup of the energy kernel
constexpr size_t EP_LDS_MAX = 40960;        // LDS per workgroup: four workgroups per CU stay resident

struct EpTile { int32_t u, f0; };           // frames [f0, f0 + FT) of recording u (chunk-local)

template <int Q> struct ep_vec;
template <> struct ep_vec<8> { typedef short t __attribute__((ext_vector_type(8))); };
template <> struct ep_vec<4> { typedef short t __attribute__((ext_vector_type(4))); };
template <> struct ep_vec<2> { typedef short t __attribute__((ext_vector_type(2))); };
template <> struct ep_vec<1> { typedef short t; };

// Q samples at p (2-byte aligned: a recording starts anywhere in the concatenated batch) and the sum of their squares
template <int Q> __device__ __forceinline__ typename ep_vec<Q>::t ep_load(const int16_t* p) {
    typename ep_vec<Q>::t v;
    __builtin_memcpy(&v, p, sizeof(v));
    return v;
}
template <int Q> __device__ __forceinline__ unsigned long long ep_squares(typename ep_vec<Q>::t v) {
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

struct EpEnergyArgs {
    const int16_t* pcm; const int64_t* s_off;     // [n + 1] first sample of every recording of the chunk in `pcm`
    const int64_t* f_off;                         // [n + 1] chunk-local frame offsets
    const EpTile* tiles; int64_t n_tiles;
    int width, stride, FT, units;                 // units: LDS slots per wave, >= ((FT - 1) stride + width) / Q
    double* E;                                    // [f_off[n]]
};

template <int Q>
__global__ __launch_bounds__(64 * EP_WAVES) void ep_energy_kernel(EpEnergyArgs a) {
    extern __shared__ unsigned long long ep_lds[];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    unsigned long long* mine = ep_lds + (size_t)wv * a.units;
    const int64_t tile = (int64_t)blockIdx.x * EP_WAVES + wv;
    int nF = 0, f0 = 0;
    int64_t fbase = 0;
    const int16_t* p = a.pcm;
    if (tile < a.n_tiles) {
        const EpTile t = a.tiles[tile];
        const int64_t nf = a.f_off[t.u + 1] - a.f_off[t.u];
        f0 = t.f0;
        nF = (int)(nf - f0 < a.FT ? nf - f0 : a.FT);
        fbase = a.f_off[t.u];
        p = a.pcm + a.s_off[t.u] + (int64_t)f0 * a.stride;
    }
    // every frame lies inside its recording (frame i ends at i stride + width <= chunks * width <= length)
    const int nu = nF > 0 ? ((nF - 1) * a.stride + a.width) / Q : 0;
    int v = lane;
    for (; v + 192 < nu; v += 256) {        // four loads in flight per lane, then their sums
        const auto t0 = ep_load<Q>(p + (int64_t)v * Q), t1 = ep_load<Q>(p + (int64_t)(v + 64) * Q),
                   t2 = ep_load<Q>(p + (int64_t)(v + 128) * Q), t3 = ep_load<Q>(p + (int64_t)(v + 192) * Q);
        mine[v] = ep_squares<Q>(t0);
        mine[v + 64] = ep_squares<Q>(t1);
        mine[v + 128] = ep_squares<Q>(t2);
        mine[v + 192] = ep_squares<Q>(t3);
    }
    for (; v < nu; v += 64) mine[v] = ep_squares<Q>(ep_load<Q>(p + (int64_t)v * Q));
    __syncthreads();
    if (lane < nF) {
        const int first = lane * (a.stride / Q), cnt = a.width / Q;
        unsigned long long s = 0;
        for (int j = 0; j < cnt; ++j) s += mine[first + j];
        // calc_energy (:26-30); frame 0 is never classified and keeps energy 0 (:132-135)
        a.E[fbase + f0 + lane] = (s <= 1 || f0 + lane == 0) ? 0.0 : 10 * log10((double)s);
    }
}

struct EpClassifyArgs {
    const int64_t* f_off; const int64_t* s_off; int64_t n;
    gh_endpoint_params p; int max_seg;
    double* E;                                   // energies; with per-frame outputs the entries behind the last classified frame are zeroed
    int64_t *start, *end; int32_t* nseg; uint8_t* open; int64_t* done;       // [n, max_seg] x 2 (zero filled), [n] x 3
    uint8_t* o_attr; double *o_level, *o_bg;     // [f_off[n]] zero filled, or all null
};

__global__ __launch_bounds__(64) void ep_classify_kernel(EpClassifyArgs a) {
    const int64_t u = (int64_t)blockIdx.x * 64 + threadIdx.x;
    if (u >= a.n) return;
    const int64_t fb = a.f_off[u], nf = a.f_off[u + 1] - fb;
    const double* e = a.E + fb;
    const double ff = a.p.forget, ff1 = a.p.forget + 1, adj = a.p.adjustment, onset = a.p.onset, offset = a.p.offset;
    const int64_t stride = a.p.stride, width = a.p.width;
    double level = 0, bg = 0;
    bool attr = false, started = false, stop = false;         // attr: the previous frame's is_speech ATTRIBUTE (:188)
    int speech = 0, silence = 0, nseg = 0;
    int64_t i = 1, done = nf > 0 ? 1 : 0;
    while (i < nf && !stop) {
        double e8[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) e8[j] = e[i + j < nf ? i + j : nf - 1];   // eight loads in flight
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            if (i < nf && !stop) {
                const double en = e8[j];
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
                    if (a.o_attr) { a.o_attr[fb + i] = now; a.o_bg[fb + i] = bg; }
                }
                if (a.o_level) a.o_level[fb + i] = level;
                attr = now;
                if (is_speech) { ++speech; silence = 0; } else { ++silence; speech = 0; }     // (:152-157)
                if (speech > a.p.speech_frames && !started) {                                  // (:159-162)
                    silence = 0;
                    started = true;
                    a.start[u * a.max_seg + nseg] = i * stride;
                } else if (silence > a.p.silence_frames && started) {                          // (:164-169)
                    started = false;
                    a.end[u * a.max_seg + nseg] = i * stride + width;
                    stop = ++nseg == a.max_seg;
                }
                done = ++i;
            }
        }
    }
    if (started) {       // speech never ended: the open segment runs to the last sample
        a.end[u * a.max_seg + nseg] = a.s_off[u + 1] - a.s_off[u] - 1;
        ++nseg;
    }
    a.nseg[u] = nseg;
    a.open[u] = started;
    a.done[u] = done;
    if (a.o_attr) for (int64_t k = done; k < nf; ++k) a.E[fb + k] = 0.0;     // frames the reference never computes
}

int ep_pick_q(int g) { return g % 8 == 0 ? 8 : (g % 4 == 0 ? 4 : (g % 2 == 0 ? 2 : 1)); }

}  // namespace

extern "C" int64_t gh_endpoint_frames(int64_t n_samples, int width, int stride) {
    if (n_samples < 0 || width < 1 || stride < 1 || stride > width) return -1;
    const int64_t chunks = n_samples / width;
    return chunks == 0 ? 0 : 1 + (int64_t)(width / stride) * (chunks - 1);     // (:132-139)
}

// d_pcm: the whole call's recordings already on the device (sample_off indexes it), or null: `samples` (host) travels
// chunk by chunk through the context's scratch.  The outputs are host arrays.
int gh_endpoints_run(gh_ctx* ctx, const int16_t* d_pcm, const int16_t* samples, int64_t U, const int64_t* sample_off,
                     const gh_endpoint_params* prm, int max_segments, int64_t* start, int64_t* end, int32_t* n_segments,
                     uint8_t* open, int64_t* frames_done, const int64_t* frame_off, uint8_t* out_is_speech,
                     double* out_level, double* out_background, double* out_energy) {
    const char* who = "gh_endpoints";
    GH_REQUIRE(ctx && prm, "%s: NULL argument", who);
    GH_REQUIRE(U >= 0 && max_segments >= 1, "%s: U=%lld max_segments=%d", who, (long long)U, max_segments);
    GH_REQUIRE(prm->width >= 1 && prm->stride >= 1 && prm->stride <= prm->width && prm->width <= (1 << 22),
               "%s: width=%d stride=%d (1 <= stride <= width <= 2^22)", who, prm->width, prm->stride);
    if (U == 0) { ctx->last_chunks = 0; return GH_OK; }
    GH_REQUIRE(sample_off && start && end && n_segments && open, "%s: NULL argument", who);
    GH_REQUIRE(sample_off[0] == 0, "%s: sample_off[0] != 0", who);
    const bool want_frames = out_is_speech || out_level || out_background || out_energy;
    GH_REQUIRE(!want_frames || (frame_off && out_is_speech && out_level && out_background && out_energy && frame_off[0] == 0),
               "%s: the per-frame outputs come together, with frame_off", who);
    const int width = prm->width, stride = prm->stride;
    std::vector<int64_t> nf(U);
    for (int64_t u = 0; u < U; ++u) {
        const int64_t len = sample_off[u + 1] - sample_off[u];
        GH_REQUIRE(len >= 0, "%s: sample_off decreases at recording %lld", who, (long long)u);
        nf[u] = gh_endpoint_frames(len, width, stride);
        GH_REQUIRE(nf[u] < ((int64_t)1 << 31), "%s: recording %lld has %lld frames", who, (long long)u, (long long)nf[u]);
        GH_REQUIRE(!want_frames || frame_off[u + 1] - frame_off[u] == nf[u],
                   "%s: frame_off gives recording %lld %lld frames, gh_endpoint_frames %lld", who, (long long)u,
                   (long long)(frame_off[u + 1] - frame_off[u]), (long long)nf[u]);
    }
    GH_REQUIRE(samples || d_pcm || sample_off[U] == 0, "%s: samples is NULL", who);
    int g = width, r = stride;
    while (r) { const int t = g % r; g = r; r = t; }
    const int Q = ep_pick_q(g);
    int FT = 64;
    auto units_of = [&](int ft) { return (size_t)((int64_t)(ft - 1) * stride + width) / Q; };
    while (FT > 1 && EP_WAVES * units_of(FT) * 8 > EP_LDS_MAX) FT >>= 1;
    if (EP_WAVES * units_of(FT) * 8 > EP_LDS_MAX) {
        gh_set_error("%s: frames of %d samples every %d are %d units of %d samples, more than the %d that fit LDS", who, width, stride,
                     width / Q, Q, (int)(EP_LDS_MAX / (EP_WAVES * 8)));
        return GH_ERR_UNSUPPORTED;
    }
    const int units = (int)units_of(FT);

    // chunks of whole recordings by the scratch budget
    // (`need` leaves out the 256-byte padding of the pieces below: the budget is a target, not a hard bound)
    auto tiles_of = [&](int64_t u) { return (nf[u] + FT - 1) / FT; };
    auto need = [&](int64_t u) {
        return (d_pcm ? 0 : (size_t)(sample_off[u + 1] - sample_off[u]) * 2) + (size_t)nf[u] * (want_frames ? 25 : 8) +
               (size_t)tiles_of(u) * sizeof(EpTile) + (size_t)max_segments * 16 + 48;
    };
    const size_t budget = gh_scratch_budget(ctx);
    std::vector<int64_t> chunk_begin{0};
    size_t acc = 0;
    for (int64_t u = 0; u < U; ++u) {
        const size_t b = need(u);
        if (u > chunk_begin.back() && acc + b > budget) { chunk_begin.push_back(u); acc = 0; }
        acc += b;
    }
    chunk_begin.push_back(U);
    int64_t max_n = 0, max_samples = 0, max_frames = 0, max_tiles = 0;
    for (size_t c = 0; c + 1 < chunk_begin.size(); ++c) {
        const int64_t b = chunk_begin[c], e = chunk_begin[c + 1];
        int64_t fr = 0, tl = 0;
        for (int64_t u = b; u < e; ++u) { fr += nf[u]; tl += tiles_of(u); }
        max_n = std::max(max_n, e - b);
        max_samples = std::max(max_samples, sample_off[e] - sample_off[b]);
        max_frames = std::max(max_frames, fr);
        max_tiles = std::max(max_tiles, tl);
    }
    GH_HIP(hipSetDevice(ctx->device));
    int16_t* d_samples; int64_t *d_soff, *d_foff, *d_start, *d_end, *d_done; EpTile* d_tiles; double *d_E, *d_level, *d_bg;
    int32_t* d_nseg; uint8_t *d_open, *d_attr;
    Carver cv;
    cv.add(&d_samples, d_pcm ? 0 : (size_t)max_samples);
    cv.add(&d_soff, (size_t)max_n + 1);
    cv.add(&d_foff, (size_t)max_n + 1);
    cv.add(&d_tiles, (size_t)max_tiles);
    cv.add(&d_E, (size_t)max_frames);
    cv.add(&d_start, (size_t)max_n * max_segments);      // start, end, done, nseg, open are neighbours: one memset, see below
    cv.add(&d_end, (size_t)max_n * max_segments);
    cv.add(&d_done, (size_t)max_n);
    cv.add(&d_nseg, (size_t)max_n);
    cv.add(&d_open, (size_t)max_n);
    cv.add(&d_level, want_frames ? (size_t)max_frames : 0);
    cv.add(&d_bg, want_frames ? (size_t)max_frames : 0);
    cv.add(&d_attr, want_frames ? (size_t)max_frames : 0);
    int rc = cv.commit(ctx);
    if (rc) return rc;
    hipStream_t st = ctx->stream;
    std::vector<int64_t> h_soff, h_foff;
    std::vector<EpTile> h_tiles;
    for (size_t c = 0; c + 1 < chunk_begin.size(); ++c) {
        const int64_t b = chunk_begin[c], e = chunk_begin[c + 1], n = e - b;
        h_soff.assign(n + 1, 0);
        h_foff.assign(n + 1, 0);
        h_tiles.clear();
        const int64_t s_base = d_pcm ? 0 : sample_off[b];
        for (int64_t i = 0; i < n; ++i) {
            h_soff[i] = sample_off[b + i] - s_base;
            h_foff[i + 1] = h_foff[i] + nf[b + i];
            for (int64_t f0 = 0; f0 < nf[b + i]; f0 += FT) h_tiles.push_back({(int32_t)i, (int32_t)f0});
        }
        h_soff[n] = sample_off[e] - s_base;
        const int64_t NF = h_foff[n], NT = (int64_t)h_tiles.size();
        const int64_t n_smp = sample_off[e] - sample_off[b];
        if (!d_pcm && n_smp) GH_HIP(hipMemcpyAsync(d_samples, samples + sample_off[b], (size_t)n_smp * 2, hipMemcpyHostToDevice, st));
        GH_HIP(hipMemcpyAsync(d_soff, h_soff.data(), (size_t)(n + 1) * 8, hipMemcpyHostToDevice, st));
        GH_HIP(hipMemcpyAsync(d_foff, h_foff.data(), (size_t)(n + 1) * 8, hipMemcpyHostToDevice, st));
        if (NT) GH_HIP(hipMemcpyAsync(d_tiles, h_tiles.data(), (size_t)NT * sizeof(EpTile), hipMemcpyHostToDevice, st));
        GH_HIP(hipMemsetAsync(d_start, 0, (size_t)((char*)d_open - (char*)d_start) + (size_t)n, st));   // start .. open: neighbours
        if (want_frames && NF) {
            GH_HIP(hipMemsetAsync(d_level, 0, (size_t)NF * 8, st));
            GH_HIP(hipMemsetAsync(d_bg, 0, (size_t)NF * 8, st));
            GH_HIP(hipMemsetAsync(d_attr, 0, (size_t)NF, st));
        }
        if (NT) {
            EpEnergyArgs ea;
            ea.pcm = d_pcm ? d_pcm : d_samples; ea.s_off = d_soff; ea.f_off = d_foff; ea.tiles = d_tiles; ea.n_tiles = NT;
            ea.width = width; ea.stride = stride; ea.FT = FT; ea.units = units; ea.E = d_E;
            const dim3 grid((unsigned)((NT + EP_WAVES - 1) / EP_WAVES)), block(64 * EP_WAVES);
            const size_t lds = (size_t)EP_WAVES * units * 8;
            if (Q == 8) hipLaunchKernelGGL(ep_energy_kernel<8>, grid, block, lds, st, ea);
            else if (Q == 4) hipLaunchKernelGGL(ep_energy_kernel<4>, grid, block, lds, st, ea);
            else if (Q == 2) hipLaunchKernelGGL(ep_energy_kernel<2>, grid, block, lds, st, ea);
            else hipLaunchKernelGGL(ep_energy_kernel<1>, grid, block, lds, st, ea);
            GH_HIP(hipGetLastError());
        }
        EpClassifyArgs ca;
        ca.f_off = d_foff; ca.s_off = d_soff; ca.n = n; ca.p = *prm; ca.max_seg = max_segments; ca.E = d_E;
        ca.start = d_start; ca.end = d_end; ca.nseg = d_nseg; ca.open = d_open; ca.done = d_done;
        ca.o_attr = want_frames ? d_attr : nullptr; ca.o_level = want_frames ? d_level : nullptr; ca.o_bg = want_frames ? d_bg : nullptr;
        hipLaunchKernelGGL(ep_classify_kernel, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, st, ca);
        GH_HIP(hipGetLastError());
        GH_HIP(hipMemcpyAsync(start + b * max_segments, d_start, (size_t)n * max_segments * 8, hipMemcpyDeviceToHost, st));
        GH_HIP(hipMemcpyAsync(end + b * max_segments, d_end, (size_t)n * max_segments * 8, hipMemcpyDeviceToHost, st));
        GH_HIP(hipMemcpyAsync(n_segments + b, d_nseg, (size_t)n * 4, hipMemcpyDeviceToHost, st));
        GH_HIP(hipMemcpyAsync(open + b, d_open, (size_t)n, hipMemcpyDeviceToHost, st));
        if (frames_done) GH_HIP(hipMemcpyAsync(frames_done + b, d_done, (size_t)n * 8, hipMemcpyDeviceToHost, st));
        if (want_frames && NF) {
            const int64_t fo = frame_off[b];
            GH_HIP(hipMemcpyAsync(out_is_speech + fo, d_attr, (size_t)NF, hipMemcpyDeviceToHost, st));
            GH_HIP(hipMemcpyAsync(out_level + fo, d_level, (size_t)NF * 8, hipMemcpyDeviceToHost, st));
            GH_HIP(hipMemcpyAsync(out_background + fo, d_bg, (size_t)NF * 8, hipMemcpyDeviceToHost, st));
            GH_HIP(hipMemcpyAsync(out_energy + fo, d_E, (size_t)NF * 8, hipMemcpyDeviceToHost, st));
        }
        GH_HIP(hipStreamSynchronize(st));      // (the chunk's host tables and device pieces are reused by the next one)
    }
    ctx->last_chunks = (int)chunk_begin.size() - 1;
    return GH_OK;
}

extern "C" int gh_endpoints(gh_ctx* ctx, int64_t U, const int16_t* samples, const int64_t* sample_off,
                            const gh_endpoint_params* prm, int max_segments, int64_t* start, int64_t* end,
                            int32_t* n_segments, uint8_t* open, int64_t* frames_done, const int64_t* frame_off,
                            uint8_t* out_is_speech, double* out_level, double* out_background, double* out_energy) {
    return gh_endpoints_run(ctx, nullptr, samples, U, sample_off, prm, max_segments, start, end, n_segments, open, frames_done,
                            frame_off, out_is_speech, out_level, out_background, out_energy);
}
