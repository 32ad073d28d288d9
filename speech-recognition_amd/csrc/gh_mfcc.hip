// MFCC front-end on the GPU (first half): PCM -> 40 log mel filterbank
// energies -> 13 cepstra per frame, the arithmetic of mfcc_features (sr/feature/feature.py:43-82) in
// fp64.  One wave per frame, four frames per workgroup:
//   pre-emphasis (:45-46, product and difference rounded separately like numpy) -> the frame's samples
//   into a zero padded power-of-two buffer, centred (:25-40) -> Hamming window over the padded length
//   (:52) -> 512-point radix-2 FFT in LDS -> power spectrum / 512 (:54-56) -> mel filters (:58-75;
//   every filter only over its own bin range) -> log10 with eps for zeros (:76-78) -> DCT-II ortho
//   rows 1..13 (:80-81).
// All tables (window, twiddles, filterbank, DCT rows) are built on the host exactly as the reference
// builds them (np.hamming, np.linspace, floor((NFFT+1) hz / rate), scipy's ortho DCT-II scaling).
#include "gh_mfcc_core.h"

namespace {

struct MfccArgs {
    const void* pcm; int fmt;
    const int64_t* s_beg; const int64_t* s_end;   // first sample of every utterance in `pcm`, one past its last
    const int64_t* f_off;                         // first frame of every utterance in the outputs
    const int64_t* p_off; const int32_t* p_utt;   // first frame pair of every utterance; the utterance of every pair
    int64_t U, P;
    int flen, fstep, pad_left;
    MfccTables t;
    double* out_fb; double* out_mfcc;
};

template <int FMT> __device__ __forceinline__ double sample_at(const void* pcm, int64_t i) {
    if (FMT == 0) return (double)static_cast<const int16_t*>(pcm)[i];
    if (FMT == 1) return (double)static_cast<const float*>(pcm)[i];
    return static_cast<const double*>(pcm)[i];
}

// One wave per PAIR of frames (A, B), four pairs per workgroup.  Frames are paired by their index INSIDE the utterance
// (2m, 2m + 1), through the host-built pair -> utterance table, and an odd last frame gets a dead partner: a frame's bits
// depend on its partner in the FFT, so an utterance comes out the same wherever it stands in the batch, alone, or streamed
// (stream_mfcc_kernel pairs the same way).  The samples are windowed here, and mfcc_pair_tail does the rest.
template <int FMT>
__global__ __launch_bounds__(256) void mfcc_kernel(MfccArgs a) {
    constexpr int S1 = MFCC_S1;
    __shared__ double s_x[4][8 * S1];                    // 4608 B per wave (the transposes move re and im one after
                                                         // the other: half the LDS, twice the resident waves), reused by every phase
    __shared__ double s_lfb[4][2][NFILT];
    __shared__ double s_wup[NBIN], s_wdn[NBIN];          // per-bin filter weights, shared by the block
    for (int k = threadIdx.x; k < NBIN; k += 256) { s_wup[k] = a.t.wup[k]; s_wdn[k] = a.t.wdn[k]; }
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    double* ex = s_x[wv];
    const int64_t pr = (int64_t)blockIdx.x * 4 + wv;     // a wave past the last pair is dead in both slots
    int64_t n0 = 0, s0[2] = {0, 0}, slen[2] = {0, 0}, sbase[2] = {0, 0};   // rows n0 (A) and n0 + 1 (B) of the outputs
    bool live[2] = {false, false};
    if (pr < a.P) {
        const int u = a.p_utt[pr];             // utterance of this pair (host-built table)
        const int64_t f0 = a.f_off[u], t0 = 2 * (pr - a.p_off[u]), T = a.f_off[u + 1] - f0;
        n0 = f0 + t0;
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            live[h] = t0 + h < T;              // (the odd last frame of an utterance has no partner)
            if (live[h]) {
                sbase[h] = a.s_beg[u];
                slen[h] = a.s_end[u] - sbase[h];
                s0[h] = (t0 + h) * a.fstep;
            }
        }
    }
    // ---- windowed, zero padded frames: lane l holds z[l + 64 j], j = 0..7 ----
    // (every load is unconditional on a clamped address, so all 32 of them are in flight together;
    //  a load behind a branch costs one memory round trip each)
    c2 v[8];
    double cur[2][8], prv[2][8];
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        const int64_t last = sbase[h] + (slen[h] > 0 ? slen[h] - 1 : 0);
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            int64_t p = sbase[h] + s0[h] + (lane + 64 * j - a.pad_left);
            p = p < sbase[h] ? sbase[h] : (p > last ? last : p);
            cur[h][j] = sample_at<FMT>(a.pcm, p);
            prv[h][j] = sample_at<FMT>(a.pcm, p > sbase[h] ? p - 1 : p);
        }
    }
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const int js = lane + 64 * j - a.pad_left;
        const double w = a.t.window[lane + 64 * j];
        double xs[2];
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const bool in = live[h] && js >= 0 && js < a.flen && s0[h] + js < slen[h];
            const double x = (s0[h] + js == 0) ? cur[h][j] : __dsub_rn(cur[h][j], __dmul_rn(0.97, prv[h][j]));
            xs[h] = in ? x * w : 0.0;
        }
        v[j] = (c2){xs[0], xs[1]};
    }
    mfcc_pair_tail(
        a.t, v, ex, s_lfb[wv], s_wup, s_wdn, lane,
        [&](double f0, double f1) {
            if (a.out_fb) {
                if (live[0]) a.out_fb[n0 * NFILT + lane - 1] = f0;
                if (live[1]) a.out_fb[(n0 + 1) * NFILT + lane - 1] = f1;
            }
        },
        [&](double acc0, double acc1) {
            if (lane < NCEPS && a.out_mfcc) {
                if (live[0]) a.out_mfcc[n0 * NCEPS + lane] = acc0;
                if (live[1]) a.out_mfcc[(n0 + 1) * NCEPS + lane] = acc1;
            }
        });
}

void launch_mfcc(const MfccArgs& a, hipStream_t st) {
    const dim3 grid((unsigned)((a.P + 3) / 4)), block(256);
    if (a.fmt == 0) hipLaunchKernelGGL(mfcc_kernel<0>, grid, block, 0, st, a);
    else if (a.fmt == 1) hipLaunchKernelGGL(mfcc_kernel<1>, grid, block, 0, st, a);
    else hipLaunchKernelGGL(mfcc_kernel<2>, grid, block, 0, st, a);
}

size_t fmt_size(int fmt) { return fmt == 0 ? 2 : (fmt == 1 ? 4 : 8); }

// the frame pairs of a batch, ceil(T_u / 2) per utterance: where every utterance's pairs begin and the utterance of every
// pair, the tables mfcc_kernel finds its frames and samples with
struct PairTable {
    std::vector<int64_t> off;      // [U + 1]
    std::vector<int32_t> utt;      // [off[U]]
    int64_t pairs() const { return off.empty() ? 0 : off.back(); }
};

void fill_pairs(int64_t U, const int64_t* f_off, PairTable& pt) {
    pt.off.assign((size_t)U + 1, 0);
    for (int64_t u = 0; u < U; ++u) pt.off[(size_t)u + 1] = pt.off[(size_t)u] + (f_off[u + 1] - f_off[u] + 1) / 2;
    pt.utt.resize((size_t)pt.off[(size_t)U]);
    for (int64_t u = 0; u < U; ++u) std::fill(pt.utt.begin() + pt.off[(size_t)u], pt.utt.begin() + pt.off[(size_t)u + 1], (int32_t)u);
}

int check_inputs(const char* who, int fmt, int64_t U, const void* samples, const int64_t* s_off, const int64_t* f_off,
                 const HostTables& h, PairTable& pt) {
    GH_REQUIRE(fmt >= 0 && fmt <= 2, "%s: sample_fmt=%d (0 int16, 1 float32, 2 float64)", who, fmt);
    GH_REQUIRE(U >= 0 && s_off && f_off && s_off[0] == 0 && f_off[0] == 0, "%s: offsets must start at 0", who);
    GH_REQUIRE(samples || s_off[U] == 0, "%s: samples is NULL", who);
    for (int64_t u = 0; u < U; ++u) {
        const int64_t len = s_off[u + 1] - s_off[u];
        GH_REQUIRE(len >= 1, "%s: utterance %lld is empty (the reference reads signal[0])", who, (long long)u);
        const int64_t nf = (len + h.fstep - 1) / h.fstep;
        GH_REQUIRE(f_off[u + 1] - f_off[u] == nf, "%s: frame_off gives utterance %lld %lld frames, ceil(%lld / %d) = %lld",
                   who, (long long)u, (long long)(f_off[u + 1] - f_off[u]), (long long)len, h.fstep, (long long)nf);
    }
    fill_pairs(U, f_off, pt);
    return GH_OK;
}

// carve the inputs + tables out of one block, upload, return the kernel arguments
// (resident: the samples are on the device already and the utterances are ranges of them -- the endpointed entry)
size_t table_bytes(int fmt, int64_t n_samples, int64_t U, int64_t P, bool resident = false) {
    auto al = [](size_t b) { return (b + 255) & ~size_t(255); };
    return (resident ? 0 : al((size_t)n_samples * fmt_size(fmt))) + 3 * al((size_t)(U + 1) * 8) + (resident ? al((size_t)(U + 1) * 8) : 0) +
           al((size_t)P * 4) + al(NFFT * 8) + al(2 * NFFT * 8) + 2 * al(NBIN * 8) + al((NFILT + 2) * 4) + al((size_t)NCEPS * NFILT * 8);
}

// samples + s_off [U+1]: utterances back to back, uploaded here; or d_pcm + s_off / s_end [U]: ranges of resident samples
hipError_t upload_inputs(char* base, hipStream_t st, int fmt, int64_t U, const void* samples, const int64_t* s_off,
                         const int64_t* f_off, const HostTables& h, const PairTable& pt, MfccArgs& a,
                         const void* d_pcm = nullptr, const int64_t* s_end = nullptr) {
    auto al = [](size_t b) { return (b + 255) & ~size_t(255); };
    char* p = base;
    hipError_t e = hipSuccess;
    auto put = [&](const void* src, size_t bytes) -> void* {
        void* dst = p;
        if (bytes && e == hipSuccess) e = hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, st);
        p += al(bytes);
        return dst;
    };
    if (d_pcm) {
        a.pcm = d_pcm;
        a.s_beg = (const int64_t*)put(s_off, (size_t)(U + 1) * 8);
        a.s_end = (const int64_t*)put(s_end, (size_t)(U + 1) * 8);
    } else {
        a.pcm = put(samples, (size_t)s_off[U] * fmt_size(fmt));
        a.s_beg = (const int64_t*)put(s_off, (size_t)(U + 1) * 8);
        a.s_end = a.s_beg + 1;
    }
    a.f_off = (const int64_t*)put(f_off, (size_t)(U + 1) * 8);
    a.p_off = (const int64_t*)put(pt.off.data(), (size_t)(U + 1) * 8);
    a.p_utt = (const int32_t*)put(pt.utt.data(), pt.utt.size() * 4);
    a.t.window = (const double*)put(h.window.data(), NFFT * 8);
    a.t.tw = (const double*)put(h.tw.data(), 2 * NFFT * 8);
    a.t.wup = (const double*)put(h.wup.data(), NBIN * 8);
    a.t.wdn = (const double*)put(h.wdn.data(), NBIN * 8);
    a.t.seg = (const int*)put(h.seg.data(), (NFILT + 2) * 4);
    a.t.dct = (const double*)put(h.dct.data(), (size_t)NCEPS * NFILT * 8);
    a.fmt = fmt; a.U = U; a.P = pt.pairs();
    a.flen = h.flen; a.fstep = h.fstep; a.pad_left = h.pad_left;
    return e;
}

}  // namespace

extern "C" int64_t gh_mfcc_frames(int64_t n_samples, int sample_rate, double frame_stride) {
    const int64_t step = (int64_t)(frame_stride * sample_rate);
    if (n_samples < 1 || step < 1) return -1;
    return (n_samples + step - 1) / step;  // math.ceil(slen / frame_step1), feature.py:13
}

extern "C" int gh_mfcc(gh_ctx* ctx, int sample_fmt, int sample_rate, double frame_size, double frame_stride,
                       double low_freq, double high_freq, int64_t U, const void* samples, const int64_t* sample_off,
                       const int64_t* frame_off, double* out_fbank, double* out_mfcc) {
    GH_REQUIRE(ctx, "gh_mfcc: ctx is NULL");
    HostTables h;
    PairTable pt;
    int rc = build_tables("gh_mfcc", sample_rate, frame_size, frame_stride, low_freq, high_freq, h);
    if (rc) return rc;
    if ((rc = check_inputs("gh_mfcc", sample_fmt, U, samples, sample_off, frame_off, h, pt))) return rc;
    const int64_t N = frame_off[U];
    if (N == 0) return GH_OK;
    GH_HIP(hipSetDevice(ctx->device));
    char* d_in;
    double *d_fb, *d_mf;
    Carver cv;
    cv.add(&d_in, table_bytes(sample_fmt, sample_off[U], U, pt.pairs()));
    cv.add(&d_fb, (size_t)N * NFILT);
    cv.add(&d_mf, (size_t)N * NCEPS);
    if ((rc = cv.commit(ctx))) return rc;
    hipStream_t st = ctx->stream;
    MfccArgs a;
    GH_HIP(upload_inputs(d_in, st, sample_fmt, U, samples, sample_off, frame_off, h, pt, a));
    a.out_fb = d_fb;
    a.out_mfcc = d_mf;
    launch_mfcc(a, st);
    GH_HIP(hipGetLastError());
    if (out_fbank) GH_HIP(hipMemcpyAsync(out_fbank, d_fb, (size_t)N * NFILT * 8, hipMemcpyDeviceToHost, st));
    if (out_mfcc) GH_HIP(hipMemcpyAsync(out_mfcc, d_mf, (size_t)N * NCEPS * 8, hipMemcpyDeviceToHost, st));
    GH_HIP(hipStreamSynchronize(st));
    return GH_OK;
}

extern "C" int gh_batch_create_from_pcm(gh_ctx* ctx, gh_dtype dtype, int mode, int sample_fmt, int sample_rate,
                                        double frame_size, double frame_stride, double low_freq, double high_freq,
                                        int64_t U, const void* samples, const int64_t* sample_off,
                                        const int64_t* frame_off, gh_batch** out) {
    GH_REQUIRE(ctx && out, "gh_batch_create_from_pcm: NULL argument");
    HostTables h;
    PairTable pt;
    int rc = build_tables("gh_mfcc", sample_rate, frame_size, frame_stride, low_freq, high_freq, h);
    if (rc) return rc;
    if ((rc = check_inputs("gh_batch_create_from_pcm", sample_fmt, U, samples, sample_off, frame_off, h, pt))) return rc;
    const int64_t N = frame_off[U];
    void* extra = nullptr;
    return gh_batch_from_device_cepstra(
        ctx, dtype, mode, NCEPS, N, U, frame_off, table_bytes(sample_fmt, sample_off[U], U, pt.pairs()), &extra,
        [&](double* d_ceps, hipStream_t st) {
            MfccArgs a;
            hipError_t e = upload_inputs(static_cast<char*>(extra), st, sample_fmt, U, samples, sample_off, frame_off, h, pt, a);
            if (e != hipSuccess) return e;
            a.out_fb = nullptr;
            a.out_mfcc = d_ceps;
            launch_mfcc(a, st);
            return hipGetLastError();
        },
        "gh_batch_create_from_pcm", out);
}

extern "C" int gh_batch_create_from_pcm_endpointed(gh_ctx* ctx, gh_dtype dtype, int mode, int sample_fmt, int sample_rate,
                                                   double frame_size, double frame_stride, double low_freq, double high_freq,
                                                   int64_t U, const void* samples, const int64_t* sample_off,
                                                   const gh_endpoint_params* prm, int start_boundary, int max_segments,
                                                   int64_t* start, int64_t* end, int32_t* n_segments, uint8_t* open,
                                                   int64_t* utt_frame_off, int64_t* n_utt, gh_batch** out) {
    const char* who = "gh_batch_create_from_pcm_endpointed";
    GH_REQUIRE(ctx && out && prm && sample_off && start && end && n_segments && open && utt_frame_off && n_utt, "%s: NULL argument", who);
    GH_REQUIRE(sample_fmt == 0, "%s: sample_fmt=%d (endpoint detection reads int16)", who, sample_fmt);
    GH_REQUIRE(U >= 0 && sample_off[0] == 0 && start_boundary >= 0 && max_segments >= 1, "%s: U=%lld start_boundary=%d max_segments=%d",
               who, (long long)U, start_boundary, max_segments);
    HostTables h;
    PairTable pt;
    int rc = build_tables("gh_mfcc", sample_rate, frame_size, frame_stride, low_freq, high_freq, h);
    if (rc) return rc;
    for (int64_t u = 0; u < U; ++u)
        GH_REQUIRE(sample_off[u + 1] >= sample_off[u], "%s: sample_off decreases at recording %lld", who, (long long)u);
    GH_REQUIRE(samples || sample_off[U] == 0, "%s: samples is NULL", who);
    GH_HIP(hipSetDevice(ctx->device));
    // the samples stay in an allocation of their own: the context's scratch is carved anew by both halves
    void* d_pcm = nullptr;
    GH_HIP(hipMalloc(&d_pcm, (size_t)sample_off[U] * 2 + 256));
    struct guard { void* p; ~guard() { (void)hipFree(p); } } free_pcm{d_pcm};
    if (sample_off[U]) GH_HIP(hipMemcpyAsync(d_pcm, samples, (size_t)sample_off[U] * 2, hipMemcpyHostToDevice, ctx->stream));
    rc = gh_endpoints_run(ctx, static_cast<const int16_t*>(d_pcm), nullptr, U, sample_off, prm, max_segments, start, end, n_segments,
                          open, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr);
    if (rc) return rc;
    if (U == 0) GH_HIP(hipStreamSynchronize(ctx->stream));
    // one utterance per segment, the slice of get_samples (record.py:243-248); a recording without a segment stays whole
    std::vector<int64_t> s_beg, s_end, f_off{0};
    for (int64_t u = 0; u < U; ++u) {
        const int64_t len = sample_off[u + 1] - sample_off[u];
        const int k = n_segments[u];
        GH_REQUIRE(k >= 0 && k <= max_segments, "%s: recording %lld came back with %d segments", who, (long long)u, k);
        for (int s = 0; s < (k > 0 ? k : 1); ++s) {
            int64_t b = 0, e = len;
            if (k > 0) {
                b = std::max<int64_t>(start[u * max_segments + s] - start_boundary, 0);
                e = std::min<int64_t>(end[u * max_segments + s] + 1, len);
            }
            GH_REQUIRE(e - b >= 1, "%s: recording %lld is empty (the reference reads signal[0])", who, (long long)u);
            s_beg.push_back(sample_off[u] + b);
            s_end.push_back(sample_off[u] + e);
            f_off.push_back(f_off.back() + (e - b + h.fstep - 1) / h.fstep);
        }
    }
    const int64_t U2 = (int64_t)s_beg.size(), N = f_off.back();
    *n_utt = U2;                                   // (U2 <= U * max_segments: the caller's table has room)
    memcpy(utt_frame_off, f_off.data(), (size_t)(U2 + 1) * 8);
    s_beg.push_back(0);       // (both tables travel with U2 + 1 entries)
    s_end.push_back(0);
    fill_pairs(U2, f_off.data(), pt);
    void* extra = nullptr;
    return gh_batch_from_device_cepstra(
        ctx, dtype, mode, NCEPS, N, U2, f_off.data(), table_bytes(0, 0, U2, pt.pairs(), true), &extra,
        [&](double* d_ceps, hipStream_t st) {
            MfccArgs a;
            hipError_t e = upload_inputs(static_cast<char*>(extra), st, 0, U2, nullptr, s_beg.data(), f_off.data(), h, pt, a, d_pcm, s_end.data());
            if (e != hipSuccess) return e;
            a.out_fb = nullptr;
            a.out_mfcc = d_ceps;
            launch_mfcc(a, st);
            return hipGetLastError();
        },
        who, out);
}
