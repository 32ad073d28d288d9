// The MFCC core, defined ONCE for the one-shot front-end (gh_mfcc.hip) and the streaming one (gh_mfcc_stream.hip): the
// tables, the radix-8 FFT pieces, and everything from a wave's windowed frame pair to its cepstra.  A kernel keeps its own
// sample addressing and its pre-emphasis / window stage and hands the registers to mfcc_pair_tail; what it stores, and
// where, comes in as two hooks.  The streams' bitwise contract with the one-shot path rests on this single text.
// Everything sits in an unnamed namespace and the device functions are __forceinline__: each including .hip compiles
// its own copy under its own flags.
#pragma once
#include "gh_internal.h"
#include "gh_host.h"

namespace {

constexpr int NFFT = 512, NBIN = NFFT / 2 + 1, NFILT = 40, NCEPS = 13;
constexpr int MFCC_S1 = 72, MFCC_S2 = 9;     // padded strides of the two transposes (elements)

struct MfccTables {           // device pointers into one scratch block
    const double* window;     // [NFFT]   hamming(pad_w) in [0, pad_w), 0 behind
    const double* tw;         // [NFFT][2] cos / -sin of 2 pi k / NFFT
    const double* wup;        // [NBIN] weight of bin k in the ASCENDING half of the filter that peaks right of it
    const double* wdn;        // [NBIN] weight of bin k in the DESCENDING half of the filter that peaks at / left of it
    const int* seg;           // [NFILT + 2] the mel bin points: segment s = bins [seg[s], seg[s+1])
    const double* dct;        // [NCEPS][NFILT]
};

typedef double c2 __attribute__((ext_vector_type(2)));   // (re, im)

__device__ __forceinline__ c2 mul_negi(c2 v) { return (c2){v.y, -v.x}; }                       // v * (-i)
__device__ __forceinline__ c2 cmul(c2 a, c2 w) { return (c2){a.x * w.x - a.y * w.y, a.x * w.y + a.y * w.x}; }

// in-place 8-point forward DFT (decimation in frequency), natural output order
__device__ __forceinline__ void dft8(c2 (&v)[8]) {
    constexpr double R = 0.70710678118654752440;
    c2 t[4], u[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) { t[j] = v[j] + v[j + 4]; u[j] = v[j] - v[j + 4]; }
    u[1] = (c2){(u[1].x + u[1].y) * R, (u[1].y - u[1].x) * R};      // * W8^1
    u[2] = mul_negi(u[2]);                                          // * W8^2
    u[3] = (c2){(u[3].y - u[3].x) * R, -(u[3].x + u[3].y) * R};     // * W8^3
    auto dft4 = [](const c2 (&x)[4], c2& o0, c2& o1, c2& o2, c2& o3) {
        const c2 s0 = x[0] + x[2], s1 = x[0] - x[2], s2 = x[1] + x[3], s3 = mul_negi(x[1] - x[3]);
        o0 = s0 + s2; o2 = s0 - s2; o1 = s1 + s3; o3 = s1 - s3;
    };
    dft4(t, v[0], v[2], v[4], v[6]);
    dft4(u, v[1], v[3], v[5], v[7]);
}

// One wave, one PAIR of frames (A, B): z = a + i b (lane l holds z[l + 64 j] in v[j], windowed and zero padded) goes
// through ONE 512-point complex FFT and the two real spectra are separated afterwards.  512 = 8 x 8 x 8: three radix-8
// passes in registers (each lane holds 8 points), two transposes through LDS (padded, 16-byte accesses) -- instead of
// 9 radix-2 stages with a barrier and 8 LDS accesses per butterfly each.  ex: the wave's 8 * MFCC_S1 doubles of LDS,
// lfb: its [2][NFILT] log filterbank row, s_wup / s_wdn: the block's copy of the per-bin weights.
// store_fbank(f0, f1): lane m + 1, m in [0, NFILT), holds log filterbank energy m of A and B.
// store_ceps(acc0, acc1): lane c < NCEPS holds cepstrum c of A and B.
template <typename StoreFbank, typename StoreCeps>
__device__ __forceinline__ void mfcc_pair_tail(const MfccTables& t, c2 (&v)[8], double* ex, double (&lfb)[2][NFILT],
                                               const double* s_wup, const double* s_wdn, int lane, StoreFbank store_fbank,
                                               StoreCeps store_ceps) {
    constexpr int S1 = MFCC_S1, S2 = MFCC_S2;
    // A frame without a non-zero windowed sample has power exactly 0 in the reference, which its `== 0` rule (feature.py:77)
    // turns into eps.  Here its partner's rounding would leak into it (Z[k] and Z[N - k] are conjugates only up to rounding,
    // some 1e-16 of the partner's spectrum): such a frame is found before the FFT and gets its zeros written below.
    bool nz0 = false, nz1 = false;
#pragma unroll
    for (int j = 0; j < 8; ++j) { nz0 |= v[j].x != 0.0; nz1 |= v[j].y != 0.0; }
    const bool any0 = __any(nz0), any1 = __any(nz1);
    // ---- pass 1: DFT over j, twiddle W512^(l q); transpose so that lane (l1 + 8 q) holds l2 = 0..7 ----
    dft8(v);
#pragma unroll
    for (int q = 1; q < 8; ++q) v[q] = cmul(v[q], *reinterpret_cast<const c2*>(t.tw + 2 * (lane * q)));
    // component-wise transpose through LDS: v[i] goes to slot wr(i), comes back from slot rd(i)
    auto transpose = [&](auto wr, auto rd) {
        double tx[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) ex[wr(i)] = v[i].x;
        __syncthreads();
#pragma unroll
        for (int i = 0; i < 8; ++i) tx[i] = ex[rd(i)];
        __syncthreads();
#pragma unroll
        for (int i = 0; i < 8; ++i) ex[wr(i)] = v[i].y;
        __syncthreads();
#pragma unroll
        for (int i = 0; i < 8; ++i) v[i] = (c2){tx[i], ex[rd(i)]};
        __syncthreads();
    };
    const int l1 = lane & 7, qq = lane >> 3;
    transpose([&](int q) { return q * S1 + lane; }, [&](int l2) { return qq * S1 + l1 + 8 * l2; });
    // ---- pass 2: DFT over l2, twiddle W64^(l1 q'); transpose so that lane (q + 8 q') holds l1 = 0..7 ----
    dft8(v);
#pragma unroll
    for (int q2 = 1; q2 < 8; ++q2) v[q2] = cmul(v[q2], *reinterpret_cast<const c2*>(t.tw + 2 * (8 * l1 * q2)));
    transpose([&](int q2) { return (qq + 8 * q2) * S2 + l1; }, [&](int i) { return lane * S2 + i; });
    // ---- pass 3: DFT over l1: register p holds Z[lane + 64 p] ----
    dft8(v);
    // ---- separate the two real spectra, power / NFFT for bins 0..256: the partner Z[N - k] comes through LDS ----
    double wx[5], wy[5];
#pragma unroll
    for (int p = 0; p < 8; ++p) ex[lane + 64 * p] = v[p].x;
    __syncthreads();
#pragma unroll
    for (int i = 0; i < 5; ++i) wx[i] = ex[(NFFT - (lane + 64 * i)) & (NFFT - 1)];
    __syncthreads();
#pragma unroll
    for (int p = 0; p < 8; ++p) ex[lane + 64 * p] = v[p].y;
    __syncthreads();
#pragma unroll
    for (int i = 0; i < 5; ++i) wy[i] = ex[(NFFT - (lane + 64 * i)) & (NFFT - 1)];
    __syncthreads();
    double* pw = ex;                                         // [2][NBIN + pad]
#pragma unroll
    for (int i = 0; i < 5; ++i) {
        const int k = lane + 64 * i;
        const c2 z = (i < 4) ? v[i] : v[4];                  // k = 256 sits in lane 0, register 4
        const double ar = z.x + wx[i], ai = z.y - wy[i], br = z.x - wx[i], bi = z.y + wy[i];
        if (k < NBIN) {
            const double pa = (ar * ar + ai * ai) * (0.25 / NFFT), pb = (br * br + bi * bi) * (0.25 / NFFT);
            pw[k] = any0 ? pa : 0.0;
            pw[264 + k] = any1 ? pb : 0.0;
        }
    }
    __syncthreads();
    // ---- mel filterbank: lane s sums segment s = [seg[s], seg[s+1]) once with the ascending weights (filter
    // s + 1) and once with the descending ones (filter s); filter m = up(segment m - 1) + down(segment m) ----
    {
        double up0 = 0.0, up1 = 0.0, dn0 = 0.0, dn1 = 0.0;
        if (lane <= NFILT) {
            const int kb = t.seg[lane], ke = t.seg[lane + 1];
            for (int k = kb; k < ke; ++k) {
                const double gu = s_wup[k], gd = s_wdn[k], x0 = pw[k], x1 = pw[264 + k];
                up0 = fma(x0, gu, up0); dn0 = fma(x0, gd, dn0);
                up1 = fma(x1, gu, up1); dn1 = fma(x1, gd, dn1);
            }
        }
        const double pu0 = __shfl_up(up0, 1), pu1 = __shfl_up(up1, 1);   // ascending half lives one segment to the left
        if (lane >= 1 && lane <= NFILT) {
            double acc0 = pu0 + dn0, acc1 = pu1 + dn1;
            if (acc0 == 0.0) acc0 = 2.220446049250313e-16;  // np.finfo(float).eps
            if (acc1 == 0.0) acc1 = 2.220446049250313e-16;
            const double f0 = log10(acc0), f1 = log10(acc1);
            lfb[0][lane - 1] = f0;
            lfb[1][lane - 1] = f1;
            store_fbank(f0, f1);
        }
    }
    __syncthreads();
    // ---- DCT-II (ortho), coefficients 1..13: lane = coefficient + 16 * quarter of the 40 filters ----
    {
        const int c = lane & 15, part = lane >> 4;
        double acc0 = 0.0, acc1 = 0.0;
        if (c < NCEPS) {
            const double* row = t.dct + c * NFILT + part * (NFILT / 4);
            const double* l0 = lfb[0] + part * (NFILT / 4);
            const double* l1f = lfb[1] + part * (NFILT / 4);
#pragma unroll
            for (int m = 0; m < NFILT / 4; ++m) { acc0 = fma(row[m], l0[m], acc0); acc1 = fma(row[m], l1f[m], acc1); }
        }
        acc0 += __shfl_xor(acc0, 16); acc0 += __shfl_xor(acc0, 32);
        acc1 += __shfl_xor(acc1, 16); acc1 += __shfl_xor(acc1, 32);
        store_ceps(acc0, acc1);
    }
}

struct HostTables {
    std::vector<double> window, tw, wup, wdn, dct;
    std::vector<int> seg;
    int flen, fstep, pad_left;
};

// tables built the way the reference builds them (feature.py:25-40,52,58-75,80); who: the caller's name in the messages
int build_tables(const char* who, int sample_rate, double frame_size, double frame_stride, double low_freq, double high_freq,
                 HostTables& h) {
    h.flen = (int)(frame_size * sample_rate);
    h.fstep = (int)(frame_stride * sample_rate);
    GH_REQUIRE(sample_rate > 0 && h.flen >= 1 && h.fstep >= 1, "%s: sample_rate=%d frame=%d step=%d samples", who,
               sample_rate, h.flen, h.fstep);
    int pad_w = 1;
    while (pad_w < h.flen) pad_w <<= 1;  // 1 << (width - 1).bit_length()
    if (pad_w > NFFT) {
        gh_set_error("%s: frames of %d samples exceed the reference's NFFT = %d", who, h.flen, NFFT);
        return GH_ERR_UNSUPPORTED;
    }
    h.pad_left = (pad_w - h.flen) / 2;
    h.window.assign(NFFT, 0.0);
    for (int k = 0; k < pad_w; ++k)
        h.window[k] = pad_w == 1 ? 1.0 : 0.54 - 0.46 * std::cos(2.0 * M_PI * k / (pad_w - 1));
    h.tw.resize(2 * NFFT);
    for (int k = 0; k < NFFT; ++k) {
        const long double ang = -2.0L * 3.14159265358979323846264338327950288L * k / NFFT;
        h.tw[2 * k] = (double)cosl(ang);
        h.tw[2 * k + 1] = (double)sinl(ang);
    }
    if (!(high_freq > 0)) high_freq = sample_rate / 2.0;
    const double low_mel = 2595 * std::log10(1 + low_freq / 700), high_mel = 2595 * std::log10(1 + high_freq / 700);
    std::vector<double> bin(NFILT + 2);
    const double step = (high_mel - low_mel) / (NFILT + 1);   // np.linspace(start, stop, NFILT + 2)
    for (int i = 0; i < NFILT + 2; ++i) {
        const double mel = (i == NFILT + 1) ? high_mel : low_mel + step * i;
        const double hz = 700 * (std::pow(10.0, mel / 2595) - 1);
        bin[i] = std::floor((NFFT + 1) * hz / sample_rate);
    }
    // the triangles (feature.py:66-75) as per-bin weights: bin k in [bin[m-1], bin[m]) rises towards filter m,
    // bin k in [bin[m], bin[m+1]) falls away from filter m
    h.wup.assign(NBIN, 0.0);
    h.wdn.assign(NBIN, 0.0);
    h.seg.assign(NFILT + 2, 0);
    for (int i = 0; i < NFILT + 2; ++i) {
        GH_REQUIRE(bin[i] >= 0 && bin[i] <= NBIN && (i == 0 || bin[i] >= bin[i - 1]),
                   "%s: mel point %d falls on bin %g outside the spectrum", who, i, bin[i]);
        h.seg[i] = (int)bin[i];
    }
    for (int m = 1; m <= NFILT; ++m) {
        const int lo = (int)bin[m - 1], ce = (int)bin[m], hi = (int)bin[m + 1];
        for (int k = lo; k < ce; ++k) h.wup[k] = (k - bin[m - 1]) / (bin[m] - bin[m - 1]);
        for (int k = ce; k < hi; ++k) h.wdn[k] = (bin[m + 1] - k) / (bin[m + 1] - bin[m]);
    }
    h.dct.resize((size_t)NCEPS * NFILT);
    for (int c = 1; c <= NCEPS; ++c)
        for (int m = 0; m < NFILT; ++m)
            h.dct[(size_t)(c - 1) * NFILT + m] = std::sqrt(2.0 / NFILT) * std::cos(M_PI * c * (2 * m + 1) / (2.0 * NFILT));
    return GH_OK;
}

}  // namespace
