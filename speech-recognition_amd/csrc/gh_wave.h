#pragma once
// The gfx950 building blocks the kernel families share: one-instruction min / max, 64-bit values through DPP, decision bits
// from a lane mask, the LDS-only barrier, 2^(y/128), np.isclose.  Device only, everything __forceinline__: a function is
// compiled under the flags of the .hip file that includes it.
#include <hip/hip_runtime.h>
#include <cstdint>

// IEEE minNum / maxNum in ONE instruction: a NaN operand loses, two NaNs give NaN (fmin() / fmax() add a canonicalising
// v_max x,x per operand around it, e.g. for every operand that comes out of an MFMA)
__device__ __forceinline__ double vmin(double a, double b) {
    double r;
    asm("v_min_f64 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
    return r;
}
__device__ __forceinline__ double vmax(double a, double b) {
    double r;
    asm("v_max_f64 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
    return r;
}
__device__ __forceinline__ float vmax(float a, float b) {
    float r;
    asm("v_max_f32 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
    return r;
}

// DPP, mov form (v_mov_b32_dpp, bound_ctrl): for controls that give every lane a source, so no `old` value has to be set up
// (a lane without one would read 0)
template <int CTRL> __device__ __forceinline__ int dpp_mov(int v) { return __builtin_amdgcn_mov_dpp(v, CTRL, 0xF, 0xF, true); }
template <int CTRL> __device__ __forceinline__ double dpp_mov(double v) {
    const int lo = dpp_mov<CTRL>(__double2loint(v));
    const int hi = dpp_mov<CTRL>(__double2hiint(v));
    return __hiloint2double(hi, lo);
}
// DPP, update form: a lane without a source (or in a row that ROW_MASK leaves out) keeps `old`; with BOUND_CTRL a lane
// without a source reads 0 instead
template <int CTRL, int ROW_MASK = 0xF, bool BOUND_CTRL = false> __device__ __forceinline__ int dpp_upd(int old, int v) {
    return __builtin_amdgcn_update_dpp(old, v, CTRL, ROW_MASK, 0xF, BOUND_CTRL);
}
template <int CTRL, int ROW_MASK = 0xF, bool BOUND_CTRL = false> __device__ __forceinline__ double dpp_upd(double old, double v) {
    const int lo = dpp_upd<CTRL, ROW_MASK, BOUND_CTRL>(__double2loint(old), __double2loint(v));
    const int hi = dpp_upd<CTRL, ROW_MASK, BOUND_CTRL>(__double2hiint(old), __double2hiint(v));
    return __hiloint2double(hi, lo);
}
// rotation inside the 16-lane rows (row_ror: CTRL = 0x120 + n)
template <int CTRL> __device__ __forceinline__ double row_rot(double v) { return dpp_mov<CTRL>(v); }
// the value of lane V of every 16-lane row, in all lanes of that row (row_newbcast: the one DPP control gfx90a+ has for
// 64-bit operands too)
template <int V> __device__ __forceinline__ double row_lane(double v) { return dpp_mov<0x150 + V>(v); }
// lane i <- lane i-1 inside the 16-lane row; lane 0 of a row keeps `fill`
__device__ __forceinline__ double row_shr1(double v, double fill) { return dpp_upd<0x111>(fill, v); }
// lane i <- lane i+1 inside the row; lane 15 keeps `fill`
__device__ __forceinline__ double row_shl1(double v, double fill) { return dpp_upd<0x101>(fill, v); }
// the same across the whole wave: lane 0 (lane 63) keeps `fill`
__device__ __forceinline__ double wave_shr1(double v, double fill) { return dpp_upd<0x138>(fill, v); }
__device__ __forceinline__ double wave_shl1(double v, double fill) { return dpp_upd<0x130>(fill, v); }

// word = 2 * word + bit, the bit taken from a compare's lane mask (SGPR pair): one VALU instruction
__device__ __forceinline__ void push_bit(uint32_t& word, unsigned long long mask) {
    unsigned long long carry_out;
    asm("v_addc_co_u32 %0, %1, %2, %2, %3" : "=v"(word), "=s"(carry_out) : "v"(word), "s"(mask));
}
// ... and for 64-bit decision words: the carry of the low half goes on
__device__ __forceinline__ void push_bit(uint64_t& word, unsigned long long mask) {
    uint32_t lo = (uint32_t)word, hi = (uint32_t)(word >> 32);
    unsigned long long c1, c2;
    asm("v_addc_co_u32 %0, %1, %2, %2, %3" : "=v"(lo), "=s"(c1) : "v"(lo), "s"(mask));
    asm("v_addc_co_u32 %0, %1, %2, %2, %3" : "=v"(hi), "=s"(c2) : "v"(hi), "s"(c1));
    word = ((uint64_t)hi << 32) | lo;
}

// Workgroup barrier that orders LDS traffic only (__syncthreads() also waits for every outstanding GLOBAL access,
// vmcnt(0) -- prefetch loads and result stores should stay in flight across it).
__device__ __forceinline__ void lds_barrier() { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); }

// 2^(y/128) for finite y <= 0 (or NaN): table of 2^(j/128) (128 entries) + degree-4 polynomial
// (c3: the k = 3 coefficient, the addend of the first Horner step.  A caller that keeps it in a register across its loop
//  saves the copy into the accumulator of a v_fmac per call; the arithmetic is the same)
__device__ __forceinline__ double exp2s(double y, const double* __restrict__ tab, double c3 = 2.6466421444330968834e-08) {
    const double n = __builtin_rint(y);
    const double r = y - n;
    const int ni = (int)n;  // v_cvt_i32_f64 saturates
    const double t = tab[ni & 127];
    double p = fma(r, 3.583032305400251285e-11, c3);  // (ln2/128)^k / k!, k = 4, 3
    p = fma(p, r, 1.4662262387640424337e-05);
    p = fma(p, r, 5.4152123481245727298e-03);
    p = p * r;  // 2^(r/128) - 1
    return __builtin_ldexp(fma(t, p, t), ni >> 7);
}
// (the float domain of gh_loglik_mfma.hip: the hardware's own exp2)
__device__ __forceinline__ float exp2s(float y, const double*, double = 0.0) { return __builtin_amdgcn_exp2f(y); }

// np.isclose(a, b) with numpy's default tolerances
__device__ __forceinline__ bool np_isclose(double a, double b) {
    if (a == b) return true;
    if (!(a - a == 0.0) || !(b - b == 0.0)) return false;
    return fabs(a - b) <= 1e-8 + 1e-5 * fabs(b);
}
