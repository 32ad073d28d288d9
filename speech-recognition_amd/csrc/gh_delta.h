// delta_feature (sr/core.py:13-22) stated once: central difference, one-sided at both ends of the utterance, and the
// delta-delta as the same rule on the delta track.  Every value is a single IEEE subtraction of rows f(r, c), r in
// [t - 2, t + 2] clipped to [0, T): whoever supplies the rows gets the same bits.  Device only.
#pragma once
#include <hip/hip_runtime.h>

// f(r, c): cepstrum c of frame r; t: the frame; T: frames of the utterance (>= 2; anything beyond reach while it is open)
template <typename I, typename F>
__device__ __forceinline__ void delta_stack(F f, I t, I T, int c, double& x, double& d, double& dd) {
    auto delta_at = [&](I r) {
        if (r == 0) return f(I(1), c) - f(I(0), c);
        if (r == T - 1) return f(r, c) - f(r - 1, c);
        return f(r + 1, c) - f(r - 1, c);
    };
    d = delta_at(t);
    if (t == 0) dd = delta_at(I(1)) - d;
    else if (t == T - 1) dd = d - delta_at(t - 1);
    else dd = delta_at(t + 1) - delta_at(t - 1);
    x = f(t, c);
}
