// cd_search.hpp -- the run search of the cut-line metrology, shared by k_measure_cd (optics.hip) and its tangent
// (metrology.hip).  The library is built without relocatable device code, so the function is inlined into both units.
#pragma once
#include <hip/hip_runtime.h>

namespace litho {

// [lo, hi] = the maximal run of inside samples through c on a line of n samples u(0 .. n - 1), given that u(c) is inside:
// the whole wave scans outward from c in 64-sample chunks, __ballot + a bit scan give the first sample of the other kind (or
// the border).  Every lane of the wave calls it and gets the same lo and hi.
template <class U>
__device__ __forceinline__ void cd_run(U&& u, int c, int n, int lane, float T, bool ex, int& lo, int& hi)
{
    lo = 0;
    hi = n - 1;
    for (int s = c + 1;; s += 64) {                                       // first sample to the right that is not inside
        const int i = s + lane;
        const unsigned long long m = __ballot(i >= n || ((u(i) >= T) != ex));
        if (m) { hi = s + __ffsll((long long)m) - 2; break; }
    }
    for (int s = c - 1;; s -= 64) {                                       // ... and to the left
        const int i = s - lane;
        const unsigned long long m = __ballot(i < 0 || ((u(i) >= T) != ex));
        if (m) { lo = s - __ffsll((long long)m) + 2; break; }
    }
}

}  // namespace litho
