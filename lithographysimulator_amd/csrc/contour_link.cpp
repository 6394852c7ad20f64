// contour_link.cpp -- litho_contour_link: the cycles of a contour's `next` permutation, in the order include/litho_abbe.h
// defines.  Plain C++ (no HIP header, no HIP call): linked into liblitho_abbe.so, and compiled on its own with g++ by
// tests/test_contour_cpu.py.
#include <cstdint>
#include <vector>

#include "../../include/litho_abbe.h"

extern "C" int litho_contour_link(const int32_t* next, int64_t V, int64_t* order, int64_t* starts, int64_t* n_cycles)
{
    if (V < 0 || !starts || !n_cycles || (V > 0 && (!next || !order))) return LITHO_E_ARG;
    *n_cycles = 0;
    starts[0] = 0;
    for (int64_t v = 0; v < V; ++v)
        if (next[v] < 0 || (int64_t)next[v] >= V) return LITHO_E_ARG;
    std::vector<uint8_t> seen((size_t)V, 0);
    int64_t at = 0, cycles = 0;
    for (int64_t v0 = 0; v0 < V; ++v0) {                // the lowest unvisited index opens the next cycle
        if (seen[(size_t)v0]) continue;
        int64_t v = v0;
        do {
            if (seen[(size_t)v]) return LITHO_E_ARG;    // reached twice: two indices share a successor
            seen[(size_t)v] = 1;
            order[at++] = v;
            v = next[v];
        } while (v != v0);
        starts[++cycles] = at;
    }
    *n_cycles = cycles;
    return LITHO_OK;
}
