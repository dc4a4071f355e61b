// Shared by the windowed-inference kernels (k_longform.hip: whole recordings, k_live.hip: live streams): the frame constants, the
// cross-fade weight and the table search.  One definition, so a streamed sample gets bit for bit the weights of an offline one.
#pragma once
#include "common.h"

namespace {

constexpr int SPF = 640;    // samples per video frame: 16 kHz / 25 fps
constexpr int VCH = 512;    // lip-embedding channels

__device__ __forceinline__ float ola_weight(int i, int window, float V) {
    return fminf(1.f, fminf(((float)i + 0.5f) / V, ((float)(window - i) - 0.5f) / V));
}

// largest r in [0, R) with key[r] <= x; key ascending, key[0] = 0 <= x
__device__ __forceinline__ int many_find(const long long* __restrict__ key, int R, long long x) {
    int lo = 0, hi = R - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (key[mid] <= x) lo = mid; else hi = mid - 1;
    }
    return lo;
}

}  // namespace
