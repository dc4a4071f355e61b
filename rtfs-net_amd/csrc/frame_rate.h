// Camera frames at any constant rate -> the model's 25 fps (DESIGN.md "Live streams at the camera's frame rate").  The single place with
// the arithmetic, shared by the host planners and the kernels; tests/frame_rate_oracle.py restates the rule by brute force.
//
// Camera frame i of a stream at a / b fps (reduced) has the 25 fps tick r(i) = floor(i 25 b / a + 1/2); model frame p shows the last camera
// frame whose tick is at or before p, c(p) = max{i : r(i) <= p}; n camera frames give the model frames p with c(p) < n, P(n) of them.
//   r(i) <= p  <=>  i 25 b / a + 1/2 < p + 1  <=>  i < a (2p + 1) / (50 b)      so  c(p) = ceil(a (2p + 1) / (50 b)) - 1
//   c(p) < n   <=>  a (2p + 1) <= 50 b n      <=>  p <= (50 b n - a) / (2 a)    so  P(n) = floor((50 b n + a) / (2 a))
// Exact in 64-bit integers for a, b <= 2^20 and n <= 2^36 (then p < 2^41 and every product stays below 2^62).
#pragma once

#if defined(__HIPCC__) || defined(__CUDACC__)
#define FR_HD __host__ __device__ __forceinline__
#else
#define FR_HD inline
#endif

constexpr long long FR_MAX_TERM = 1LL << 20;    // the largest reduced numerator / denominator
constexpr long long FR_MAX_FRAMES = 1LL << 36;  // the most camera frames of one stream
constexpr long long FR_MIN_FPS = 1, FR_MAX_FPS = 240;

// c(p): the camera frame that model frame p shows
FR_HD long long fr_source(long long a, long long b, long long p) { return (a * (2 * p + 1) + 50 * b - 1) / (50 * b) - 1; }

// P(n): the model frames that n camera frames give
FR_HD long long fr_count(long long a, long long b, long long n) { return (50 * b * n + a) / (2 * a); }

// num / den -> reduced a / b; false for what the rule does not cover
inline bool fr_reduce(long long num, long long den, long long* a, long long* b) {
    if (num < 1 || den < 1) return false;
    long long x = num, y = den;
    while (y) {
        const long long t = x % y;
        x = y;
        y = t;
    }
    num /= x;
    den /= x;
    if (num > FR_MAX_TERM || den > FR_MAX_TERM || num < FR_MIN_FPS * den || num > FR_MAX_FPS * den) return false;
    *a = num;
    *b = den;
    return true;
}
