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

// PER-FRAME TIMESTAMPS (DESIGN.md "Live streams with per-frame timestamps"; tests/timestamp_oracle.py restates this by brute force).  The
// same rule with t_i = tau_i / tb seconds in place of i b / a: camera frame i, stamped tau_i in a timebase of tb ticks per second, has the
// 25 fps tick r(i) = floor(25 tau_i / tb + 1/2) = G(tau_i) with G(W) = floor((50 W + tb) / (2 tb)), and model frame p shows
// c(p) = max(0, max{i : r(i) <= p}): the last camera frame whose tick is at or before p, and the first camera frame before that.
//   r(i) <= p  <=>  25 tau_i / tb + 1/2 < p + 1  <=>  50 tau_i < tb (2p + 1)
// Once every frame stamped below W is in, exactly the model frames p < G(W) are final: p < G(W) <=> tb (2p + 1) <= 50 W, so every
// frame the predicate admits for such a p is stamped below W.  Conversely p >= G(W) <=> tb (2p + 1) > 50 W: any frame stamped <= W is
// admitted, so c(p) is the last frame received or a later one.
// Exact in 64-bit integers for 1 <= tb <= 2^30 and 0 <= tau, W <= 2^40 (50 W + tb < 2^46; p <= G(W) gives tb (2p + 1) <= 50 W + 2 tb).
constexpr long long FR_MAX_TIMEBASE = 1LL << 30;  // ticks per second
constexpr long long FR_MAX_STAMP = 1LL << 40;     // stamps lie below it, watermarks at or below it

// G(W): the model frames that are final once every camera frame stamped below W is in; G(tau) is also the tick of a frame stamped tau
FR_HD long long fr_stamp_count(long long tb, long long W) { return (50 * W + tb) / (2 * tb); }

// the source predicate: the tick of a frame stamped tau is at or before model frame p
FR_HD bool fr_stamp_shows(long long tb, long long tau, long long p) { return 50 * tau < tb * (2 * p + 1); }

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
