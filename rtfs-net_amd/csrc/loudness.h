// ITU-R BS.1770 K-weighting (DESIGN.md "Loudness"; include/rtfs_amd.h "Loudness").  The single place with the filter design: the host
// planner of k_loudness.hip takes the coefficients, the state-space form and its powers from here; tests/loudness_oracle.py restates
// the formulas.  Host only, float64 (the matrix powers are multiplied out in long double and rounded once).
//
// Two biquads in series, zero initial state, each in transposed direct form II:
//   shelf      v = b0 x + z1;  z1' = b1 x - a1 v + z2;  z2' = b2 x - a2 v
//   high-pass  y = v + w1;     w1' = -2 v - c1 y + w2;  w2' = v - c2 y           (its numerator is 1, -2, 1)
// As a linear system of the state s = (z1, z2, w1, w2):  s' = A s + B x,  y = C s + D x  with
//   A = [-a1 1 0 0 | -a2 0 0 0 | -2-c1 0 -c1 1 | 1-c2 0 -c2 0],  B = b0 (A's first column) + (b1, b2, 0, 0),  C = (1 0 1 0),  D = b0.
// Only A's powers are needed: a piece of n samples run from zero state ends in e, and from state s it ends in A^n s + e.
#pragma once
#include <math.h>

struct LoudFilter {
    double b0, b1, b2, a1, a2;  // the shelf
    double c1, c2;              // the high-pass denominator
};

// one biquad denominator (and the shelf's numerator) from the design formulas; every product and quotient in this order
inline LoudFilter loud_design(int fs) {
    const double pi = 3.141592653589793;
    LoudFilter f;
    {
        const double f0 = 1681.974450955533, G = 3.999843853973347, Q = 0.7071752369554196;
        const double K = tan(pi * f0 / (double)fs), Vh = pow(10.0, G / 20.0), Vb = pow(Vh, 0.4996667741545416);
        const double a0 = 1.0 + K / Q + K * K;
        f.b0 = (Vh + Vb * K / Q + K * K) / a0;
        f.b1 = 2.0 * (K * K - Vh) / a0;
        f.b2 = (Vh - Vb * K / Q + K * K) / a0;
        f.a1 = 2.0 * (K * K - 1.0) / a0;
        f.a2 = (1.0 - K / Q + K * K) / a0;
    }
    {
        const double f0 = 38.13547087602444, Q = 0.5003270373238773;
        const double K = tan(pi * f0 / (double)fs);
        const double a0 = 1.0 + K / Q + K * K;
        f.c1 = 2.0 * (K * K - 1.0) / a0;
        f.c2 = (1.0 - K / Q + K * K) / a0;
    }
    return f;
}

// A^n, row-major 4 x 4, by binary powering in long double, rounded to double at the end; n >= 0
inline void loud_power(const LoudFilter& f, long long n, double* out) {
    long double base[16] = {-f.a1, 1, 0, 0, -f.a2, 0, 0, 0, -2.0L - f.c1, 0, -f.c1, 1, 1.0L - f.c2, 0, -f.c2, 0};
    long double acc[16], tmp[16];
    for (int i = 0; i < 16; ++i) acc[i] = (i % 5 == 0) ? 1.0L : 0.0L;
    auto mul = [&](const long double* x, const long double* y, long double* z) {
        for (int i = 0; i < 4; ++i)
            for (int j = 0; j < 4; ++j) {
                long double s = 0;
                for (int k = 0; k < 4; ++k) s += x[4 * i + k] * y[4 * k + j];
                tmp[4 * i + j] = s;
            }
        for (int i = 0; i < 16; ++i) z[i] = tmp[i];
    };
    for (; n > 0; n >>= 1) {
        if (n & 1) mul(acc, base, acc);
        mul(base, base, base);
    }
    for (int i = 0; i < 16; ++i) out[i] = (double)acc[i];
}

// the absolute gate on the mean square of a block: -70 LUFS
inline double loud_abs_gate() { return pow(10.0, (-70.0 + 0.691) / 10.0); }
