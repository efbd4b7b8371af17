// fft_plan.h -- the pass plan of the LDS FFT (fft_lds.h): plain C++, no
// device code, so that a host-only program can include it
// (tests/hostsim/dft_plan_main.cpp).
#pragma once

namespace sgpu {
namespace fft {

constexpr int kMaxFactors = 24;

// radices of an n-point transform in pass order: 8s, 10s (fft_lds.h bfly10),
// 5s, then 4, 3, 2, then any other prime up to 61, with the first odd radix
// moved to the front.  false: n has a larger prime factor (not supported by
// the LDS kernel) or more than kMaxFactors passes.
inline bool factorize(int n, int (&radix)[kMaxFactors], int &nf) {
    nf = 0;
    auto push = [&](int r) {
        if (nf >= kMaxFactors) return false;
        radix[nf++] = r;
        return true;
    };
    int m = n;
    while (m % 8 == 0) { if (!push(8)) return false; m /= 8; }
    while (m % 10 == 0) { if (!push(10)) return false; m /= 10; }
    while (m % 5 == 0) { if (!push(5)) return false; m /= 5; }
    while (m % 4 == 0) { if (!push(4)) return false; m /= 4; }
    while (m % 3 == 0) { if (!push(3)) return false; m /= 3; }
    while (m % 2 == 0) { if (!push(2)) return false; m /= 2; }
    for (int p = 7; m > 1 && p <= m; p += 2)
        while (m % p == 0) {
            if (p > 61) return false;          // large primes: not supported by the LDS kernel
            if (!push(p)) return false;
            m /= p;
        }
    if (m != 1) return false;
    // an odd radix first: the first pass writes its outputs R words apart
    // (Ns = 1), and an even R (8, 10) puts lanes 4-16 ways onto the same LDS
    // banks; 5 x 10 x 10 x 8 runs the 4000-point rows 5.7 % faster than
    // 8 x 10 x 10 x 5; every odd-first order measured alike (profiles/r05al_*,
    // r05am_*)
    for (int p = 0; p < nf; p++)
        if (radix[p] & 1) {
            const int r = radix[p];
            for (int q = p; q > 0; q--) radix[q] = radix[q - 1];
            radix[0] = r;
            break;
        }
    return true;
}

}  // namespace fft
}  // namespace sgpu
