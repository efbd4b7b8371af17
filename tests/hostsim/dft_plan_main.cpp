// dft_plan_main.cpp -- stand-alone check that the FFT pass plan
// (siril_amd/csrc/fft_plan.h factorize) is, for every length n in [2, 8192],
// the plan the registration ran with before the plan-shape A/B knobs
// (SGPU_DFT_R10, SGPU_DFT_PLAN) were retired:
//   c++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all \
//       dft_plan_main.cpp -o dft_plan_main
// `old_plan` below is that function as it stood in sgpu_dft.cpp, verbatim
// (its knobs are cleared from the environment first: the comparison is with
// both unset).  Prints every difference, then "dft plan ok <lengths> <with a
// plan>"; exit status 0 when there is none.
#include <cstdio>
#include <cstdlib>

#include "../../siril_amd/csrc/fft_plan.h"

namespace old_plan {
namespace sgpu {
namespace fft {
constexpr int kMaxFactors = 24;
}
}  // namespace sgpu
struct Plan {
    int n;
    int nf;
    int radix[sgpu::fft::kMaxFactors];
};

// radix-10 passes (fft_lds.h bfly10); SGPU_DFT_R10=0 keeps the 8 / 5 / 4 plans (A/B)
bool r10_enabled() {
    static const bool on = !(std::getenv("SGPU_DFT_R10") && std::atoi(std::getenv("SGPU_DFT_R10")) == 0);
    return on;
}

// radices in pass order: 8s, 10s, 5s, then 4, 3, 2, then any other prime
bool factorize(int n, Plan &pl) {
    pl.n = n;
    pl.nf = 0;
    auto push = [&](int r) {
        if (pl.nf >= sgpu::fft::kMaxFactors) return false;
        pl.radix[pl.nf++] = r;
        return true;
    };
    // SGPU_DFT_PLAN="10,10,8,5": an explicit pass order (A/B of the plan
    // shape; used when its radices multiply to n and all have butterflies)
    if (const char *e = std::getenv("SGPU_DFT_PLAN")) {
        int prod = 1;
        for (const char *q = e; *q;) {
            const int r = std::atoi(q);
            if (r != 2 && r != 3 && r != 4 && r != 5 && r != 8 && r != 10) { prod = 0; break; }
            if (!push(r)) return false;
            prod *= r;
            while (*q && *q != ',') q++;
            if (*q == ',') q++;
        }
        if (prod == n) return true;
        pl.nf = 0;
    }
    int m = n;
    while (m % 8 == 0) { if (!push(8)) return false; m /= 8; }
    if (r10_enabled())
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
    for (int p = 0; p < pl.nf; p++)
        if (pl.radix[p] & 1) {
            const int r = pl.radix[p];
            for (int q = p; q > 0; q--) pl.radix[q] = pl.radix[q - 1];
            pl.radix[0] = r;
            break;
        }
    return true;
}
}  // namespace old_plan

int main() {
    unsetenv("SGPU_DFT_R10");
    unsetenv("SGPU_DFT_PLAN");
    static_assert(sgpu::fft::kMaxFactors == old_plan::sgpu::fft::kMaxFactors, "same pass limit");
    int differences = 0, planned = 0, lengths = 0;
    for (int n = 2; n <= 8192; n++, lengths++) {
        old_plan::Plan was;
        int radix[sgpu::fft::kMaxFactors], nf = 0;
        const bool ok_was = old_plan::factorize(n, was);
        const bool ok = sgpu::fft::factorize(n, radix, nf);
        bool same = ok == ok_was;
        if (same && ok) {
            planned++;
            same = nf == was.nf;
            long long prod = 1;
            for (int p = 0; same && p < nf; p++) {
                same = radix[p] == was.radix[p];
                prod *= radix[p];
            }
            same = same && prod == n;
        }
        if (!same) {
            std::printf("n = %d: plan differs (ok %d / %d, passes %d / %d)\n", n, (int)ok, (int)ok_was, nf, was.nf);
            differences++;
        }
    }
    std::printf("dft plan ok %d %d\n", lengths, planned);
    return differences ? 1 : 0;
}
