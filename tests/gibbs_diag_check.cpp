// gibbs_diag_check.cpp -- the Gibbs convergence diagnostics on the host, through the same source the device runs
// (rsem_amd/csrc/gibbs_diag_math.hpp).  Built by tests/test_gibbs_diag_cpu.py with -fsanitize=address,undefined.
//
//   gibbs_diag_check FILE L0
// FILE: int32 M+1, int32 nchains, int32 nsamples[nchains], then the blocks, nsamples[k] x (M+1) int32 each.
// Prints one line per column 0 .. M: id mean sd rhat ess lag long   (%.17g; long = 1: the rule's lag exceeds L0, the column
// would have been finished by the long path).
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../rsem_amd/csrc/gibbs_diag_math.hpp"

using namespace rsem_diag;

int main(int argc, char** argv) {
    if (argc < 3) { fprintf(stderr, "usage: gibbs_diag_check FILE L0\n"); return 2; }
    FILE* f = fopen(argv[1], "rb");
    if (!f) { perror(argv[1]); return 2; }
    const int L0 = atoi(argv[2]);
    int32_t M1 = 0, nchains = 0;
    if (fread(&M1, 4, 1, f) != 1 || fread(&nchains, 4, 1, f) != 1 || M1 < 1 || nchains < 1) { fprintf(stderr, "bad header\n"); return 2; }
    std::vector<int32_t> ns(nchains);
    if (fread(ns.data(), 4, nchains, f) != (size_t)nchains) { fprintf(stderr, "bad header\n"); return 2; }
    std::vector<std::vector<int32_t>> cv(nchains);
    int32_t nmin = ns[0];
    for (int k = 0; k < nchains; k++) {
        if (ns[k] < 0) { fprintf(stderr, "bad header\n"); return 2; }
        cv[k].resize((size_t)ns[k] * M1);
        if (fread(cv[k].data(), 4, cv[k].size(), f) != cv[k].size()) { fprintf(stderr, "short file\n"); return 2; }
        if (ns[k] < nmin) nmin = ns[k];
    }
    fclose(f);
    const int n = nmin / 2, m = 2 * nchains;
    if (n < 2) { fprintf(stderr, "n < 2\n"); return 3; }
    for (int col = 0; col < M1; col++) {
        auto X = [&](int j, int s) -> int64_t {  // sample s of sequence j
            const int k = j / 2;
            return cv[k][(size_t)(ns[k] - 2 * n + (j % 2) * n + s) * M1 + col];
        };
        std::vector<int64_t> s1(m, 0), s2(m, 0);
        for (int j = 0; j < m; j++)
            for (int s = 0; s < n; s++) {
                const int64_t y = X(j, s) - X(j, 0);
                s1[j] += y;
                s2[j] += y * y;
            }
        auto seq = [&](int j, int64_t& x0, int64_t& a, int64_t& b) { x0 = X(j, 0); a = s1[j]; b = s2[j]; };
        auto lagf = [&](int j, int t, int64_t& c_t, int64_t& e_t) {
            const int64_t x0 = X(j, 0);
            c_t = e_t = 0;
            for (int s = 0; s < n - t; s++) c_t += (X(j, s) - x0) * (X(j, s + t) - x0);
            for (int s = 0; s < t; s++) e_t += (X(j, s) - x0) + (X(j, n - 1 - s) - x0);
        };
        const Result shortr = gd_evaluate(n, m, L0, seq, lagf);
        const Result r = shortr.is_long ? gd_evaluate(n, m, n, seq, lagf) : shortr;
        printf("%d %.17g %.17g %.17g %.17g %d %d\n", col, r.mean, r.sd, r.rhat, r.ess, r.lag, shortr.is_long);
    }
    return 0;
}
