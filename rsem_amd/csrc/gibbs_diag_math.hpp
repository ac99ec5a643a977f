// gibbs_diag_math.hpp -- the arithmetic of the Gibbs convergence diagnostics (split-R-hat, effective sample size with Geyer's
// initial monotone sequence), as RSEM_DEVFN functions: gibbs_diag.hip runs them on the device, and
// tests/gibbs_diag_check.cpp runs the same source on the host.
//
// The series are integers.  Everything up to here is exact: per sequence (one half of one chain, n values x_0 .. x_{n-1}) the
// sums are taken over y_s = x_s - x_0 in int64,
//     s1 = sum y_s,  s2 = sum y_s^2,  c_t = sum_{s < n-t} y_s y_{s+t},  e_t = (y_0 + .. + y_{t-1}) + (y_{n-t} + .. + y_{n-1}),
// and variances and autocovariances do not depend on the shift.  The functions below are the few double operations that follow,
// in one fixed order (the sequences are always combined in the order j = 0 .. m-1).
#pragma once
#include <cmath>
#include <cstdint>
#include <limits>

#ifndef RSEM_DEVFN
#define RSEM_DEVFN inline  // a host program that includes this header alone
#endif

namespace rsem_diag {

// variance of a sequence, denominator n - 1
RSEM_DEVFN double gd_seq_var(int n, int64_t s1, int64_t s2) {
    const double a = (double)s1;
    return ((double)s2 - a * a / (double)n) / (double)(n - 1);
}
// mean of a sequence relative to a base value c common to all sequences: (x_0 - c) + s1 / n
RSEM_DEVFN double gd_seq_mean_rel(int n, int64_t x0_minus_c, int64_t s1) { return (double)x0_minus_c + (double)s1 / (double)n; }
// autocovariance at lag t, denominator n - 1: sum_{s < n-t} (y_s - ybar)(y_{s+t} - ybar) = c_t - ybar (2 s1 - e_t) + (n - t) ybar^2
RSEM_DEVFN double gd_gamma(int n, int t, int64_t s1, int64_t c_t, int64_t e_t) {
    const double yb = (double)s1 / (double)n;
    return ((double)c_t - yb * (double)(2 * s1 - e_t) + (double)(n - t) * yb * yb) / (double)(n - 1);
}
RSEM_DEVFN double gd_rho(double W, double gamma_mean, double varp) { return 1.0 - (W - gamma_mean) / varp; }

struct Moments {
    double mean, sd, rhat, W, varp;
    int defined;  // 1: W > 0, the autocorrelations exist; 0: rhat is +inf (B > 0) or NaN (B = 0)
};

// seq(j, x0, s1, s2) hands out the sums of sequence j
template <class Seq>
RSEM_DEVFN Moments gd_moments(int n, int m, Seq seq) {
    int64_t c, x0, s1, s2;
    seq(0, c, s1, s2);
    double sm = 0.0, sv = 0.0;
    for (int j = 0; j < m; j++) {
        seq(j, x0, s1, s2);
        sm += gd_seq_mean_rel(n, x0 - c, s1);
        sv += gd_seq_var(n, s1, s2);
    }
    const double mrel = sm / (double)m, W = sv / (double)m;
    double sb = 0.0;
    for (int j = 0; j < m; j++) {
        seq(j, x0, s1, s2);
        const double d = gd_seq_mean_rel(n, x0 - c, s1) - mrel;
        sb += d * d;
    }
    const double B = (double)n * (sb / (double)(m - 1));
    Moments r;
    r.W = W;
    r.varp = (double)(n - 1) / (double)n * W + B / (double)n;
    r.mean = (double)c + mrel;
    r.sd = sqrt(r.varp);
    r.defined = W > 0.0;
    r.rhat = W > 0.0 ? sqrt(r.varp / W) : (B > 0.0 ? std::numeric_limits<double>::infinity() : std::numeric_limits<double>::quiet_NaN());
    return r;
}

// Geyer's initial monotone sequence over the pairs P_k = rho_2k + rho_2k+1, k = 0, 1, ..
struct Geyer {
    double sum, prev;
    int lag, taken;
};
RSEM_DEVFN void gd_geyer_init(Geyer& g) { g.sum = 0.0; g.prev = 0.0; g.lag = 0; g.taken = 0; }
// false: the rule stops in front of pair k (P_k <= 0) and nothing changes
RSEM_DEVFN bool gd_geyer_take(Geyer& g, int k, double rho_even, double rho_odd) {
    double P = rho_even + rho_odd;
    if (!(P > 0.0)) return false;
    if (g.taken && P > g.prev) P = g.prev;
    g.sum += P;
    g.prev = P;
    g.lag = 2 * k + 1;
    g.taken++;
    return true;
}
// S = m n draws in all; tau is held at 1 / log10 S from below (an antithetic series is worth at most S log10 S draws)
RSEM_DEVFN double gd_ess(int64_t S, const Geyer& g) {
    double tau = -1.0 + 2.0 * g.sum;
    const double floor_tau = 1.0 / log10((double)S);
    if (tau < floor_tau) tau = floor_tau;
    return (double)S / tau;
}

struct Result {
    double mean, sd, rhat, ess;
    int lag;
    int is_long;  // the rule took a pair beyond lag L0: ess and lag are not set, the long path redoes the rule with every lag
};

// One transcript from the sums of its m sequences.  lagf(j, t, c_t, e_t) hands out the lag sums, asked for 1 <= t <= L0 + 2 only
// (and t <= n - 1).  The pair behind L0 is looked at as well, so that "long" means exactly: the answer's lag is larger than L0.
// L0 >= n - 1 evaluates every lag.
template <class Seq, class Lag>
RSEM_DEVFN Result gd_evaluate(int n, int m, int L0, Seq seq, Lag lagf) {
    const Moments mo = gd_moments(n, m, seq);
    Result r;
    r.mean = mo.mean; r.sd = mo.sd; r.rhat = mo.rhat;
    r.ess = std::numeric_limits<double>::quiet_NaN();
    r.lag = 0;
    r.is_long = 0;
    if (!mo.defined) return r;
    Geyer g;
    gd_geyer_init(g);
    for (int k = 0; 2 * k + 1 <= n - 1; k++) {
        double rho[2];
        for (int h = 0; h < 2; h++) {
            const int t = 2 * k + h;
            if (t == 0) { rho[h] = 1.0; continue; }
            double gs = 0.0;
            for (int j = 0; j < m; j++) {
                int64_t x0, s1, s2, c_t, e_t;
                seq(j, x0, s1, s2);
                lagf(j, t, c_t, e_t);
                gs += gd_gamma(n, t, s1, c_t, e_t);
            }
            rho[h] = gd_rho(mo.W, gs / (double)m, mo.varp);
        }
        if (!gd_geyer_take(g, k, rho[0], rho[1])) break;
        if (g.lag > L0) { r.is_long = 1; return r; }
    }
    r.ess = gd_ess((int64_t)m * n, g);
    r.lag = g.lag;
    return r;
}

}  // namespace rsem_diag
