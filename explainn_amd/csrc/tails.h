// The fp64 tail probabilities the motif tests share (spacing.hip, enrich.hip, central.hip): each is summed
// from its first term upwards, the first term from lgammas, until a term no longer changes the sum.
#pragma once

#include "common.h"

namespace {

// log of the Binomial(n, q) probability of x
__device__ __forceinline__ double binom_logpmf(double n, double x, double logq, double log1mq) {
    return lgamma(n + 1.0) - lgamma(x + 1.0) - lgamma(n - x + 1.0) + x * logq + (n - x) * log1mq;
}

// ln P[X >= a], X ~ Hypergeometric(N, Np, n), for an enriched threshold: the first term from nine lgammas,
// the following ones from the ratio of neighbouring terms, summed (relative to the first) until x reaches
// min(Np, n) or a term no longer changes the sum
__device__ __noinline__ double hypergeom_logsf(long long a, long long n, long long Np, long long Nc) {
    const double N = (double)(Np + Nc), b = (double)(n - a);
    const double first = lgamma((double)Np + 1.0) - lgamma((double)a + 1.0) - lgamma((double)(Np - a) + 1.0)
                       + lgamma((double)Nc + 1.0) - lgamma(b + 1.0) - lgamma((double)Nc - b + 1.0)
                       - lgamma(N + 1.0) + lgamma((double)n + 1.0) + lgamma(N - (double)n + 1.0);
    const long long top = Np < n ? Np : n;
    double sum = 1.0, term = 1.0;
    for (long long x = a; x < top; ++x) {
        term *= ((double)(Np - x) * (double)(n - x)) / ((double)(x + 1) * (double)(Nc - n + x + 1));
        const double s = sum + term;
        if (s == sum) break;
        sum = s;
    }
    return fmin(0.0, first + log(sum));
}

}  // namespace
