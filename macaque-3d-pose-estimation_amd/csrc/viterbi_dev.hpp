// Transition log-probability of the anipose Viterbi filter (filter_pose.py:48-120), shared by the
// single-candidate kernels (geometry.hip) and the multi-candidate kernel (candidates.hip).
// Translation units including this are built with -ffp-contract=off (scipy's rounding order).
#pragma once
#include "common.hpp"

namespace mq {

// scipy log_ndtr (Faddeeva form): x < -1: log(erfcx(-t)/2) - t^2, else log1p(-erfc(t)/2), t = x/sqrt(2),
// erfc(t) = exp(-t^2) erfcx(t) (t >= 0) or 2 - exp(-t^2) erfcx(-t).
__device__ __forceinline__ double log_ndtr_d(double x) {
  const double t = x * 0.70710678118654752440;
  if (x < -1.0) return log(erfcx(-t) / 2) - t * t;
  const double e = (t < 0) ? (2. - exp(-t * t) * erfcx(-t)) : exp(-t * t) * erfcx(t);
  return log1p(-e / 2);
}

// log(Phi((d+2)/s) - Phi((d-2)/s)) evaluated as scipy's logsumexp(b=[1,-1]) does, clamped at -100.
__device__ __forceinline__ double trans_logprob(double d, double thres) {
  const double hi = log_ndtr_d((d + 2) / thres);
  const double lo = log_ndtr_d((d - 2) / thres);
  double r;
  if (hi > lo) {
    r = log1p(-exp(lo - hi)) + hi;
  } else if (hi == lo) {
    r = -INFINITY;
  } else {
    r = NAN;
  }
  if (r < -100) r = -100;
  return r;
}

}  // namespace mq
