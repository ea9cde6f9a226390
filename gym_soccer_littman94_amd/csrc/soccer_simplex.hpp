// soccer_simplex.hpp — the Euclidean projection of five numbers onto the probability simplex, in float64, the same on the
// host and on the device (soccer_gradient_play_run's step; tests/host/simplex_host.cpp runs it on the host).
// The definition, every operation its own rounding:
//   u   = v sorted in descending order
//   css = the running sum of u from 0.0:  css_k = css_{k-1} + u_k
//   for k = 1 .. 5:  t = (css_k - 1.0) / (double)k;  tau = t for k = 1, and for k > 1 whenever u_k - t > 0.0
//   out[a] = v[a] - tau if that is > 0.0, else 0.0 (never -0.0)
// (k = 1 always holds in exact arithmetic; taking it unconditionally gives tau a value for rows so large that u_1 - t
// rounds to 0.)  Values that compare equal may be sorted either way: +0.0 and -0.0 give the same css, t and tau.
#pragma once

#if defined(__HIPCC__) || defined(__CUDACC__)
#define SOCCER_SIMPLEX_HD __host__ __device__
#else
#define SOCCER_SIMPLEX_HD
#endif

namespace soccer {

SOCCER_SIMPLEX_HD inline void simplex_order(double& hi, double& lo) {
    const double a = hi, b = lo;
    const bool swap = b > a;
    hi = swap ? b : a;
    lo = swap ? a : b;
}

SOCCER_SIMPLEX_HD inline void project_simplex5(const double* v, double* out) {
    double u0 = v[0], u1 = v[1], u2 = v[2], u3 = v[3], u4 = v[4];
    // a sorting network of nine exchanges (named scalars: nothing is indexed at run time)
    simplex_order(u0, u1); simplex_order(u3, u4); simplex_order(u2, u4);
    simplex_order(u2, u3); simplex_order(u0, u3); simplex_order(u0, u2);
    simplex_order(u1, u4); simplex_order(u1, u3); simplex_order(u1, u2);
    double css = 0.0 + u0;
    double tau = (css - 1.0) / 1.0;
    double t;
    css = css + u1; t = (css - 1.0) / 2.0; tau = u1 - t > 0.0 ? t : tau;
    css = css + u2; t = (css - 1.0) / 3.0; tau = u2 - t > 0.0 ? t : tau;
    css = css + u3; t = (css - 1.0) / 4.0; tau = u3 - t > 0.0 ? t : tau;
    css = css + u4; t = (css - 1.0) / 5.0; tau = u4 - t > 0.0 ? t : tau;
    const double d0 = v[0] - tau, d1 = v[1] - tau, d2 = v[2] - tau, d3 = v[3] - tau, d4 = v[4] - tau;
    out[0] = d0 > 0.0 ? d0 : 0.0; out[1] = d1 > 0.0 ? d1 : 0.0; out[2] = d2 > 0.0 ? d2 : 0.0;
    out[3] = d3 > 0.0 ? d3 : 0.0; out[4] = d4 > 0.0 ? d4 : 0.0;
}

}  // namespace soccer
