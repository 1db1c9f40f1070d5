// send_rule.h -- one component of the send rule (approx_match, maxsum.py:688-710): the same
// text for the device kernels, the emulated build of the CPU tests and a stand-alone host
// program (tests/test_send_rule_exact.py), so that what is proved and tested here is what runs.
#pragma once

#ifndef MXS_HD
#if defined(__HIPCC__)
#define MXS_HD __host__ __device__ __forceinline__
#else
#define MXS_HD inline
#endif
#endif

#ifndef MXS_SWEEP_SKIP
#define MXS_SWEEP_SKIP 0  // timing experiments only (results wrong): 1 the neighbour sums of variable_pack read the
#endif                    // lane's own record (no lane crossing), 2 the send rule never divides

namespace mxs {

MXS_HD double sr_abs(double x) { return __builtin_fabs(x); }
MXS_HD float sr_abs(float x) { return __builtin_fabsf(x); }

// The reference's expressions, in its order: `2 * delta / abs(prev + c) < stability`.
template <typename T>
MXS_HD bool comp_match_div(T c, T prev_c, T stability) {
    if (prev_c != c) {
        const T delta = sr_abs(prev_c - c);
        if (prev_c + c != (T)0) {
            if (!(((T)2 * delta / sr_abs(prev_c + c)) < stability)) return false;
        } else {
            return false;
        }
    }
    return true;
}

template <typename T>
struct SendRuleBand;
template <>
struct SendRuleBand<double> {  // u = 2^-53, g = 8 u
    static constexpr double LO = 1.0 - 0x1p-50, HI = 1.0 + 0x1p-50, STAB_MIN = 0x1p-1021;
};
template <>
struct SendRuleBand<float> {  // u = 2^-24, g = 8 u
    static constexpr float LO = 1.0f - 0x1p-21f, HI = 1.0f + 0x1p-21f, STAB_MIN = 0x1p-125f;
};

// The two edges of the band around `stability` inside which only the division decides; they depend on
// `stability` alone (wave-uniform on the GPU: computed once, not per component).
template <typename T>
struct SendRuleEdges {
    T lo, hi;   // fl(stability * (1 - g)), fl(stability * (1 + g))
    bool safe;  // stability is finite and >= 2 * the smallest normal number: lo and hi are normal or +inf
};
template <typename T>
MXS_HD SendRuleEdges<T> send_rule_edges(T stability) {
    using B = SendRuleBand<T>;
    return {stability * B::LO, stability * B::HI, stability >= B::STAB_MIN};
}

// The decision of comp_match_div without the division where the answer is clear: `yes` the quotient
// rounds below `stability`, `no` it does not, neither: undecided (take the division).
//
// Let u be the unit roundoff of T (2^-53 / 2^-24), g = 8 u, a = fl(2 * |prev - c|) and
// s = |fl(prev + c)| exactly as the reference computes them, q = fl(a / s) its quotient, and
// lo = fl(fl(stability * (1 - g)) * s), hi = fl(fl(stability * (1 + g)) * s); 1 - g and 1 + g are exact in T.
// A decision is taken only if stability >= STAB_MIN (so the inner products are normal: relative
// error <= u each) and lo is a NORMAL number, which implies: s > 0, no NaN in `stability` or s,
// lo has a relative error <= u of its own, and hi >= lo is normal too (or +inf, which decides
// nothing).  A NaN in `a` fails both comparisons below.
//   a < lo:  a < stability * s * (1 - 8u) (1 + u)^2 < stability * s * (1 - 5u), so the exact
//     quotient a / s is below stability * (1 - 5u).  The predecessor of a normal `stability` is at
//     least stability * (1 - 2u), rounding to nearest is monotonic, hence
//     q <= fl(stability * (1 - 5u)) <= pred(stability) < stability: a match.  (q may underflow to a
//     subnormal or to zero: still monotonic, still below.)
//   a > hi:  a > stability * s * (1 + 8u) (1 - u)^2 > stability * s * (1 + 5u), so a / s > stability,
//     and since `stability` is representable, q >= stability (q = +inf included: a = +inf, or
//     the quotient overflows): no match.
// prev == c, finite and non-zero, is decided only through a = 0 < lo, where the reference returns a
// match as well; prev + c == 0 gives lo = 0 (or NaN) and is never decided here.
template <typename T>
MXS_HD void quotient_below_fast(T a, T s, const SendRuleEdges<T>& e, bool& yes, bool& no) {
    const T lo = e.lo * s, hi = e.hi * s;
#if MXS_SWEEP_SKIP & 2
    yes = a < lo, no = !yes;
    return;
#endif
    const bool safe = e.safe & (bool)__builtin_isnormal(lo);
    yes = safe & (a < lo);
    no = safe & (a > hi);
}
template <typename T>
MXS_HD void comp_match_fast(T c, T prev_c, const SendRuleEdges<T>& e, bool& yes, bool& no) {
    quotient_below_fast((T)2 * sr_abs(prev_c - c), sr_abs(prev_c + c), e, yes, no);
}

// approx_match, maxsum.py:688-710, one component (prev is not None).  Bit for bit the decision
// of comp_match_div; the division runs only for the rare inputs comp_match_fast leaves open (on
// the GPU: the branch is skipped unless some lane of the wave needs it).
template <typename T>
MXS_HD bool comp_match(T c, T prev_c, T stability) {
    bool yes, no;
    comp_match_fast(c, prev_c, send_rule_edges(stability), yes, no);
    if (__builtin_expect(!(yes | no), 0)) return comp_match_div(c, prev_c, stability);
    return yes;
}

// All D components of a message match: the D fast decisions side by side, then ONE rare branch to the
// divisions if they leave the answer open (no component says no, some component is undecided).
template <typename T, int D>
MXS_HD bool msg_match(const T (&m)[D], const T (&prev)[D], T stability) {
    const SendRuleEdges<T> e = send_rule_edges(stability);
    bool all_yes = true, any_no = false;
    for (int d = 0; d < D; ++d) {
        bool yes, no;
        comp_match_fast(m[d], prev[d], e, yes, no);
        all_yes &= yes;
        any_no |= no;
    }
    if (__builtin_expect(!(all_yes | any_no), 0)) {
        all_yes = true;
        for (int d = 0; d < D; ++d) all_yes &= comp_match_div(m[d], prev[d], stability);
    }
    return all_yes;
}

}  // namespace mxs
