// Stand-alone host program of tests/test_send_rule_exact.py: the send rule the kernels run
// (pydcop_amd/csrc/send_rule.h: comp_match, division only where two products do not settle it)
// against the plain formula (comp_match_div, the reference's quotient), for double and float.
// Exit status 0 and one "OK" line per type, or the first differing input and status 1.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <type_traits>
#include <vector>

#include "send_rule.h"

template <typename T>
struct Stats {
    long long cases = 0, decided = 0;
};

template <typename T>
static const char* name() { return std::is_same<T, double>::value ? "double" : "float"; }

// the (a, s) level: whatever quotient_below_fast decides is what the rounded quotient says
template <typename T>
static void check_as(T a, T s, T stab, Stats<T>& st) {
    ++st.cases;
    bool yes, no;
    mxs::quotient_below_fast(a, s, mxs::send_rule_edges(stab), yes, no);
    if (!(yes | no)) return;
    ++st.decided;
    volatile T q = a / s;
    const bool plain = q < stab;
    if (s == (T)0 || (yes & no) || plain != yes) {
        std::printf("FAIL %s quotient_below_fast: a=%a s=%a stability=%a yes=%d no=%d plain=%d\n", name<T>(), (double)a, (double)s,
                    (double)stab, (int)yes, (int)no, (int)plain);
        std::exit(1);
    }
}

// the (c, prev) level: comp_match == comp_match_div
template <typename T>
static void check_cp(T c, T prev, T stab, Stats<T>& st) {
    ++st.cases;
    bool yes, no;
    mxs::comp_match_fast(c, prev, mxs::send_rule_edges(stab), yes, no);
    if (yes | no) ++st.decided;
    const bool got = mxs::comp_match(c, prev, stab), want = mxs::comp_match_div(c, prev, stab);
    if (got != want) {
        std::printf("FAIL %s comp_match: c=%a prev=%a stability=%a new=%d plain=%d\n", name<T>(), (double)c, (double)prev,
                    (double)stab, (int)got, (int)want);
        std::exit(1);
    }
}

// a whole message: msg_match == the conjunction of the plain formula over its components
template <typename T>
static void check_msg(const T (&m)[3], const T (&prev)[3], T stab) {
    bool want = true;
    for (int d = 0; d < 3; ++d) want = want && mxs::comp_match_div(m[d], prev[d], stab);
    const bool got = mxs::msg_match<T, 3>(m, prev, stab);
    if (got != want) {
        std::printf("FAIL %s msg_match: m={%a,%a,%a} prev={%a,%a,%a} stability=%a new=%d plain=%d\n", name<T>(), (double)m[0],
                    (double)m[1], (double)m[2], (double)prev[0], (double)prev[1], (double)prev[2], (double)stab, (int)got, (int)want);
        std::exit(1);
    }
}

template <typename T>
static T step(T x, int ulps) {
    const T to = ulps > 0 ? std::numeric_limits<T>::infinity() : -std::numeric_limits<T>::infinity();
    for (int i = 0; i < std::abs(ulps); ++i) x = std::nextafter(x, to);
    return x;
}

static uint64_t g_rng = 0x9e3779b97f4a7c15ull;
static double uniform01() {  // xorshift64*, 53 bits
    g_rng ^= g_rng >> 12, g_rng ^= g_rng << 25, g_rng ^= g_rng >> 27;
    return (double)((g_rng * 0x2545f4914f6cdd1dull) >> 11) * 0x1p-53;
}

template <typename T>
static int run() {
    using L = std::numeric_limits<T>;
    const T inf = L::infinity(), nan = L::quiet_NaN();
    const T stabs[] = {(T)0, (T)0x1p-20, (T)0.1, (T)0.5, (T)1, (T)8};
    const int e_min = L::min_exponent - L::digits, e_max = L::max_exponent - 1;  // 2^e_min: the smallest subnormal

    // 1. a at 0, +-1 .. +-64 ulps around fl(stability * s), s over the full exponent range (subnormals included)
    Stats<T> near;
    const T mant[] = {(T)1, (T)1.25, (T)(2 - 4 * (double)L::epsilon()), (T)1.7320508075688772};
    for (T stab : stabs)
        for (int e = e_min; e <= e_max; ++e)
            for (T m : mant) {
                const T s = std::ldexp(m, e);
                if (!(s > 0) || std::isinf(s)) continue;
                const T mid = stab * s;
                if (std::isinf(mid)) continue;
                T a = step(mid, -64);
                for (int k = -64; k <= 64; ++k, a = std::nextafter(a, inf))
                    if (a >= 0) check_as(a, s, stab, near);
            }
    // ... and with a subnormal, s anything (the quotient underflows or is tiny), a anything over a subnormal s
    for (T stab : stabs)
        for (int ea = e_min; ea < L::min_exponent + 2; ea += 3)
            for (int es = e_min; es <= e_max; es += 7) {
                check_as(std::ldexp((T)1.5, ea), std::ldexp((T)1.25, es), stab, near);
                check_as(std::ldexp((T)1.25, es), std::ldexp((T)1.5, ea), stab, near);
            }

    // 2. special operands, every pair, both orders: zeros, subnormals, the ends of the range, +-inf, NaN;
    //    prev + c == 0 (c = -prev) and prev == c are among the pairs
    Stats<T> special;
    std::vector<T> v = {(T)0, L::denorm_min(), 3 * L::denorm_min(), L::min() / 2, L::min(), step(L::min(), 1), (T)0x1p-20, (T)0.1, (T)1,
                        step((T)1, 1), step((T)1, -1), (T)1.5, (T)3, (T)1000, L::max() / 4, L::max() / 2, L::max(), inf, nan};
    const size_t n_pos = v.size();
    for (size_t i = 0; i < n_pos; ++i) v.push_back(-v[i]);
    const T more_stabs[] = {(T)0, (T)0x1p-20, (T)0.1, (T)0.5, (T)1, (T)8, L::denorm_min(), L::min(), L::max(), inf, nan, (T)-0.5};
    for (T stab : more_stabs)
        for (T c : v)
            for (T prev : v) check_cp(c, prev, stab, special);

    // ... and as components of a message: every position, beside components that match, do not, or are undecided
    for (T stab : stabs)
        for (size_t i = 0; i < v.size(); ++i)
            for (size_t j = 0; j < v.size(); ++j) {
                const T und_prev = ((T)1 + stab / 2) * (T)1.1, und_c = ((T)1 - stab / 2) * (T)1.1;  // (quotient ~stability)
                const T others[3][2] = {{(T)1, (T)1}, {(T)1, (T)-3}, {und_c, und_prev}};
                for (int pos = 0; pos < 3; ++pos)
                    for (const auto& o : others)
                        for (const auto& o2 : others) {
                            T m[3] = {o[0], o2[0], o[0]}, p[3] = {o[1], o2[1], o[1]};
                            m[pos] = v[i], p[pos] = v[j];
                            check_msg(m, p, stab);
                        }
            }

    // 3. pairs at the threshold: prev = (1 + stability / 2) x, c = (1 - stability / 2) x has the quotient
    //    ~stability; c a few ulps either side, x over the exponent range
    Stats<T> edge;
    for (T stab : stabs)
        for (int e = e_min + 2; e <= e_max - 4; ++e) {
            const T x = std::ldexp((T)1.1, e), prev = ((T)1 + stab / 2) * x, c0 = ((T)1 - stab / 2) * x;
            for (int k = -8; k <= 8; ++k) {
                check_cp(step(c0, k), prev, stab, edge);
                check_cp(prev, step(c0, k), stab, edge);
                check_cp(-step(c0, k), -prev, stab, edge);
            }
        }

    // 4. ordinary inputs: random messages of either sign; the fast path must decide nearly all of them
    Stats<T> ordinary;
    for (T stab : {(T)0x1p-20, (T)0.1, (T)0.5, (T)1, (T)8})
        for (int i = 0; i < 200000; ++i) {
            const T prev = (T)(20.0 * uniform01() - 10.0);
            const T c = (i & 1) ? (T)(20.0 * uniform01() - 10.0) : (T)((double)prev * (1.0 + 0.2 * (uniform01() - 0.5)));  // (near prev)
            check_cp(c, prev, stab, ordinary);
        }
    if (ordinary.decided < ordinary.cases * 0.999) {
        std::printf("FAIL %s: the fast path decided only %lld of %lld ordinary inputs\n", name<T>(), ordinary.decided, ordinary.cases);
        return 1;
    }
    std::printf("OK %s near=%lld (decided %lld) special=%lld edge=%lld (decided %lld) ordinary=%lld (decided %lld)\n", name<T>(),
                near.cases, near.decided, special.cases, edge.cases, edge.decided, ordinary.cases, ordinary.decided);
    return 0;
}

int main() {
    const int rc = run<double>() | run<float>();
    return rc;
}
