// div_q1_check — gsx::div_q1 (csrc/gsx_ops.h) against the plain int64 division,
// on the host.  Prints "ok <cases>" and exits 0, or the first mismatches and 1.
// Built by tests/test_div_q1.py (hipcc, host pass only).
#include <cinttypes>
#include <cstdio>
#include <vector>

#include "gsx_ops.h"

namespace {

uint64_t n_cases = 0, n_bad = 0;

void check(int64_t mt, int64_t q1) {
    const int64_t got = gsx::div_q1(mt, q1, gsx::q1_inverse(q1));
    const int64_t want = mt / q1;
    ++n_cases;
    if (got != want && n_bad++ < 20)
        std::printf("mismatch: %" PRId64 " / %" PRId64 " = %" PRId64 ", div_q1 gave %" PRId64 "\n", mt, q1, want, got);
}

// mt, its neighbours and its negative, kept inside [INT64_MIN + 1, INT64_MAX]
void around(std::vector<int64_t>& v, __int128 x) {
    for (int d = -1; d <= 1; ++d)
        for (int sg = -1; sg <= 1; sg += 2) {
            const __int128 y = sg * (x + d);
            if (y >= -(__int128)INT64_MAX && y <= (__int128)INT64_MAX) v.push_back((int64_t)y);
        }
}

}  // namespace

int main() {
    const int64_t quanta[] = {1, 2, 3, 1000000000LL, 999999937LL, (1LL << 32) - 1, (1LL << 32) + 1, 1LL << 62};
    const double caps[] = {1.0, 10.0, 3600.0, 3600.5, 1e9};  // TimeInMeshCap, also a non-integer one
    for (const int64_t q1 : quanta) {
        std::vector<int64_t> mts = {0, 1, -1, INT64_MAX, INT64_MIN + 1};
        for (const int e : {31, 32, 52, 53}) around(mts, (__int128)1 << e);
        around(mts, (__int128)gsx::DIV_Q1_BOUND);
        // k * q1 and k * q1 +- 1 for k around 0, around the cap and around the fast-path bound
        std::vector<__int128> ks;
        for (int k = -3; k <= 3; ++k) ks.push_back(k);
        for (const double c : caps)
            for (int k = -2; k <= 2; ++k) ks.push_back((__int128)c + k);
        for (int k = -3; k <= 3; ++k) ks.push_back((__int128)(gsx::DIV_Q1_BOUND / q1) + k);
        for (const __int128 k : ks) around(mts, k * q1);
        for (const int64_t mt : mts) check(mt, q1);
        // a quantum the engine lets through when TimeInMeshWeight is 0
        for (const int64_t mt : mts) check(mt, -q1);
    }
    // 10^7 seeded pairs: mt over every magnitude (a random shift), q1 likewise, half
    // of them with q1 drawn near mt's magnitude so that quotients are small too
    gsx::Rng rng{0x5eed, 1, 2, 0, 0};
    auto r64 = [&]() { return gsx::h4(rng.seed, rng.tag, rng.vertex, rng.k++); };
    for (int i = 0; i < 10000000; ++i) {
        const uint64_t a = r64(), b = r64(), c = r64();
        int64_t mt = (int64_t)(a >> 1 >> (c & 63));
        if (c & 64) mt = -mt;
        int64_t q1 = (int64_t)(b >> 1 >> ((c >> 8) & 63));
        if (c & 128) q1 = (int64_t)(b >> 1 >> ((c & 63) | 1));
        if (q1 == 0) q1 = 1;
        check(mt, q1);
    }
    if (n_bad) {
        std::printf("FAILED: %" PRIu64 " of %" PRIu64 " cases\n", n_bad, n_cases);
        return 1;
    }
    std::printf("ok %" PRIu64 "\n", n_cases);
    return 0;
}
