// Stand-alone host check of the decision line's encoding (sentinel_amd/csrc/cluster_line.hpp): round trips
// at the boundaries, and every fits-test against a plain wide-integer comparison.  Built by
// tests/test_cluster_line_host.py with -fsanitize=address,undefined; exits 0 when everything holds.
#include <cstdint>
#include <cstdio>
#include <cstring>

#include "cluster_line.hpp"

using namespace sga;

static int fails = 0;
#define CHECK(c)                                                  \
    do {                                                          \
        if (!(c)) {                                               \
            std::printf("FAIL line %d: %s\n", __LINE__, #c);      \
            ++fails;                                              \
        }                                                         \
    } while (0)

// the line as a record holds it: 32 words, the base word and the threshold as 64-bit fields inside
struct Line {
    uint32_t w[32];
    uint64_t bw() const {
        uint64_t v;
        std::memcpy(&v, w + LN_BASE, 8);
        return v;
    }
    void set_bw(uint64_t v) { std::memcpy(w + LN_BASE, &v, 8); }
};

int main() {
    const __int128 two32 = (__int128)1 << 32, two47 = (__int128)1 << 47;
    // ---- bucket deltas: 0, 2^32 - 2 (largest), 2^32 - 1 (the null marker: does not fit), negative
    const int64_t bases[] = {0, 1, 12345, (int64_t)(two47 - 1) - (int64_t)two32, (int64_t)(two47 - 1)};
    const int64_t deltas[] = {0, 1, 0x7FFFFFFFll, 0x80000000ll, (int64_t)two32 - 2, (int64_t)two32 - 1, (int64_t)two32,
                              -1, -2, -(int64_t)two32, (int64_t)1 << 40, -((int64_t)1 << 40)};
    for (int64_t base : bases)
        for (int64_t d : deltas) {
            const int64_t q = base + d;
            const bool plain = (__int128)q - base >= 0 && (__int128)q - base <= two32 - 2;
            CHECK(ln_delta_fits(q, base) == plain);
            if (plain) {
                const uint32_t e = ln_enc_delta(q, base);
                CHECK(e != kLnNoBucket);
                CHECK(ln_dec_bucket(e, base) == q);
                Line l{};
                l.w[2 * 3] = e;  // through a pair's word
                CHECK(ln_dec_bucket(l.w[2 * 3], base) == q);
            }
        }
    CHECK(ln_delta_fits(5, 5) && ln_enc_delta(5, 5) == 0u);
    CHECK(ln_delta_fits(5 + 0xFFFFFFFEll, 5) && ln_enc_delta(5 + 0xFFFFFFFEll, 5) == 0xFFFFFFFEu);
    CHECK(!ln_delta_fits(5 + 0xFFFFFFFFll, 5));
    CHECK(!ln_delta_fits(4, 5));
    // extreme bucket numbers against the largest base: no overflow in the test itself
    CHECK(!ln_delta_fits(INT64_MAX, (int64_t)(two47 - 1)));
    CHECK(!ln_delta_fits(INT64_MIN, (int64_t)(two47 - 1)));
    CHECK(!ln_delta_fits(INT64_MIN, 0));
    // ---- counters: 2^32 - 1 fits, 2^32 does not, negative does not
    const int64_t counts[] = {0, 1, 0x7FFFFFFFll, 0x80000000ll, (int64_t)two32 - 1, (int64_t)two32, (int64_t)two32 + 1,
                              -1, INT64_MAX, INT64_MIN};
    for (int64_t v : counts) {
        const bool plain = (__int128)v >= 0 && (__int128)v <= two32 - 1;
        CHECK(ln_count_fits(v) == plain);
        if (plain) CHECK((int64_t)(uint32_t)v == v);
    }
    // ---- base: 2^47 - 1 fits, 2^47 does not; the flags survive any base and the base any flags
    const int64_t qs[] = {0, 1, kLnBaseMargin, kLnBaseMargin + 1, (int64_t)(two47 - 1), (int64_t)two47,
                          (int64_t)(two47 - 1) + kLnBaseMargin, (int64_t)two47 + kLnBaseMargin, -1, INT64_MAX};
    for (int64_t q : qs) {
        const bool plain = (__int128)q >= 0 && (__int128)q < two47;
        CHECK(ln_base_fits(q) == plain);
        if (q < 0) continue;
        const int64_t nb = ln_pick_base(q);
        CHECK(nb >= 0 && nb <= q && q - nb <= kLnBaseMargin);
        if (!ln_base_fits(nb)) continue;
        CHECK(ln_delta_fits(q, nb));
        const uint64_t flag_sets[] = {0, kLnHasOcc, kLnTagValid | ((uint64_t)9 << kLnTagShift), kLnHasOcc | kLnBaseSet};
        for (uint64_t flags : flag_sets) {
            Line l{};
            l.set_bw(flags | kLnBaseSet | (uint64_t)nb);
            CHECK(ln_base(l.bw()) == nb);
            CHECK((l.bw() & ~kLnBaseMask) == (flags | kLnBaseSet));
            CHECK(!(l.bw() & kLnWide));
        }
    }
    CHECK(ln_base_fits((int64_t)(two47 - 1)) && !ln_base_fits((int64_t)two47));
    // ---- the cache tag: valid + bucket index, beside the other flags
    for (int j = -1; j < kLnPairs; ++j) {
        const uint64_t other = kLnHasOcc | kLnBaseSet | (uint64_t)(two47 - 1);
        const uint64_t b = ln_with_tag(other | kLnTagValid | (5ull << kLnTagShift), j);
        CHECK(ln_tag(b) == j);
        CHECK((b & ~(kLnTagMask | kLnTagValid)) == other);
        CHECK(ln_tag(ln_with_tag(b, -1)) == -1);
    }
    CHECK(ln_tag(0) == -1);
    if (fails) return 1;
    std::printf("cluster_line: ok\n");
    return 0;
}
