// Host-only driver of csrc/vct_tilediv.h -- the multiply-high division of a tile index by tiles_x and the unit light
// vector -- for a run with and without -fsanitize=address,undefined (tests/test_tilediv.py).  No GPU call.
//   tilediv_check_main                   the checks of the division; prints "tilediv_check ok"
//   tilediv_check_main LIGHTS OUT        LIGHTS: n x 3 floats (raw, native); OUT: vct_light_unit of each (n x 3 floats)
//
// vct_create accepts every positive int32 width, so tiles_x goes up to 2^28 and a tile index up to 2^31: that range cannot
// be enumerated, so the division is checked in two parts (the issue's fallback rule, stated here and in the test):
//   A  every d in 1 .. 2048 (frames up to 16384 pixels wide) over n in [0, d * 2048): all n of the first and the last 4 d
//      of the range, 10^6 seeded n, and the two ends k d and k d + d - 1 of every quotient k -- the quotient is monotone
//      in n (a product and a shift), so equal ends settle every n between them: with them part A covers its whole range;
//   B  2^28, the powers of two and their neighbours and seeded d in (2048, 2^28] over n in [0, 2^31): the first and the
//      last 4 d (capped at 2^12 values each), the ends of seeded quotients, seeded n.
// The seeded values of a divisor come from a generator seeded with the divisor, so the divisors can be dealt to threads
// (up to 8) without changing what is checked.
// A quotient is checked by q d <= n < q d + d in 64 bits -- the definition, with no division to trust.
#include <stdio.h>
#include <stdint.h>

#include <atomic>
#include <thread>
#include <vector>

#include "../voxel-cone-tracing_amd/csrc/vct_tilediv.h"

static std::atomic<int> failures{0};
#define EXPECT(cond) do { if (!(cond)) { if (failures < 20) printf("FAILED line %d: %s\n", __LINE__, #cond); ++failures; } } while (0)

struct Rng {
    uint64_t state;
    explicit Rng(uint64_t seed) : state(seed * 0x9e3779b97f4a7c15ull + 1u) {}
    uint32_t bits31() {
        state = state * 6364136223846793005ull + 1442695040888963407ull;
        return (uint32_t)(state >> 33);
    }
    uint32_t below(uint64_t range) { return (uint32_t)(((uint64_t)bits31() * range) >> 31); }   // range <= 2^31
};

static inline bool exact(uint32_t n, uint32_t d, VctTileDiv t) {
    const uint64_t q = vct_tilediv(n, d, t.mul, t.shift);
    return q * d <= n && (uint64_t)n < q * d + d;
}

static void report(uint32_t n, uint32_t d, VctTileDiv t) {
    if (failures < 20) printf("FAILED: %u / %u gives %u (mul %u shift %u)\n", n, d, vct_tilediv(n, d, t.mul, t.shift), t.mul, t.shift);
    ++failures;
}

// n in [0, range): the first and last `edge` values, the ends of the quotients `k` (all below kmax, or `nk` seeded ones), `nrand` seeded n
static void check_divisor(uint32_t d, uint64_t range, uint64_t edge, uint32_t nk_seeded, uint32_t nrand) {
    const VctTileDiv t = vct_tilediv_make(d);
    Rng rng(d);
    if (d >= 2u && d <= VCT_TILEDIV_MAX_D) EXPECT(t.mul != 0u);            // every divisor a frame can have, but 1, is certified
    if (edge > range) edge = range;
    for (uint64_t n = 0; n < edge; ++n)
        if (!exact((uint32_t)n, d, t)) report((uint32_t)n, d, t);
    for (uint64_t n = range - edge; n < range; ++n)
        if (!exact((uint32_t)n, d, t)) report((uint32_t)n, d, t);
    const uint64_t kmax = range / d;             // quotients whose whole run [k d, k d + d) lies in the range
    if (nk_seeded == 0u) {
        for (uint64_t k = 0; k < kmax; ++k) {
            const uint32_t lo = (uint32_t)(k * d), hi = lo + d - 1u;
            if (vct_tilediv(lo, d, t.mul, t.shift) != k) report(lo, d, t);
            if (vct_tilediv(hi, d, t.mul, t.shift) != k) report(hi, d, t);
        }
    } else {
        for (uint32_t i = 0; i < nk_seeded && kmax > 0; ++i) {
            const uint64_t k = rng.below(kmax);
            const uint32_t lo = (uint32_t)(k * d), hi = lo + d - 1u;
            if (vct_tilediv(lo, d, t.mul, t.shift) != k) report(lo, d, t);
            if (vct_tilediv(hi, d, t.mul, t.shift) != k) report(hi, d, t);
        }
    }
    for (uint32_t i = 0; i < nrand; ++i) {
        const uint32_t n = rng.below(range);
        if (!exact(n, d, t)) report(n, d, t);
    }
}

static bool read_floats(const char* path, std::vector<float>& out) {
    FILE* f = fopen(path, "rb");
    if (!f) return false;
    fseek(f, 0, SEEK_END);
    const long bytes = ftell(f);
    fseek(f, 0, SEEK_SET);
    out.resize(bytes > 0 ? (size_t)bytes / sizeof(float) : 0);
    const bool ok = bytes >= 0 && (size_t)bytes % sizeof(float) == 0 && fread(out.data(), sizeof(float), out.size(), f) == out.size();
    fclose(f);
    return ok;
}

static int lights(const char* in_path, const char* out_path) {
    std::vector<float> in;
    if (!read_floats(in_path, in) || in.size() % 3 != 0) return 2;
    std::vector<float> out(in.size());          // exactly sized: a write past it is an ASan report
    for (size_t i = 0; i < in.size() / 3; ++i) vct_light_unit(&in[3 * i], &out[3 * i]);
    FILE* f = fopen(out_path, "wb");
    if (!f) return 2;
    const bool ok = fwrite(out.data(), sizeof(float), out.size(), f) == out.size();
    return fclose(f) == 0 && ok ? 0 : 2;
}

int main(int argc, char** argv) {
    if (argc == 3) return lights(argv[1], argv[2]);
    // not certified: the plain division behind mul == 0
    for (uint32_t d : {0u, 1u, VCT_TILEDIV_MAX_D + 1u, 0x7fffffffu, 0xffffffffu}) {
        const VctTileDiv t = vct_tilediv_make(d);
        EXPECT(t.mul == 0u && t.shift == 0u);
    }
    for (uint32_t n : {0u, 1u, 63u, 0x7fffffffu}) EXPECT(vct_tilediv(n, 1u, 0u, 0u) == n);
    EXPECT(vct_tilediv(1000u, 7u, 0u, 0u) == 142u);
    EXPECT((uint64_t)VCT_TILEDIV_MAX_D * 8u >= 0x7fffffffull && (uint64_t)(VCT_TILEDIV_MAX_D - 1u) * 8u < 0x7fffffffull);
    // part A (below), part B
    unsigned long long checked = 0;
    Rng rng(0);
    std::vector<uint32_t> big = {VCT_TILEDIV_MAX_D, VCT_TILEDIV_MAX_D - 1u, 2049u, 2050u, 240u * 17u + 1u};
    for (uint32_t l = 11; l <= 28; ++l)
        for (uint32_t d : {(1u << l) - 1u, 1u << l, (1u << l) + 1u})
            if (d > 2048u && d <= VCT_TILEDIV_MAX_D) big.push_back(d);
    for (int i = 0; i < 2000; ++i) big.push_back(2049u + rng.below(VCT_TILEDIV_MAX_D - 2048u));
    for (int i = 0; i < 2000; ++i) big.push_back(2049u + rng.below(1u << (12 + i % 16)));      // every magnitude
    for (uint32_t& d : big)
        if (d > VCT_TILEDIV_MAX_D) d = VCT_TILEDIV_MAX_D;
    unsigned nthreads = std::thread::hardware_concurrency();
    nthreads = nthreads < 1u ? 1u : (nthreads > 8u ? 8u : nthreads);
    std::vector<std::thread> pool;
    for (unsigned w = 0; w < nthreads; ++w)
        pool.emplace_back([&, w] {
            for (uint32_t d = 1u + w; d <= 2048u; d += nthreads) check_divisor(d, (uint64_t)d * 2048u, 4ull * d, 0u, 1000000u);
            for (size_t i = w; i < big.size(); i += nthreads) check_divisor(big[i], VCT_TILEDIV_MAX_N, 4096u, 10000u, 20000u);
        });
    for (std::thread& th : pool) th.join();
    for (uint32_t d = 1; d <= 2048u; ++d) checked += 8ull * d + 2ull * 2048u + 1000000u;
    checked += big.size() * (2ull * 4096u + 20000u + 20000u);
    if (failures) { printf("%d failures\n", failures.load()); return 1; }
    printf("tilediv_check ok (%llu quotients)\n", checked);
    return 0;
}
