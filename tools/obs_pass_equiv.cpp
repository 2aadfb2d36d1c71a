// Equivalence check of set_problem's observation pass (obs_pass.hpp) against a plain reference loop
// written here: one observation at a time, no SIMD, masks by read-modify-write, duplicates and
// landmarks in two runs found by explicit checks.  For every case and every dispatch level the host
// supports (scalar included): equal return value, and, when that is true, equal bytes of key[],
// m2[], uv32[] and equal *narrowed.  Every array is a heap block of exactly its size, so a build with
// -fsanitize=address,undefined also checks the unaligned loads and the tails against reads and
// writes past the arrays' ends.
//   g++ -O2 -std=c++17 -pthread -I rs-vio_amd/csrc tools/obs_pass_equiv.cpp -o tools/obs_pass_equiv
//   tools/obs_pass_equiv [--levels | --level scalar|avx2|avx512]     (default: every level of the host)
#include <cmath>
#include <cstdio>
#include <limits>
#include <random>
#include <string>

#include "obs_pass.hpp"

namespace {

struct Win {
    int n_lm = 1, n_kf = 1;
    std::vector<int32_t> lm, kf;
    std::vector<uint8_t> cam;
    std::vector<double> uv;
    int n() const { return (int)lm.size(); }
    void add(int l, int k, int c) {
        lm.push_back(l);
        kf.push_back(k);
        cam.push_back((uint8_t)c);
        const int i = n();
        uv.push_back((float)(0.37 * i - 3.0));
        uv.push_back((float)(1.0 / (i + 1)));
    }
    // a run of `len` observations of landmark l: (keyframe, camera) pairs from k0 on, both cameras
    // (cams == 2) or one (cams == 1, camera c1)
    void run(int l, int len, int k0 = 0, int cams = 2, int c1 = 0) {
        for (int j = 0; j < len; ++j) {
            if (cams == 2)
                add(l, (k0 + j / 2) % n_kf, j % 2);
            else
                add(l, (k0 + j) % n_kf, c1);
        }
    }
};

// ---- the reference
bool ref_pass(int n_obs, const int32_t* lm, const int32_t* kf, const uint8_t* cam, const double* uv, int n_lm,
              int n_kf, unsigned* key, unsigned long long* m2, float* uv32, bool* narrowed) {
    if (n_lm <= 0 || n_kf <= 0) return false;
    bool exact = uv32 != nullptr;
    if (uv32)
        for (size_t i = 0; i < 2 * (size_t)n_obs; ++i) {
            uv32[i] = (float)uv[i];
            if (!((double)uv32[i] == uv[i])) exact = false;  // (a NaN is not exact)
        }
    *narrowed = exact;
    for (int l = 0; l < n_lm; ++l) m2[l] = 0;
    std::vector<char> closed(n_lm, 0);  // the landmark's run has ended
    for (int i = 0; i < n_obs; ++i) {
        const int l = lm[i], k = kf[i], c = cam[i];
        if (l < 0 || l >= n_lm || k < 0 || k >= n_kf || c > 1) return false;
        if (i > 0 && lm[i - 1] != l) closed[lm[i - 1]] = 1;
        if (closed[l]) return false;  // a landmark in two runs
        const unsigned long long bit = 1ull << (2 * k + c);
        if (m2[l] & bit) return false;  // a duplicate
        m2[l] = m2[l] | bit;
        key[i] = (unsigned)l << 6 | (unsigned)k << 1 | (unsigned)c;
    }
    return true;
}

long long g_cases = 0, g_true = 0, g_fail = 0;

void check(const Win& w, const char* what, bool with_uv32 = true) {
    const int n = w.n();
    // exact-size copies of the inputs (the sanitizer build's red zones sit right behind them)
    std::vector<int32_t> lm(w.lm), kf(w.kf);
    std::vector<uint8_t> cam(w.cam);
    std::vector<double> uv(w.uv);
    lm.shrink_to_fit(); kf.shrink_to_fit(); cam.shrink_to_fit(); uv.shrink_to_fit();
    std::vector<unsigned> k1(n, 0xabababab), k2(n, 0xabababab);
    std::vector<unsigned long long> m1(w.n_lm, 0x5555aaaa5555aaaaull), m2(w.n_lm, 0x5555aaaa5555aaaaull);
    std::vector<float> u1(2 * (size_t)n, -77.f), u2(2 * (size_t)n, -77.f);
    bool n1 = false, n2 = false;
    const bool r1 = ref_pass(n, lm.data(), kf.data(), cam.data(), uv.data(), w.n_lm, w.n_kf, k1.data(), m1.data(),
                             with_uv32 ? u1.data() : nullptr, &n1);
    const bool r2 = rsvio_obs::observation_pass(n, lm.data(), kf.data(), cam.data(), uv.data(), w.n_lm, w.n_kf,
                                                k2.data(), m2.data(), with_uv32 ? u2.data() : nullptr, &n2);
    ++g_cases;
    g_true += r1;
    bool ok = r1 == r2;
    if (ok && r1) {
        ok = n1 == n2 && (n == 0 || std::memcmp(k1.data(), k2.data(), sizeof(unsigned) * n) == 0) &&
             std::memcmp(m1.data(), m2.data(), sizeof(unsigned long long) * w.n_lm) == 0 &&
             (n == 0 || std::memcmp(u1.data(), u2.data(), sizeof(float) * 2 * n) == 0);
    }
    if (!ok) {
        if (++g_fail <= 20)
            fprintf(stderr, "MISMATCH %s: n_obs %d n_lm %d n_kf %d: reference %d (narrowed %d), pass %d (narrowed %d)\n",
                    what, n, w.n_lm, w.n_kf, (int)r1, (int)n1, (int)r2, (int)n2);
    }
}

// a window of mixed run lengths with gaps in the landmark ids: 37 observations (4 groups of 8 and a
// tail of 5), 9 runs
Win mixed() {
    Win w;
    w.n_lm = 14;
    w.n_kf = 7;
    const int len[] = {3, 8, 1, 5, 2, 9, 4, 1, 4};
    const int id[] = {0, 2, 3, 5, 6, 8, 9, 12, 13};
    for (int r = 0; r < 9; ++r) w.run(id[r], len[r], r);
    return w;
}

void sizes_and_shapes() {
    const int sizes[] = {0, 1, 3, 4, 5, 7, 8, 9, 15, 16, 17};
    for (int n : sizes) {
        {  // one run (n_kf 32: up to 64 observations per landmark)
            Win w;
            w.n_lm = 3;
            w.n_kf = 32;
            w.run(1, n);
            check(w, "one run");
            check(w, "one run, no uv32", false);
        }
        for (int len = 1; len <= 3; ++len) {  // runs of 1, 2, 3
            Win w;
            w.n_lm = n + 2;
            w.n_kf = 5;
            for (int l = 0; w.n() < n; ++l) w.run(l, std::min(len, n - w.n()), l);
            check(w, "short runs");
        }
    }
    for (int len = 1; len <= 13; ++len)  // runs of every length 1-13, at every offset against the groups
        for (int lead = 0; lead < 8; ++lead) {
            Win w;
            w.n_lm = 12;
            w.n_kf = 8;
            if (lead) w.run(0, lead);
            for (int l = 1; l <= 9; ++l) w.run(l, len, l);
            check(w, "runs of one length");
        }
    check(mixed(), "mixed run lengths, landmarks with no observation");
    for (int c1 = 0; c1 < 2; ++c1) {  // one camera only
        Win w;
        w.n_lm = 9;
        w.n_kf = 11;
        for (int l = 0; l < 9; ++l) w.run(l, 1 + (l * 5) % 11, l, 1, c1);
        check(w, "one camera");
    }
    {  // n_kf 32: bit 63
        Win w;
        w.n_lm = 4;
        w.n_kf = 32;
        w.run(0, 64);
        w.add(1, 31, 1);
        w.run(3, 9, 27);
        check(w, "n_kf 32");
    }
    for (int n = 0; n <= 20; ++n) {  // n_lm 1
        Win w;
        w.n_lm = 1;
        w.n_kf = 10;
        w.run(0, n);
        check(w, "n_lm 1");
    }
    {  // n_lm or n_kf not positive
        Win w = mixed();
        w.n_lm = 0;
        check(w, "n_lm 0");
        w = mixed();
        w.n_kf = 0;
        check(w, "n_kf 0");
    }
}

void random_windows() {
    std::mt19937 rng(20240611);
    for (int t = 0; t < 1000; ++t) {
        Win w;
        w.n_kf = 1 + (int)(rng() % 32);
        const int target = (int)(rng() % 601);
        const int max_len = 1 + (int)(rng() % std::min(2 * w.n_kf, 13 + (int)(rng() % 52)));
        int l = 0;
        std::vector<int> pairs(2 * w.n_kf);
        while (w.n() < target) {
            l += rng() % 4 == 0 ? 1 + (int)(rng() % 3) : 0;  // landmarks with no observation
            const int len = std::min(1 + (int)(rng() % max_len), target - w.n());
            for (int j = 0; j < 2 * w.n_kf; ++j) pairs[j] = j;  // `len` distinct (keyframe, camera) pairs
            std::shuffle(pairs.begin(), pairs.end(), rng);
            for (int j = 0; j < len; ++j) w.add(l, pairs[j] >> 1, pairs[j] & 1);
            ++l;
        }
        w.n_lm = l + (int)(rng() % 3) + (l == 0);
        check(w, "random window");
    }
}

void rejects() {
    const Win base = mixed();
    const int n = base.n();
    for (int pos = 0; pos < n; ++pos) {  // every lane of every group, and the tail
        Win w = base;
        w.lm[pos] = w.n_lm;
        check(w, "obs_lm == n_lm");
        w = base;
        w.lm[pos] = -1;
        check(w, "obs_lm == -1");
        w = base;
        w.kf[pos] = w.n_kf;
        check(w, "obs_kf == n_kf");
        w = base;
        w.cam[pos] = 2;
        check(w, "obs_cam == 2");
    }
    // a duplicate: every pair of positions inside one run -- inside a group, across a group boundary
    // and into the tail; one long run as well, so that both observations can be groups apart
    Win lng;
    lng.n_lm = 3;
    lng.n_kf = 20;
    lng.run(0, 2);
    lng.run(1, 33, 1);
    lng.run(2, 2);
    const Win* const both[] = {&base, &lng};
    for (const Win* b : both)
        for (int i = 0; i < b->n(); ++i)
            for (int j = i + 1; j < b->n() && b->lm[j] == b->lm[i]; ++j) {
                Win w = *b;
                w.kf[j] = w.kf[i];
                w.cam[j] = w.cam[i];
                check(w, "duplicate");
            }
    // a landmark in two runs: the observation at `pos` (and the `len` from it) given to the
    // landmark of the run before, of the run after (adjacent runs), of the first and of the last
    // run (distant runs).  Where that only moves a run's end it is one run again, and the reference
    // says whether the list is then valid.
    std::vector<int> ids;
    for (int i = 0; i < n; ++i)
        if (ids.empty() || ids.back() != base.lm[i]) ids.push_back(base.lm[i]);
    for (int pos = 0; pos < n; ++pos)
        for (int len = 1; len <= 3 && pos + len <= n; ++len) {
            int r = 0;
            for (int i = 1; i <= pos; ++i) r += base.lm[i] != base.lm[i - 1];
            const int from[] = {r > 0 ? ids[r - 1] : -1, r + 1 < (int)ids.size() ? ids[r + 1] : -1,
                                r + 2 < (int)ids.size() ? ids[r + 2] : -1, r > 1 ? ids[r - 2] : -1, ids.front(),
                                ids.back()};
            for (int l : from) {
                if (l < 0) continue;
                Win w = base;
                for (int j = 0; j < len; ++j) {
                    w.lm[pos + j] = l;
                    w.kf[pos + j] = (w.kf[pos + j] + 3) % w.n_kf;  // (mostly no duplicate: the run check alone)
                }
                check(w, "landmark in two runs");
                w = base;
                for (int j = 0; j < len; ++j) w.lm[pos + j] = l;
                check(w, "landmark in two runs (same keyframes)");
            }
        }
    // A B A, the second run of A a whole run
    for (int len = 1; len <= 9; ++len) {
        Win w;
        w.n_lm = 4;
        w.n_kf = 16;
        w.run(1, len, 0);
        w.run(2, 3, 0);
        w.run(1, len, 8);
        w.run(3, 2, 0);
        check(w, "A B A");
    }
}

void uv_cases() {
    const Win base = mixed();
    for (size_t pos = 0; pos < base.uv.size(); ++pos) {
        Win w = base;
        w.uv[pos] = 0.1;  // not an f32
        check(w, "(u, v) not an f32");
        w = base;
        w.uv[pos] = std::numeric_limits<double>::quiet_NaN();
        check(w, "(u, v) NaN");
        w = base;
        w.uv[pos] = 1e300;  // beyond f32: infinity after narrowing
        check(w, "(u, v) beyond f32");
    }
    Win w = base;
    w.uv[5] = -0.0;
    w.uv[6] = std::numeric_limits<double>::infinity();
    check(w, "(u, v) -0 and inf");
}

}  // namespace

int main(int argc, char** argv) {
    static const char* names[] = {"scalar", "avx2", "avx512"};
    const int top = rsvio_obs::simd_host_level();
    int only = -1;
    for (int i = 1; i < argc; ++i) {
        const std::string a = argv[i];
        if (a == "--levels") {
            for (int lv = 0; lv <= top; ++lv) printf("%s\n", names[lv]);
            return 0;
        }
        if (a == "--level" && i + 1 < argc) {
            const std::string v = argv[++i];
            for (int lv = 0; lv < 3; ++lv)
                if (v == names[lv]) only = lv;
            if (only < 0 || only > top) {
                fprintf(stderr, "level %s is unknown or not supported by this host\n", v.c_str());
                return 2;
            }
        }
    }
    for (int lv = 0; lv <= top; ++lv) {
        if (only >= 0 && lv != only) continue;
        rsvio_obs::simd_level() = lv;
        g_cases = g_true = g_fail = 0;
        sizes_and_shapes();
        random_windows();
        rejects();
        uv_cases();
        printf("level %s: %lld cases (%lld accepted, %lld rejected), %lld mismatches\n", names[lv], g_cases, g_true,
               g_cases - g_true, g_fail);
        if (g_fail) return 1;
    }
    return 0;
}
