// Prints the camera-system envelopes set_problem computes (ba_envelope.hpp) for visibility patterns
// read from stdin: tests/test_ba_envelope_cpu.py compares them with a numpy symbolic elimination.
//   g++ -O2 -std=c++17 -I rs-vio_amd/csrc tools/ba_envelope_dump.cpp -o /tmp/ba_envelope_dump
// Input:  the number of cases, then per case "n_kf n_lm", n_kf fixed flags (0 / 1) and n_lm masks
//         in hex (bit 2 k + c: keyframe k seen by camera c).
// Output: per case one line "env_on env[0] ... env[kMaxFree - 1]".
#include <cstdio>
#include <vector>

#include "ba_envelope.hpp"

int main() {
    int n_case = 0;
    if (scanf("%d", &n_case) != 1) return 2;
    for (int t = 0; t < n_case; ++t) {
        int n_kf = 0, n_lm = 0;
        if (scanf("%d %d", &n_kf, &n_lm) != 2 || n_kf < 1 || n_kf > 32 || n_lm < 0) return 2;
        std::vector<int> free_idx(n_kf, -1);
        int n_free = 0;
        for (int k = 0; k < n_kf; ++k) {
            int fixed = 0;
            if (scanf("%d", &fixed) != 1) return 2;
            if (!fixed) free_idx[k] = n_free++;
        }
        if (n_free > rsvio_env::kMaxFree) return 2;
        std::vector<unsigned long long> m2(n_lm);
        for (int l = 0; l < n_lm; ++l)
            if (scanf("%llx", &m2[l]) != 1) return 2;
        unsigned char env[rsvio_env::kMaxFree];
        int env_on = -1;
        rsvio_env::camera_envelope(n_lm, m2.data(), free_idx.data(), n_kf, n_free, env, &env_on);
        printf("%d", env_on);
        for (int k = 0; k < rsvio_env::kMaxFree; ++k) printf(" %d", (int)env[k]);
        printf("\n");
    }
    return 0;
}
