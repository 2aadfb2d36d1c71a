// ba_envelope.hpp -- the symbolic envelope of the BA's reduced camera system (host code, no
// device code), computed by rsvio_ba_set_problem from the landmarks' (keyframe, camera) masks.
//
// Past 10 free keyframes the 6x6-block LDL^T (bk_update) skips the tiles outside the envelope and
// the Schur chunks outside it write zeros (schur_chunks_body).  A landmark couples every pair of
// free keyframes that see it; taking all free keyframes between its first and its last one is a
// superset of its pairs.  cand[a] = the last free keyframe of the landmarks whose first one is a;
// env[k] = max(k, max_{a <= k} cand[a]): block elimination in column order fills column k at most
// down to the largest last row of the columns before it (LDL^T keeps the envelope), so the prefix
// maximum bounds both S and its factor.  Up to 10 free keyframes the envelope is off and dense.
#pragma once

#include <algorithm>

namespace rsvio_env {

constexpr int kMaxFree = 20;  // free keyframes of the largest camera system (ba.hip's kMaxFree)

// m2 of a landmark: bit 2 k + c = keyframe k seen by camera c (obs_pass.hpp's masks).
struct Envelope {
    const int* free_idx;  // keyframe -> free block or -1
    int n_free;
    bool on;
    unsigned long long freebits = 0;  // bit 2 k: keyframe k is free
    int cand[kMaxFree];

    Envelope(const int* free_idx_, int n_kf, int n_free_) : free_idx(free_idx_), n_free(n_free_), on(n_free_ > 10) {
        for (int k = 0; k < n_kf; ++k)
            if (free_idx[k] >= 0) freebits |= 1ull << (2 * k);
        for (int k = 0; k < kMaxFree; ++k) cand[k] = -1;
    }

    // one landmark's mask (a landmark seen by no free keyframe adds nothing)
    void add(unsigned long long m2) {
        if (!on) return;
        const unsigned long long kb = (m2 | (m2 >> 1)) & freebits;  // either camera -> the keyframe's bit
        if (kb) {
            const int a = free_idx[__builtin_ctzll(kb) >> 1], b = free_idx[(63 - __builtin_clzll(kb)) >> 1];
            cand[a] = std::max(cand[a], b);
        }
    }

    // env[kMaxFree]: the envelope (k itself past n_free: the padded template's identity blocks)
    void finish(unsigned char* env, int* env_on) const {
        for (int k = 0, run = -1; k < kMaxFree; ++k) {
            run = std::max(run, cand[k]);
            env[k] = (unsigned char)(k >= n_free ? k : on ? std::max(k, run) : n_free - 1);
        }
        *env_on = on ? 1 : 0;
    }
};

static inline void camera_envelope(int n_lm, const unsigned long long* m2, const int* free_idx, int n_kf, int n_free,
                                   unsigned char* env, int* env_on) {
    Envelope E(free_idx, n_kf, n_free);
    for (int l = 0; l < n_lm; ++l) E.add(m2[l]);
    E.finish(env, env_on);
}

// The envelope a sharded solve factors with: the all-reduced system holds every rank's landmarks,
// this rank's envelope only its own, so the factorisation takes the dense one.
static inline void dense_envelope(int n_free, unsigned char* env) {
    for (int k = 0; k < kMaxFree; ++k) env[k] = (unsigned char)(k >= n_free ? k : n_free - 1);
}

}  // namespace rsvio_env
