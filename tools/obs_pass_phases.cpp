// Times the sub-passes of set_problem's observation pass (obs_pass.hpp) one by one on the host it runs
// on: uv_narrow, obs_keys, the run masks (memset + masks_of_runs), mask_bits, the whole
// observation_pass and, where the header has it, the fused key + mask sweep at every dispatch level
// the host supports.  Shapes: config 3 (2,000 landmarks x 12 observations) and config 5 (5,000 x 16),
// landmark-major, (u, v) exact f32 values.  Median and best of `reps` repetitions, in us.
// It compiles against any revision of the header, so one source gives the before and the after:
//   g++ -O2 -std=c++17 -pthread -I rs-vio_amd/csrc tools/obs_pass_phases.cpp -o tools/obs_pass_phases
//   tools/obs_pass_phases [reps]
#include <chrono>
#include <cstdio>
#include <random>

#include "obs_pass.hpp"

namespace {

struct Window {
    int n_lm, n_kf, n_obs;
    std::vector<int32_t> lm, kf;
    std::vector<uint8_t> cam;
    std::vector<double> uv;
    std::vector<unsigned> key;
    std::vector<unsigned long long> m2;
    std::vector<float> uv32;
};

Window make(int n_lm, int kf_per_lm, int n_kf) {
    Window w;
    w.n_lm = n_lm;
    w.n_kf = n_kf;
    w.n_obs = n_lm * kf_per_lm * 2;
    std::mt19937 rng(7);
    for (int l = 0; l < n_lm; ++l)
        for (int k = 0; k < kf_per_lm; ++k)
            for (int c = 0; c < 2; ++c) {
                w.lm.push_back(l);
                w.kf.push_back((l + k) % n_kf);
                w.cam.push_back((uint8_t)c);
                w.uv.push_back((float)(rng() * 1e-9));
                w.uv.push_back((float)(rng() * 1e-9));
            }
    w.key.resize(w.n_obs);
    w.m2.resize(n_lm);
    w.uv32.resize(2 * (size_t)w.n_obs);
    return w;
}

template <class F>
void time_it(const char* name, int reps, F&& f) {
    std::vector<double> t(reps);
    for (int r = 0; r < reps; ++r) {
        const auto t0 = std::chrono::steady_clock::now();
        f();
        const auto t1 = std::chrono::steady_clock::now();
        t[r] = std::chrono::duration<double, std::micro>(t1 - t0).count();
    }
    std::sort(t.begin(), t.end());
    printf("  %-34s median %7.2f  best %7.2f\n", name, t[reps / 2], t[0]);
}

volatile long long g_sink;

void phases(Window& w, int reps) {
    using namespace rsvio_obs;
    time_it("uv_narrow", reps, [&] { g_sink = uv_narrow(2 * (size_t)w.n_obs, w.uv.data(), w.uv32.data()); });
    time_it("obs_keys", reps,
            [&] { g_sink = obs_keys(w.n_obs, w.lm.data(), w.kf.data(), w.cam.data(), w.n_lm, w.n_kf, w.key.data()); });
    time_it("masks (memset + masks_of_runs)", reps, [&] {
        std::memset(w.m2.data(), 0, sizeof(unsigned long long) * (size_t)w.n_lm);
        masks_of_runs(0, w.n_obs, w.key.data(), w.m2.data());
    });
    time_it("mask_bits", reps, [&] { g_sink = mask_bits(w.n_lm, w.m2.data()); });
#ifdef RSVIO_OBS_FUSED
    time_it("keys + masks fused (memset + sweep)", reps, [&] {
        std::memset(w.m2.data(), 0, sizeof(unsigned long long) * (size_t)w.n_lm);
        g_sink = keys_masks(0, w.n_obs, w.lm.data(), w.kf.data(), w.cam.data(), w.n_lm, w.n_kf, w.key.data(),
                            w.m2.data());
    });
#endif
    time_it("observation_pass (all of it)", reps, [&] {
        bool narrowed = false;
        g_sink = observation_pass(w.n_obs, w.lm.data(), w.kf.data(), w.cam.data(), w.uv.data(), w.n_lm, w.n_kf,
                                  w.key.data(), w.m2.data(), w.uv32.data(), &narrowed);
    });
}

}  // namespace

int main(int argc, char** argv) {
    const int reps = argc > 1 ? std::max(3, atoi(argv[1])) : 3000;
    Window w3 = make(2000, 6, 10), w5 = make(5000, 8, 12);
#ifdef RSVIO_OBS_FUSED
    static const char* names[] = {"scalar", "avx2", "avx512"};
    const int top = rsvio_obs::simd_host_level();
    for (int lv = 0; lv <= top; ++lv) {
        rsvio_obs::simd_level() = lv;
        printf("dispatch level %s\n", names[lv]);
#else
    {
        printf("header without the fused sweep (dispatch: avx2 where the host has it)\n");
#endif
        printf(" config 3 shape: %d landmarks x 12 = %d observations\n", w3.n_lm, w3.n_obs);
        phases(w3, reps);
        printf(" config 5 shape: %d landmarks x 16 = %d observations\n", w5.n_lm, w5.n_obs);
        phases(w5, reps);
    }
    return 0;
}
