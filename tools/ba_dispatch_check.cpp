// ba_dispatch_check.cpp -- rs-vio_amd/csrc/ba_dispatch.hpp with a host compiler alone:
//   g++ -O2 -std=c++17 -I rs-vio_amd/csrc tools/ba_dispatch_check.cpp -o /tmp/ba_dispatch_check
// Prints, for every nf in 0..24 and both dispatchers, one line
//   <panel|block> <nf> <returned 0|1> <calls of f> <the constant f got, or -1>
// (tests/test_ba_dispatch_cpu.py reads them).
#include <cstdio>

#include "ba_dispatch.hpp"

int main() {
    for (int which = 0; which < 2; ++which)
        for (int nf = 0; nf <= 24; ++nf) {
            int calls = 0, got = -1;
            auto f = [&](auto c) {
                static_assert(std::is_same<decltype(c), std::integral_constant<int, decltype(c)::value>>::value,
                              "the template constant, usable as a template argument");
                ++calls;
                got = decltype(c)::value;
            };
            const bool hit = which ? rsvio::dispatch_block_nf(nf, f) : rsvio::dispatch_panel_nf(nf, f);
            std::printf("%s %d %d %d %d\n", which ? "block" : "panel", nf, hit ? 1 : 0, calls, got);
        }
    return 0;
}
