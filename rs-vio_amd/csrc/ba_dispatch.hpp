// ba_dispatch.hpp -- host: the one map from a window's free-keyframe count to the camera-solve
// templates' NF.  Every K5 kernel (VALU, panel, block, x2, descriptor mode, covariance) is a
// template over NF; a launch site hands its launch as a generic lambda and gets the template
// constant back.  No HIP here: a host compiler takes this header alone
// (tests/test_ba_dispatch_cpu.py).
#pragma once

#include <type_traits>
#include <utility>  // std::integer_sequence

namespace rsvio {

template <class F>
bool dispatch_nf(std::integer_sequence<int>, int, F&&) {
    return false;
}
// first match of the list, head first: the kernels are then instantiated -- and laid out in the
// code object -- in the list's order, as a switch with one case per NF would
template <int N0, int... NF, class F>
bool dispatch_nf(std::integer_sequence<int, N0, NF...>, int nf, F&& f) {
    if (nf == N0) {
        f(std::integral_constant<int, N0>{});
        return true;
    }
    return dispatch_nf(std::integer_sequence<int, NF...>{}, nf, f);
}

// f(std::integral_constant<int, NF>{}) for the template that serves nf; false when none does
// 1..10 free keyframes: one instantiation each (one row per lane)
template <class F>
bool dispatch_panel_nf(int nf, F&& f) {
    return dispatch_nf(std::integer_sequence<int, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10>{}, nf, f);
}

// 11..20 free keyframes pad up to 13, 16 or 20: callers pass bk_template_nf(n_free)
template <class F>
bool dispatch_block_nf(int nf, F&& f) {
    return dispatch_nf(std::integer_sequence<int, 13, 16, 20>{}, nf, f);
}

}  // namespace rsvio
