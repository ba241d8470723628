// Run-time choice of a template instantiation (host only, C++17).  A kernel here is a template over
// a few small integers (lanes per row, vector width, epilogue, flags); the host holds them as ints.
//   dispatch([&](auto g, auto epi) { launch(..., k<T, g, epi>, ...); }, RowGroups{M->group}, RowEpis{epi});
// calls the lambda once with one std::integral_constant per selector; the lists name the legal values.
#pragma once

#include <type_traits>

namespace hgm {

// A run-time int to be matched against Vs.  Outside the list it takes the LAST entry (a ladder's
// default: arm) or, with fallback = false, nothing is called.
template <int... Vs>
struct Ints {
    int v;
    bool fallback = true;
    static constexpr bool has(int x) { return ((x == Vs) || ...); }
    // f(std::integral_constant<int, V>{}) for the V that v selects; false when there is none
    template <typename F>
    bool pick(F&& f) const {
        constexpr int vs[] = {Vs...};
        if (!has(v) && !fallback) return false;
        const int w = has(v) ? v : vs[sizeof...(Vs) - 1];
        return ((w == Vs && (f(std::integral_constant<int, Vs>{}), true)) || ...);
    }
};
using Flag = Ints<1, 0>;
inline Flag flag(bool b) { return Flag{b ? 1 : 0}; }

// f(c1, c2, ...) with one constant per selector, in order; false (and no call) when a selector
// without a fallback did not match.  The call itself is not inlined: one small function per
// instantiation, as a ladder of launcher templates had (a 240-arm ladder inlined into one body
// takes the optimiser three times as long).
template <typename F>
[[gnu::noinline]] bool dispatch(F&& f) {
    f();
    return true;
}
template <typename F, typename S, typename... Rest>
bool dispatch(F&& f, S s, Rest... rest) {
    bool called = false;
    s.pick([&](auto c) { called = dispatch([&](auto... cs) { f(c, cs...); }, rest...); });
    return called;
}

}  // namespace hgm
