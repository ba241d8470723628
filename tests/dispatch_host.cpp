// Stand-alone check of csrc/dispatch.h (host C++17, no HIP): tests/test_dispatch_host.py builds and runs it.
#include <cstdio>

#include "dispatch.h"

using namespace hgm;

using Groups = Ints<64, 32, 16, 8, 4>;
using Strict = Ints<3, 5, 7>;   // used without a fallback

static int fails = 0;
#define CHECK(cond)                                                   \
    do {                                                              \
        if (!(cond)) {                                                \
            std::printf("line %d: %s\n", __LINE__, #cond);            \
            ++fails;                                                  \
        }                                                             \
    } while (0)

template <int N>
struct Tag {
    static constexpr int value = N;
};

int main() {
    const int groups[] = {64, 32, 16, 8, 4};
    for (int x = -70; x <= 130; ++x) {
        bool in = false;
        for (int g : groups) in = in || g == x;
        CHECK(Groups::has(x) == in);
        CHECK(Strict::has(x) == (x == 3 || x == 5 || x == 7));
        CHECK(Flag::has(x) == (x == 0 || x == 1));
    }
    static_assert(Groups::has(16) && !Groups::has(2), "has() is a constant expression");

    long calls = 0, walked = 0;
    for (int g = -1; g <= 130; ++g)
        for (int b = 0; b <= 1; ++b)
            for (int v = 0; v <= 9; ++v) {
                int seen = 0, gc = -1, bc = -1, vc = -1;
                const bool ok = dispatch(
                    [&](auto gg, auto bb, auto vv) {
                        // the constants are usable as template arguments
                        constexpr int G = gg, B = bb;
                        gc = Tag<G>::value;
                        bc = Tag<B>::value;
                        vc = Tag<decltype(vv)::value>::value;
                        ++seen;
                    },
                    Groups{g}, flag(b != 0), Strict{v, false});
                const bool legal = v == 3 || v == 5 || v == 7;
                CHECK(ok == legal);
                CHECK(seen == (legal ? 1 : 0));
                if (legal) {
                    CHECK(gc == (Groups::has(g) ? g : 4));   // outside the list: the last entry
                    CHECK(bc == b);
                    CHECK(vc == v);
                }
                calls += seen;
                ++walked;
            }
    CHECK(calls == walked * 3 / 10);

    // the fallback is the LAST entry, not the smallest; an unmatched selector stops the later ones
    int got = 0;
    CHECK((dispatch([&](auto g) { got = g; }, Ints<64, 32, 16, 8, 2, 4>{3})) && got == 4);
    CHECK((dispatch([&](auto g) { got = g; }, Ints<64, 32, 16, 8, 2, 4>{2})) && got == 2);
    int later = 0;
    CHECK(!dispatch([&](auto, auto) { ++later; }, Strict{4, false}, Groups{8}));
    CHECK(!dispatch([&](auto, auto) { ++later; }, Groups{8}, Strict{4, false}));
    CHECK(later == 0);
    int none = 0;
    CHECK(dispatch([&] { ++none; }) && none == 1);

    if (fails) return 1;
    std::printf("dispatch ok: %ld calls over %ld triples\n", calls, walked);
    return 0;
}
