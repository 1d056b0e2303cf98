// stripes_check.cpp -- sirius_amd/csrc/stripes.h against a brute-force owner map (TEST INFRASTRUCTURE ONLY).
//
// A stand-alone host program, built with g++ -fsanitize=address,undefined by tests/test_stripes_host.py.  For worlds 1..9 and every rank:
//   a stripe of 4 elements, every 0 <= a <= b <= 80, every element of every run looked at;
//   the product's stripe (2^STRIPE_LOG), a and b at and around the stripe boundaries 0..20, every piece looked at at both ends.
// Checked: owns, count(n), count(a, b), global_index, and for runs(a, b): at most three runs, ascending and disjoint, inside [a, b), every
// piece inside one owned stripe, as many elements as the map says (so: every owned element once, nothing else), local offsets contiguous
// from count(a), global_index(local + e) == global + e; each_piece walks the same pieces.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "stripes.h"

using srs::Run;

#define CHECK(cond)                                                                                                              \
    do {                                                                                                                         \
        if (!(cond)) {                                                                                                           \
            std::printf("FAILED %s  (line %d: log %u world %u rank %u a %zu b %zu)\n", #cond, __LINE__, LOG, world, rank, a, b); \
            std::exit(1);                                                                                                        \
        }                                                                                                                        \
    } while (0)

template <uint32_t LOG>
static size_t check(const std::vector<size_t> &points, bool every_element) {
    const size_t S = (size_t)1 << LOG, top = points.back();
    size_t cases = 0;
    for (uint32_t world = 1; world <= 9; ++world) {
        for (uint32_t rank = 0; rank < world; ++rank) {
            const srs::StripesT<LOG> sp{rank, world};
            size_t a = 0, b = 0;
            // the brute-force map: before[i] = owned elements below i, mine = their global indices in order
            std::vector<size_t> before(top + 2, 0), mine;
            for (size_t i = 0; i <= top; ++i) {
                const bool own = (i / S) % world == rank;
                CHECK(sp.owns(i) == own);
                before[i + 1] = before[i] + (own ? 1 : 0);
                if (own) mine.push_back(i);
            }
            for (size_t n : points) CHECK(sp.count(n) == before[n]);
            for (size_t l = 0; l < mine.size(); l += (every_element ? 1 : S - 1)) {
                CHECK(sp.global_index(l) == mine[l]);
                CHECK(sp.global_index((uint32_t)l) == (uint32_t)mine[l]);
            }
            for (size_t ia = 0; ia < points.size(); ++ia) {
                for (size_t ib = ia; ib < points.size(); ++ib) {
                    a = points[ia];
                    b = points[ib];
                    ++cases;
                    CHECK(sp.count(a, b) == before[b] - before[a]);
                    Run run[3];
                    const int nr = sp.runs(a, b, run);
                    CHECK(nr >= 0 && nr <= 3);
                    size_t local = sp.count(a), end = a, total = 0;      // next local offset, end of the previous piece
                    std::vector<Run> pieces;
                    for (int i = 0; i < nr; ++i) {
                        const Run &r = run[i];
                        CHECK(r.width >= 1 && r.rows >= 1 && (r.rows == 1 || r.width == S));
                        CHECK(world > 1 || (nr == 1 && r.global == a && r.local == a && r.width == b - a && r.rows == 1));
                        for (size_t p = 0; p < r.rows; ++p) {
                            const size_t g = r.global + p * world * S, l = r.local + p * S;
                            CHECK(g >= end && g + r.width <= b);                           // ascending, disjoint, inside [a, b)
                            CHECK(l == local);                                             // contiguous from count(a)
                            CHECK(world == 1 || g / S == (g + r.width - 1) / S);           // one stripe,
                            CHECK(sp.owns(g) && before[g + 1] == before[g] + 1);           //   an owned one
                            for (size_t e = 0; e < r.width; e += (every_element || e + 1 == r.width ? 1 : r.width - 1 - e))
                                CHECK(sp.global_index(l + e) == g + e);
                            pieces.push_back(Run{g, l, r.width, 1});
                            end = g + r.width;
                            local += r.width;
                            total += r.width;
                        }
                    }
                    CHECK(total == before[b] - before[a]);                                 // every owned element once, nothing else
                    size_t at = 0;
                    sp.each_piece(a, b, [&](size_t g, size_t l, size_t w) {
                        CHECK(at < pieces.size() && pieces[at].global == g && pieces[at].local == l && pieces[at].width == w);
                        ++at;
                    });
                    CHECK(at == pieces.size());
                }
            }
        }
    }
    return cases;
}

int main() {
    std::vector<size_t> tiny, real;
    for (size_t i = 0; i <= 80; ++i) tiny.push_back(i);
    const size_t S = (size_t)1 << srs::STRIPE_LOG;
    for (size_t s = 0; s <= 20; ++s)
        for (size_t d : {S - 1, S, S + 1, S + S / 2 - 1})        // s * S - 1, s * S, s * S + 1, s * S + 511
            if (s * S + d >= S) real.push_back(s * S + d - S);
    const size_t n_tiny = check<2>(tiny, true), n_real = check<srs::STRIPE_LOG>(real, false);
    static_assert(sizeof(srs::Stripes) == 8 && srs::Stripes::S == 1024, "the product's instantiation");
    std::printf("ok tiny=%zu real=%zu\n", n_tiny, n_real);
    return 0;
}
