// pair_template_seeded_dump.cpp -- test harness (tests/test_pair_template_seeded.py): reads one molecule's directed edge list from
// stdin ("A E" then E lines "src dst type"), runs the product's pair-template builder (csrc/pair_template.hpp; argv[1] = "packed":
// build_pair_template_packed, "tile": build_pair_template) and prints
//   "ok G nblk n_tile seeded rechecked" | "none", then nblk*16 row words.
// seeded: what the builder stored in the template.  rechecked: pair_template_seeded() on the template after argv[2] (optional, >= 0)
// has cleared the valid bit of that general row (counted from the first general row) -- a template that lost a general pair.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../thermodynamic-interpolation_amd/csrc/pair_template.hpp"

int main(int argc, char** argv)
{
    int A, E;
    if (argc < 2 || std::scanf("%d %d", &A, &E) != 2) return 2;
    std::vector<int32_t> s(E), d(E), t(E);
    for (int k = 0; k < E; ++k) if (std::scanf("%d %d %d", &s[k], &d[k], &t[k]) != 3) return 2;
    ti::PairTemplate pt;
    const bool packed = std::strcmp(argv[1], "packed") == 0;
    const bool ok = packed ? ti::build_pair_template_packed(A, E, s.data(), d.data(), t.data(), pt, /*first_touch=*/true)
                           : ti::build_pair_template(A, E, s.data(), d.data(), t.data(), pt, /*first_touch=*/true);
    if (!ok) { std::printf("none\n"); return 0; }
    const int seeded = pt.seeded ? 1 : 0;
    const long drop = argc > 2 ? std::atol(argv[2]) : -1;
    if (drop >= 0) {
        const size_t r = (size_t)pt.n_tile * 16 + (size_t)drop;
        if (r >= pt.rows.size()) return 2;
        pt.rows[r] &= ~1u;
    }
    std::printf("ok %d %d %d %d %d\n", pt.G, pt.nblk, pt.n_tile, seeded, ti::pair_template_seeded(pt, A) ? 1 : 0);
    for (uint32_t w : pt.rows) std::printf("%u ", w);
    std::printf("\n");
    return 0;
}
