// pair_template_packed_dump.cpp -- test harness (tests/test_pair_template_packed.py): reads one molecule's directed edge list from
// stdin ("A E" then E lines "src dst type"), runs the product's packed pair-template builder (csrc/pair_template.hpp:
// build_pair_template_packed, with the first-touch marks the product uses whenever every atom has incoming edges) and prints the
// template as plain integers:  "ok G nblk n_tile" | "none", then nblk*16 row words, nblk*16 slot words, G*A*A pair_pos entries.
#include <cstdio>
#include <vector>

#include "../../thermodynamic-interpolation_amd/csrc/pair_template.hpp"

int main()
{
    int A, E;
    if (std::scanf("%d %d", &A, &E) != 2) return 2;
    std::vector<int32_t> s(E), d(E), t(E);
    for (int k = 0; k < E; ++k) if (std::scanf("%d %d %d", &s[k], &d[k], &t[k]) != 3) return 2;
    ti::PairTemplate pt;
    if (!ti::build_pair_template_packed(A, E, s.data(), d.data(), t.data(), pt, /*first_touch=*/true)) { std::printf("none\n"); return 0; }
    std::printf("ok %d %d %d\n", pt.G, pt.nblk, pt.n_tile);
    for (uint32_t w : pt.rows) std::printf("%u ", w);
    std::printf("\n");
    for (int32_t w : pt.slotnode) std::printf("%d ", w);
    std::printf("\n");
    for (int w : pt.pair_pos) std::printf("%d ", w);
    std::printf("\n");
    return 0;
}
