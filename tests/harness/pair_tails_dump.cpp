// pair_tails_dump.cpp -- test harness (tests/test_pair_tails_host.py): reads one molecule's directed edge list from stdin ("A E"
// then E lines "src dst type"), builds the packed pair template (csrc/pair_template.hpp) and prints
//   "ok G nblk n_tile seeded r S" | "none", then nblk*16 row words, then G*A*A pair_pos entries, then the merged-tail row map of
//   pair_template_tails as 16 triples "group block row" (nothing when r == 0).
// argv[1] (optional, >= 0): that row of the LAST general block has its valid bit cleared before pair_template_tails runs.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../thermodynamic-interpolation_amd/csrc/pair_template.hpp"

int main(int argc, char** argv)
{
    int A, E;
    if (std::scanf("%d %d", &A, &E) != 2) return 2;
    std::vector<int32_t> s(E), d(E), t(E);
    for (int k = 0; k < E; ++k) if (std::scanf("%d %d %d", &s[k], &d[k], &t[k]) != 3) return 2;
    ti::PairTemplate pt;
    if (!ti::build_pair_template_packed(A, E, s.data(), d.data(), t.data(), pt, /*first_touch=*/true)) { std::printf("none\n"); return 0; }
    const long drop = argc > 1 ? std::atol(argv[1]) : -1;
    if (drop >= 16) return 2;
    if (drop >= 0) pt.rows[(size_t)(pt.nblk - 1) * 16 + (size_t)drop] &= ~1u;
    const ti::PairTails tails = ti::pair_template_tails(pt, A);
    std::printf("ok %d %d %d %d %d %d\n", pt.G, pt.nblk, pt.n_tile, pt.seeded ? 1 : 0, tails.r, tails.S);
    for (uint32_t w : pt.rows) std::printf("%u ", w);
    std::printf("\n");
    for (int v : pt.pair_pos) std::printf("%d ", v);
    std::printf("\n");
    for (const auto& m : tails.map) std::printf("%d %d %d ", m[0], m[1], m[2]);
    std::printf("\n");
    return 0;
}
