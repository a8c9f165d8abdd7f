// pair_template.hpp -- builds the pair-major edge template of the message kernel (painn_pair_kernel.hpp; word formats in
// ti_internal.hpp).  Pure host C++ with no HIP dependency: tests/test_pair_template.py and tests/test_pair_template_packed.py compile
// it with g++ (tests/harness/pair_template_dump.cpp, pair_template_packed_dump.cpp) and check its invariants on complete and sparse
// graphs.
//
// The filter branch w(enc(|r_ij|)) of SE3Message (/root/reference/mdqm9/thermo/ambient/models/cpainn.py:283-289) is shared by the
// edges i -> j and j -> i, so the kernel walks PAIRS.  Every pair of the G molecules of a group must lie in exactly one valid row.
//
// TILE blocks (build_pair_template, and the leading blocks of build_pair_template_packed): a row block is a 4 x 4 tile, row 4a + b =
// pair (I[a], J[b]) of up to four I slots and four J slots (a slot = molecule-in-group, atom).  Construction: atoms are cut into
// tiles of four by index; every tile pair with edges between them is a block; spare slots of those blocks then absorb the pairs
// INSIDE a tile (an atom may sit on both sides of a block), greedily by the number of uncovered pairs an added atom brings; what is
// left ("loose" pairs, of all G molecules) is packed into further blocks, preferring pairs that reuse slots already opened.  A
// complete graph on A atoms needs at least ceil((A - 1) / 4) slot places per atom, i.e. A * ceil((A - 1) / 4) / 8 tile blocks per
// molecule; this construction meets that bound for A = 18 (11.25 blocks per molecule at G = 4: 85 % of the rows are pairs), A = 9
// (3 blocks) and A = 25 (21 blocks).  That bound is a property of the tile, not of the work: an atom with 17 neighbours pays for a
// fifth slot place that holds one pair.
//
// GENERAL blocks (build_pair_template_packed only, after the n_tile tile blocks): 16 unrelated pairs of the group, each named by
// its row word alone; no slots (slot words -1), no first touch -- the kernel adds every row's two contributions to its two atoms
// (painn_pair_kernel_body.inc, GENERAL).  The packed builder dissolves the emptiest tile blocks into general rows while that lowers
// the block count, and never moves a pair unless both its atoms keep a slot in a tile block (that slot's first touch replaces the
// accumulator's stale contents before any general row adds to it).  The complete graph on 18 atoms has a tile stage of its own (nine
// full tiles from a cyclic 4-cycle decomposition of K9, twin_tiles below): 36 full tiles and 3 general blocks per group of 4
// molecules, 9.75 blocks per molecule, the floor ceil(4 * 153 / 16) / 4 of the rows alone.
#pragma once
#include <stdint.h>

#include <algorithm>
#include <array>
#include <stdexcept>
#include <vector>

namespace ti {

struct PairTemplate {
    int G = 0, nblk = 0;                     // molecules per group, row blocks per group
    int n_tile = 0;                          // blocks [0, n_tile) are tiles, [n_tile, nblk) general (build_pair_template_packed; else nblk)
    std::vector<uint32_t> rows;              // [nblk * 16] row words
    std::vector<int32_t> slotnode;           // [nblk * 16] slot words (k = 0..3 I slots, 4..7 J slots, rest unused = -1)
    std::vector<int> pair_pos;               // [(m * A + src) * A + dst] -> (block * 2 + direction) * 16 + pair row, -1 = no such edge
    double fill = 0.0;                       // valid rows / all rows
    bool seeded = false;                     // the general rows name every atom of every molecule of the group exactly once (pair_template_seeded)
};

// SEEDED: the valid rows of the general blocks [n_tile, nblk) name each of the group's G * A atoms exactly once.  A general launch that
// runs BEFORE the tile launch then meets every accumulator row as the atom's first contribution of the layer: it stores, and the tile
// blocks only add (painn_pair_kernel.hpp: the SEEDED builds).  Counted from the row words, never assumed: the twin rows of the complete
// graph on 18 atoms have it (36 pairs = 72 atoms at G = 4); a tile-only template has no general row and never does.
inline bool pair_template_seeded(const PairTemplate& t, int A)
{
    if (t.n_tile >= t.nblk || A <= 0 || A > 32) return false;
    std::vector<int> hits((size_t)t.G * 32, 0);
    for (size_t r = (size_t)t.n_tile * 16; r < (size_t)t.nblk * 16; ++r) {
        const uint32_t w = t.rows[r];
        if (!(w & 1u)) continue;
        const int mI = (w >> 1) & 7, aI = (w >> 4) & 31, mJ = (w >> 9) & 7, aJ = (w >> 12) & 31;
        if (mI >= t.G || mJ >= t.G || aI >= A || aJ >= A) return false;
        ++hits[(size_t)mI * 32 + aI]; ++hits[(size_t)mJ * 32 + aJ];
    }
    for (int m = 0; m < t.G; ++m) for (int a = 0; a < A; ++a) if (hits[(size_t)m * 32 + a] != 1) return false;
    return true;
}

// MERGED TAILS: a seeded template whose LAST general block holds r valid rows -- its leading ones -- with r < 16 and 16 % r == 0.  The
// last blocks of S = 16 / r neighbouring groups then fill one block between them: merged row j is row j % r of the last block of
// group j / r of the S (painn_pair_kernel.hpp: painn_pair_general_tails_kernel walks them so; storage and row words stay as they are).
// Counted from the row words, like pair_template_seeded: the twin rows of 18 atoms at G = 4 leave r = 4 (36 = 16 + 16 + 4), S = 4.
// r == 0: no merge.
struct PairTails {
    int r = 0, S = 0;
    std::vector<std::array<int, 3>> map;      // [16] merged row -> (group in super-group, block, row in block)
};
inline PairTails pair_template_tails(const PairTemplate& t, int A)
{
    PairTails out;
    if (!pair_template_seeded(t, A)) return out;
    const size_t last = (size_t)(t.nblk - 1) * 16;
    int r = 0;
    for (int k = 0; k < 16; ++k) r += (int)(t.rows[last + k] & 1u);
    if (r <= 0 || r >= 16 || 16 % r) return out;
    for (int k = 0; k < r; ++k) if (!(t.rows[last + k] & 1u)) return out;      // valid rows lead the block
    out.r = r; out.S = 16 / r;
    for (int j = 0; j < 16; ++j) out.map.push_back({j / r, t.nblk - 1, j % r});
    return out;
}

namespace pair_detail {
struct Blk {
    int I[4], J[4];                          // slot keys mol * 32 + atom, -1 = empty
    Blk() { for (int k = 0; k < 4; ++k) I[k] = J[k] = -1; }
    static int count(const int* s) { int n = 0; for (int k = 0; k < 4; ++k) n += s[k] >= 0; return n; }
    static bool has(const int* s, int key) { for (int k = 0; k < 4; ++k) if (s[k] == key) return true; return false; }
    static void add(int* s, int key) { for (int k = 0; k < 4; ++k) if (s[k] < 0) { s[k] = key; return; } }
};

// the molecule's graph as a type matrix: pt[src * A + dst] = type of that directed edge, -1 = none.  false: not the symmetric closure
// of an undirected graph with one type per pair (or too large)
inline bool read_graph(int A, int E, const int32_t* src, const int32_t* dst, const int32_t* etype, std::vector<int>& pt)
{
    if (E <= 0 || (E & 1) || A > 32) return false;
    pt.assign((size_t)A * A, -1);
    for (int k = 0; k < E; ++k) {
        if (src[k] == dst[k] || pt[(size_t)src[k] * A + dst[k]] >= 0) return false;        // self loop / duplicate edge
        pt[(size_t)src[k] * A + dst[k]] = etype[k];
    }
    for (int i = 0; i < A; ++i)
        for (int j = 0; j < A; ++j)
            if (pt[(size_t)i * A + j] != pt[(size_t)j * A + i]) return false;              // j -> i missing or of another type
    return true;
}

// the tile blocks of a group of G molecules (header comment: tiles of four, spare slots, loose pairs)
inline std::vector<Blk> tile_blocks(int A, const std::vector<int>& pt, int G)
{
    auto exists = [&](int i, int j) { return i != j && pt[(size_t)i * A + j] >= 0; };
    const int NT = (A + 3) / 4;
    std::vector<Blk> blocks;
    std::vector<char> cov((size_t)G * A * A, 0);
    auto covered = [&](int m, int i, int j) -> char& { return cov[((size_t)m * A + std::min(i, j)) * A + std::max(i, j)]; };
    // rows a block would newly cover if atom u of molecule m joined its I side (to_I) or J side
    auto gain = [&](const Blk& b, bool to_I, int m, int u) {
        const int* other = to_I ? b.J : b.I;
        int g = 0;
        for (int k = 0; k < 4; ++k)
            if (other[k] >= 0 && other[k] / 32 == m) { const int x = other[k] % 32; if (exists(u, x) && !covered(m, u, x)) ++g; }
        return g;
    };
    auto mark = [&](const Blk& b) {
        for (int a = 0; a < 4; ++a)
            for (int c = 0; c < 4; ++c)
                if (b.I[a] >= 0 && b.J[c] >= 0 && b.I[a] / 32 == b.J[c] / 32 && exists(b.I[a] % 32, b.J[c] % 32))
                    covered(b.I[a] / 32, b.I[a] % 32, b.J[c] % 32) = 1;
    };
    for (int m = 0; m < G; ++m) {
        const size_t first_block = blocks.size();
        for (int ta = 0; ta < NT; ++ta)
            for (int tb = ta + 1; tb < NT; ++tb) {
                Blk b;
                for (int i = 4 * ta; i < std::min(A, 4 * ta + 4); ++i)
                    for (int j = 4 * tb; j < std::min(A, 4 * tb + 4); ++j)
                        if (exists(i, j)) {
                            if (!Blk::has(b.I, m * 32 + i)) Blk::add(b.I, m * 32 + i);
                            if (!Blk::has(b.J, m * 32 + j)) Blk::add(b.J, m * 32 + j);
                        }
                if (Blk::count(b.I) == 0) continue;
                mark(b);
                blocks.push_back(b);
            }
        for (;;) {                                   // spare slots absorb uncovered pairs of this molecule
            int bg = 0, bb = -1, bu = -1; bool b_to_I = false;
            for (size_t bi = first_block; bi < blocks.size(); ++bi)
                for (int side = 0; side < 2; ++side) {
                    const Blk& b = blocks[bi];
                    const int* mine = side ? b.I : b.J;
                    if (Blk::count(mine) == 4) continue;
                    for (int u = 0; u < A; ++u) {
                        if (Blk::has(mine, m * 32 + u)) continue;
                        const int g = gain(b, side != 0, m, u);
                        if (g > bg) { bg = g; bb = (int)bi; bu = u; b_to_I = side != 0; }
                    }
                }
            if (bg == 0) break;
            Blk& b = blocks[bb];
            Blk::add(b_to_I ? b.I : b.J, m * 32 + bu);
            mark(b);
        }
    }
    std::vector<std::array<int, 3>> loose;           // pairs nothing covers yet, of all G molecules
    for (int m = 0; m < G; ++m)
        for (int i = 0; i < A; ++i)
            for (int j = i + 1; j < A; ++j)
                if (exists(i, j) && !covered(m, i, j)) loose.push_back({m, i, j});
    while (!loose.empty()) {
        Blk b;
        for (;;) {
            int best_new = 99, best_k = -1; bool best_swap = false;
            for (size_t k = 0; k < loose.size(); ++k) {
                if (covered(loose[k][0], loose[k][1], loose[k][2])) continue;
                for (int sw = 0; sw < 2; ++sw) {
                    const int ki = loose[k][0] * 32 + loose[k][sw ? 2 : 1], kj = loose[k][0] * 32 + loose[k][sw ? 1 : 2];
                    const int ni = Blk::has(b.I, ki) ? 0 : 1, nj = Blk::has(b.J, kj) ? 0 : 1;
                    if (Blk::count(b.I) + ni > 4 || Blk::count(b.J) + nj > 4) continue;
                    if (ni + nj < best_new) { best_new = ni + nj; best_k = (int)k; best_swap = sw != 0; }
                }
            }
            if (best_k < 0) break;
            const int ki = loose[best_k][0] * 32 + loose[best_k][best_swap ? 2 : 1], kj = loose[best_k][0] * 32 + loose[best_k][best_swap ? 1 : 2];
            if (!Blk::has(b.I, ki)) Blk::add(b.I, ki);
            if (!Blk::has(b.J, kj)) Blk::add(b.J, kj);
            mark(b);
        }
        blocks.push_back(b);
        std::vector<std::array<int, 3>> rest;
        for (auto& l : loose) if (!covered(l[0], l[1], l[2])) rest.push_back(l);
        loose.swap(rest);
    }
    return blocks;
}

using Pair = std::array<int, 3>;             // (molecule in group, atom i, atom j), i < j

// The template's words: the tile blocks in order, then the `general` pairs 16 to a block.  A pair two tile blocks could both hold
// belongs to the first of them (an atom pair may appear twice when both atoms sit on both sides); a general pair belongs to no tile.
constexpr int32_t SLOT_FIRST_TOUCH_BIT = 1 << 30;
inline void emit(int A, int E, const std::vector<int>& pt, int G, const std::vector<Blk>& tiles, const std::vector<Pair>& general,
                 bool first_touch, PairTemplate& out)
{
    auto exists = [&](int i, int j) { return i != j && pt[(size_t)i * A + j] >= 0; };
    constexpr int RB = 16;
    const int n_tile = (int)tiles.size(), nblk = n_tile + ((int)general.size() + RB - 1) / RB;
    out.G = G; out.nblk = nblk; out.n_tile = n_tile;
    out.rows.assign((size_t)nblk * RB, 0u); out.slotnode.assign((size_t)nblk * RB, -1);
    out.pair_pos.assign((size_t)G * A * A, -1);
    std::vector<char> done((size_t)G * A * A, 0), touched((size_t)G * 32, 0);
    for (const Pair& g : general) done[((size_t)g[0] * A + g[1]) * A + g[2]] = 1;
    size_t n_valid = 0;
    auto row_word = [&](bool valid, int m, int i, int j) {
        const int type = valid ? pt[(size_t)i * A + j] : 0;
        return (valid ? 1u : 0u) | ((uint32_t)m << 1) | ((uint32_t)i << 4) | ((uint32_t)m << 9) | ((uint32_t)j << 12) | ((uint32_t)type << 17);
    };
    for (int bi = 0; bi < n_tile; ++bi) {
        const Blk& b = tiles[bi];
        int safeI = -1, safeJ = -1;                      // rows of empty slots point at an atom that exists
        for (int k = 0; k < 4; ++k) { if (safeI < 0 && b.I[k] >= 0) safeI = b.I[k]; if (safeJ < 0 && b.J[k] >= 0) safeJ = b.J[k]; }
        for (int a = 0; a < 4; ++a)
            for (int c = 0; c < 4; ++c) {
                const int ki = b.I[a] >= 0 ? b.I[a] : safeI, kj = b.J[c] >= 0 ? b.J[c] : safeJ;
                const int m = ki / 32, i = ki % 32, j = kj % 32;
                bool valid = b.I[a] >= 0 && b.J[c] >= 0 && kj / 32 == m && exists(i, j);
                if (valid) {                             // first row wins
                    char& d = done[((size_t)m * A + std::min(i, j)) * A + std::max(i, j)];
                    if (d) valid = false; else d = 1;
                }
                const int type = valid ? pt[(size_t)i * A + j] : 0;
                out.rows[(size_t)bi * RB + 4 * a + c] = (valid ? 1u : 0u) | ((uint32_t)(ki / 32) << 1) | ((uint32_t)i << 4) |
                                                        ((uint32_t)(kj / 32) << 9) | ((uint32_t)j << 12) | ((uint32_t)type << 17);
                if (valid) {
                    ++n_valid;
                    out.pair_pos[((size_t)m * A + i) * A + j] = (bi * 2 + 0) * RB + 4 * a + c;       // direction A: I[a] -> J[c]
                    out.pair_pos[((size_t)m * A + j) * A + i] = (bi * 2 + 1) * RB + 4 * a + c;       // direction B: J[c] -> I[a]
                }
            }
        for (int side = 0; side < 2; ++side)               // J slots first (see first_touch below)
            for (int k = 0; k < 4; ++k) {
                const int key = side ? b.I[k] : b.J[k];
                if (key < 0) continue;
                const int32_t first = (first_touch && !touched[key]) ? SLOT_FIRST_TOUCH_BIT : 0;
                touched[key] = 1;
                out.slotnode[(size_t)bi * RB + (side ? k : 4 + k)] = first | ((key / 32) << 8) | (key % 32);
            }
    }
    for (size_t k = 0; k < (size_t)(nblk - n_tile) * RB; ++k) {      // general rows; the padding names the block's first pair
        const bool valid = k < general.size();
        const Pair& g = general[valid ? k : k / RB * RB];
        const size_t r = (size_t)n_tile * RB + k;
        out.rows[r] = row_word(valid, g[0], g[1], g[2]);
        if (valid) {
            ++n_valid;
            const int bi = (int)(r / RB), row = (int)(r % RB);
            out.pair_pos[((size_t)g[0] * A + g[1]) * A + g[2]] = (bi * 2 + 0) * RB + row;
            out.pair_pos[((size_t)g[0] * A + g[2]) * A + g[1]] = (bi * 2 + 1) * RB + row;
        }
    }
    if (n_valid * 2 != (size_t)G * E) throw std::logic_error("pair template: not every edge was placed exactly once");
    out.fill = (double)n_valid / ((double)nblk * RB);
    out.seeded = pair_template_seeded(out, A);
}

// the pairs every tile block owns (emit's rule: the first block that could hold a pair)
inline std::vector<std::vector<Pair>> owned_pairs(int A, const std::vector<int>& pt, int G, const std::vector<Blk>& tiles)
{
    auto exists = [&](int i, int j) { return i != j && pt[(size_t)i * A + j] >= 0; };
    std::vector<char> done((size_t)G * A * A, 0);
    std::vector<std::vector<Pair>> own(tiles.size());
    for (size_t bi = 0; bi < tiles.size(); ++bi)
        for (int a = 0; a < 4; ++a)
            for (int c = 0; c < 4; ++c) {
                const int ki = tiles[bi].I[a], kj = tiles[bi].J[c];
                if (ki < 0 || kj < 0 || ki / 32 != kj / 32 || !exists(ki % 32, kj % 32)) continue;
                const int m = ki / 32, i = std::min(ki % 32, kj % 32), j = std::max(ki % 32, kj % 32);
                char& d = done[((size_t)m * A + i) * A + j];
                if (!d) { d = 1; own[bi].push_back({m, i, j}); }
            }
    return own;
}

// What a general block costs the kernel in tile blocks: four times the accumulator atomics and v gathers of the output stage.  Measured
// at the headline shape (F = 128, five layers): 1.45 in a middle layer, 1.59 in the last, 2.35 in layer 0 on the phi table, 1.57 over
// the five launches.  Every choice below weighs general blocks with it: an unweighted generic pass took A = 9 from 3
// to 2.63 blocks per molecule and A = 25 from 21 to 19.5 and LOST 10 % and 11 % of their steps/s.
constexpr double PAIR_GENERAL_WEIGHT = 1.6;
inline double weighted_blocks(size_t tiles, size_t general_pairs) { return (double)tiles + PAIR_GENERAL_WEIGHT * (double)((general_pairs + 15) / 16); }

// Dissolve tile blocks into general rows, emptiest first, as long as the weighted block count falls: weighted_blocks is
// evaluated after every block taken and the best prefix is kept.  A block is passed over when taking it would leave an atom of a
// general pair without a slot in a tile block (header comment).
inline void dissolve(int A, const std::vector<int>& pt, int G, std::vector<Blk>& tiles, std::vector<Pair>& general)
{
    const std::vector<std::vector<Pair>> own = owned_pairs(A, pt, G, tiles);
    const int n = (int)tiles.size();
    std::vector<int> order(n), slots((size_t)G * 32, 0), need((size_t)G * 32, 0);
    for (int b = 0; b < n; ++b) order[b] = b;
    std::stable_sort(order.begin(), order.end(), [&](int x, int y) { return own[x].size() < own[y].size(); });
    auto each_slot = [&](const Blk& b, int delta) {
        for (int k = 0; k < 4; ++k) { if (b.I[k] >= 0) slots[b.I[k]] += delta; if (b.J[k] >= 0) slots[b.J[k]] += delta; }
    };
    for (const Blk& b : tiles) each_slot(b, 1);
    for (const Pair& g : general) { need[g[0] * 32 + g[1]] = 1; need[g[0] * 32 + g[2]] = 1; }
    std::vector<int> taken;
    size_t moved = general.size(), best_count = 0;
    double best_total = weighted_blocks(n, moved);
    for (int b : order) {
        if (own[b].size() == 16) break;                  // a full tile is never worth a general block
        each_slot(tiles[b], -1);
        std::vector<int> fresh;
        for (const Pair& g : own[b]) for (int a : {g[1], g[2]}) if (!need[g[0] * 32 + a]) { need[g[0] * 32 + a] = 1; fresh.push_back(g[0] * 32 + a); }
        bool ok = true;
        for (size_t key = 0; key < need.size() && ok; ++key) ok = !need[key] || slots[key] > 0;
        if (!ok) { each_slot(tiles[b], 1); for (int key : fresh) need[key] = 0; continue; }
        taken.push_back(b);
        moved += own[b].size();
        const double total = weighted_blocks((size_t)n - taken.size(), moved);
        if (total < best_total) { best_total = total; best_count = taken.size(); }
    }
    std::vector<char> gone(n, 0);
    for (size_t k = 0; k < best_count; ++k) gone[taken[k]] = 1;
    std::vector<Blk> kept;
    for (int b = 0; b < n; ++b) { if (!gone[b]) kept.push_back(tiles[b]); else general.insert(general.end(), own[b].begin(), own[b].end()); }
    tiles.swap(kept);
}

// Full tiles of the complete graph on 18 atoms.  Pair the atoms as twins (2a, 2a + 1), a in Z_9: K18 minus the twin matching is the
// 2-blow-up of K9, and the 4-cycle (0, 1, 5, 3) developed mod 9 -- its edges have the differences 1, 4, 2, 3, each once -- decomposes
// K9 into nine 4-cycles.  Cycle i is the bipartite square {i, i + 5} x {i + 1, i + 3}: its blow-up is one full 4 x 4 tile, I the
// twins of the first two, J the twins of the other two.  Nine full tiles (144 pairs) per molecule; the nine twin pairs are left for
// general rows.  false: not that graph (other complete graphs take the generic pass alone; n = A / 2 would need n = 1 mod 8).
inline bool twin_tiles(int A, const std::vector<int>& pt, int G, std::vector<Blk>& tiles, std::vector<Pair>& general)
{
    if (A != 18) return false;
    for (int i = 0; i < A; ++i) for (int j = 0; j < A; ++j) if (i != j && pt[(size_t)i * A + j] < 0) return false;
    tiles.clear(); general.clear();
    for (int m = 0; m < G; ++m) {
        for (int i = 0; i < 9; ++i) {
            Blk b;
            const int I[2] = {i, (i + 5) % 9}, J[2] = {(i + 1) % 9, (i + 3) % 9};
            for (int k = 0; k < 4; ++k) { b.I[k] = m * 32 + 2 * I[k / 2] + k % 2; b.J[k] = m * 32 + 2 * J[k / 2] + k % 2; }
            tiles.push_back(b);
        }
        for (int a = 0; a < 9; ++a) general.push_back({m, 2 * a, 2 * a + 1});
    }
    return true;
}
}  // namespace pair_detail

// src / dst / etype: the E directed edges of ONE molecule (A <= 32 atoms).  Returns false (no pair template) when the directed graph
// is not the symmetric closure of an undirected one with one type per pair.
// first_touch: mark (PAIR_SLOT_FIRST_TOUCH), per atom, the first slot that holds it in walk order -- blocks ascending, inside a block
// the J slots (direction A) before the I slots (direction B): the order the kernel issues its accumulator updates in.  That update
// replaces the accumulator's stale contents, the later ones add (ti_internal.hpp SLOT_FIRST_TOUCH).
// Tile blocks only (n_tile == nblk): stage 1 of build_pair_template_packed, and the template TI_PAIR_PACKED=0 keeps.
constexpr int32_t PAIR_SLOT_FIRST_TOUCH = pair_detail::SLOT_FIRST_TOUCH_BIT;      // == ti::SLOT_FIRST_TOUCH (ti_internal.hpp)
inline bool build_pair_template(int A, int E, const int32_t* src, const int32_t* dst, const int32_t* etype, PairTemplate& out, bool first_touch)
{
    using pair_detail::Blk;
    std::vector<int> pt;
    if (!pair_detail::read_graph(A, E, src, dst, etype, pt)) return false;
    int bestG = 0; std::vector<Blk> best;
    for (int G : {1, 2, 4, 8}) {
        std::vector<Blk> blocks = pair_detail::tile_blocks(A, pt, G);
        // fewest blocks per molecule wins; a larger G must save at least 2 % to be preferred (fewer, longer waves otherwise)
        if (bestG == 0 || (double)blocks.size() / G < 0.98 * (double)best.size() / bestG) { bestG = G; best = blocks; }
    }
    pair_detail::emit(A, E, pt, bestG, best, {}, first_touch, out);
    return true;
}

// Tile blocks first, then general blocks (header comment); out.n_tile counts the tiles.  Per G the candidates are the tile template
// with its emptiest blocks dissolved and, for the complete graph on 18 atoms, the twin tiles; the one that costs less is taken
// (twin tiles on a tie), and G is chosen by the rule above, on cost: a general block counts PAIR_GENERAL_WEIGHT tiles throughout.
inline bool build_pair_template_packed(int A, int E, const int32_t* src, const int32_t* dst, const int32_t* etype, PairTemplate& out, bool first_touch)
{
    using pair_detail::Blk; using pair_detail::Pair;
    std::vector<int> pt;
    if (!pair_detail::read_graph(A, E, src, dst, etype, pt)) return false;
    int bestG = 0; std::vector<Blk> best; std::vector<Pair> best_general;
    auto count = [](const std::vector<Blk>& t, const std::vector<Pair>& g) { return pair_detail::weighted_blocks(t.size(), g.size()); };
    for (int G : {1, 2, 4, 8}) {
        std::vector<Blk> tiles = pair_detail::tile_blocks(A, pt, G), twin;
        std::vector<Pair> general, twin_general;
        pair_detail::dissolve(A, pt, G, tiles, general);
        if (pair_detail::twin_tiles(A, pt, G, twin, twin_general) && count(twin, twin_general) <= count(tiles, general)) { tiles.swap(twin); general.swap(twin_general); }
        if (bestG == 0 || count(tiles, general) / G < 0.98 * count(best, best_general) / bestG) { bestG = G; best = tiles; best_general = general; }
    }
    pair_detail::emit(A, E, pt, bestG, best, best_general, first_touch, out);
    return true;
}

}  // namespace ti
