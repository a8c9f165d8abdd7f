// painn_pack.hip -- host side of the PaiNN handle at creation: weight packing into the kernels' chunk streams, and the edge templates
// (row / slot words of the message kernels) with their per-call selection and per-molecule masked copies.
#include "message_stream.hpp"
#include "pair_template.hpp"
#include "ti_handle.hpp"

namespace ti {

// ---------------------------------------------------------------------------------------------------- packing
// 16-row kernels (mfma_chain.hpp, namespace r16): chunk[(blk*NBK + nbi)*64 + l][r] = W[row0 + 16*blk + (l&15)][col0 + 16*nbi + 4*(l>>4) + r]
void pack_chunk16(std::vector<float>& dst, const float* W, int ld, int n_rows, int row0, int col0, int NBK)
{
    const size_t base = dst.size();
    dst.resize(base + (size_t)2 * NBK * 64 * 4);
    for (int blk = 0; blk < 2; ++blk)
        for (int nbi = 0; nbi < NBK; ++nbi)
            for (int l = 0; l < 64; ++l)
                for (int r = 0; r < 4; ++r) {
                    const int row = row0 + 16 * blk + (l & 15), col = col0 + 16 * nbi + 4 * (l >> 4) + r;
                    dst[base + ((size_t)(blk * NBK + nbi) * 64 + l) * 4 + r] = row < n_rows ? W[(size_t)row * ld + col] : 0.f;
                }
}

// split-fp16 chunk of the edge kernel (mfma_chain.hpp, r16::Opnd<NBK,true>): 16-byte h8 fragments
//   frag[((blk*(NBK/2) + m)*2 + {0 hi, 1 lo})*64 + l][i] = half of W[row0 + 16*blk + (l&15)][col0 + 16*(2m + (i>>2)) + 4*(l>>4) + (i&3)]
// with hi = fp16(w), lo = fp16((w - hi) * 2^11).  Same byte size as the fp32 chunk.
void pack_chunk16_split(std::vector<float>& dst, const float* W, int ld, int n_rows, int row0, int col0, int NBK)
{
    const size_t base = dst.size();
    dst.resize(base + (size_t)2 * NBK * 64 * 4);
    _Float16* out = reinterpret_cast<_Float16*>(dst.data() + base);
    const int KS = NBK / 2;
    for (int blk = 0; blk < 2; ++blk)
        for (int m = 0; m < KS; ++m)
            for (int l = 0; l < 64; ++l)
                for (int i = 0; i < 8; ++i) {
                    const int row = row0 + 16 * blk + (l & 15), col = col0 + 16 * (2 * m + (i >> 2)) + 4 * (l >> 4) + (i & 3);
                    const float w = row < n_rows ? W[(size_t)row * ld + col] : 0.f;
                    const _Float16 h = (_Float16)w;
                    const _Float16 lo = (_Float16)((w - (float)h) * 2048.0f);
                    out[((size_t)((blk * KS + m) * 2 + 0) * 64 + l) * 8 + i] = h;
                    out[((size_t)((blk * KS + m) * 2 + 1) * 64 + l) * 8 + i] = lo;
                }
}

// one-accumulator format of the message kernel (mfma_chain.hpp: Opnd1 / gemm_split_chunk1): the matrix is scaled by the power of two S
// first and the residual is NOT scaled:  hi = fp16(S w), lo = fp16(S w - hi).  Same layout and size as pack_chunk16_split.
void pack_chunk16_split1(std::vector<float>& dst, const float* W, int ld, int n_rows, int row0, int col0, int NBK, float S)
{
    const size_t base = dst.size();
    dst.resize(base + (size_t)2 * NBK * 64 * 4);
    _Float16* out = reinterpret_cast<_Float16*>(dst.data() + base);
    const int KS = NBK / 2;
    for (int blk = 0; blk < 2; ++blk)
        for (int m = 0; m < KS; ++m)
            for (int l = 0; l < 64; ++l)
                for (int i = 0; i < 8; ++i) {
                    const int row = row0 + 16 * blk + (l & 15), col = col0 + 16 * (2 * m + (i >> 2)) + 4 * (l >> 4) + (i & 3);
                    const float w = (row < n_rows ? W[(size_t)row * ld + col] : 0.f) * S;
                    const _Float16 h = (_Float16)w;
                    out[((size_t)((blk * KS + m) * 2 + 0) * 64 + l) * 8 + i] = h;
                    out[((size_t)((blk * KS + m) * 2 + 1) * 64 + l) * 8 + i] = (_Float16)(w - (float)h);
                }
}
// power of two that brings the largest |entry| of W[0..rows)[col0..col0+cols) into [2^13, 2^14)   (1 for an all-zero matrix).
// `bias` (n_bias entries, may be NULL) is the layer's bias row, which the kernel multiplies by the same factor: the factor is capped so
// that S |b| stays <= 2^14 -- a near-zero matrix beside O(1) biases (a pruned or freshly initialised layer) would otherwise scale the
// biases to 1e18 and overflow the LayerNorm's sum of squares; what the cap costs is precision of a product that is negligible beside
// that bias anyway.  phi's first Linear packs only its e half (columns F..2F), but the kernel multiplies the per-atom P = s W_s^T + b0
// by the same factor, so its factor is taken over all 2F columns and b0: S |W_s| <= 2^14 bounds S |P| by 2^14 (|s|_1 + 1).
float matrix_pow2_scale(const float* W, int ld, int rows, int col0, int cols, const float* bias = nullptr, int n_bias = 0)
{
    float mx = 0.f, mb = 0.f;
    for (int r = 0; r < rows; ++r)
        for (int c = 0; c < cols; ++c) mx = std::max(mx, std::fabs(W[(size_t)r * ld + col0 + c]));
    for (int i = 0; i < n_bias; ++i) mb = std::max(mb, std::fabs(bias[i]));
    if (!(mx > 0.f) || !std::isfinite(mx)) return 1.0f;
    int e; std::frexp(mx, &e);                      // mx = f * 2^e, f in [0.5, 1)
    int k = std::min(60, std::max(-60, 14 - e));
    if (mb > 0.f && std::isfinite(mb)) { int eb; std::frexp(mb, &eb); k = std::min(k, std::max(-60, 14 - eb)); }
    return std::ldexp(1.0f, k);
}

// fp16 storage mode (r16::OpndH): the hi fragments alone, half the bytes:  frag[(blk*(NBK/2) + m)*64 + l][i]
void pack_chunk16_half(std::vector<float>& dst, const float* W, int ld, int n_rows, int row0, int col0, int NBK)
{
    const size_t base = dst.size();
    dst.resize(base + (size_t)NBK * 64 * 4);
    _Float16* out = reinterpret_cast<_Float16*>(dst.data() + base);
    const int KS = NBK / 2;
    for (int blk = 0; blk < 2; ++blk)
        for (int m = 0; m < KS; ++m)
            for (int l = 0; l < 64; ++l)
                for (int i = 0; i < 8; ++i) {
                    const int row = row0 + 16 * blk + (l & 15), col = col0 + 16 * (2 * m + (i >> 2)) + 4 * (l >> 4) + (i & 3);
                    out[((size_t)(blk * KS + m) * 64 + l) * 8 + i] = (_Float16)(row < n_rows ? W[(size_t)row * ld + col] : 0.f);
                }
}

size_t take_mlp(MlpOff& m, size_t o, int f_in, int f_h, int f_out)
{
    m.f_in = f_in; m.f_h = f_h; m.f_out = f_out;
    m.W0 = o; o += (size_t)f_h * f_in; m.b0 = o; o += f_h; m.g0 = o; o += f_h; m.be0 = o; o += f_h;
    m.W1 = o; o += (size_t)f_h * f_h;  m.b1 = o; o += f_h; m.g1 = o; o += f_h; m.be1 = o; o += f_h;
    m.W2 = o; o += (size_t)f_out * f_h; m.b2 = o; o += f_out;
    return o;
}

// ------------------------------------------------------------------------------------------------ edge templates
// Packs the rows of `count` molecules' edges with sorted position in [k0, k1) into 16-row blocks: rows keep their (molecule, dst,
// src) order; a block takes at most EDGE_MAX_SLOTS destination atoms (a further one starts the next block, the rest is padding).
// pos[m * (k1 - k0) + (k - k0)] = row of that edge inside the part; returns the number of blocks used.
static int pack_part(const ti_handle* h, const int32_t* dst, int count, int k0, int k1, std::vector<int>& pos)
{
    constexpr int RB = ti::EDGE_ROWS_PER_BLOCK;
    const int per = k1 - k0;
    pos.assign((size_t)count * per, 0);
    int row = 0, nslot = 0, last_key = -1;
    for (int m = 0; m < count; ++m)
        for (int k = k0; k < k1; ++k) {
            const int key = m * 256 + dst[h->perm[k]];
            if (row % RB == 0) { nslot = 0; last_key = -1; }
            if (key != last_key) {
                if (nslot == ti::EDGE_MAX_SLOTS) { row = (row + RB - 1) / RB * RB; nslot = 0; }
                ++nslot; last_key = key;
            }
            pos[(size_t)m * per + (k - k0)] = row++;
        }
    return (row + RB - 1) / RB;
}

// row / slot words of a packed part (ti_internal.hpp); returns the most slots any block holds
static int fill_part(const ti_handle* h, const int32_t* src, const int32_t* dst, const int32_t* etype, int count, int k0, int k1, int nblk,
                     const std::vector<int>& pos, uint32_t* rw, int32_t* sn)
{
    constexpr int RB = ti::EDGE_ROWS_PER_BLOCK;
    const int per = k1 - k0;
    for (int i = 0; i < nblk * RB; ++i) { rw[i] = (uint32_t)63 << 18; sn[i] = -1; }
    std::vector<int> nslot(std::max(nblk, 1), 0), last_key(std::max(nblk, 1), -1);
    std::vector<char> touched((size_t)count * 256, 0);          // rows are visited in increasing order: the first block seen is the first executed
    int most = 0;
    for (int m = 0; m < count; ++m)
        for (int kk = 0; kk < per; ++kk) {
            const int r = pos[(size_t)m * per + kk], blk = r / RB, k = h->perm[k0 + kk];
            const int key = m * 256 + dst[k];
            if (key != last_key[blk]) {
                const int32_t first = (h->first_touch && !touched[key]) ? ti::SLOT_FIRST_TOUCH : 0;
                touched[key] = 1;
                sn[(size_t)blk * RB + nslot[blk]] = first | (m << 8) | dst[k]; ++nslot[blk]; last_key[blk] = key;
            }
            most = std::max(most, nslot[blk]);
            rw[r] = 1u | ((uint32_t)m << 1) | ((uint32_t)src[k] << 6) | ((uint32_t)dst[k] << 11) | ((uint32_t)etype[k] << 16) |
                    ((uint32_t)(nslot[blk] - 1) << 18);
        }
    return most;
}

void build_templates(ti_handle* h, const int32_t* src, const int32_t* dst, const int32_t* etype)
{
    const int A = h->d.n_atoms, E = h->d.n_edges;
    constexpr int RB = ti::EDGE_ROWS_PER_BLOCK;
    {
        std::vector<char> has_in(A, 0);
        for (int k = 0; k < E; ++k) has_in[dst[k]] = 1;
        h->first_touch = E > 0 && std::all_of(has_in.begin(), has_in.end(), [](char c) { return c != 0; });
        // triage switch: TI_ZERO_ACC=1 at creation forces the zeroing path (memsets before an evaluation, the update kernel clears
        // what it consumed, every accumulator update is an add) -- tests/test_gpu_pair.py compares the two paths on poisoned accumulators
        if (const char* z = std::getenv("TI_ZERO_ACC")) if (z[0] == '1') h->first_touch = false;
    }
    h->perm.resize(E);
    for (int k = 0; k < E; ++k) h->perm[k] = k;
    std::stable_sort(h->perm.begin(), h->perm.end(), [&](int a, int b) {
        return dst[a] != dst[b] ? dst[a] < dst[b] : src[a] < src[b];
    });
    // ---- throughput template: smallest G in 1..8 whose padding waste is <= 2 %, else the least wasteful
    {
        int bestG = 1; double bestW = 2.0;
        std::vector<int> pos;
        for (int G = 1; G <= 8 && E > 0; ++G) {
            const int rows = G * E, padded = pack_part(h, dst, G, 0, E, pos) * RB;
            const double waste = double(padded - rows) / padded;
            if (waste < bestW - 1e-12) { bestW = waste; bestG = G; }
            if (waste <= 0.02) { bestG = G; break; }
        }
        ti_handle::Tpl& T = h->tpl[0];
        T.G = bestG; T.P = 1;
        T.nblk = E > 0 ? pack_part(h, dst, bestG, 0, E, T.pos) : 0;
        T.part_of.assign(E, 0); T.part_start.assign(1, 0); T.part_len.assign(1, E);
        std::vector<uint32_t> rw((size_t)std::max(T.nblk, 1) * RB); std::vector<int32_t> sn(rw.size());
        T.max_slots = fill_part(h, src, dst, etype, bestG, 0, E, T.nblk, T.pos, rw.data(), sn.data());
        if (T.nblk == 0) { rw[0] = (uint32_t)63 << 18; sn[0] = -1; }
        T.rows.upload(rw); T.slotnode.upload(sn); T.rows_h = rw;
    }
    // ---- latency template: one molecule per group, its destination atoms cut into P ranges of near-equal row count; the
    // largest P <= 8 whose padding waste stays <= 15 % (parts need whole row blocks).  Built only if it offers more waves.
    h->n_tpl = 1;
    if (E >= 2 * RB) {
        std::vector<int> first_of(A + 1, E);           // first sorted edge with destination >= a
        for (int k = E - 1; k >= 0; --k) first_of[dst[h->perm[k]]] = k;
        for (int a = A - 1; a >= 0; --a) first_of[a] = std::min(first_of[a], first_of[a + 1]);
        std::vector<int> pos;
        int bestP = 1, best_nblk = pack_part(h, dst, 1, 0, E, pos); std::vector<int> best_cut{0, E};
        for (int P = 2; P <= 8; ++P) {
            std::vector<int> cut{0};
            for (int q = 1; q < P; ++q) {             // atom boundary closest to q/P of the rows
                const int want = (int)((long long)E * q / P);
                int bk = cut.back();
                for (int a = 0; a <= A; ++a) if (first_of[a] > cut.back() && std::abs(first_of[a] - want) < std::abs(bk - want)) bk = first_of[a];
                if (bk <= cut.back()) { cut.clear(); break; }
                cut.push_back(bk);
            }
            if (cut.empty() || cut.back() >= E) continue;
            cut.push_back(E);
            int nblk = 0;
            for (int q = 0; q < P; ++q) nblk = std::max(nblk, pack_part(h, dst, 1, cut[q], cut[q + 1], pos));
            if (double(P * nblk * RB - E) / (P * nblk * RB) <= 0.15) { bestP = P; best_nblk = nblk; best_cut = cut; }
        }
        if (bestP * h->tpl[0].G > 1) {
            ti_handle::Tpl& T = h->tpl[1];
            T.G = 1; T.P = bestP; T.nblk = best_nblk; T.max_slots = 0;
            T.part_start.assign(best_cut.begin(), best_cut.end() - 1);
            T.part_of.resize(E); T.part_len.resize(bestP); T.pos.assign(E, 0);
            for (int q = 0; q < bestP; ++q) for (int k = best_cut[q]; k < best_cut[q + 1]; ++k) T.part_of[k] = q;
            std::vector<uint32_t> rw((size_t)bestP * best_nblk * RB); std::vector<int32_t> sn(rw.size());
            for (int q = 0; q < bestP; ++q) {
                T.part_len[q] = best_cut[q + 1] - best_cut[q];
                pack_part(h, dst, 1, best_cut[q], best_cut[q + 1], pos);
                std::copy(pos.begin(), pos.end(), T.pos.begin() + best_cut[q]);
                T.max_slots = std::max(T.max_slots, fill_part(h, src, dst, etype, 1, best_cut[q], best_cut[q + 1], best_nblk, pos,
                                                              rw.data() + (size_t)q * best_nblk * RB, sn.data() + (size_t)q * best_nblk * RB));
            }
            T.rows.upload(rw); T.slotnode.upload(sn); T.rows_h = rw;
            h->n_tpl = 2;
        }
    }
    h->esrc.assign(src, src + E); h->edst.assign(dst, dst + E);
}

// ---- pair-major template: pair_template.hpp builds it (pure host code, unit-tested on the CPU); this uploads it
bool build_pair_template(ti_handle* h, const int32_t* src, const int32_t* dst, const int32_t* etype)
{
    ti::PairTemplate pt;
    // triage switch, read like TI_PHI0_TABLE: TI_PAIR_PACKED=0 at creation keeps the tile-only template
    bool packed = ti::pair_general_build_exists(h->d.precision);      // (f32 handles: the tile-only template, ti_internal.hpp)
    if (const char* z = std::getenv("TI_PAIR_PACKED")) if (z[0] == '0') packed = false;
    const bool ok = packed ? ti::build_pair_template_packed(h->d.n_atoms, h->d.n_edges, src, dst, etype, pt, h->first_touch)
                           : ti::build_pair_template(h->d.n_atoms, h->d.n_edges, src, dst, etype, pt, h->first_touch);
    if (!ok) return false;
    ti_handle::Tpl& T = h->tpl[2];
    T.G = pt.G; T.P = 1; T.nblk = pt.nblk; T.n_tile = pt.n_tile; T.max_slots = 4;
    T.rows.upload(pt.rows); T.slotnode.upload(pt.slotnode); T.rows_h = pt.rows;
    h->pair_pos = pt.pair_pos; h->pair_fill = pt.fill;
    // triage switch, read like TI_PAIR_PACKED: TI_PAIR_SEEDED=0 at creation keeps the first-touch order on a seeded template
    h->pair_seeded = pt.seeded; h->pair_seeded_on = pt.seeded;
    if (const char* z = std::getenv("TI_PAIR_SEEDED")) if (z[0] == '0') h->pair_seeded_on = false;
    // merged tails of the seeded general launch: where the template has them and the kernel takes them (whole lane rows per group: r a
    // multiple of 4); TI_PAIR_TAILS=0 at creation, read the same way, keeps the walk of one group per wave
    const ti::PairTails tails = ti::pair_template_tails(pt, h->d.n_atoms);
    h->pair_tail_S = tails.r % 4 == 0 ? tails.S : 0; h->pair_tail_r = tails.r % 4 == 0 ? tails.r : 0;
    h->pair_tails_on = h->pair_tail_S > 0;
    if (const char* z = std::getenv("TI_PAIR_TAILS")) if (z[0] == '0') h->pair_tails_on = false;
    return true;
}

// The layout the handle is pinned to (ti_painn_set_template, or TI_TEMPLATE in the environment), TI_TEMPLATE_AUTO if none.
int pinned_template(const ti_handle* h)
{
    int want = h->pinned_tpl;
    if (const char* e = std::getenv("TI_TEMPLATE"))
        want = std::strcmp(e, "latency") == 0 ? 1 : std::strcmp(e, "throughput") == 0 ? 0 : std::strcmp(e, "pair") == 0 ? 2 : want;
    return want;
}
// an edge mask is in force whose molecules' sets are not all symmetric: the pair rows (one w factor for both directions) cannot take it
bool mask_blocks_pair(const ti_handle* h) { return h->emask_B > 0 && !h->emask_sym; }

// Template for a call over B molecules: the latency template while the throughput one would leave SIMDs without a wave
// (fewer groups than the 1024 SIMDs of the chip); TI_TEMPLATE=throughput|latency pins it (tests, reproducibility across shards).
int template_for(const ti_handle* h, long long B, bool allow_pair)
{
    int dir_pick = 0;                        // among the directed layouts: latency while the throughput one would leave SIMDs idle
    if (h->n_tpl > 1) dir_pick = (B + h->tpl[0].G - 1) / h->tpl[0].G < 1024 ? 1 : 0;
    const bool pair_ok = h->has_pair && allow_pair && !mask_blocks_pair(h);
    // pair-major rows once they fill the chip (one wave per group of G molecules) and cost less than the directed rows: a pair block
    // runs 84 chunk products for 16 pairs where a directed block runs 56 for 16 edges, at half the weight-chunk visits per edge; a
    // general block counts PAIR_GENERAL_WEIGHT tile blocks (pair_template.hpp)
    int pick = dir_pick;
    if (pair_ok) {
        const ti_handle::Tpl &T = h->tpl[2], &D = h->tpl[0];
        const double pair_blocks = T.n_tile + ti::pair_detail::PAIR_GENERAL_WEIGHT * (T.nblk - T.n_tile);
        if ((B + T.G - 1) / T.G >= 1024 && 1.5 * pair_blocks / T.G <= (double)D.nblk / D.G) pick = 2;
    }
    const int want = pinned_template(h);
    if (want == TI_TEMPLATE_THROUGHPUT) pick = 0;
    else if (want == TI_TEMPLATE_LATENCY) pick = h->n_tpl > 1 ? 1 : 0;
    else if (want == TI_TEMPLATE_PAIR) pick = pair_ok ? 2 : dir_pick;
    return pick;
}

// allow_pair = false: the divergence / tangent entry points (their kernels walk directed rows)
void select_template(ti_handle* h, long long B, bool allow_pair)
{
    if (h->emask_B > 0 && B != h->emask_B)
        throw std::invalid_argument("the edge mask in force is for " + std::to_string(h->emask_B) + " molecules, the call has " + std::to_string(B));
    if (allow_pair && h->has_pair && mask_blocks_pair(h) && pinned_template(h) == TI_TEMPLATE_PAIR)
        throw Unsupported("the pair layout is pinned, and the edge mask in force is not symmetric for every molecule");
    const int pick = template_for(h, B, allow_pair);
    const ti_handle::Tpl& T = h->tpl[pick];
    h->active = pick; h->G = T.G; h->parts = T.P; h->nblk = T.nblk; h->n_tile = pick == 2 ? T.n_tile : T.nblk; h->rows.p = T.rows.p; h->slotnode.p = T.slotnode.p;
    h->max_slots = T.max_slots;
}

// Row words of template t for the emask_B molecules of the edge mask, per (group, part) -- [groups][P][nblk * 16] -- with every edge
// absent from its molecule (every edge of a pad atom among them: set_graph_state cleared their bits) switched off: slot 63 in directed rows (weight 0 in the per-atom sums, like padding), the valid bit cleared
// in pair rows (w factor 0).  The masked twins of the message kernels read these instead of the template's shared rows.
const uint32_t* masked_rows(ti_handle* h, int t)
{
    if (h->mrows_ok[t]) return h->mrows[t].p;
    const ti_handle::Tpl& T = h->tpl[t];
    const long long B = h->emask_B, groups = (B + T.G - 1) / T.G;
    const int A = h->d.n_atoms;
    const size_t per = (size_t)T.nblk * ti::EDGE_ROWS_PER_BLOCK;
    std::vector<uint32_t> out((size_t)groups * T.P * per);
    const uint32_t* m = h->emask.data();
    const uint8_t* pt = h->ptype.empty() ? nullptr : h->ptype.data();      // per-molecule edge types of the present rows (ti_painn_set_molecules)
    for (long long g = 0; g < groups; ++g)
        for (int part = 0; part < T.P; ++part) {
            const uint32_t* src = T.rows_h.data() + (size_t)part * per;
            uint32_t* dst = out.data() + ((size_t)g * T.P + part) * per;
            for (size_t i = 0; i < per; ++i) {
                uint32_t w = src[i];
                if (w & 1u) {
                    if (t == 2) {
                        const long long mol = g * T.G + ti::prow_molI(w);
                        if (mol < B && !((m[mol * A + ti::prow_atomJ(w)] >> ti::prow_atomI(w)) & 1u)) w &= ~1u;
                        else if (mol < B && pt) w = (w & ~(3u << 17)) | ((uint32_t)pt[((size_t)mol * A + ti::prow_atomI(w)) * A + ti::prow_atomJ(w)] << 17);
                    } else {
                        const long long mol = g * T.G + ti::row_mol(w);
                        if (mol < B && !((m[mol * A + ti::row_dst(w)] >> ti::row_src(w)) & 1u)) w |= 63u << 18;
                        else if (mol < B && pt) w = (w & ~(3u << 16)) | ((uint32_t)pt[((size_t)mol * A + ti::row_src(w)) * A + ti::row_dst(w)] << 16);
                    }
                }
                dst[i] = w;
            }
        }
    h->mrows[t].upload(out);
    h->mrows_ok[t] = true;
    return h->mrows[t].p;
}

// row of (molecule m, sorted edge k) in the e / te layout of the active template
size_t edge_row_of(const ti_handle* h, size_t m, size_t k)
{
    const ti_handle::Tpl& T = h->tpl[h->active];
    if (h->active == 2) {                   // pair-major rows: [group][block][direction][16]
        const size_t A = h->d.n_atoms;
        return (m / T.G) * (size_t)T.nblk * 2 * ti::EDGE_ROWS_PER_BLOCK + (size_t)h->pair_pos[((m % T.G) * A + h->esrc[h->perm[k]]) * A + h->edst[h->perm[k]]];
    }
    // throughput template: one part, pos over (molecule in group, sorted edge); latency template: G = 1, pos over the sorted edge
    const size_t part = T.part_of[k], r = T.pos[(m % T.G) * (size_t)h->d.n_edges + k];
    return ((m / T.G) * T.P + part) * T.nblk * ti::EDGE_ROWS_PER_BLOCK + r;
}

// edge rows (e, te) per molecule-group slot, the larger of the two templates: rows a batch of B molecules needs
size_t edge_rows_for(const ti_handle* h, long long B, long long copies)
{
    size_t best = 1;
    for (int t = 0; t < h->n_tpl; ++t) {
        const ti_handle::Tpl& T = h->tpl[t];
        best = std::max<size_t>(best, (size_t)((B + T.G - 1) / T.G) * (size_t)copies * T.P * T.nblk * ti::EDGE_ROWS_PER_BLOCK);
    }
    if (h->has_pair && copies == 1)         // two directions per pair row
        best = std::max<size_t>(best, (size_t)((B + h->tpl[2].G - 1) / h->tpl[2].G) * h->tpl[2].nblk * 2 * ti::EDGE_ROWS_PER_BLOCK);
    return best;
}

// ------------------------------------------------------------------------------------------------ weight streams
void pack_painn(ti_handle* h, const float* wts)
{
    const int F = h->d.n_features, L = h->d.n_layers, NB = h->NB, nE = h->nE;
    std::vector<float> pk;
    auto begin_stream = [&]() { return pk.size() / 4; };
    size_t o = 0;
    const int NBK = F / 16;
    const int prec = h->d.precision;          // 16-row chunks: f32 image, (hi, lo) fp16 image of the same size, or hi-only fp16 image of half the size
    const size_t ch4 = (prec == TI_PREC_F16 ? 128 : 256) * (size_t)NB;      // float4 per 16-row chunk
    auto chunk16 = [&](size_t W, int ld, int n_rows, int row0, int col0) {
        if (prec == TI_PREC_F16) pack_chunk16_half(pk, wts + W, ld, n_rows, row0, col0, NBK);
        else if (prec == TI_PREC_F16X2) pack_chunk16_split(pk, wts + W, ld, n_rows, row0, col0, NBK);
        else pack_chunk16(pk, wts + W, ld, n_rows, row0, col0, NBK);
    };
    auto layer16 = [&](size_t W, int ld, int n_rows, int col0) { for (int nbo = 0; nbo < NB; ++nbo) chunk16(W, ld, n_rows, 32 * nbo, col0); };
    auto end_stream16 = [&](size_t off4) { return Stream{off4, (int)((pk.size() / 4 - off4) / ch4)}; };
    auto pad_even = [&](size_t off4) { if (((pk.size() / 4 - off4) / ch4) % 2) pk.resize(pk.size() + 4 * ch4, 0.f); };
    o = begin_stream();                              // embed kernel, 16-row chunk format: L1 by input segment, L2, L3, then P for the first message block
    for (int seg = 0; seg < nE; ++seg) layer16(h->embed.W0, nE * F, F, seg * F);
    layer16(h->embed.W1, F, F, 0); layer16(h->embed.W2, F, F, 0);
    if (L > 0) layer16(h->phi[0].W0, 2 * F, F, 0);
    else pk.resize(pk.size() + 4 * ch4 * NB, 0.f);
    pad_even(o);
    h->st_embed16 = end_stream16(o);
    for (int l = 0; l < L; ++l) {
        const bool first = l == 0, last = l == L - 1;
        o = begin_stream();                          // edge kernel: 16-row chunk format
        layer16(h->w[l].W0, F, F, 0); layer16(h->w[l].W1, F, F, 0);
        layer16(h->phi[l].W0, 2 * F, F, F);        // the e half of [s[src] | e]
        layer16(h->phi[l].W1, F, F, 0);
        for (int nbo = 0; nbo < NB; ++nbo)
            for (int c : {2, 3, 1, 0, 4}) {       // consumption order of painn_edge_kernel: ds, de, sed, gates, cross gates
                if (c == 3 && last) continue;
                if ((c == 0 || c == 4) && first) continue;
                chunk16(h->phi[l].W2, F, 5 * F, c * F + 32 * nbo, 0);
                chunk16(h->w[l].W2, F, 5 * F, c * F + 32 * nbo, 0);
            }
        h->st_edge.push_back(end_stream16(o));
        if (edge_one_chain(prec)) {         // the same chunks in the one-accumulator format, each matrix scaled by its own power of two
            const float S[6] = {matrix_pow2_scale(wts + h->w[l].W0, F, F, 0, F, wts + h->w[l].b0, F), matrix_pow2_scale(wts + h->w[l].W1, F, F, 0, F, wts + h->w[l].b1, F),
                                matrix_pow2_scale(wts + h->phi[l].W0, 2 * F, F, 0, 2 * F, wts + h->phi[l].b0, F), matrix_pow2_scale(wts + h->phi[l].W1, F, F, 0, F, wts + h->phi[l].b1, F),
                                matrix_pow2_scale(wts + h->phi[l].W2, F, 5 * F, 0, F, wts + h->phi[l].b2, 5 * F), matrix_pow2_scale(wts + h->w[l].W2, F, 5 * F, 0, F, wts + h->w[l].b2, 5 * F)};
            // one chunk list (message_stream.hpp) for the message kernels' stream and, in layer 0, for the two streams of the phi table path
            auto pack_message = [&](MsgPart part) {
                for (const MsgChunk& ch : message_chunks(NB, first, last, part)) {
                    const size_t W = ch.matrix == MSG_W_W0 ? h->w[l].W0 : ch.matrix == MSG_W_W1 ? h->w[l].W1 : ch.matrix == MSG_PHI_W0E ? h->phi[l].W0
                                   : ch.matrix == MSG_PHI_W1 ? h->phi[l].W1 : ch.matrix == MSG_PHI_W2 ? h->phi[l].W2 : h->w[l].W2;
                    const int ld = ch.matrix == MSG_PHI_W0E ? 2 * F : F, n_rows = ch.matrix >= MSG_PHI_W2 ? 5 * F : F, col0 = ch.matrix == MSG_PHI_W0E ? F : 0;
                    pack_chunk16_split1(pk, wts + W, ld, n_rows, ch.row0, col0, NBK, S[ch.matrix]);
                }
            };
            o = begin_stream();
            pack_message(MSG_ALL);
            h->st_edge1.push_back(end_stream16(o));
            h->edge_scale.insert(h->edge_scale.end(), S, S + 6);
            if (first && h->has_pair && pair_table_build_exists(NB, prec, false)) {
                // layer 0's chunks once more, cut in two for the phi table path (painn_phi0_kernels.hip): the w chunks alone in the walk
                // order of the pair kernel's table build, the phi chunks alone in the table kernel's; an odd count is padded to whole
                // superchunks
                o = begin_stream();
                pack_message(MSG_W);
                h->phi0_wpad = end_stream16(o).nch & 1;
                pad_even(o);
                h->st_phi0_w = end_stream16(o);
                o = begin_stream();
                pack_message(MSG_PHI);
                pad_even(o);
                h->st_phi0_tab = end_stream16(o);
                h->phi0_ok = true;
                // triage switch, read like TI_ZERO_ACC: TI_PHI0_TABLE=0 at creation pins the kernels of before
                if (const char* z = std::getenv("TI_PHI0_TABLE")) if (z[0] == '0') h->phi0_ok = false;
                // and, read the same way, TI_EMBED_CLASSES=0: the table path keeps the embed launch over every atom
                h->embed_cls_on = true;
                if (const char* z = std::getenv("TI_EMBED_CLASSES")) if (z[0] == '0') h->embed_cls_on = false;
            }
        }
        o = begin_stream();                          // update kernel: 16-row chunk format, order of painn_update_kernel
        layer16(h->V[l], F, F, 0);                                                    // phase A (3 components per visit)
        layer16(h->upd[l].W0, 2 * F, F, 0); layer16(h->upd[l].W0, 2 * F, F, F);      // MLP L1: |vv| part, s part
        layer16(h->upd[l].W1, F, F, 0);
        for (int nbo = 0; nbo < NB; ++nbo) {
            chunk16(h->upd[l].W2, F, 3 * F, F + 32 * nbo, 0);                         // scale_squared_norm
            chunk16(h->upd[l].W2, F, 3 * F, 2 * F + 32 * nbo, 0);                     // add_invariant_features
        }
        layer16(h->upd[l].W2, F, 3 * F, 0);                                           // gates
        for (int c = 0; c < 3; ++c) layer16(h->U[l], F, F, 0);                        // phase C (one spatial component per walk)
        if (!last) layer16(h->phi[l + 1].W0, 2 * F, F, 0);                            // phase D
        pad_even(o);                                                                  // whole superchunks
        h->st_update.push_back(end_stream16(o));
        // tangent edge kernel (painn_jvp_kernels.hip): the phi branch's chunks in the consumption order of the edge kernels
        for (int which = 1; which < 2; ++which) {      // the phi branch alone (the primal pass reads the primal edge stream)
            const MlpOff& m = h->phi[l];
            o = begin_stream();
            layer16(m.W0, 2 * F, F, F);
            layer16(m.W1, F, F, 0);
            for (int nbo = 0; nbo < NB; ++nbo)
                for (int c : {2, 3, 1, 0, 4}) {
                    if (c == 3 && last) continue;
                    if ((c == 0 || c == 4) && first) continue;
                    chunk16(m.W2, F, 5 * F, c * F + 32 * nbo, 0);
                }
            const int real = end_stream16(o).nch;   // an odd count gets one pad chunk, which the kernels swallow once per row block
            pad_even(o);
            h->st_jvp_phi.push_back(end_stream16(o));
            h->jvp_phi_pad.push_back(real & 1);
        }
        o = begin_stream();                          // tangent update kernel: same order, V and U once per spatial component
        for (int c = 0; c < 3; ++c) layer16(h->V[l], F, F, 0);
        layer16(h->upd[l].W0, 2 * F, F, 0); layer16(h->upd[l].W0, 2 * F, F, F);
        layer16(h->upd[l].W1, F, F, 0);
        for (int nbo = 0; nbo < NB; ++nbo) {
            chunk16(h->upd[l].W2, F, 3 * F, F + 32 * nbo, 0);
            chunk16(h->upd[l].W2, F, 3 * F, 2 * F + 32 * nbo, 0);
        }
        layer16(h->upd[l].W2, F, 3 * F, 0);
        for (int c = 0; c < 3; ++c) layer16(h->U[l], F, F, 0);
        if (!last) layer16(h->phi[l + 1].W0, 2 * F, F, 0);
        pad_even(o);
        h->st_jvp_update.push_back(end_stream16(o));
    }
    // readout kernels (primal and tangent): 16-row chunk format
    o = begin_stream();
    for (size_t Wm : {h->readout.W0, h->readout.W1})
        for (int nbo = 0; nbo < NB; ++nbo) {
            chunk16(Wm, F, F, 32 * nbo, 0);
        }
    pad_even(o);
    h->st_jvp_readout = end_stream16(o);
    h->packed.upload(pk);
    {
        std::vector<float> rv;                       // order = struct RV in painn_jvp_kernels.hip
        const MlpOff& r = h->readout;
        // Vr follows the 2-float readout bias in the canonical layout (h->Vr itself points at an aligned copy inside `flat`)
        for (size_t off : {r.b0, r.g0, r.be0, r.b1, r.g1, r.be1, r.W2 + (size_t)F, r.b2 + 2}) rv.insert(rv.end(), wts + off, wts + off + F);
        h->jvp_ro_vecs.upload(rv);
    }
    // per-layer vector block of the edge kernel (order = struct EV in painn_kernels.hip)
    std::vector<float> ev;
    for (int l = 0; l < L; ++l) {
        const MlpOff &w = h->w[l], &ph = h->phi[l];
        for (size_t off : {w.b0, w.g0, w.be0, w.b1, w.g1, w.be1, ph.g0, ph.be0, ph.b1, ph.g1, ph.be1}) ev.insert(ev.end(), wts + off, wts + off + F);
        ev.insert(ev.end(), wts + ph.b2, wts + ph.b2 + 5 * F);
        ev.insert(ev.end(), wts + w.b2, wts + w.b2 + 5 * F);
    }
    h->edge_vecs.upload(ev);
    if (edge_one_chain(prec)) {             // the message kernel's copy: bias rows times the scale of their matrix (EV order: W_B0 = 0, W_B1 = 3, P_B1 = 8, P_B2 = 11..15, W_B2 = 16..20)
        std::vector<float> ev1 = ev;
        for (int l = 0; l < L; ++l) {
            const float* S = h->edge_scale.data() + (size_t)l * 6;
            float* b = ev1.data() + (size_t)l * 21 * F;
            auto mul = [&](int row, int n, float sc) { for (int i = 0; i < n * F; ++i) b[(size_t)row * F + i] *= sc; };
            mul(0, 1, S[0]); mul(3, 1, S[1]); mul(8, 1, S[3]); mul(11, 5, S[4]); mul(16, 5, S[5]);
        }
        h->edge_vecs1.upload(ev1);
    }
    std::vector<float> uv;                           // order = struct UV in painn_kernels.hip
    for (int l = 0; l < L; ++l) {
        const MlpOff& u = h->upd[l];
        for (size_t off : {u.b0, u.g0, u.be0, u.b1, u.g1, u.be1}) uv.insert(uv.end(), wts + off, wts + off + F);
        uv.insert(uv.end(), wts + u.b2, wts + u.b2 + 3 * F);
        if (l + 1 < L) uv.insert(uv.end(), wts + h->phi[l + 1].b0, wts + h->phi[l + 1].b0 + F);
        else uv.insert(uv.end(), F, 0.f);
    }
    h->upd_vecs.upload(uv);
}

}  // namespace ti
