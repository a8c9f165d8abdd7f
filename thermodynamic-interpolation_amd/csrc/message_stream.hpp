// message_stream.hpp -- the order in which a message block's weight chunks are packed (painn_pack.hip) and walked (painn_pair_kernel.hpp,
// painn_edge_kernel.hpp, painn_phi0_kernels.hip).  Pure host C++ with no HIP dependency: tests/test_phi0_streams.py compiles it with g++
// (tests/harness/message_stream_dump.cpp).
//
// A chunk is 32 output rows of one of the block's six matrices; a stream is a list of chunks.  MSG_ALL is the message kernels' stream.
// The layer-0 phi table path cuts it in two: MSG_W, the filter branch's chunks in the walk order of the pair kernel's
// table build, and MSG_PHI, the phi branch's in the table kernel's.  Together they hold every chunk of MSG_ALL exactly once.
#pragma once
#include <vector>

namespace ti {

enum MsgMatrix { MSG_W_W0 = 0, MSG_W_W1 = 1, MSG_PHI_W0E = 2 /* the e half of phi.W0 */, MSG_PHI_W1 = 3, MSG_PHI_W2 = 4, MSG_W_W2 = 5 };
enum MsgPart { MSG_ALL = 0, MSG_W = 1, MSG_PHI = 2 };
struct MsgChunk { int matrix, row0; };      // rows row0 .. row0 + 31 of the matrix

inline bool msg_is_phi(int matrix) { return matrix == MSG_PHI_W0E || matrix == MSG_PHI_W1 || matrix == MSG_PHI_W2; }

// NB = n_features / 32.  Output slices of W2 (5 F rows): 0 gates, 1 scale_edge_dir, 2 ds, 3 de, 4 cross gates, consumed per 32 features
// in the order ds, de, scale_edge_dir, gates, cross gates; the last layer has no de slice, the first neither kind of gates.
inline std::vector<MsgChunk> message_chunks(int NB, bool first, bool last, MsgPart part)
{
    std::vector<MsgChunk> out;
    auto put = [&](int matrix, int row0) {
        if (part == MSG_ALL || (part == MSG_PHI) == msg_is_phi(matrix)) out.push_back(MsgChunk{matrix, row0});
    };
    for (int m : {MSG_W_W0, MSG_W_W1, MSG_PHI_W0E, MSG_PHI_W1})
        for (int nbo = 0; nbo < NB; ++nbo) put(m, 32 * nbo);
    const int F = 32 * NB;
    for (int nbo = 0; nbo < NB; ++nbo)
        for (int c : {2, 3, 1, 0, 4}) {
            if (c == 3 && last) continue;
            if ((c == 0 || c == 4) && first) continue;
            put(MSG_PHI_W2, c * F + 32 * nbo);
            put(MSG_W_W2, c * F + 32 * nbo);
        }
    return out;
}

}  // namespace ti
