// message_stream_dump.cpp -- test harness (tests/test_phi0_streams.py): prints the chunk lists of the product's message-block streams
// (csrc/message_stream.hpp, the lists painn_pack.hip packs from) for "NB first last" read from stdin, one line per stream --
// all, w only, phi only -- as "matrix:row0" tokens.
#include <cstdio>

#include "../../thermodynamic-interpolation_amd/csrc/message_stream.hpp"

int main()
{
    int NB, first, last;
    if (std::scanf("%d %d %d", &NB, &first, &last) != 3) return 2;
    for (ti::MsgPart part : {ti::MSG_ALL, ti::MSG_W, ti::MSG_PHI}) {
        for (const ti::MsgChunk& c : ti::message_chunks(NB, first != 0, last != 0, part)) std::printf("%d:%d ", c.matrix, c.row0);
        std::printf("\n");
    }
    return 0;
}
