"""The two layer-0 streams of the phi table path (csrc/message_stream.hpp: the w chunks alone, the phi chunks alone) hold together
exactly the chunks of the message kernels' layer-0 stream, each once, and each in the order its kernel walks them.  Checked on the
CPU: the chunk lists painn_pack.hip packs from are printed by a small g++ harness (tests/harness/message_stream_dump.cpp)."""
import os
import subprocess
from collections import Counter

import pytest

from conftest import ROOT

W_W0, W_W1, PHI_W0E, PHI_W1, PHI_W2, W_W2 = range(6)


@pytest.fixture(scope="module")
def chunks(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("msg") / "message_stream_dump")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-o", exe, os.path.join(ROOT, "tests", "harness", "message_stream_dump.cpp")])

    def run(NB, first, last):
        out = subprocess.run([exe], input=f"{NB} {int(first)} {int(last)}\n", capture_output=True, text=True, check=True).stdout.split("\n")
        return [[tuple(int(v) for v in tok.split(":")) for tok in line.split()] for line in out[:3]]

    return run


@pytest.mark.parametrize("last", [False, True])
@pytest.mark.parametrize("NB", [1, 2, 4])
def test_layer0_streams_partition_the_message_stream(chunks, NB, last):
    F = 32 * NB
    every, w, phi = chunks(NB, True, last)
    slices = [2, 1] if last else [2, 3, 1]                        # layer 0: ds, de (unless it is also the last), scale_edge_dir; no gates
    assert len(every) == 4 * NB + 2 * len(slices) * NB and len(set(every)) == len(every)
    assert Counter(w) + Counter(phi) == Counter(every) and not set(w) & set(phi)
    assert all(m in (W_W0, W_W1, W_W2) for m, _ in w) and all(m in (PHI_W0E, PHI_W1, PHI_W2) for m, _ in phi)
    # walk orders: the hidden layers by 32 output rows, then per 32 features the slices in consumption order
    hidden = lambda a, b: [(a, 32 * n) for n in range(NB)] + [(b, 32 * n) for n in range(NB)]
    out = lambda m: [(m, c * F + 32 * n) for n in range(NB) for c in slices]
    assert w == hidden(W_W0, W_W1) + out(W_W2)
    assert phi == hidden(PHI_W0E, PHI_W1) + out(PHI_W2)
    # and the split keeps the relative order of the stream it came from
    assert [c for c in every if c in set(w)] == w and [c for c in every if c in set(phi)] == phi


@pytest.mark.parametrize("first,last", [(False, False), (False, True), (True, False), (True, True)])
def test_message_stream_order_is_the_kernels(chunks, first, last):
    """The full stream as the message kernels consume it: w.W0, w.W1, phi.W0 (e half), phi.W1, then per 32 features (phi.W2, w.W2) of
    ds, de, scale_edge_dir, gates, cross gates -- without de in the last layer and without either kind of gates in the first."""
    NB, F = 2, 64
    every = chunks(NB, first, last)[0]
    want = [(m, 32 * n) for m in (W_W0, W_W1, PHI_W0E, PHI_W1) for n in range(NB)]
    for n in range(NB):
        for c in (2, 3, 1, 0, 4):
            if (c == 3 and last) or (c in (0, 4) and first):
                continue
            want += [(PHI_W2, c * F + 32 * n), (W_W2, c * F + 32 * n)]
    assert every == want
