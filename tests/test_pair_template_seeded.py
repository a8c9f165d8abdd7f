"""The `seeded` property of a pair-major template (csrc/pair_template.hpp: pair_template_seeded), checked on the CPU.  A packed
template is seeded when the valid rows of its general blocks name every atom of every molecule of the group exactly once: a general
launch that runs before the tile launch then meets every accumulator row as its first contribution of the layer and may store it,
and the tile blocks only add (csrc/painn_pair_kernel.hpp).  The builder computes the property; nothing assumes it.  Here it is
recounted from the row words alone, for the headline molecule (K18: 36 tiles + 3 general blocks of the 36 twin pairs of 4 molecules),
the tile-only template, the other complete graphs and a template that lost one twin row."""
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT, pkg

SIZES = (9, 12, 17, 18, 25, 32)


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("pair_seeded") / "pair_template_seeded_dump")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-o", out, os.path.join(ROOT, "tests", "harness", "pair_template_seeded_dump.cpp")])
    return out


def template(exe, A, kind, drop=-1):
    """(G, nblk, n_tile, seeded as built, seeded as rechecked after `drop`, row words [nblk, 16]) of the complete graph on A atoms"""
    src, dst, et = pkg().synthetic.fully_connected_template(A)
    text = f"{A} {len(src)}\n" + "".join(f"{int(s)} {int(d)} {int(t)}\n" for s, d, t in zip(src, dst, et))
    out = subprocess.run([exe, kind, str(drop)], input=text, capture_output=True, text=True, check=True).stdout.split("\n")
    assert out[0].split()[0] == "ok"
    G, nblk, n_tile, seeded, rechecked = (int(v) for v in out[0].split()[1:])
    rows = np.array(out[1].split(), dtype=np.int64).reshape(nblk, 16)
    return G, nblk, n_tile, bool(seeded), bool(rechecked), rows


def recount(A, G, n_tile, rows):
    """times every (molecule, atom) of the group is named by a valid general row; the number of invalid general rows"""
    hits = np.zeros((G, A), np.int64)
    invalid = 0
    for w in rows[n_tile:].reshape(-1):
        w = int(w)
        if not w & 1:
            invalid += 1
            continue
        mI, aI, mJ, aJ = w >> 1 & 7, w >> 4 & 31, w >> 9 & 7, w >> 12 & 31
        hits[mI, aI] += 1
        hits[mJ, aJ] += 1
    return hits, invalid


def seeded_by_count(A, G, nblk, n_tile, rows):
    hits, _ = recount(A, G, n_tile, rows)
    return n_tile < nblk and bool(np.all(hits == 1))


def test_headline_template_is_seeded(exe):
    G, nblk, n_tile, seeded, rechecked, rows = template(exe, 18, "packed")
    assert (G, nblk, n_tile) == (4, 39, 36)
    hits, invalid = recount(18, G, n_tile, rows)
    assert hits.shape == (4, 18) and hits.size == 72 and np.all(hits == 1) and invalid == 12
    assert seeded and rechecked
    for w in rows[n_tile:].reshape(-1):                      # the general rows are the twin pairs (2a, 2a + 1)
        if int(w) & 1:
            aI, aJ = int(w) >> 4 & 31, int(w) >> 12 & 31
            assert aI % 2 == 0 and aJ == aI + 1


@pytest.mark.parametrize("A", SIZES)
def test_builder_agrees_with_a_recount(exe, A):
    for kind in ("packed", "tile"):
        G, nblk, n_tile, seeded, rechecked, rows = template(exe, A, kind)
        assert seeded == rechecked == seeded_by_count(A, G, nblk, n_tile, rows), (A, kind)
        if kind == "tile":
            assert n_tile == nblk and not seeded                 # tile-only templates never have it
        print(f"A {A} {kind}: G {G}, {n_tile} tiles + {nblk - n_tile} general blocks, seeded {seeded}")
        if kind == "packed" and A == 12:                         # the generic packed templates: 24 + 9 and 28 + 3
            assert (G, nblk, n_tile) == (8, 33, 24)
        if kind == "packed" and A == 32:
            assert (nblk, n_tile) == (31, 28)


@pytest.mark.parametrize("drop", [0, 17, 35])
def test_a_template_without_one_twin_row_is_not_seeded(exe, drop):
    G, nblk, n_tile, seeded, rechecked, rows = template(exe, 18, "packed", drop)
    assert seeded and not rechecked                          # seeded as built; not after the row left
    rows[n_tile + drop // 16, drop % 16] &= ~1
    hits, invalid = recount(18, G, n_tile, rows)
    assert invalid == 13 and np.count_nonzero(hits == 0) == 2 and not seeded_by_count(18, G, nblk, n_tile, rows)
