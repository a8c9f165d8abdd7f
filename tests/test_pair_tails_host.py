"""Merged tails of a seeded pair-major template (csrc/pair_template.hpp: pair_template_tails), checked on the CPU.  The 36 twin pairs
of 4 molecules of K18 go 16 to a general block: 16, 16 and 4 valid rows.  The last blocks of S = 4 neighbouring groups then fill one
block between them, and the seeded general launch walks them as one (csrc/painn_pair_kernel.hpp: painn_pair_general_tails_kernel):
merged row j is row j % r of the last block of group j / r.  The property is counted from the row words; here it is recounted, the
map is checked against the storage rows pair_pos names, and templates without the property must report no merge."""
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT, pkg


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("pair_tails") / "pair_tails_dump")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-o", out, os.path.join(ROOT, "tests", "harness", "pair_tails_dump.cpp")])
    return out


def dump(exe, A, src, dst, et, drop=-1):
    """(G, nblk, n_tile, seeded, r, S, rows [nblk, 16], pair_pos [G, A, A], map [16, 3] or empty) of the packed template"""
    text = f"{A} {len(src)}\n" + "".join(f"{int(s)} {int(d)} {int(t)}\n" for s, d, t in zip(src, dst, et))
    out = subprocess.run([exe, str(drop)], input=text, capture_output=True, text=True, check=True).stdout.split("\n")
    assert out[0].split()[0] == "ok"
    G, nblk, n_tile, seeded, r, S = (int(v) for v in out[0].split()[1:])
    rows = np.array(out[1].split(), dtype=np.int64).reshape(nblk, 16)
    pos = np.array(out[2].split(), dtype=np.int64).reshape(G, A, A)
    tmap = np.array(out[3].split(), dtype=np.int64).reshape(-1, 3)
    return G, nblk, n_tile, bool(seeded), r, S, rows, pos, tmap


def complete(A):
    return pkg().synthetic.fully_connected_template(A)


def sparse(A=18, p=0.3, seed=3):
    rs = np.random.RandomState(seed)
    adj = np.triu(rs.rand(A, A) < p, 1)
    for a in range(A - 1):
        adj[a, a + 1] = True
    i, j = np.nonzero(adj)
    ty = rs.randint(0, 4, i.size)
    src, dst, et = np.concatenate([i, j]), np.concatenate([j, i]), np.concatenate([ty, ty])
    order = np.lexsort((dst, src))
    return src[order], dst[order], et[order]


def test_k18_tails_cover_every_valid_row_of_the_last_blocks_once(exe):
    A = 18
    G, nblk, n_tile, seeded, r, S, rows, pos, tmap = dump(exe, A, *complete(A))
    assert (G, nblk, n_tile) == (4, 39, 36) and seeded
    valid_last = np.nonzero(rows[nblk - 1] & 1)[0]
    assert (r, S) == (4, 4) and r == valid_last.size and list(valid_last) == list(range(r))      # counted from the row words: the leading rows
    assert tmap.shape == (16, 3)
    # every valid row of the S last blocks, named (group in super-group, block, row), appears exactly once in the map
    want = {(g, nblk - 1, int(k)) for g in range(S) for k in valid_last}
    got = [tuple(int(v) for v in t) for t in tmap]
    assert len(set(got)) == 16 and set(got) == want
    for j, (g, b, k) in enumerate(got):
        assert (g, b, k) == (j // r, nblk - 1, j % r)                                          # the walk the kernel takes
    # merged rows point at the storage rows pair_pos names: the pair of row word k of the last block sits at (block * 2 + dir) * 16 + k
    for g, b, k in got:
        w = int(rows[b, k])
        assert w & 1
        m, aI, mJ, aJ = w >> 1 & 7, w >> 4 & 31, w >> 9 & 7, w >> 12 & 31
        assert m == mJ
        assert pos[m, aI, aJ] == (b * 2 + 0) * 16 + k and pos[m, aJ, aI] == (b * 2 + 1) * 16 + k
    # and the full general blocks before them are full
    assert np.all(rows[n_tile:nblk - 1] & 1)


@pytest.mark.parametrize("A", [9, 12, 17, 25, 32])
def test_other_complete_graphs_report_no_merge(exe, A):
    G, nblk, n_tile, seeded, r, S, rows, pos, tmap = dump(exe, A, *complete(A))
    assert (r, S) == (0, 0) and tmap.size == 0, (A, G, nblk, n_tile, seeded)


def test_a_sparse_graph_reports_no_merge(exe):
    G, nblk, n_tile, seeded, r, S, rows, pos, tmap = dump(exe, 18, *sparse())
    assert (r, S) == (0, 0) and tmap.size == 0


@pytest.mark.parametrize("drop", [0, 2, 3])
def test_k18_without_one_tail_row_reports_no_merge(exe, drop):
    """A last block that lost a row is no longer seeded (and 3 does not divide 16, and its valid rows no longer lead): no merge."""
    G, nblk, n_tile, seeded, r, S, rows, pos, tmap = dump(exe, 18, *complete(18), drop=drop)
    assert seeded and (r, S) == (0, 0) and tmap.size == 0
