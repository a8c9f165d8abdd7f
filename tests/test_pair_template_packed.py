"""The packed pair-major edge template (csrc/pair_template.hpp: build_pair_template_packed), checked on the CPU: tile blocks first,
held to the invariants the tile path of the kernel relies on (the checker of test_pair_template.py, restated here for the leading
blocks), then general blocks of 16 unrelated pairs, held to the rules that let the kernel add their rows one by one.  The old
builder is stage 1 of the new one and the template TI_PAIR_PACKED=0 keeps: its output is pinned word for word by the hashes of
tests/golden/pair_template_old_sha256.json, taken before the builder was split into stages."""
import hashlib
import json
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT, pkg

COMPLETE = (2, 3, 5, 9, 12, 17, 18, 25, 32)


def _text(A, src, dst, et):
    return f"{A} {len(src)}\n" + "".join(f"{s} {d} {t}\n" for s, d, t in zip(src, dst, et))


@pytest.fixture(scope="module")
def exes(tmp_path_factory):
    d = tmp_path_factory.mktemp("pair_packed")
    out = {}
    for name in ("pair_template_dump", "pair_template_packed_dump"):
        out[name] = str(d / name)
        subprocess.check_call(["g++", "-O1", "-std=c++17", "-o", out[name], os.path.join(ROOT, "tests", "harness", name + ".cpp")])
    return out


def _parse(text, A, packed):
    out = text.split("\n")
    if out[0].strip() == "none":
        return None
    head = [int(v) for v in out[0].split()[1:]]
    G, nblk = head[0], head[1]
    n_tile = head[2] if packed else nblk
    rows = np.array(out[1].split(), dtype=np.int64).reshape(nblk, 16)
    slots = np.array(out[2].split(), dtype=np.int64).reshape(nblk, 16)
    pos = np.array(out[3].split(), dtype=np.int64).reshape(G, A, A)
    return G, nblk, n_tile, rows, slots, pos


def _run(exe, A, src, dst, et):
    return subprocess.run([exe], input=_text(A, src, dst, et), capture_output=True, text=True, check=True).stdout


def sparse_graphs():
    rs = np.random.RandomState(3)                             # the four graphs of test_pair_template.py, drawn the same way
    for A, p in ((9, 0.5), (18, 0.3), (25, 0.6), (18, 0.9)):
        adj = np.triu(rs.rand(A, A) < p, 1)
        for a in range(A - 1):
            adj[a, a + 1] = True
        i, j = np.nonzero(adj)
        ty = rs.randint(0, 4, i.size)
        src, dst, et = np.concatenate([i, j]), np.concatenate([j, i]), np.concatenate([ty, ty])
        order = np.lexsort((dst, src))
        yield A, [int(v) for v in src[order]], [int(v) for v in dst[order]], [int(v) for v in et[order]]


def graphs():
    syn = pkg().synthetic
    for A in COMPLETE:
        src, dst, et = syn.fully_connected_template(A)
        yield f"complete_{A}", A, [int(v) for v in src], [int(v) for v in dst], [int(v) for v in et]
    for k, (A, src, dst, et) in enumerate(sparse_graphs()):
        yield f"sparse_{k}", A, src, dst, et


def check_packed(A, src, dst, et, tpl):
    """every invariant of a packed template; returns the valid rows of each block"""
    G, nblk, n_tile, rows, slots, pos = tpl
    assert 0 <= n_tile <= nblk and 1 <= G <= 8
    etype = {(s, d): t for s, d, t in zip(src, dst, et)}
    seen, owner = set(), {}
    key_of = lambda w: (int(w) >> 8 & 0x3FFFFF, int(w) & 255)
    for b in range(n_tile):                                   # tile blocks: the checker of test_pair_template.py
        I, J = slots[b, :4], slots[b, 4:8]
        assert np.all(slots[b, 8:] == -1)
        keys = lambda s: [key_of(w) for w in s if w >= 0]
        assert len(set(keys(I))) == len(keys(I)) and len(set(keys(J))) == len(keys(J))
        for k in range(8):
            if slots[b, k] >= 0:
                owner[8 * b + k] = key_of(slots[b, k])
        for a in range(4):
            for c in range(4):
                w = int(rows[b, 4 * a + c])
                mI, aI, mJ, aJ, ty = w >> 1 & 7, w >> 4 & 31, w >> 9 & 7, w >> 12 & 31, w >> 17 & 3
                assert mI < G and mJ < G and aI < A and aJ < A
                if I[a] >= 0:
                    assert key_of(I[a]) == (mI, aI)
                if J[c] >= 0:
                    assert key_of(J[c]) == (mJ, aJ)
                if w & 1:
                    assert I[a] >= 0 and J[c] >= 0 and mI == mJ and (aI, aJ) in etype and etype[(aI, aJ)] == ty
                    for e in ((mI, aI, aJ), (mI, aJ, aI)):
                        assert e not in seen
                        seen.add(e)
                    assert pos[mI, aI, aJ] == (2 * b) * 16 + 4 * a + c and pos[mI, aJ, aI] == (2 * b + 1) * 16 + 4 * a + c
    walk = [8 * b + k for b in range(n_tile) for k in (4, 5, 6, 7, 0, 1, 2, 3) if 8 * b + k in owner]
    first = {}
    for place in walk:
        first.setdefault(owner[place], place)
    marked = {8 * b + k for b in range(n_tile) for k in range(16) if slots[b, k] >= 0 and int(slots[b, k]) >> 30 & 1}
    assert marked == set(first.values())
    slotted = set(owner.values())                             # atoms that own a tile slot: all of them precede the general blocks
    for b in range(n_tile, nblk):                             # general blocks come last: no slots, hence no first touch
        assert np.all(slots[b] == -1)
        assert np.any(rows[b] & 1)                            # no general block without a pair
        for r in range(16):
            w = int(rows[b, r])
            mI, aI, mJ, aJ, ty = w >> 1 & 7, w >> 4 & 31, w >> 9 & 7, w >> 12 & 31, w >> 17 & 3
            assert mI < G and mJ < G and aI < A and aJ < A    # invalid rows name existing atoms of the group
            if w & 1:
                assert mI == mJ and (aI, aJ) in etype and etype[(aI, aJ)] == ty
                assert (mI, aI) in slotted and (mJ, aJ) in slotted
                for e in ((mI, aI, aJ), (mI, aJ, aI)):
                    assert e not in seen
                    seen.add(e)
                assert pos[mI, aI, aJ] == (2 * b) * 16 + r and pos[mI, aJ, aI] == (2 * b + 1) * 16 + r
    assert seen == {(m, s, d) for m in range(G) for s, d in zip(src, dst)}
    assert np.count_nonzero(pos >= 0) == len(seen)
    return (rows & 1).sum(axis=1)


def test_packed_templates(exes):
    golden = json.load(open(os.path.join(ROOT, "tests", "golden", "pair_template_old_sha256.json")))
    for name, A, src, dst, et in graphs():
        old_text = _run(exes["pair_template_dump"], A, src, dst, et)
        assert hashlib.sha256(old_text.encode()).hexdigest() == golden[name], name          # the 7-argument builder, word for word
        old = _parse(old_text, A, False)
        tpl = _parse(_run(exes["pair_template_packed_dump"], A, src, dst, et), A, True)
        assert tpl is not None
        valid = check_packed(A, src, dst, et, tpl)
        G, nblk, n_tile = tpl[:3]
        pairs = len(src) // 2
        assert nblk / G <= old[1] / old[0] + 1e-12, name
        assert nblk >= -(-G * pairs // 16), name
        if name == "complete_18":
            assert (G, nblk, n_tile) == (4, 39, 36)
            assert np.all(valid[:36] == 16) and valid[36:].sum() == 36
        if name in ("complete_2", "complete_3", "complete_5"):                                # no atom is eligible for a general row
            assert n_tile == nblk
        if name == "complete_12":                                                             # the generic pass alone: groups of 8
            assert (G, nblk, n_tile) == (8, 33, 24)
        # a general block is weighed at 1.6 tiles (pair_template.hpp PAIR_GENERAL_WEIGHT): never dearer than the tile-only template
        assert (n_tile + 1.6 * (nblk - n_tile)) / G <= old[1] / old[0] + 1e-9, name


def test_refusals(exes):
    for A, src, dst, et in ((3, [0, 1, 1], [1, 0, 2], [0, 0, 0]), (3, [0, 1, 1, 2], [1, 0, 2, 1], [0, 1, 0, 0]), (3, [0, 1, 0, 2], [1, 0, 2, 2], [0, 0, 0, 0])):
        assert _parse(_run(exes["pair_template_packed_dump"], A, src, dst, et), A, True) is None
        assert _parse(_run(exes["pair_template_dump"], A, src, dst, et), A, False) is None
