#!/usr/bin/env python
"""Generate tests/golden/zmat_reference.npz: the reference's Z-matrix functions on seeded, well-conditioned inputs.

    python tests/golden/make_golden_zmat.py --reference /path/to/thermodynamic-interpolation

Only imports from the reference checkout (mdqm9/analysis/utils/z_matrix.py: construct_z_matrix_batch, deconstruct_z_matrix_batch
with jacobian=True, compute_jacobian_batch, correct_conf_indexes; mdqm9/analysis/utils/sensititvity.py: filter_iqr) and records what
they return, at generation time only.

Cases A in {4, 5, 18, 25}, 64 conformations each, over random trees whose references come from the from_bonds rule
(tests/zmat_numpy.py); the atoms are relabelled at random, so `order` is not the identity, and the cases cover both branches of the
placement of the third atom (ref[2][0] == 0 and != 0).  The inputs are generated from internal coordinates d in [0.9, 1.6],
a in [1.2, 2.6], |t| <= 3.1; the coordinates of a case are the fp64 restatement's placement of those, rounded to fp32.  Asserted for
every case: sin a >= 0.3, |n| >= 0.05 |p2 - p1| before normalisation, constructed torsions at least 1e-3 from +-pi.  Per case and
quantity the file stores e_ref = max |reference - fp64 restatement| and asserts e_ref <= 1e-3 (1 + |value|): a condition on the
inputs (the reference computes in fp32), not a tolerance of any test.  The validity cases hold the three pi32 edge values, a NaN and
a d = 0."""
import argparse
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import zmat_numpy as zn  # noqa: E402

CASES = [(4, 0), (4, 1), (5, 0), (5, 1), (18, 1), (25, 0)]          # (A, wanted ref[2][0])


def random_tree(A, rs):
    """bonds of a random tree over relabelled atoms: node i hangs on a random earlier node"""
    label = rs.permutation(A)
    return np.array([[label[i], label[rs.randint(0, i)]] for i in range(1, A)], np.int64), int(label[0])


def topology(A, want, rs):
    for _ in range(1000):
        bonds, root = random_tree(A, rs)
        order, ref = zn.from_bonds(bonds, A, root)
        if int(ref[2][0]) == want and not (order == np.arange(A)).all():
            return bonds, root, order, ref
    raise RuntimeError("no tree found")


def internal(A, B, rs):
    z = np.zeros((B, A - 1, 3))
    z[:, :, 0] = rs.uniform(0.9, 1.6, (B, A - 1))
    z[:, 1:, 1] = rs.uniform(1.2, 2.6, (B, A - 2))
    z[:, 2:, 2] = rs.uniform(-3.1, 3.1, (B, A - 3))
    return z.astype(np.float32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", default=os.environ.get("TI_REFERENCE"), required=os.environ.get("TI_REFERENCE") is None)
    ap.add_argument("--out", default=os.path.join(HERE, "zmat_reference.npz"))
    args = ap.parse_args()
    import torch
    sys.path.insert(0, args.reference)
    from mdqm9.analysis.utils import z_matrix as rz
    from mdqm9.analysis.utils import sensititvity as rsens

    out = {"cases": np.array([a for a, _ in CASES], np.int32)}
    cap = lambda e, v: e <= 1e-3 * (1.0 + np.abs(v).max())
    for ci, (A, want) in enumerate(CASES):
        rs = np.random.RandomState(1000 + ci)
        for attempt in range(200):
            bonds, root, order, ref = topology(A, want, rs)
            z_in = internal(A, 64, rs)
            x64, logdet64, _, cond = zn.deconstruct(z_in, order, ref)
            x = x64.astype(np.float32)
            z64 = zn.construct(x, order, ref)
            tors = z64[:, 2:, 2]
            if cond.min() >= 0.05 and (np.pi - np.abs(tors)).min() >= 1e-3:
                break
        else:
            raise RuntimeError(f"case {ci}: no well-conditioned draw")
        assert np.sin(z_in[:, 1:, 1].astype(np.float64)).min() >= 0.3
        assert cond.min() >= 0.05 and (np.pi - np.abs(tors)).min() >= 1e-3
        ref_list = [tuple(int(v) for v in r) for r in ref]
        # construct: the reference on the sorted atoms (results_00031.py gen_z_matrix)
        z_ref = rz.construct_z_matrix_batch(torch.tensor(x[:, order, :], dtype=torch.float32), ref_list).numpy()
        # deconstruct: the reference places the sorted atoms; stored in the caller's numbering
        xs_ref, ld_ref = rz.deconstruct_z_matrix_batch(torch.tensor(z_in), ref_list, jacobian=True)
        ld2_ref = rz.compute_jacobian_batch(torch.tensor(z_in), ref_list).numpy()
        x_ref = np.zeros((64, A, 3), np.float32)
        x_ref[:, order] = xs_ref.numpy()
        ld_ref = ld_ref.numpy()
        e_z = float(np.abs(z_ref - z64).max())
        e_x = float(np.abs(x_ref - x64).max())
        e_ld = float(max(np.abs(ld_ref - logdet64).max(), np.abs(ld2_ref - logdet64).max()))
        assert cap(e_z, z64) and cap(e_x, x64) and cap(e_ld, logdet64), (ci, e_z, e_x, e_ld)
        pre = f"c{ci}_"
        out.update({pre + "bonds": bonds.astype(np.int32), pre + "root": np.int32(root), pre + "order": order.astype(np.int32),
                    pre + "ref": ref.astype(np.int32), pre + "x": x, pre + "z_in": z_in, pre + "z_ref": z_ref.astype(np.float32),
                    pre + "x_ref": x_ref, pre + "logdet_ref": ld_ref.astype(np.float32), pre + "logdet2_ref": ld2_ref.astype(np.float32),
                    pre + "e_ref": np.array([e_z, e_x, e_ld])})
        print(f"case {ci}: A = {A}, ref[2][0] = {int(ref[2][0])}, e_ref z {e_z:.2e} xyz {e_x:.2e} (scale {np.abs(x64).max():.1f}) "
              f"logdet {e_ld:.2e}, min |n|/|p2-p1| {cond.min():.3f}")

    # validity: A = 4 rows that are fine except for one entry
    pi32 = np.float32(np.pi)
    base = np.array([[1.0, 0.0, 0.0], [1.2, 1.9, 0.0], [1.1, 2.0, 0.5]], np.float32)
    edits = [None, (1, 1, pi32), (2, 2, pi32), (2, 2, -pi32), (2, 1, np.float32(np.nan)), (1, 0, np.float32(0.0)),
             (2, 1, np.nextafter(pi32, np.float32(4.0))), (1, 1, np.float32(-1e-6)), (0, 0, np.float32(-1.0)), (2, 2, np.float32(np.nan)),
             (2, 2, np.nextafter(-pi32, np.float32(0.0)))]
    zv = np.stack([base.copy() for _ in edits])
    for i, e in enumerate(edits):
        if e is not None:
            zv[i, e[0], e[1]] = e[2]
    good = rz.correct_conf_indexes(torch.tensor(zv))
    mask = np.zeros(len(edits), np.uint8)
    mask[good] = 1
    assert mask.tolist() == [1, 1, 1, 0, 0, 0, 0, 0, 0, 0, 1], mask
    out.update(valid_z=zv, valid_mask=mask)

    # filter_iqr on exp(logw - max)
    rs = np.random.RandomState(7)
    logw = (rs.standard_normal(500) * 2.0).astype(np.float32)
    logw[::50] += 6.0                                     # a few heavy weights for the filter to cut
    w = np.exp(logw.astype(np.float64) - logw.astype(np.float64).max())
    ks = np.array([0.5, 1.5, 10.0, 100.0])
    out.update(iqr_logw=logw, iqr_k=ks, iqr_keep=np.stack([rsens.filter_iqr(w, k=float(k)) for k in ks]).astype(np.uint8))
    assert 0 < out["iqr_keep"][0].sum() < out["iqr_keep"][-1].sum() <= 500
    np.savez_compressed(args.out, **out)
    print("wrote", args.out, os.path.getsize(args.out), "bytes; iqr kept", out["iqr_keep"].sum(axis=1))


if __name__ == "__main__":
    main()
