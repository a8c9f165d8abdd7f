"""Force fields for the on-device energy evaluator (include/ti_hip.h ti_obs_ff_set / ti_obs_ff_energy).

``ForceField`` is a plain container of what the reference's mdqm9/analysis/eval_energy.py evaluates through OpenMM for one species:
the HarmonicBondForce, HarmonicAngleForce, PeriodicTorsionForce and NonbondedForce (NoCutoff, vacuum) of
``forcefield.createSystem(topology)``.  Units are OpenMM's: kJ/mol, nm, radians, elementary charges.

    bonds     idx [nb, 2] (i, j),        par [nb, 2] (r0, k)            E = k (r - r0)^2 / 2
    angles    idx [na, 3] (i, j, k),     par [na, 2] (theta0, k)        E = k (theta - theta0)^2 / 2, theta at j
    torsions  idx [nt, 4] (i, j, k, l),  par [nt, 3] (n, phase, k)      E = k (1 + cos(n phi - phase)), n an integer in 1..6
    particles [A, 3] (q, sigma, eps)     exceptions [ne, 5] (i, j, qq, sigma, eps)
    pairs     E = 4 eps ((sigma / r)^12 - (sigma / r)^6) + coulomb qq / r over the dense table ``pair_table(A)``

``from_openmm_xml`` reads what ``openmm.XmlSerializer.serialize(system)`` writes -- the user's one-time export of the ``system``
eval_energy.py:39 builds.  OpenMM itself is not needed (and its parity is unpinned: DESIGN.md §2).
"""
from __future__ import annotations

import os
import xml.etree.ElementTree as ET

import numpy as np

from . import _lib

COULOMB = _lib.FF_COULOMB         # OpenMM's ONE_4PI_EPS0, kJ nm / (mol e^2)


def pair_row(i, j, A):
    """Row of the pair i < j in the dense table of A atoms: i (2A - i - 1) / 2 + (j - i - 1)."""
    return i * (2 * A - i - 1) // 2 + (j - i - 1)


def _table(a, cols, dtype, what):
    a = np.zeros((0, cols), dtype) if a is None else np.asarray(a)
    if a.size == 0:
        a = a.reshape(0, cols)
    if a.ndim != 2 or a.shape[1] != cols:
        raise ValueError(f"{what} must be [n, {cols}], got {a.shape}")
    if dtype is np.int32 and a.size and not np.array_equal(a, np.round(np.asarray(a, np.float64))):
        raise ValueError(f"{what} must hold integers")
    return np.ascontiguousarray(a, dtype)


class ForceField:
    """The tables of one species (module docstring).  Index ranges, repeated atoms, caps and parameter signs are the library's to
    check (ti_obs_ff_set): they depend on the engine."""

    def __init__(self, bond_idx=None, bond_par=None, angle_idx=None, angle_par=None, torsion_idx=None, torsion_par=None,
                 particles=None, exceptions=None, coulomb=COULOMB, masses=None, has_constraints=False):
        self.bond_idx, self.bond_par = _table(bond_idx, 2, np.int32, "bond_idx"), _table(bond_par, 2, np.float64, "bond_par")
        self.angle_idx, self.angle_par = _table(angle_idx, 3, np.int32, "angle_idx"), _table(angle_par, 2, np.float64, "angle_par")
        self.torsion_idx, self.torsion_par = _table(torsion_idx, 4, np.int32, "torsion_idx"), _table(torsion_par, 3, np.float64, "torsion_par")
        self.particles = _table(particles, 3, np.float64, "particles")
        self.exceptions = _table(exceptions, 5, np.float64, "exceptions")
        self.coulomb = float(coulomb)
        # for dynamics only (PainnEngine.langevin): [A] float64 amu or None, and whether the source listed constraints (not integrated)
        self.masses = None if masses is None else np.ascontiguousarray(masses, np.float64).reshape(-1)
        self.has_constraints = bool(has_constraints)
        if self.masses is not None and len(self.masses) != len(self.particles):
            raise ValueError(f"masses must be [{len(self.particles)}], got {self.masses.shape}")
        for name in ("bond", "angle", "torsion"):
            if len(getattr(self, name + "_idx")) != len(getattr(self, name + "_par")):
                raise ValueError(f"{name}_idx and {name}_par differ in length")

    @property
    def n_atoms(self):
        return int(self.particles.shape[0])

    def pair_table(self, A=None):
        """[A (A - 1) / 2, 3] float64 (qq, sigma, eps), row ``pair_row(i, j, A)`` for i < j.  Lorentz-Berthelot for the pairs
        without an exception: qq = q_i q_j, sigma = (sigma_i + sigma_j) / 2, eps = sqrt(eps_i eps_j); an exception replaces its
        pair (the last one if a pair is listed twice).  Excluded pairs (qq = eps = 0) are the rows the kernel skips."""
        A = self.n_atoms if A is None else int(A)
        if A != self.n_atoms:
            raise ValueError(f"the force field has {self.n_atoms} particles, the table was asked for {A} atoms")
        i, j = np.triu_indices(A, 1)                                     # row-major i < j: the row order above
        q, sig, eps = self.particles[:, 0], self.particles[:, 1], self.particles[:, 2]
        out = np.stack([q[i] * q[j], (sig[i] + sig[j]) / 2.0, np.sqrt(eps[i] * eps[j])], axis=1)
        for e in self.exceptions:
            a, b = int(e[0]), int(e[1])
            if a != e[0] or b != e[1] or not (0 <= a < A and 0 <= b < A) or a == b:
                raise ValueError(f"exception ({e[0]:g}, {e[1]:g}) does not name two atoms of 0..{A - 1}")
            out[pair_row(min(a, b), max(a, b), A)] = e[2:5]
        return np.ascontiguousarray(out)

    @classmethod
    def from_openmm_xml(cls, path_or_text, coulomb=COULOMB):
        """The force field of a serialized OpenMM System (XmlSerializer.serialize(system)); a path or the XML text.  Reads
        HarmonicBondForce, HarmonicAngleForce, PeriodicTorsionForce and NonbondedForce and the particle masses (``masses``), ignores
        CMMotionRemover and -- for the energies -- <Constraints>, whose presence is recorded (``has_constraints``), and raises
        ValueError -- naming the offender -- for anything that would change the energy and is not evaluated: another force type, a
        NonbondedForce method other than 0 (NoCutoff), global parameters or parameter offsets."""
        text = path_or_text
        if isinstance(text, bytes):
            text = text.decode()
        if isinstance(text, os.PathLike) or "<" not in str(text):
            with open(text) as f:
                text = f.read()
        root = ET.fromstring(text)
        forces = root.find("Forces")
        if root.tag != "System" or forces is None:
            raise ValueError("not a serialized OpenMM System (no <System><Forces>)")
        system_particles = root.findall("./Particles/Particle")
        n_particles = len(system_particles)
        masses = [float(p.attrib["mass"]) for p in system_particles] if all("mass" in p.attrib for p in system_particles) else None
        constraints = root.find("Constraints")
        has_constraints = constraints is not None and len(list(constraints)) > 0
        tab = {k: [] for k in ("bi", "bp", "ai", "ap", "ti", "tp", "pa", "ex")}
        seen_nb = False
        num = lambda el, k: float(el.attrib[k])
        for f in forces.findall("Force"):
            kind = f.attrib.get("type", "")
            if kind == "CMMotionRemover":
                continue
            if kind == "HarmonicBondForce":
                for b in f.findall("./Bonds/Bond"):
                    tab["bi"].append([int(b.attrib["p1"]), int(b.attrib["p2"])])
                    tab["bp"].append([num(b, "d"), num(b, "k")])
            elif kind == "HarmonicAngleForce":
                for a in f.findall("./Angles/Angle"):
                    tab["ai"].append([int(a.attrib[k]) for k in ("p1", "p2", "p3")])
                    tab["ap"].append([num(a, "a"), num(a, "k")])
            elif kind == "PeriodicTorsionForce":
                for t in f.findall("./Torsions/Torsion"):
                    tab["ti"].append([int(t.attrib[k]) for k in ("p1", "p2", "p3", "p4")])
                    tab["tp"].append([num(t, "periodicity"), num(t, "phase"), num(t, "k")])
            elif kind == "NonbondedForce":
                if seen_nb:
                    raise ValueError("more than one NonbondedForce")
                seen_nb = True
                if int(f.attrib.get("method", "0")) != 0:
                    raise ValueError(f"NonbondedForce method {f.attrib.get('method')} is not 0 (NoCutoff): cutoffs and PME are not evaluated")
                for group, item in (("GlobalParameters", "Parameter"), ("ParticleOffsets", "Offset"), ("ExceptionOffsets", "Offset")):
                    g = f.find(group)
                    if g is not None and len(list(g)):
                        raise ValueError(f"NonbondedForce has a non-empty {group}: parameter offsets are not evaluated")
                for p in f.findall("./Particles/Particle"):
                    tab["pa"].append([num(p, "q"), num(p, "sig"), num(p, "eps")])
                for e in f.findall("./Exceptions/Exception"):
                    tab["ex"].append([int(e.attrib["p1"]), int(e.attrib["p2"]), num(e, "q"), num(e, "sig"), num(e, "eps")])
            else:
                raise ValueError(f"force type {kind!r} is not evaluated (HarmonicBondForce, HarmonicAngleForce, PeriodicTorsionForce, "
                                 "NonbondedForce; CMMotionRemover is ignored)")
        if not seen_nb:
            raise ValueError("the system has no NonbondedForce")
        if n_particles and len(tab["pa"]) != n_particles:
            raise ValueError(f"the system has {n_particles} particles, its NonbondedForce {len(tab['pa'])}")
        return cls(tab["bi"], tab["bp"], tab["ai"], tab["ap"], tab["ti"], tab["tp"], tab["pa"], tab["ex"], coulomb=coulomb,
                   masses=masses if n_particles else None, has_constraints=has_constraints)
