"""Shared implementation of the ambient / latent cPaiNN shells and MoleculeIntegrator mirrors.

The reference batch is a PyG ``Batch``; here any object with the attributes the reference reads is accepted
(/root/reference/mdqm9/thermo/ambient/models/ode_wrapper.py:111-112, graph.py:27, embedding.py:78):
    x0 / x [N,3] f32, atoms | atom_number [N] i64, T0,T1 | T [N], edge_index [2,E] i64 (edge_index[0] = source),
    edge_type [E] i64, batch [N] i64.
Every batch is homogeneous (one species per run); ``split_batch`` verifies that and extracts the
per-molecule template the C ABI takes.  ``split_graph_batch`` also takes batches whose molecules have different edge sets (the
reference's finite-cutoff radius graphs): a superset template plus a per-molecule edge mask.
"""
from __future__ import annotations

import numpy as np

from .. import engine as _engine
from .. import observables as _obs
from .. import synthetic as _syn
from .. import weights as _W
from . import _common as C

DEFAULT_TEMPS = [300, 400, 500, 600, 700, 800, 900, 1000]


def molecule_times(t, B, A, like=None):
    """batch.t (per node [N], or one value) -> one float for a uniform time, else the [B] float32 per-molecule times (a CUDA tensor
    when `like` is one).  A time that varies inside a molecule raises ValueError (the drift takes one time per molecule)."""
    tn = C.to_numpy(t, np.float32).ravel()
    if tn.size == 0:
        raise ValueError("batch.t is empty")
    if np.ptp(tn) == 0.0:
        return float(tn[0])
    if tn.size != B * A:
        raise ValueError(f"batch.t must hold one value or one per node ({B * A}), got {tn.size}")
    per = tn.reshape(B, A)
    if np.any(per != per[:, :1]):
        raise ValueError("batch.t must be constant within each molecule (one time per molecule)")
    tv = np.ascontiguousarray(per[:, 0])
    if C.is_cuda(like):
        import torch
        return torch.from_numpy(tv).to(like.device)
    return tv


def split_batch(batch, atom_key: str):
    """-> (B, A, edge_src[E_m], edge_dst[E_m], edge_type[E_m], atom_ids[A]); raises ValueError for heterogeneous batches."""
    bidx = C.to_numpy(batch.batch, np.int64)
    N = bidx.size
    if N == 0:
        raise ValueError("empty batch")
    B = int(bidx.max()) + 1
    if N % B or not np.array_equal(bidx, np.repeat(np.arange(B), N // B)):
        raise ValueError("batch.batch must be molecule-major with equally sized molecules (one species per run)")
    A = N // B
    ei = C.to_numpy(batch.edge_index, np.int64)
    et = C.to_numpy(batch.edge_type, np.int64)
    atoms = C.to_numpy(getattr(batch, atom_key), np.int64)
    if ei.ndim != 2 or ei.shape[0] != 2 or ei.shape[1] != et.size:
        raise ValueError("edge_index must be [2, E] and edge_type [E]")
    E = ei.shape[1]
    if E % B:
        raise ValueError("edge count is not a multiple of the number of molecules")
    Em = E // B
    off = (np.arange(B, dtype=np.int64) * A)[:, None]
    src = ei[0].reshape(B, Em) - off
    dst = ei[1].reshape(B, Em) - off
    ty = et.reshape(B, Em)
    at = atoms.reshape(B, A)
    if (src != src[0]).any() or (dst != dst[0]).any() or (ty != ty[0]).any() or (at != at[0]).any():
        raise ValueError("molecules of the batch differ in graph or atom ids; the sampler handles one species per batch")
    if Em and (src[0].min() < 0 or src[0].max() >= A or dst[0].min() < 0 or dst[0].max() >= A):
        raise ValueError("edges cross molecule boundaries")
    return B, A, src[0].astype(np.int32), dst[0].astype(np.int32), ty[0].astype(np.int32), at[0].astype(np.int32)


def split_graph_batch(batch, atom_key: str):
    """-> (B, A, edge_src[E], edge_dst[E], edge_type[E], atom_ids[A], mask [B, A] uint32 | None).

    A batch whose molecules all have the same graph (same edges in the same order) gives split_batch's template and mask None.
    Otherwise the template is the superset: the complete directed graph on A atoms sorted by (src, dst), each pair with the type
    the batch shows (type 0 where no molecule has the pair; it is masked everywhere), and bit s of mask[b, d] is set when molecule b
    has the edge s -> d.  Bonds are in every molecule, so the superset is the same for every batch of a species.  Edges are assigned
    to molecules through batch.batch[edge_index[0]]; molecules may hold different numbers of edges.  Raises ValueError when the
    molecules differ in atom ids or give one pair different types."""
    try:
        return (*split_batch(batch, atom_key), None)
    except ValueError:
        pass
    bidx = C.to_numpy(batch.batch, np.int64)
    N = bidx.size
    if N == 0:
        raise ValueError("empty batch")
    B = int(bidx.max()) + 1
    if N % B or not np.array_equal(bidx, np.repeat(np.arange(B), N // B)):
        raise ValueError("batch.batch must be molecule-major with equally sized molecules (one species per run)")
    A = N // B
    if A > 32:
        raise ValueError(f"per-molecule edge sets need A <= 32 atoms, got {A}")
    ei = C.to_numpy(batch.edge_index, np.int64)
    et = C.to_numpy(batch.edge_type, np.int64)
    if ei.ndim != 2 or ei.shape[0] != 2 or ei.shape[1] != et.size:
        raise ValueError("edge_index must be [2, E] and edge_type [E]")
    at = C.to_numpy(getattr(batch, atom_key), np.int64).reshape(B, A)
    if (at != at[0]).any():
        raise ValueError("molecules of the batch differ in atom ids; the sampler handles one species per batch")
    if ei.size and (ei.min() < 0 or ei.max() >= N):
        raise ValueError("edge_index points outside the batch")
    mol = bidx[ei[0]]
    if (bidx[ei[1]] != mol).any():
        raise ValueError("edges cross molecule boundaries")
    src, dst = ei[0] - mol * A, ei[1] - mol * A
    if (src == dst).any():
        raise ValueError("self loops are not supported in batches with per-molecule edge sets")
    if et.size and (et.min() < 0 or et.max() > 3):
        raise ValueError("edge types must be in 0..3 (the edge-type embedding has 4 rows, cpainn.py:70)")
    # every pair's type, from one counting pass per type (vectorised: a batch holds up to ~2e7 edges)
    pair = src * A + dst
    seen = np.stack([np.bincount(pair[et == t], minlength=A * A) > 0 for t in range(4)])      # [type, pair]
    clash = np.nonzero(seen.sum(axis=0) > 1)[0]
    if clash.size:
        raise ValueError(f"molecules of the batch differ in the type of the edge {clash[0] // A} -> {clash[0] % A}")
    ty = np.where(seen.any(axis=0), seen.argmax(axis=0), 0).reshape(A, A)   # type 0 where no molecule has the pair
    # bit s of mask[b, d]: a sum of distinct powers of two below 2^32, exact in the float64 weights of bincount
    mask = np.bincount(mol * A + dst, weights=np.ldexp(1.0, src), minlength=B * A).astype(np.uint32).reshape(B, A)
    if int(np.unpackbits(mask.view(np.uint8)).sum()) != src.size:
        raise ValueError("a molecule of the batch holds an edge twice (coalesce the graph first)")
    s_all, d_all = np.nonzero(~np.eye(A, dtype=bool))                   # (src, dst) order, no self loops
    etype = ty[s_all, d_all]
    return B, A, s_all.astype(np.int32), d_all.astype(np.int32), etype.astype(np.int32), at[0].astype(np.int32), mask


class SpeciesBatch:
    """What split_species_batch returns: the engine's template (B, A, src, dst, etype, atom_ids), the per-molecule graph state
    (mask [B, A] uint32 | None, n_atoms [B] int32 | None, pair_type [B, A, A] uint8 | None) and the index maps between the
    reference's flat node order [N] and the padded [B, A] layout: node_index [N] = b * A + a of every flat node (pads are the
    padded positions no node maps to).  n_atoms is None for a batch split_graph_batch accepts: its result, unchanged."""

    def __init__(self, B, A, src, dst, etype, atom_ids, mask, n_atoms=None, pair_type=None, node_index=None):
        self.B, self.A, self.src, self.dst, self.etype, self.atom_ids, self.mask = B, A, src, dst, etype, atom_ids, mask
        self.n_atoms, self.pair_type = n_atoms, pair_type
        self.node_index = np.arange(B * A, dtype=np.int64) if node_index is None else node_index
        self.N = int(self.node_index.size)

    def template(self):
        return self.B, self.A, self.src, self.dst, self.etype, self.atom_ids, self.mask

    def pad(self, flat, comps, dtype=np.float32):
        """[N, comps] (or [N]) per-node values -> [B, A, comps], zeros on pad atoms; a CUDA tensor stays on its device."""
        if C.is_cuda(flat):
            import torch
            v = flat.detach().to(torch.float32).reshape(self.N, comps)
            if self.n_atoms is None:
                return v.reshape(self.B, self.A, comps).contiguous()
            out = v.new_zeros((self.B * self.A, comps))
            out[torch.from_numpy(self.node_index).to(v.device)] = v
            return out.reshape(self.B, self.A, comps)
        v = C.to_numpy(flat).astype(dtype, copy=False).reshape(self.N, comps)
        if self.n_atoms is None:
            return np.ascontiguousarray(v.reshape(self.B, self.A, comps))
        out = np.zeros((self.B * self.A, comps), dtype)
        out[self.node_index] = v
        return out.reshape(self.B, self.A, comps)

    def unpad(self, padded):
        """[..., B, A, 3] -> [..., N, 3] in the reference's flat node order, pads removed."""
        lead = tuple(padded.shape[:-3])
        flat = padded.reshape(lead + (self.B * self.A, 3))
        if self.n_atoms is None:
            return flat
        if C.is_torch(flat):
            import torch
            return flat[..., torch.from_numpy(self.node_index).to(flat.device), :]
        return flat[..., self.node_index, :]

    def molecule_values(self, per_node):
        """[N] per-node values -> [B, A] with every pad carrying its molecule's first value (so 'constant within a molecule' holds)."""
        v = C.to_numpy(per_node).ravel()
        if self.n_atoms is None or v.size != self.N:
            return v
        first = np.concatenate([[0], np.cumsum(self.n_atoms)[:-1]])
        out = np.repeat(v[first], self.A)
        out[self.node_index] = v
        return out


def _is_mixed(batch) -> bool:
    """True for the two things split_graph_batch refuses and split_species_batch takes: molecules of different size, or equally
    sized molecules that give one atom pair different edge types.  Anything else, malformed batches included, is split_graph_batch's
    to accept or to refuse with its own message."""
    bidx = C.to_numpy(batch.batch, np.int64)
    N = bidx.size
    if N == 0 or bidx.min() < 0:
        return False
    B = int(bidx.max()) + 1
    if N % B or not np.array_equal(bidx, np.repeat(np.arange(B), N // B)):
        return True                                            # sizes differ (or the order is wrong: refused below)
    A = N // B
    ei = C.to_numpy(batch.edge_index, np.int64)
    et = C.to_numpy(batch.edge_type, np.int64)
    if ei.ndim != 2 or ei.shape[0] != 2 or ei.shape[1] != et.size or not ei.size or ei.min() < 0 or ei.max() >= N:
        return False
    if (ei[0] // A != ei[1] // A).any() or et.min() < 0 or et.max() > 3:
        return False
    pair = (ei[0] % A) * A + ei[1] % A
    seen = np.stack([np.bincount(pair[et == t], minlength=A * A) > 0 for t in range(4)])
    return bool((seen.sum(axis=0) > 1).any())


def split_species_batch(batch, atom_key: str) -> SpeciesBatch:
    """A reference-style batch whose molecules may differ in size, graph and edge types -> SpeciesBatch.

    A batch split_graph_batch accepts takes that path unchanged (n_atoms None).  Otherwise A is the largest molecule, the template
    the complete directed graph on A atoms sorted by (src, dst) with type 0 (every present edge carries its own type in pair_type),
    atom_ids = arange(A): the reference's distinguish=True atom features, so every molecule's atoms must be numbered 0 .. n_b - 1
    and A must not exceed the model's n_types.  bit s of mask[b, d] is set when molecule b has the edge s -> d; pads have no bits."""
    if not _is_mixed(batch):
        return SpeciesBatch(*split_graph_batch(batch, atom_key))       # today's path, today's refusals
    bidx = C.to_numpy(batch.batch, np.int64)
    N = bidx.size
    B = int(bidx.max()) + 1
    n_atoms = np.bincount(bidx, minlength=B)
    if bidx.min() < 0 or (n_atoms < 1).any() or not np.array_equal(bidx, np.repeat(np.arange(B), n_atoms)):
        raise ValueError("batch.batch must be molecule-major: 0 .. B - 1 in order, no molecule empty")
    A = int(n_atoms.max())
    if A > 32:
        raise ValueError(f"mixed-species batches need A <= 32 atoms, got {A}")
    first = np.concatenate([[0], np.cumsum(n_atoms)[:-1]])
    local = np.arange(N, dtype=np.int64) - first[bidx]
    atoms = C.to_numpy(getattr(batch, atom_key), np.int64)
    if atoms.shape != (N,) or (atoms != local).any():
        raise ValueError("a mixed-species batch needs every molecule's atom ids to be 0 .. n_atoms - 1 (distinguish=True)")
    ei = C.to_numpy(batch.edge_index, np.int64)
    et = C.to_numpy(batch.edge_type, np.int64)
    if ei.ndim != 2 or ei.shape[0] != 2 or ei.shape[1] != et.size:
        raise ValueError("edge_index must be [2, E] and edge_type [E]")
    if ei.size and (ei.min() < 0 or ei.max() >= N):
        raise ValueError("edge_index points outside the batch")
    mol = bidx[ei[0]]
    if (bidx[ei[1]] != mol).any():
        raise ValueError("edges cross molecule boundaries")
    src, dst = local[ei[0]], local[ei[1]]
    if (src == dst).any():
        raise ValueError("self loops are not supported in mixed-species batches")
    if et.size and (et.min() < 0 or et.max() > 3):
        raise ValueError("edge types must be in 0..3 (the edge-type embedding has 4 rows, cpainn.py:70)")
    mask = np.bincount(mol * A + dst, weights=np.ldexp(1.0, src), minlength=B * A).astype(np.uint32).reshape(B, A)
    if int(np.unpackbits(mask.view(np.uint8)).sum()) != src.size:
        raise ValueError("a molecule of the batch holds an edge twice (coalesce the graph first)")
    pair_type = np.zeros((B, A, A), np.uint8)
    pair_type[mol, src, dst] = et
    s_all, d_all = np.nonzero(~np.eye(A, dtype=bool))
    return SpeciesBatch(B, A, s_all.astype(np.int32), d_all.astype(np.int32), np.zeros(s_all.size, np.int32), np.arange(A, dtype=np.int32),
                        mask, n_atoms.astype(np.int32), pair_type, bidx * A + local)


class PaiNNShell:
    """Weights-only stand-in for the reference ``cPaiNN`` modules (subclasses fix the variant)."""
    VARIANT = _W.AMBIENT
    ATOM_KEY = "atoms"
    COND_KEYS = ("T0", "T1")

    def _init(self, n_features, score_layers, n_types, temp_length, time_length, temperatures):
        self.n_features, self.score_layers, self.n_types = int(n_features), int(score_layers), int(n_types)
        self.temp_length, self.time_length = float(temp_length), float(time_length)
        self.temperatures = list(temperatures)
        self._spec = _W.painn_param_spec(self.VARIANT, self.n_features, self.score_layers, self.n_types)
        self._sd = _syn.make_state_dict(self._spec, seed=0)       # placeholder init; real weights come from load_state_dict
        self._engines, self._device = {}, 0
        self.precision = "f32"                  # 'f16x2': split-fp16 matrix path; 'f16': fp16 storage mode; set before first use
        self.training = False

    # -- torch.nn.Module surface used by the sampling drivers (sample_ambient.py:71-72,125-131)
    def state_dict(self):
        return dict(self._sd)

    def load_state_dict(self, state_dict, strict=True):
        flat = _W.flatten_state_dict(state_dict, self._spec, strict=strict)
        self._sd = _W.unflatten(flat, self._spec)
        self._engines = {}
        return self

    def eval(self):
        self.training = False
        return self

    def to(self, device=None, *a, **k):
        idx = getattr(device, "index", None)
        if isinstance(device, int):
            idx = device
        elif isinstance(device, str) and ":" in device:
            idx = int(device.split(":")[1])
        if idx is not None and idx != self._device:
            self._device, self._engines = idx, {}
        return self

    def parameters(self):
        return iter(self._sd.values())

    def engine_for(self, A, src, dst, ety, atom_ids) -> _engine.PainnEngine:
        key = (A, src.tobytes(), dst.tobytes(), ety.tobytes(), atom_ids.tobytes(), self.precision)
        if key not in self._engines:
            flat = _W.flatten_state_dict(self._sd, self._spec)
            self._engines[key] = _engine.PainnEngine(self.VARIANT, self.n_features, self.score_layers, A, src, dst, ety, atom_ids, flat,
                                                     n_types=self.n_types, temp_length=self.temp_length, time_length=self.time_length,
                                                     temperatures=self.temperatures, device=self._device, precision=self.precision)
        return self._engines[key]

    def engine_with_mask(self, A, src, dst, ety, ids, mask) -> _engine.PainnEngine:
        """engine_for with a batch's per-molecule edge mask set (split_graph_batch; None clears it: a uniform batch)."""
        eng = self.engine_for(A, src, dst, ety, ids)
        eng.set_edge_mask(mask)
        return eng

    def engine_of(self, sb: SpeciesBatch) -> _engine.PainnEngine:
        """The engine of a split_species_batch result with its per-molecule graph state set (a uniform batch: engine_with_mask)."""
        if sb.n_atoms is None:
            return self.engine_with_mask(sb.A, sb.src, sb.dst, sb.etype, sb.atom_ids, sb.mask)
        if sb.A > self.n_types:
            raise ValueError(f"the largest molecule has {sb.A} atoms but the model embeds n_types = {self.n_types} atom ids")
        eng = self.engine_for(sb.A, sb.src, sb.dst, sb.etype, sb.atom_ids)
        eng.set_molecules(sb.n_atoms, sb.mask, sb.pair_type)
        return eng

    def cond_of(self, batch, B, A, on_gpu=False, sb=None):
        """[B, A, n_cond] float32 conditioning; a CUDA tensor when `on_gpu` (the batch lives on the GPU), else numpy.  sb: the
        batch's SpeciesBatch when its molecules differ in size (pads get 0)."""
        if not self.COND_KEYS:
            return None
        if sb is not None and sb.n_atoms is not None:
            cols = [sb.pad(getattr(batch, k), 1) for k in self.COND_KEYS]
            if on_gpu:
                import torch
                return torch.cat(cols, dim=-1).contiguous()
            return np.ascontiguousarray(np.concatenate(cols, axis=-1))
        if on_gpu:
            import torch
            cols = [getattr(batch, k).detach().to(torch.float32).reshape(B, A) for k in self.COND_KEYS]
            return torch.stack(cols, dim=-1).contiguous()
        cols = [C.to_numpy(getattr(batch, k)).astype(np.float32).reshape(B, A) for k in self.COND_KEYS]   # latent T is int64 (mdqm9_latent.py:184)
        return np.ascontiguousarray(np.stack(cols, axis=-1))

    def forward(self, batch):
        """Evaluates the drift at batch.x, time batch.t (per node: one value for the call, or one value per molecule) and writes
        batch.output [N,3] like the reference."""
        sb = split_species_batch(batch, self.ATOM_KEY)
        B, A = sb.B, sb.A
        x = sb.pad(batch.x, 3) if sb.n_atoms is not None else C.as_f32(batch.x, (B, A, 3))      # a CUDA batch is evaluated in place, no host round trip
        t = molecule_times(sb.molecule_values(batch.t), B, A, x)
        out = self.engine_of(sb).drift(x, t, self.cond_of(batch, B, A, C.is_cuda(x), sb))
        batch.output = C.like(sb.unpad(out), batch.x)
        return batch

    __call__ = forward


class ODEWrapperBase:
    """Mirror of the reference ``ODEWrapper`` (mdqm9/thermo/{ambient,latent}/models/ode_wrapper.py): the right-hand side the
    integrator sees.  forward(t, states, batch[, n_steps]) -> b, or (b, -div * DIV_SCALE) with return_dlogp (reverse_ode:
    (-b, +div * DIV_SCALE)); compute_divergence(b, batch) -> div * DIV_SCALE evaluated at batch.x, batch.t."""
    DIV_SCALE = 1.0

    def __init__(self, b, return_dlogp=False, reverse_ode=False):
        self.b, self.return_dlogp, self.reverse_ode = b, return_dlogp, reverse_ode

    def _eval(self, batch, x, t, with_div):
        """t: one float, or batch.t-like per-node times (one value per molecule)."""
        sb = split_species_batch(batch, self.b.ATOM_KEY)
        B, A = sb.B, sb.A
        xs = sb.pad(x, 3) if sb.n_atoms is not None else C.as_f32(x, (B, A, 3))
        if not isinstance(t, float):
            t = molecule_times(sb.molecule_values(t), B, A, xs)
        eng = self.b.engine_of(sb)
        cond = self.b.cond_of(batch, B, A, C.is_cuda(xs), sb)
        if with_div:
            out, div = eng.drift_div(xs, t, cond)
            return sb.unpad(out), div
        return sb.unpad(eng.drift(xs, t, cond)), None

    def forward(self, integration_time, states, batch, n_steps=None):
        if n_steps is not None:
            n_steps.append(n_steps[-1] + 1)                       # ambient wrapper's evaluation counter (ode_wrapper.py:44)
        t = float(C.to_numpy(integration_time).reshape(-1)[0])
        if self.return_dlogp:
            x, _ = states
            b, div = self._eval(batch, x, t, True)
            b, d = C.like(b, x), C.like(div * self.DIV_SCALE if C.is_torch(div) else div * np.float32(self.DIV_SCALE), x)
            return (b, -d) if not self.reverse_ode else (-b, d)
        b, _ = self._eval(batch, states, t, False)
        return C.like(b, states)

    __call__ = forward

    @classmethod
    def compute_divergence(cls, b, batch):
        """div * DIV_SCALE at batch.x and batch.t (one time per call or per molecule, like cPaiNN.forward)."""
        _, div = cls(b)._eval(batch, batch.x, batch.t, True)
        return C.like(div * cls.DIV_SCALE if C.is_torch(div) else div * np.float32(cls.DIV_SCALE), batch.x)

    @staticmethod
    def reset_batch(batch, x, integration_time):
        batch.x = x.clone() if hasattr(x, "clone") else np.array(x, copy=True)
        ids = getattr(batch, "atoms", None)
        ids = getattr(batch, "atom_number") if ids is None else ids
        batch.t = integration_time * (ids * 0 + 1)                # integration_time * ones_like(atoms)  (ode_wrapper.py:112)
        return batch


class MoleculeIntegratorBase:
    """rollout(batch) with the reference's constructor.  method: 'dopri5' (the reference default; adaptive with rtol / atol, the
    grid linspace(start, end, n_step) selects the output times) or a scheme on that grid (see _common.check_method).

    return_dlogp=True integrates the second state of the reference ODEWrapper with the same scheme: d(dlogp)/dt = -DIV_SCALE *
    div b (exact divergence, 3A forward-mode passes per molecule on the GPU), returned * SCALE_DLOGP as [n_saved, B].  With
    reverse_ode the pair is (-b, +DIV_SCALE * div) on linspace(end, start) (ode_wrapper.py:49, integrators.py:40-43).

    step_control (keyword-only, build-defined): 'batch' (default) -- one step size for the whole batch, the reference's single
    odeint per mini-batch, so a molecule's result depends on its batch; 'trajectory' (method='dopri5' only) -- every molecule gets
    its own step sizes, accept / reject decisions and dense output: what the reference computes for it at batch size 1, the same
    bits for any batch, order or sharding.  self.n_steps_per_molecule then holds (accepted, rejected) [B] of the last rollout.

    divergence (keyword-only, build-defined; needs return_dlogp=True for 'hutchinson'): 'exact' (default) or 'hutchinson' --
    Hutchinson's estimate with n_probes Rademacher probes per molecule (k tangent passes instead of 3A), drawn from (probe_seed,
    traj_offset + b) once per rollout and fixed along it.  Unbiased but noisy: each molecule's dlogp carries an estimator error.

    observe (keyword-only, build-defined): dict(descriptors=[...], ref=None, select=None, every=1) -- collective variables
    (observables.py) evaluated on the GPU at the grid points i % every == 0 and at the last one, whatever save_every is; after rollout
    they are in self.cv [rows, B, K] (a CUDA tensor when the batch is one).  Descriptor indices and ref [A, 3] are local to a
    molecule; in a mixed-species batch A is the largest molecule and a descriptor naming an atom a molecule lacks gives NaN there."""
    SCALE_DLOGP = 1.0      # integrators.py:68 (ambient: 1e2)
    DIV_SCALE = 1.0        # ode_wrapper.py:91 (ambient: 1e-2)

    def __init__(self, b, method: str = "dopri5", n_step: int = 100, atol: float = 1e-4, rtol: float = 1e-4, start: float = 0.0,
                 end: float = 1.0, return_dlogp: bool = False, reverse_ode: bool = False, *, eps: float = 0.0, seed: int = 0,
                 save_every: int = 1, com_free_noise: bool = False, step_control: str = "batch", divergence: str = "exact",
                 n_probes: int = 1, probe_seed: int = 0, observe=None):
        self.method = C.check_method(method)
        self.observe, self.cv = _obs.check_observe(observe), None
        if self.observe is not None and step_control == "trajectory":
            raise ValueError("observe= is not available with step_control='trajectory' (its rows are written per trajectory)")
        self.step_control = C.check_step_control(step_control, self.method)
        self.divergence, self.n_probes = C.check_divergence(divergence, n_probes, return_dlogp)
        self.probe_seed = int(probe_seed)
        if return_dlogp and self.method == "em" and eps > 0:
            raise ValueError("return_dlogp=True needs a deterministic scheme ('euler' or 'heun')")
        self.b = b
        self.start, self.end, self.rtol, self.atol = start, end, rtol, atol
        self.n_step, self.return_dlogp, self.reverse_ode = n_step, return_dlogp, reverse_ode
        self.eps, self.seed, self.save_every, self.com_free_noise = eps, seed, save_every, com_free_noise

    def _record_counts(self, eng, B):
        self.n_steps_per_molecule = eng.step_counts(B) if self.step_control == "trajectory" else None

    def _rollout(self, batch, traj_offset=0):
        sb = split_species_batch(batch, self.b.ATOM_KEY)
        B, A = sb.B, sb.A
        x0 = sb.pad(batch.x0, 3) if sb.n_atoms is not None else C.as_f32(batch.x0, (B, A, 3))      # CUDA batches stay in HBM: data_ptr() in, CUDA tensors out
        gpu = C.is_cuda(x0)
        # without dlogp the reference always integrates on linspace(start, end) (integrators.py:54-55), reverse_ode or not
        grid = _engine.time_grid(self.start, self.end, self.n_step)
        eng = self.b.engine_of(sb)
        if self.observe is None:
            return self._rollout_on(eng, sb, batch, x0, gpu, grid, traj_offset)
        o = self.observe
        rows = int(_engine._lib.lib().ti_rollout_rows(int(self.n_step), o["every"]))
        self.cv = _engine._alloc_like(x0 if gpu else None, (rows, B, int(o["descriptors"].shape[0])))
        eng.set_observer(o["descriptors"], o["ref"], o["select"], o["every"], self.cv)
        try:
            return self._rollout_on(eng, sb, batch, x0, gpu, grid, traj_offset)
        finally:
            eng.set_observer(None)

    def _rollout_on(self, eng, sb, batch, x0, gpu, grid, traj_offset):
        B, A = sb.B, sb.A
        if self.return_dlogp:
            if self.reverse_ode:
                grid = _engine.time_grid(self.end, self.start, self.n_step)
            kw = dict(scheme="euler" if self.method == "em" else self.method, save_every=self.save_every, div_scale=self.DIV_SCALE,
                      out_scale=self.SCALE_DLOGP, reverse_ode=self.reverse_ode, rtol=self.rtol, atol=self.atol, step_control=self.step_control)
            cond = self.b.cond_of(batch, B, A, gpu, sb)
            if self.divergence == "hutchinson":
                path, dl, nfe = eng.rollout_dlogp_est(x0, cond, grid, n_probes=self.n_probes, probe_seed=self.probe_seed,
                                                      traj_offset=traj_offset, **kw)
            else:
                path, dl, nfe = eng.rollout_dlogp(x0, cond, grid, **kw)
            self._record_counts(eng, B)
            return C.like(sb.unpad(path), batch.x0), C.like(dl, batch.x0), nfe
        path, nfe = eng.rollout(x0, self.b.cond_of(batch, B, A, gpu, sb), grid, scheme=self.method, save_every=self.save_every, eps=self.eps,
                                seed=self.seed, traj_offset=traj_offset, com_free_noise=self.com_free_noise, rtol=self.rtol, atol=self.atol,
                                step_control=self.step_control)
        self._record_counts(eng, B)
        xts = C.like(sb.unpad(path), batch.x0)
        dlogp = batch.x0.new_zeros(B) if gpu else C.like(np.zeros(B, np.float32) * self.SCALE_DLOGP, batch.x0)      # reference: zeros(batch_size) (* 1e2 in ambient)
        return xts, dlogp, nfe


class MoleculeTrainerBase:
    """The optimiser side of mdqm9/train_ambient.py:124-149 and its latent twin on the device (engine.PainnTrainer): loss_fn
    differentiated with respect to every parameter of cPaiNN, clip_grad_norm_ at max_grad_norm, torch.optim.Adam(lr, betas, eps,
    weight_decay), the NaN skip.  ``b`` is a thermo cPaiNN whose weights are the starting point; ``loss_fn`` a thermo.losses loss,
    which gives the kind, gamma, a and t_distr.  The fp64 master weights live on the device; ``sync()`` writes them back into ``b``.
    A trainer serves one species: the device trainer is built from the first batch's template, and a batch with another template,
    an edge mask or mixed species is refused -- unless with_batches("per_molecule", max_atoms=A) was chosen, which trains one model on
    batches whose molecules differ in size, graph and bond types."""
    BETA_NAME = "beta_half"              # what t_distr='beta' means for this workflow's loss

    def __init__(self, b, loss_fn, lr, weight_decay=0.0, max_grad_norm=1.0, betas=(0.9, 0.999), eps=1e-8, max_workspace_bytes=0):
        ip = loss_fn.interpolant
        self.b, self.loss_fn, self.lr = b, loss_fn, float(lr)
        self._kw = dict(kind=loss_fn.KIND, gamma=ip.gamma_name, a=ip.a_param, t_distr="uniform" if loss_fn.t_distr == "uniform" else self.BETA_NAME)
        self._opt = dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, max_grad_norm=max_grad_norm, max_workspace_bytes=max_workspace_bytes)
        self.engine, self._key, self._pending = None, None, None
        self.batches, self.max_atoms = "uniform", None

    def with_batches(self, batches="uniform", max_atoms=None):
        """How the trainer reads its batches -> self.  "uniform" (the default): one species, one graph, anything else is refused.
        "per_molecule" with max_atoms=A: the device trainer is built on the fully connected template over A atoms with atom ids
        0 .. A - 1 (the reference's distinguish=True features), and step / loss take whatever split_species_batch takes -- molecules
        of different size, graph and bond types, padded as SpeciesBatch pads them -- through engine.PainnTrainer.set_graphs.  Chosen
        before the first batch."""
        if batches not in ("uniform", "per_molecule"):
            raise ValueError(f"batches must be 'uniform' or 'per_molecule', got {batches!r}")
        if self.engine is not None:
            raise RuntimeError("the device trainer exists already: choose the batch form before the first batch")
        if batches == "per_molecule":
            if max_atoms is None or not 1 <= int(max_atoms) <= 32:
                raise ValueError("batches='per_molecule' needs max_atoms in 1..32, the largest molecule the trainer will see")
            if int(max_atoms) > self.b.n_types:
                raise ValueError(f"max_atoms = {int(max_atoms)} but the model embeds n_types = {self.b.n_types} atom ids")
        elif max_atoms is not None:
            raise ValueError("max_atoms belongs to batches='per_molecule'")
        self.batches, self.max_atoms = batches, None if max_atoms is None else int(max_atoms)
        return self

    def _build(self, A, src, dst, ety, ids, key):
        b = self.b
        flat = _W.flatten_state_dict(b._sd, b._spec, dtype=np.float64)
        self.engine = _engine.PainnTrainer(b.VARIANT, b.n_features, b.score_layers, A, src, dst, ety, ids, flat, n_types=b.n_types,
                                           temp_length=b.temp_length, time_length=b.time_length, temperatures=b.temperatures,
                                           device=b._device, **self._opt)
        self._key = key
        if self._pending is not None:
            self.load_state_dict(self._pending)

    def _per_molecule_engine(self):
        """The device trainer of batches='per_molecule': the complete directed graph on max_atoms atoms in (src, dst) order, type 0"""
        if self.engine is None:
            A = self.max_atoms
            s_all, d_all = np.nonzero(~np.eye(A, dtype=bool))
            if not s_all.size:
                raise ValueError("batches='per_molecule' needs max_atoms >= 2: the trainer needs an edge template")
            self._build(A, s_all.astype(np.int32), d_all.astype(np.int32), np.zeros(s_all.size, np.int32), np.arange(A, dtype=np.int32), ("per_molecule", A))
        return self.engine

    def _graphs_of(self, sb):
        """(n_atoms [B], mask [B, A], pair_type [B, A, A]) of a SpeciesBatch over the trainer's max_atoms = A"""
        A, a = self.max_atoms, sb.A
        if a > A:
            raise ValueError(f"the batch's largest molecule has {a} atoms, the trainer was built for max_atoms = {A}")
        if sb.n_atoms is None and not np.array_equal(sb.atom_ids, np.arange(a)):
            raise ValueError("batches='per_molecule' needs every molecule's atom ids to be 0 .. n_atoms - 1 (distinguish=True)")
        n = np.full(sb.B, a, np.int32) if sb.n_atoms is None else np.asarray(sb.n_atoms, np.int32)
        mask = np.zeros((sb.B, A), np.uint32)
        if sb.mask is not None:
            mask[:, :a] = sb.mask
        else:
            mask[:, :a] = np.bincount(sb.dst, weights=np.ldexp(1.0, sb.src), minlength=a).astype(np.uint32)[None]
        pt = np.zeros((sb.B, A, A), np.uint8)
        if sb.pair_type is not None:
            pt[:, :a, :a] = sb.pair_type
        else:
            pt[:, sb.src, sb.dst] = sb.etype.astype(np.uint8)[None]
        return n, mask, pt

    def _args_per_molecule(self, batch, x0, x1, conds, t, z):
        """_args for batches='per_molecule': the padded arrays of the call, with the batch's graphs set on the device trainer"""
        sb = split_species_batch(batch, self.b.ATOM_KEY)
        eng = self._per_molecule_engine()
        if len(conds) != eng.ncond:
            raise ValueError(f"this model takes {eng.ncond} conditioning value(s) per node, the batch form gives {len(conds)}")
        eng.set_graphs(*self._graphs_of(sb))
        B, A = sb.B, self.max_atoms

        def padded(flat, comps):
            out = np.zeros((B, A, comps), np.float32)
            out[:, :sb.A] = sb.pad(C.to_numpy(flat, np.float32), comps)
            return out

        cond = np.ascontiguousarray(np.concatenate([padded(c, 1) for c in conds], axis=-1)) if conds else None
        tv = None
        if t is not None:
            tn = C.to_numpy(t, np.float32).reshape(-1)
            if tn.size == B:
                tv = np.ascontiguousarray(tn)
            elif tn.size != sb.N:
                raise ValueError(f"t must hold one value per molecule ({B}) or per node ({sb.N}), got {tn.size}")
            else:
                per = sb.molecule_values(tn).reshape(B, sb.A)
                if np.any(per != per[:, :1]):
                    raise ValueError("t must be constant within each molecule")
                tv = np.ascontiguousarray(per[:, 0])
        return padded(x0, 3), padded(x1, 3), cond, tv, None if z is None else padded(z, 3)

    def _engine_for(self, batch):
        try:
            B, A, src, dst, ety, ids = split_batch(batch, self.b.ATOM_KEY)
        except ValueError as e:
            raise NotImplementedError(f"the trainer takes uniform batches (one species, one graph, no edge mask): {e}") from None
        key = (A, src.tobytes(), dst.tobytes(), ety.tobytes(), ids.tobytes())
        if self.engine is None:
            self._build(A, src, dst, ety, ids, key)
        elif key != self._key:
            raise NotImplementedError("a trainer serves one species: this batch has another template or other atom ids")
        return B, A

    def _args(self, batch, x0, x1, conds, t, z):
        from .losses import _molecule_t
        if self.batches == "per_molecule":
            return self._args_per_molecule(batch, x0, x1, conds, t, z)
        B, A = self._engine_for(batch)
        if len(conds) != self.engine.ncond:
            raise ValueError(f"this model takes {self.engine.ncond} conditioning value(s) per node, the batch form gives {len(conds)}")
        gpu = C.is_cuda(x0)
        x0, x1 = C.as_f32(x0, (B, A, 3)), C.as_f32(x1, (B, A, 3))
        cond = None
        if conds and gpu:
            import torch
            cond = torch.stack([c.detach().to(x0.device, torch.float32).reshape(B, A) for c in conds], dim=-1).contiguous()
        elif conds:
            cond = np.ascontiguousarray(np.stack([C.to_numpy(c).astype(np.float32).reshape(B, A) for c in conds], axis=-1))
        tv, zv = _molecule_t(t, B, A), (None if z is None else C.as_f32(z, (B, A, 3)))
        if gpu:
            import torch
            tv = None if tv is None else torch.from_numpy(tv).to(x0.device)
            zv = None if zv is None else (zv if C.is_cuda(zv) else torch.from_numpy(zv).to(x0.device))
        elif zv is not None and C.is_cuda(zv):
            zv = C.to_numpy(zv, np.float32)
        return x0, x1, cond, tv, zv

    def _step(self, batch, x0, x1, conds, t, z, seed, draw, traj_offset, center):
        x0, x1, cond, tv, zv = self._args(batch, x0, x1, conds, t, z)
        return self.engine.step(x0, x1, cond, center=center or "batch", t=tv, z=zv, seed=seed, draw=draw, traj_offset=traj_offset, **self._kw)[0]

    def _loss(self, batch, x0, x1, conds, t, z, seed, draw, traj_offset, center):
        x0, x1, cond, tv, zv = self._args(batch, x0, x1, conds, t, z)
        return self.engine.grad(x0, x1, cond, center=center or "batch", t=tv, z=zv, seed=seed, draw=draw, traj_offset=traj_offset, **self._kw)["mean"]

    def _resident(self, x0, x1, temps0, temps1, template_batch):
        """The resident sets of fit / evaluate as the device call takes them: x [n, A, 3] float32 and one temperature per molecule,
        numpy or CUDA tensors (all in one memory space).  template_batch builds the device trainer when no step has done so yet."""
        if self.engine is None and self.batches == "per_molecule":
            self._per_molecule_engine()
        if self.engine is None:
            if template_batch is None:
                raise ValueError("the trainer has seen no batch yet: pass template_batch, one uniform batch of the species")
            self._engine_for(template_batch)
        A = self.engine.A

        def arr(v, shape, what):
            if v is None:
                return None
            if C.is_cuda(v):
                import torch
                return v.detach().to(torch.float32).reshape(shape).contiguous()
            return np.ascontiguousarray(C.to_numpy(v, np.float32).reshape(shape))

        x0, x1 = arr(x0, (-1, A, 3), "x0"), arr(x1, (-1, A, 3), "x1")
        t0 = None if x0 is None else arr(temps0, (x0.shape[0],), "temps0")
        return x0, x1, t0, arr(temps1, (x1.shape[0],), "temps1")

    def _fit(self, x0, x1, temps0, temps1, batch_size, n_steps, seed, draw, noise_seed, center, template_batch, noise, update, track_best,
             masks=None):
        from .adw import minibatch_indices
        x0, x1, t0, t1 = self._resident(x0, x1, temps0, temps1, template_batch)
        if masks is not None:
            if noise != "given" or x0 is None:
                raise ValueError("masks are the graphs of the resident set 0: they need noise='given' and an x0")
            m = masks if C.is_cuda(masks) else np.ascontiguousarray(C.to_numpy(masks))
            if tuple(m.shape) != (int(x0.shape[0]), self.engine.A):
                raise ValueError(f"masks must be [n0, A] = [{int(x0.shape[0])}, {self.engine.A}], got {tuple(m.shape)}")
            self.engine.set_graphs(None, m, None)              # one species: every count A, the template's types
        else:
            self.engine.set_graphs()                           # the table a per-molecule step may have left
        rng = np.random.default_rng(seed)
        i0 = minibatch_indices(x0.shape[0], batch_size, n_steps, rng) if x0 is not None else None
        i1 = minibatch_indices(x1.shape[0], batch_size, n_steps, rng)
        if C.is_cuda(x1):
            import torch
            i0, i1 = (None if i is None else torch.from_numpy(i).to(x1.device) for i in (i0, i1))
        return self.engine.steps(x0, x1, t0, t1, i0, i1, update=update, noise=noise, track_best=track_best, center=center or "batch",
                                 seed=seed if noise_seed is None else noise_seed, draw=draw, **self._kw)

    def fit(self, x0, x1, temps0, temps1, batch_size, n_steps, seed, *, draw=0, noise_seed=None, center=None, template_batch=None,
            noise="given", track_best=True, masks=None):
        """n_steps optimiser steps in one device call on resident sets (engine.PainnTrainer.steps): minibatches from permutations drawn
        on the host with `seed` (thermo.adw.minibatch_indices, set 0 first, independently for the two sets), step k with the (t, z) of
        draw + k under noise_seed (default: seed).  x0 [n0, A, 3], x1 [n1, A, 3]; temps0 [n0], temps1 [n1] or None as the model takes
        them.  noise="drawn" | "aligned" with x0=None: the base samples of every minibatch are drawn on the device.  track_best keeps the
        weights of the step with the smallest loss (best_state_dict).  masks [n0, A] uint32 (noise="given", one species): the edge
        sets of the resident set 0 over the trainer's template, bit s of masks[i, d] set when row i has the edge s -> d; a minibatch
        molecule takes the graph of its set-0 row, as the reference's loss evaluates both states on batch0's graph.
        -> (mean loss of every step [n_steps], NaN where skipped; the number of skipped steps)"""
        return self._fit(x0, x1, temps0, temps1, batch_size, n_steps, seed, draw, noise_seed, center, template_batch, noise, True, track_best,
                         masks)

    def evaluate(self, x0, x1, temps0, temps1, batch_size, n_steps, seed, *, draw=0, noise_seed=None, center=None, template_batch=None,
                 noise="given", masks=None):
        """fit without the update: the forward pass and the loss of the same minibatches at the current weights; nothing changes.
        -> the mean loss of every minibatch [n_steps]"""
        return self._fit(x0, x1, temps0, temps1, batch_size, n_steps, seed, draw, noise_seed, center, template_batch, noise, False, False,
                         masks)[0]

    def best_state_dict(self, reset=False):
        """(state dict in the reference's keys, loss, step) of the step with the smallest loss since the last reset: the weights that
        produced that loss, as `copy.deepcopy(model) if loss < epoch_best_loss` keeps them.  (None, inf, -1) where every step was skipped."""
        if self.engine is None:
            raise RuntimeError("the trainer has seen no batch yet: there are no best weights")
        r = self.engine.best(reset=reset)
        sd = None if r["w"] is None else _W.unflatten(r["w"], self.b._spec)
        return sd, r["loss"], r["step"]

    def set_lr(self, lr):
        self.lr = float(lr)
        self._opt["lr"] = self.lr
        if self.engine is not None:
            self.engine.set_lr(lr)

    def sync(self):
        """Write the master weights back into ``b`` in the reference's keys (load_state_dict: its drift engines are rebuilt on next use) -> b"""
        if self.engine is None:
            return self.b
        return self.b.load_state_dict(_W.unflatten(self.engine.weights(), self.b._spec))

    def state_dict(self):
        """The optimiser state for resuming: master weights, moments, counters, learning rate"""
        if self.engine is None:
            raise RuntimeError("the trainer has seen no batch yet: there is no device state to save")
        return dict(self.engine.state(), lr=self.lr)

    def load_state_dict(self, state):
        if self.engine is None:              # applied when the first batch builds the device trainer
            self._pending = dict(state)
            self.lr = float(state["lr"]); self._opt["lr"] = self.lr
            return self
        self._pending = None
        self.engine.load_state(w=state["w"], m=state["m"], v=state["v"], n_applied=int(state["n_applied"]))
        self.set_lr(float(state["lr"]))
        return self
