"""Molecule sampling: generator forward + graph decode (``dg_decode_graph``), optionally as ONE replayed hipGraph.

The reference's ``inference.py:180-206`` runs the generator eagerly at ``inf_batch_size`` (default 1) -- the
launch-bound regime -- and pulls dense label matrices to the host per molecule.  ``MoleculeSampler.sample`` returns a
``decode.MoleculeBatch`` instead: one ``.cpu()`` for the batch, bond lists in ``matrices2mol``'s order.  The capture
follows ``trainer.GraphedGANStep``: warm-up on a side stream, the packed-weight epoch bumped before and after capture
(so that the pack kernels are recorded and a replay re-packs from the live parameters), static int32 label buffers for
one-hot edge batches."""
from __future__ import annotations

import torch

from .decode import _order2_table, decode_molecule_graphs
from .functional import (activation_dtype, as_one_hot, attach_one_hot_labels, bump_weights_epoch, one_hot_labels)
from .smiles_out import SmilesTables, write_smiles
from .validity import ValenceTables, check_molecules
from .descriptors import DescriptorTables, describe_molecules
from .substructure import SubstructureTables, match_molecules
from .scaffolds import murcko_scaffolds

__all__ = ["MoleculeSampler"]


class MoleculeSampler:
    """``MoleculeSampler(G, edge, node)`` -- ``edge`` [B,N,N,E], ``node`` [B,N,M]: a batch of the shape to sample at (the
    generator's input graphs, as ``G(edge, node)`` takes them).

    ``graph=True``: forward and decode are captured once, at construction, into one hipGraph (a single chain of kernels
    on one stream) at the activation dtype then current, and ``sample`` copies each new batch into static buffers and
    replays.  Everything ``sample`` returns then lives in static buffers too: the ``MoleculeBatch`` and the logits are
    OVERWRITTEN by the next ``sample`` -- take ``.cpu()`` (or a clone) before it.  A capture made with a one-hot edge batch
    embeds edges through their labels and accepts one-hot batches only.  ``graph=False``: the same work, launched eagerly.

    ``G`` runs in ``eval()`` under ``torch.inference_mode()``; its training flags are restored.  In-place weight updates
    (``load_state_dict``, an optimizer step) are seen by the next ``sample`` in both modes; parameters that were MOVED
    since the capture (``optim.FlatAdamW`` re-points them into its flat buffer at its first step) make ``sample`` capture
    again.

    ``smiles``: ``smiles_out.SmilesTables`` on the batch's device -- every sample then also writes the SMILES string of each
    molecule's largest fragment (``smiles_out.write_smiles``: one more launch behind the decode, inside the captured graph when
    there is one), and ``sampler.smiles`` is the ``SmilesBatch`` of the last sample (graphed: a static buffer like the
    ``MoleculeBatch``).  None: nothing is written and ``sampler.smiles`` stays None.

    ``validity``: ``validity.ValenceTables`` on the batch's device -- every sample then also checks each molecule's largest
    fragment (``validity.check_molecules``: one more launch behind the decode, inside the captured graph when there is one); the
    ``MoleculeValidity`` is ``batch.validity`` of the returned batch and ``sampler.validity`` (graphed: a static buffer like the
    ``MoleculeBatch``).  None: nothing is checked and both stay None.

    ``descriptors``: ``descriptors.DescriptorTables`` on the batch's device, together with ``validity=`` (``ValueError``
    without it: the descriptors are made of the verdicts) -- every sample then also describes each molecule's largest fragment
    (``descriptors.describe_molecules``: one more launch behind the check, inside the captured graph when there is one); the
    ``MoleculeDescriptors`` is ``batch.descriptors`` and ``sampler.descriptors``.  None: both stay None.

    ``substructures``: ``substructure.SubstructureTables`` on the batch's device, together with ``validity=`` and
    ``descriptors=`` (``ValueError`` without them: the matcher reads the descriptors' keys and bond classes) -- every sample then
    also matches the tables' patterns (``substructure.match_molecules``: one more launch behind the descriptors, inside the
    captured graph when there is one); the ``MoleculeMatches`` is ``batch.matches`` and ``sampler.matches``.  None: both stay
    None.

    ``scaffolds``: True, together with ``validity=`` and ``descriptors=`` (``ValueError`` without them: the scaffolds are cut
    along the descriptors' bond classes, with the descriptor tables' bond table) -- every sample then also cuts out each
    molecule's scaffold (``scaffolds.murcko_scaffolds``: one more launch behind the descriptors, inside the captured graph when
    there is one); the ``MoleculeScaffolds`` is ``batch.scaffolds`` and ``sampler.scaffolds``.  False: both stay None."""

    def __init__(self, G, edge, node, *, graph: bool = True, bond_order2=None, bond_cap=None, warmup: int = 3, smiles=None,
                 validity=None, descriptors=None, substructures=None, scaffolds=False):
        if not (edge.is_cuda and node.is_cuda):
            raise RuntimeError("druggen_amd.sampling runs on the GPU (no CPU fallback)")
        if smiles is not None and not isinstance(smiles, SmilesTables):
            raise TypeError("smiles= takes smiles_out.SmilesTables (SmilesTables.from_decoders)")
        if validity is not None and not isinstance(validity, ValenceTables):
            raise TypeError("validity= takes validity.ValenceTables (ValenceTables.from_decoders)")
        if descriptors is not None and not isinstance(descriptors, DescriptorTables):
            raise TypeError("descriptors= takes descriptors.DescriptorTables (DescriptorTables.from_decoders)")
        if descriptors is not None and validity is None:
            raise ValueError("descriptors= needs validity= as well: the descriptors are made of the validity check's verdicts")
        if substructures is not None and not isinstance(substructures, SubstructureTables):
            raise TypeError("substructures= takes substructure.SubstructureTables (SubstructureTables.from_decoders)")
        if substructures is not None and (validity is None or descriptors is None):
            raise ValueError("substructures= needs validity= and descriptors= as well: the matcher reads the descriptors' atom "
                             "keys and bond classes")
        if scaffolds and (validity is None or descriptors is None):
            raise ValueError("scaffolds=True needs validity= and descriptors= as well: the scaffolds are cut along the "
                             "descriptors' atom keys and bond classes")
        self.G = G
        self.smiles_tables, self.smiles = smiles, None
        self.validity_tables, self.validity = validity, None
        self.descriptor_tables, self.descriptors = descriptors, None
        self.substructure_tables, self.matches = substructures, None
        self.with_scaffolds, self.scaffolds = bool(scaffolds), None
        self.bond_cap = bond_cap
        self._order2 = _order2_table(bond_order2, edge.shape[-1], node.device)      # on the device before any capture
        self.graph = None
        self._labels = None
        self._shape = (tuple(edge.shape), tuple(node.shape))
        if not graph:
            return
        self._act_dtype = activation_dtype()
        self.static_edge, self.static_node = edge.detach().clone(), node.detach().clone()
        # label buffer of the edge batch: validated HERE, outside the graph (as_one_hot syncs once); None when the capture
        # batch is not one-hot -- the graph then records the dense embedding kernel and needs no labels
        lab = one_hot_labels(as_one_hot(edge))
        if lab is not None:
            self._labels = lab.clone()
            attach_one_hot_labels(self.static_edge, self._labels)
        self._warmup = warmup
        self._capture()

    def _capture(self):
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):          # warm-up off the default stream: allocator pools, packed weights, scratch
            for _ in range(self._warmup):
                self._run(self.static_edge, self.static_node)
        torch.cuda.current_stream().wait_stream(side)
        bump_weights_epoch()      # every first use of a weight inside the capture records its pack kernel
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            out = self._run(self.static_edge, self.static_node)
        bump_weights_epoch()      # cache entries made during capture point into the graph's private pool
        # the graph reads the parameters where they are NOW: an optimizer that re-points them into a flat buffer at its
        # first step (optim.FlatAdamW) moves them, and `sample` then captures again
        self._param_ptrs = [p.data_ptr() for p in self.G.parameters()]
        self.graph, self._static_out = graph, out

    def _run(self, edge, node):
        modes = [(m, m.training) for m in self.G.modules()]
        self.G.eval()
        try:
            with torch.inference_mode():
                _, _, node_sample, edge_sample = self.G(edge, node)
                batch = decode_molecule_graphs(node_sample, edge_sample, bond_order2=self._order2, bond_cap=self.bond_cap)
                if self.smiles_tables is not None:
                    self.smiles = write_smiles(batch, self.smiles_tables)
                if self.validity_tables is not None:
                    self.validity = batch.validity = check_molecules(batch, self.validity_tables)
                if self.descriptor_tables is not None:
                    self.descriptors = batch.descriptors = describe_molecules(batch, batch.validity, self.descriptor_tables)
                if self.substructure_tables is not None:
                    self.matches = batch.matches = match_molecules(batch, batch.descriptors, self.substructure_tables)
                if self.with_scaffolds:
                    self.scaffolds = batch.scaffolds = murcko_scaffolds(batch, batch.descriptors, self.descriptor_tables)
        finally:
            for m, was in modes:
                m.training = was
        return batch, node_sample, edge_sample

    def sample(self, edge, node, *, keep_logits: bool = False, check_one_hot: bool = True):
        """Decode ``G(edge, node)``: a ``MoleculeBatch``, or ``(batch, node_sample, edge_sample)`` with
        ``keep_logits=True`` (graphed: views of static buffers, overwritten by the next ``sample``).  A capture made on
        a one-hot edge batch validates every new edge tensor (one device->host read per new tensor object; labels
        attached by ``data.load_molecules`` are trusted; ``check_one_hot=False`` skips the check and trusts ``argmax``)."""
        if self.graph is None:
            out = self._run(as_one_hot(edge) if check_one_hot else edge, node)
        else:
            if tuple(edge.shape) != tuple(self.static_edge.shape) or tuple(node.shape) != tuple(self.static_node.shape):
                raise RuntimeError(f"MoleculeSampler was captured for edge {tuple(self.static_edge.shape)} / node "
                                   f"{tuple(self.static_node.shape)}: build a new sampler for another batch shape")
            self._check_activation_dtype()
            # validate BEFORE touching a static buffer: a rejected batch leaves the dense buffer and its labels consistent
            lab = None
            new_edge = edge.data_ptr() != self.static_edge.data_ptr()
            if new_edge and self._labels is not None:
                lab = one_hot_labels(as_one_hot(edge)) if check_one_hot else one_hot_labels(edge)
                if lab is None:
                    if check_one_hot:
                        raise RuntimeError("MoleculeSampler was captured with a one-hot edge batch (table-gather embedding); "
                                           "the new batch is not one-hot: build a sampler on a dense batch for dense inputs")
                    lab = edge.argmax(-1)
            if new_edge:
                self.static_edge.copy_(edge)
                if lab is not None:
                    self._labels.copy_(lab)      # in place: the captured kernel reads this buffer
                    attach_one_hot_labels(self.static_edge, self._labels)
            if node.data_ptr() != self.static_node.data_ptr():
                self.static_node.copy_(node)
            out = self.replay()
        return out if keep_logits else out[0]

    def _check_activation_dtype(self):
        if activation_dtype() != self._act_dtype:
            raise RuntimeError(f"MoleculeSampler was captured with {self._act_dtype} activations: build a new sampler "
                               f"after set_activation_dtype")

    def inputs(self):
        """``(a, labels, x)``: the static dense buffers and the static int32 label buffer the captured kernels read -- an
        ``out=`` of ``ResidentMolecules.batch``.  Whoever writes ``a`` writes ``labels`` too, then calls ``replay``."""
        if self.graph is None:
            raise RuntimeError("MoleculeSampler(graph=False) has no static inputs")
        if self._labels is None:
            raise RuntimeError("MoleculeSampler was captured with an edge batch that is not one-hot: it has no label buffer "
                               "(the graph embeds the dense tensor); refresh it through sample()")
        return self.static_edge, self._labels, self.static_node

    def replay(self):
        """Forward and decode of whatever the static inputs hold now: ``(batch, node_sample, edge_sample)`` in static buffers."""
        if self.graph is None:
            raise RuntimeError("MoleculeSampler(graph=False) has nothing to replay")
        if [p.data_ptr() for p in self.G.parameters()] != self._param_ptrs:
            self._capture()      # parameters were moved (not just overwritten) since the capture
        self.graph.replay()
        return self._static_out

    def sample_from(self, store, index, *, keep_logits: bool = False):
        """``sample`` on the molecules ``index`` (int64 ``[B]``) of a ``resident.ResidentMolecules``.  Graphed: ``dg_mol_gather``
        writes straight into the static inputs -- dense buffers and labels together -- and the graph is replayed; eager:
        ``sample`` on the gathered batch, whose one-hot labels the store guarantees.  ``ValueError`` before any launch when the
        store's ``(N, b_dim, m_dim)`` differ from the sampler's batch or, graphed, the index length from its ``B``."""
        B = int(index.shape[0]) if torch.is_tensor(index) else len(index)
        edge_shape, node_shape = self._shape
        N, E, M = store.vertexes, store.b_dim, store.m_dim
        if (N, N, E) != edge_shape[1:] or (N, M) != node_shape[1:]:
            raise ValueError(f"sample_from: the store holds N={N}, b_dim={E}, m_dim={M}; the sampler was built for edge "
                             f"{edge_shape} / node {node_shape}")
        if self.graph is None:
            _, a, x = store.batch(index)
            return self.sample(a, x, keep_logits=keep_logits, check_one_hot=False)
        if B != edge_shape[0]:
            raise ValueError(f"sample_from: {B} indices, the sampler was captured for batches of {edge_shape[0]}")
        self._check_activation_dtype()
        store.batch(index, out=self.inputs())
        out = self.replay()
        return out if keep_logits else out[0]
