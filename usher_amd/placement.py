"""Python mirror of the placement C ABI (include/usher_amd.h).

Mirrors, for a batch of samples on a static tree, the reference's per-sample
block usher_common.cpp:342-449 (`mapper2_body` over every BFS node, then the
tie pass): `Placer.place` returns per sample the reference's
`best_set_difference`, `num_best`, `best_j` (BFS index) and `has_unique`
(usher_graph.hpp:79-92).  All compute happens in libusher_amd.so on the GPU.
"""
from __future__ import annotations

import ctypes as C
from typing import Dict, List, Optional, Sequence

import numpy as np

from . import _lib
from ._lib import build_library  # noqa: F401

RESULT_DTYPE = np.dtype([("best_set_difference", np.int32), ("num_best", np.uint32), ("best_j", np.uint32),
                         ("best_has_unique", np.uint32)])


class UgpError(RuntimeError):
    def __init__(self, code: int, msg: str):
        super().__init__("ugp error %d: %s" % (code, msg))
        self.code = code


def _check(rc: int) -> None:
    if rc != 0:
        raise UgpError(rc, (_lib.lib().ugp_last_error() or b"").decode())


def _ptr(a: Optional[np.ndarray]):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


class _TreeArrays:
    """Keeps numpy arrays alive and typed for a ugp_tree_desc."""

    def __init__(self, arrays: Dict):
        n = int(arrays["n"])
        parent = np.asarray(arrays["parent"]).astype(np.int64)
        par32 = np.where(parent < 0, 0xFFFFFFFF, parent).astype(np.uint32)
        self.n = n
        self.parent = np.ascontiguousarray(par32)
        self.mut_off = np.ascontiguousarray(arrays["mut_off"], dtype=np.uint64)
        self.mut_pos = np.ascontiguousarray(arrays["mut_pos"], dtype=np.int32)
        self.mut_ref = np.ascontiguousarray(arrays["mut_ref"]).astype(np.uint8)
        self.mut_par = np.ascontiguousarray(arrays["mut_par"]).astype(np.uint8)
        self.mut_nuc = np.ascontiguousarray(arrays["mut_nuc"]).astype(np.uint8)
        self.desc = _lib.ugp_tree_desc(n, _ptr(self.parent), _ptr(self.mut_off), _ptr(self.mut_pos),
                                       _ptr(self.mut_ref), _ptr(self.mut_par), _ptr(self.mut_nuc))


class QueryBatch:
    """CSR batch of query samples (the rows read_vcf() puts in Missing_Sample::mutations)."""

    def __init__(self, samples: Sequence[Dict]):
        self.names = [s.get("name", "q%d" % i) for i, s in enumerate(samples)]
        lens = [len(s["pos"]) for s in samples]
        self.ent_off = np.zeros(len(samples) + 1, dtype=np.uint64)
        if lens:
            self.ent_off[1:] = np.cumsum(lens)
        cat = lambda k, dt: (np.concatenate([np.asarray(s[k]) for s in samples]).astype(dt) if lens and sum(lens)
                             else np.zeros(0, dt))
        self.pos = np.ascontiguousarray(cat("pos", np.int32))
        self.ref = np.ascontiguousarray(cat("ref", np.uint8))
        self.nuc = np.ascontiguousarray(cat("nuc", np.uint8))
        self.is_missing = np.ascontiguousarray(cat("is_missing", np.uint8))
        self.desc = _lib.ugp_queries(len(samples), _ptr(self.ent_off), _ptr(self.pos), _ptr(self.ref), _ptr(self.nuc),
                                     _ptr(self.is_missing))

    @classmethod
    def from_csr(cls, ent_off, pos, ref, nuc, is_missing, names=None) -> "QueryBatch":
        self = cls.__new__(cls)
        self.ent_off = np.ascontiguousarray(ent_off, dtype=np.uint64)
        self.pos = np.ascontiguousarray(pos, dtype=np.int32)
        self.ref = np.ascontiguousarray(ref, dtype=np.uint8)
        self.nuc = np.ascontiguousarray(nuc, dtype=np.uint8)
        self.is_missing = np.ascontiguousarray(is_missing, dtype=np.uint8)
        n = len(self.ent_off) - 1
        self.names = list(names) if names is not None else ["q%d" % i for i in range(n)]
        self.desc = _lib.ugp_queries(n, _ptr(self.ent_off), _ptr(self.pos), _ptr(self.ref), _ptr(self.nuc),
                                     _ptr(self.is_missing))
        return self

    def __len__(self) -> int:
        return len(self.ent_off) - 1

    def slice(self, lo: int, hi: int) -> "QueryBatch":
        e0, e1 = int(self.ent_off[lo]), int(self.ent_off[hi])
        return QueryBatch.from_csr(self.ent_off[lo:hi + 1] - self.ent_off[lo], self.pos[e0:e1], self.ref[e0:e1],
                                   self.nuc[e0:e1], self.is_missing[e0:e1], self.names[lo:hi])


class FlatTreeView:
    """Host-only view of the flattened tree (no GPU needed): what ugp_mat_create uploads."""

    IDS = {"stream": (0, np.uint32), "pre_stream": (1, np.uint32), "chunk_body_off": (2, np.uint32),
           "chunk_pre_off": (3, np.uint32), "chunk_node_off": (4, np.uint32), "pos2site": (5, np.int32),
           "site_ref": (6, np.uint8), "rank2bfs": (7, np.uint32), "dfs2bfs": (8, np.uint32),
           "stream8": (10, np.uint32), "pre8_stream": (11, np.uint32), "chunk8_body_off": (12, np.uint32),
           "chunk8_pre_off": (13, np.uint32), "stream_t": (15, np.uint32), "chunk_t_off": (16, np.uint32),
           "b3_group_off": (18, np.uint32), "b3_events": (19, np.uint32)}

    def __init__(self, arrays: Dict, chunk_nodes: int = 0):
        L = _lib.lib()
        self._t = _TreeArrays(arrays)
        h = C.c_void_p()
        _check(L.ugp_flat_create(C.byref(self._t.desc), chunk_nodes, C.byref(h)))
        try:
            for name, (which, dt) in self.IDS.items():
                p = C.c_void_p()
                n = C.c_uint64()
                _check(L.ugp_flat_get(h, which, C.byref(p), C.byref(n)))
                if n.value:
                    buf = (C.c_char * (n.value * np.dtype(dt).itemsize)).from_address(p.value)
                    setattr(self, name, np.frombuffer(buf, dtype=dt).copy())
                else:
                    setattr(self, name, np.zeros(0, dt))
            p = C.c_void_p()
            n = C.c_uint64()
            _check(L.ugp_flat_get(h, 9, C.byref(p), C.byref(n)))
            self.max_slots = int(n.value)
            _check(L.ugp_flat_get(h, 14, C.byref(p), C.byref(n)))
            self.max_path_muts = int(n.value)
            _check(L.ugp_flat_get(h, 17, C.byref(p), C.byref(n)))
            self.lds_slots = int(n.value)
        finally:
            L.ugp_flat_destroy(h)


class Placer:
    """A flattened MAT resident on one GPU (ugp_mat) plus the batch entry points."""

    def __init__(self, arrays: Dict, device: int = 0, chunk_nodes: Optional[int] = None, experiments: bool = False, flat_file: Optional[str] = None):
        """experiments=True binds libusher_amd_exp.so (built with -DUGP_EXPERIMENTS: UGP_STATS, UGP_TRACE, UGP_SEED_*,
        UGP_PHASE2_PACKED, UGP_KBEST_EXCLUSIVE); the release library ignores those variables.  The tuning switches are read
        from the environment here, once; reload_knobs() reads them again.  flat_file: a flattening of these arrays written by
        save_flat() (ugp_flat_save) -- uploaded as it is, no flattening in this process (the other ranks of a multi-GPU launch)."""
        L = self._L = _lib.lib(experiments)
        self._t = _TreeArrays(arrays)
        self.n_nodes = self._t.n
        self._h = C.c_void_p()
        if flat_file is not None:
            self._ck(L.ugp_mat_create_from_flat(flat_file.encode(), device, C.byref(self._h)))
        elif chunk_nodes is None:
            self._ck(L.ugp_mat_create(C.byref(self._t.desc), device, C.byref(self._h)))
        else:
            self._ck(L.ugp_mat_create_chunked(C.byref(self._t.desc), device, int(chunk_nodes), C.byref(self._h)))
        self.device = device

    def _ck(self, rc: int) -> None:
        if rc != 0:
            raise UgpError(rc, (self._L.ugp_last_error() or b"").decode())

    @staticmethod
    def save_flat(arrays: Dict, path: str, experiments: bool = False) -> None:
        """ugp_flat_save: flatten `arrays` once and write the result to `path` for Placer(..., flat_file=path) in other processes."""
        L = _lib.lib(experiments)
        t = _TreeArrays(arrays)
        rc = L.ugp_flat_save(C.byref(t.desc), path.encode())
        if rc != 0:
            raise UgpError(rc, (L.ugp_last_error() or b"").decode())

    def reload_knobs(self) -> None:
        """ugp_mat_reload_knobs: the per-call tuning switches from the environment again (test / tuning hook)."""
        self._ck(self._L.ugp_mat_reload_knobs(self._h))

    def close(self) -> None:
        if getattr(self, "_h", None) and self._h.value:
            self._L.ugp_mat_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def info(self) -> Dict:
        out = _lib.ugp_info()
        self._ck(self._L.ugp_mat_info(self._h, C.byref(out)))
        return {k: getattr(out, k) for k, _ in out._fields_}

    def place(self, batch: QueryBatch) -> np.ndarray:
        """ugp_place_batch: structured array (best_set_difference, num_best, best_j, best_has_unique)."""
        out = np.zeros(len(batch), dtype=RESULT_DTYPE)
        self._ck(self._L.ugp_place_batch(self._h, C.byref(batch.desc), _ptr(out)))
        return out

    def place_async(self, batch: QueryBatch):
        """ugp_place_batch_async: starts the batch and returns a job; job_wait(job) gives the same array as place().  At most
        pipeline_depth() jobs may be outstanding (two for batches of more than 32,768 samples or of 128 rows per sample and more); the
        batch's arrays may be reused as soon as this returns."""
        out = np.zeros(len(batch), dtype=RESULT_DTYPE)
        job = C.c_void_p()
        self._ck(self._L.ugp_place_batch_async(self._h, C.byref(batch.desc), _ptr(out), C.byref(job)))
        return (job, out)

    def job_wait(self, job) -> np.ndarray:
        h, out = job
        self._ck(self._L.ugp_job_wait(h))
        return out

    def scores_per_node(self, batch: QueryBatch) -> np.ndarray:
        out = np.zeros((len(batch), self.n_nodes), dtype=np.int32)
        self._ck(self._L.ugp_scores_per_node(self._h, C.byref(batch.desc), _ptr(out)))
        return out

    def tied_nodes(self, batch: QueryBatch, cap: int):
        tj = np.zeros((len(batch), max(cap, 1)), dtype=np.uint32)
        th = np.zeros((len(batch), max(cap, 1)), dtype=np.uint8)
        tc = np.zeros(len(batch), dtype=np.uint32)
        self._ck(self._L.ugp_tied_nodes(self._h, C.byref(batch.desc), cap, _ptr(tj), _ptr(th), _ptr(tc)))
        return [tj[i, :min(int(tc[i]), cap)].copy() for i in range(len(batch))], \
               [th[i, :min(int(tc[i]), cap)].astype(bool) for i in range(len(batch))], tc

    # ---- the other callers of mapper2_body (matUtils uncertainty / annotate / merge, ripples) -------------
    def _opts(self, batch, order, node_mask, skip_node, distance, scores):
        keep = [None if a is None else np.ascontiguousarray(a, dtype=dt) for a, dt in
                ((node_mask, np.uint8), (skip_node, np.uint32), (distance, np.uint32))]
        if keep[0] is not None and len(keep[0]) != self.n_nodes or keep[2] is not None and len(keep[2]) != self.n_nodes:
            raise ValueError("node_mask / distance need one entry per node")
        if keep[1] is not None and len(keep[1]) != len(batch):
            raise ValueError("skip_node needs one entry per sample")
        o = _lib.ugp_place_opts({"bfs": 0, "dfs": 1}[order], _ptr(keep[0]), _ptr(keep[1]), _ptr(keep[2]), _ptr(scores))
        return o, keep

    def place_ex(self, batch: QueryBatch, order: str = "bfs", node_mask=None, skip_node=None, distance=None, want_scores: bool = False):
        """ugp_place_batch_ex: every node index (mask, skip_node, best_j, score columns) is a position in `order`."""
        out = np.zeros(len(batch), dtype=RESULT_DTYPE)
        scores = np.zeros((len(batch), self.n_nodes), dtype=np.int32) if want_scores else None
        o, keep = self._opts(batch, order, node_mask, skip_node, distance, scores)
        self._ck(self._L.ugp_place_batch_ex(self._h, C.byref(batch.desc), C.byref(o), _ptr(out)))
        return (out, scores) if want_scores else out

    def tied_nodes_ex(self, batch: QueryBatch, cap: int, order: str = "bfs", node_mask=None, skip_node=None, distance=None):
        tj = np.zeros((len(batch), max(cap, 1)), dtype=np.uint32)
        th = np.zeros((len(batch), max(cap, 1)), dtype=np.uint8)
        tc = np.zeros(len(batch), dtype=np.uint32)
        o, keep = self._opts(batch, order, node_mask, skip_node, distance, None)
        self._ck(self._L.ugp_tied_nodes_ex(self._h, C.byref(batch.desc), C.byref(o), cap, _ptr(tj), _ptr(th), _ptr(tc)))
        return [tj[i, :min(int(tc[i]), cap)].copy() for i in range(len(batch))], \
               [th[i, :min(int(tc[i]), cap)].astype(bool) for i in range(len(batch))], tc

    def prepare_ex(self, order: str = "bfs", node_mask=None, distance=None):
        """ugp_ex_prepare: the node-level options of an extended search (order, mask, distance) made ready once; returns a handle for
        place_prepared / free_ex."""
        o, keep = self._opts(None, order, node_mask, None, distance, None)
        h = C.c_void_p()
        self._ck(self._L.ugp_ex_prepare(self._h, C.byref(o), C.byref(h)))
        return h

    def free_ex(self, h) -> None:
        if h:
            self._L.ugp_ex_destroy(h)

    def place_prepared(self, batch: QueryBatch, ex, skip_node=None, d_scores: int = 0):
        """ugp_place_batch_prepared; d_scores = device pointer to len(batch) * n_nodes int32 (e.g. torch tensor .data_ptr()), or 0."""
        out = np.zeros(len(batch), dtype=RESULT_DTYPE)
        sk = None if skip_node is None else np.ascontiguousarray(skip_node, dtype=np.uint32)
        if sk is not None and len(sk) != len(batch):
            raise ValueError("skip_node must have one entry per query")
        self._ck(self._L.ugp_place_batch_prepared(self._h, C.byref(batch.desc), ex, None if sk is None else _ptr(sk), _ptr(out), C.c_void_p(d_scores) if d_scores else None))
        return out

    def uncertainty_attach(self, arrays: Optional[Dict] = None):
        """ugp_uncertainty_attach with the placer's own tree, or with other mutation arrays on the same topology (masked entries,
        ambiguous alleles: trees the placement tables refuse).  The depth-first tables are shared as genotypes_attach describes."""
        t = self._t if arrays is None else _TreeArrays(arrays)
        self._ck(self._L.ugp_uncertainty_attach(self._h, C.byref(t.desc)))
        self._unc_ready = True

    def uncertainty(self, nodes, cap: int = 64):
        """matUtils uncertainty (ugp_uncertainty) for tree nodes given by BFS index: (epps, neighborhood_size, ties, tie_count),
        ties[i] = the first min(cap, tie_count[i]) tied nodes as depth-first positions, ascending.  The tables are made on
        the first call (uncertainty_attach) from the arrays this Placer was built from; on a handle whose depth-first tables
        another attach built from other arrays, call uncertainty_attach with those arrays first."""
        if not getattr(self, "_unc_ready", False):
            self.uncertainty_attach()
        nodes = np.ascontiguousarray(nodes, dtype=np.uint32)
        n = len(nodes)
        epps = np.zeros(n, np.uint32); nsize = np.zeros(n, np.uint32); cnt = np.zeros(n, np.uint32)
        ties = np.zeros((n, cap), np.uint32)
        self._ck(self._L.ugp_uncertainty(self._h, _ptr(nodes), n, int(cap), _ptr(epps), _ptr(nsize), _ptr(ties), _ptr(cnt)))
        return epps, nsize, [ties[i, :min(int(cnt[i]), cap)].copy() for i in range(n)], cnt

    # ---- matUtils annotate (ugp_annotate_attach / ugp_clade_alleles / ugp_clade_descendants / ugp_annotate_search) ------
    def annotate_attach(self, arrays: Optional[Dict] = None):
        """ugp_annotate_attach with the placer's own tree, or with other mutation arrays on the same topology (masked entries,
        ambiguous alleles, a position twice on one node: trees the placement tables refuse).  The depth-first tables are shared as
        genotypes_attach describes."""
        t = self._t if arrays is None else _TreeArrays(arrays)
        self._ck(self._L.ugp_annotate_attach(self._h, C.byref(t.desc)))
        self._ann_attached = True

    def _ann_ready(self):
        """The annotate tables, made on the first call (annotate_attach) from the arrays this Placer was built from."""
        if not getattr(self, "_ann_attached", False):
            self.annotate_attach()

    @staticmethod
    def _clades_csr(clades):
        off = np.zeros(len(clades) + 1, np.uint64)
        if len(clades):
            off[1:] = np.cumsum([len(c) for c in clades])
        nodes = np.ascontiguousarray(np.concatenate([np.asarray(c, np.uint32) for c in clades]) if int(off[-1]) else
                                     np.zeros(0, np.uint32), dtype=np.uint32)
        return off, nodes

    def clade_alleles(self, clades):
        """Clade allele counts of matUtils annotate (annotate.cpp:355-390): clades[c] = exemplar nodes (BFS indices, repeats
        count).  Returns one (entries, counts) pair per clade: the tree's mutation entries (indices into the mutation CSR) that
        the exemplars' root-path walks add, in depth-first order of their node, and how many exemplars add each."""
        self._ann_ready()
        off, nodes = self._clades_csr(clades)
        n = len(clades)
        out_off = np.zeros(n + 1, np.uint64)
        n_out = C.c_uint64(0)
        cap = max(1024, 8 * len(nodes))
        while True:
            ent = np.zeros(cap, np.uint32); cnt = np.zeros(cap, np.uint32)
            self._ck(self._L.ugp_clade_alleles(self._h, _ptr(off), _ptr(nodes), n, _ptr(out_off), _ptr(ent), _ptr(cnt), cap,
                                               C.byref(n_out)))
            if n_out.value <= cap:
                break
            cap = int(n_out.value)
        return [(ent[int(out_off[c]):int(out_off[c + 1])].copy(), cnt[int(out_off[c]):int(out_off[c + 1])].copy()) for c in range(n)]

    def clade_descendants(self, clades, pair_clade, pair_node) -> np.ndarray:
        """Exemplars of clade pair_clade[i] strictly below node pair_node[i] (BFS): get_freq_overlap's count (annotate.cpp:466-481)."""
        self._ann_ready()
        off, nodes = self._clades_csr(clades)
        pc = np.ascontiguousarray(pair_clade, dtype=np.uint32)
        pn = np.ascontiguousarray(pair_node, dtype=np.uint32)
        if len(pc) != len(pn):
            raise ValueError("pair_clade and pair_node need the same length")
        out = np.zeros(len(pc), np.uint32)
        self._ck(self._L.ugp_clade_descendants(self._h, _ptr(off), _ptr(nodes), len(clades), _ptr(pc), _ptr(pn), len(pc), _ptr(out)))
        return out

    def annotate_search(self, batch: QueryBatch, cap: int = 1024):
        """annotate's search (annotate.cpp:611-638) run literally for any rows (repeated or masked positions included):
        (best, ties, tie_count), ties[i] = the first min(cap, tie_count[i]) tied depth-first positions, ascending."""
        self._ann_ready()
        n = len(batch)
        best = np.zeros(n, np.int32); cnt = np.zeros(n, np.uint32)
        ties = np.zeros((n, max(cap, 1)), np.uint32)
        self._ck(self._L.ugp_annotate_search(self._h, C.byref(batch.desc), int(cap), _ptr(best), _ptr(ties), _ptr(cnt)))
        return best, [ties[i, :min(int(cnt[i]), cap)].copy() for i in range(n)], cnt

    NEAREST_INFO = np.dtype([("count", np.uint32), ("anc", np.uint32), ("last_anc", np.uint32), ("cut_dist", np.uint32),
                             ("n_at_cut", np.uint32)])

    def nearest_attach(self, arrays: Optional[Dict] = None):
        """ugp_nearest_attach with the placer's own tree, or with other mutation arrays on the same topology (masked entries, a
        position twice on one node: trees the placement tables refuse).  The depth-first tables are shared as genotypes_attach
        describes."""
        t = self._t if arrays is None else _TreeArrays(arrays)
        self._ck(self._L.ugp_nearest_attach(self._h, C.byref(t.desc)))
        self._near_ready = True

    def nearest_k(self, nodes, k, out_stride: Optional[int] = None, chunk_queries: int = 0):
        """matUtils extract's k nearest samples (ugp_nearest_k, select.cpp:206-276) for tree nodes given by BFS index; k is a
        scalar or one value per query.  Returns (out_nodes, out_dist, info): row i holds min(info[i].count, out_stride) leaves
        (BFS indices) and their distances to info[i].anc -- the leaves of last_anc in depth-first order, then the nearest others,
        ties in depth-first order; info is a NEAREST_INFO array.  out_stride defaults to the largest k; chunk_queries (test hook)
        sets the queries per workspace chunk.  The tables are made on the first call (nearest_attach) from the arrays this Placer
        was built from."""
        if not getattr(self, "_near_ready", False):
            self.nearest_attach()
        nodes = np.ascontiguousarray(nodes, dtype=np.uint32)
        n = len(nodes)
        ks = np.ascontiguousarray(np.broadcast_to(np.asarray(k, dtype=np.uint32), (n,)))
        stride = int(out_stride) if out_stride is not None else (int(ks.max()) if n else 1)
        out_nodes = np.full((n, max(stride, 1)), 0xFFFFFFFF, np.uint32)
        out_dist = np.full((n, max(stride, 1)), 0xFFFFFFFF, np.uint32)
        info = np.zeros(n, self.NEAREST_INFO)
        self._ck(self._L.ugp_nearest_k_chunked(self._h, n, _ptr(nodes), _ptr(ks), stride, _ptr(out_nodes), _ptr(out_dist), _ptr(info),
                                               int(chunk_queries)))
        return out_nodes, out_dist, info

    GT_SITE = np.dtype([("pos", np.int32), ("ref", np.uint8), ("n_alt", np.uint8), ("alt", np.uint8, (14,)), ("ac", np.uint32, (14,)),
                        ("covered", np.uint32)])

    def genotypes_attach(self, arrays: Optional[Dict] = None):
        """ugp_genotypes_attach with the placer's own tree, or with other mutation arrays on the same topology (trees the
        placement tables refuse: ambiguous alleles, a node with two mutations at one position).  The depth-first tables are
        shared with uncertainty, annotate and nearest_k and built by the first of these calls on the handle: once they exist,
        arrays other than theirs are refused (UgpError -1) and the handle stays as it was."""
        t = self._t if arrays is None else _TreeArrays(arrays)
        self._ck(self._L.ugp_genotypes_attach(self._h, C.byref(t.desc)))
        self._gt_ready = True
        self._gt_shape = None

    def genotype_select(self, nodes=None):
        """matUtils extract -v for a selection of tree nodes (BFS indices; None or empty: all leaves): ranks the selection, counts
        the alleles and builds the VCF site table on the device (ugp_genotype_select, convert.cpp:53-292).  Returns
        (n_cols, n_sites); the selection stays on the handle until the next call.  The tables are made on the first call
        (ugp_genotypes_attach)."""
        if not getattr(self, "_gt_ready", False):
            self.genotypes_attach()
        sel = np.ascontiguousarray(nodes if nodes is not None else [], dtype=np.uint32)
        ncols, nsites = C.c_uint32(0), C.c_uint64(0)
        self._ck(self._L.ugp_genotype_select(self._h, _ptr(sel) if len(sel) else None, len(sel), C.byref(ncols), C.byref(nsites)))
        self._gt_shape = (int(ncols.value), int(nsites.value))
        return self._gt_shape

    def _gt_range(self, lo, hi):
        if getattr(self, "_gt_shape", None) is None:
            raise UgpError(-1, "no selection: call genotype_select first")
        return int(lo), self._gt_shape[1] if hi is None else int(hi)

    def genotype_columns(self):
        """The selected nodes (BFS indices) in depth-first order: the columns of genotype_rows."""
        self._gt_range(0, 0)
        out = np.zeros(self._gt_shape[0], np.uint32)
        self._ck(self._L.ugp_genotype_columns(self._h, _ptr(out)))
        return out

    def genotype_sites(self, lo=0, hi=None):
        """Rows [lo, hi) of the site table as a GT_SITE array, ascending by position."""
        lo, hi = self._gt_range(lo, hi)
        out = np.zeros(max(hi - lo, 0), self.GT_SITE)
        self._ck(self._L.ugp_genotype_sites(self._h, lo, hi, _ptr(out)))
        return out

    def genotype_rows(self, lo=0, hi=None, chunk_cells: int = 0):
        """The genotype codes of sites [lo, hi): a uint8 array [hi - lo, n_cols].  chunk_cells (test hook) sets the cells per
        workspace window."""
        lo, hi = self._gt_range(lo, hi)
        out = np.zeros((max(hi - lo, 0), self._gt_shape[0]), np.uint8)
        self._ck(self._L.ugp_genotype_rows_chunked(self._h, lo, hi, _ptr(out), int(chunk_cells)))
        return out

    def genotype_rows_time(self, lo=0, hi=None, reps: int = 5) -> float:
        """Bench hook: milliseconds of device time of the row kernel alone over sites [lo, hi), no copy to the host."""
        lo, hi = self._gt_range(lo, hi)
        ms = C.c_double(0)
        self._ck(self._L.ugp_genotype_rows_time(self._h, lo, hi, int(reps), C.byref(ms)))
        return float(ms.value)

    # ---- matUtils summary (ugp_summary_attach / _mutations / _roho / _clades) ---------------------------------------------
    SM_MUTATION = np.dtype([("pos", np.int32), ("par", np.uint8), ("nuc", np.uint8), ("pad", np.uint8, (2,)), ("count", np.uint32)])
    SM_ROHO = np.dtype([("parent", np.uint32), ("child", np.uint32), ("entry", np.uint32), ("child_count", np.uint32),
                        ("offspring_with", np.uint32), ("median_without", np.uint32)])
    SM_CLADE = np.dtype([("column", np.uint32), ("node", np.uint32), ("inclusive", np.uint32), ("exclusive", np.uint32)])

    def summary_attach(self, arrays: Optional[Dict] = None):
        """ugp_summary_attach with the placer's own tree, or with other mutation arrays on the same topology (masked entries, a key
        twice on one node: trees the placement tables refuse).  The depth-first tables are shared as genotypes_attach describes."""
        t = self._t if arrays is None else _TreeArrays(arrays)
        self._ck(self._L.ugp_summary_attach(self._h, C.byref(t.desc)))
        self._sm_ready = True

    def _sm_records(self, fn, dtype, chunk_items, cap):
        if not getattr(self, "_sm_ready", False):
            self.summary_attach()
        n_out = C.c_uint64(0)
        if cap is None:   # the two-call convention: the count, then the records
            self._ck(fn(self._h, None, 0, C.byref(n_out), int(chunk_items)))
            cap = int(n_out.value)
        out = np.zeros(int(cap), dtype)
        self._ck(fn(self._h, _ptr(out) if cap else None, int(cap), C.byref(n_out), int(chunk_items)))
        self._sm_n_out = int(n_out.value)
        return out[:min(int(cap), self._sm_n_out)]

    def summary_mutations(self, chunk_items: int = 0, cap: Optional[int] = None):
        """matUtils summary -m (summary.cpp:139-174): an SM_MUTATION array of the distinct non-masked (pos, stored parent allele,
        allele) with their number of occurrences over all nodes, ascending.  chunk_items (test hook): list entries per launch
        window; cap (test hook): room for that many records only, the true count is then in _sm_n_out."""
        return self._sm_records(self._L.ugp_summary_mutations_chunked, self.SM_MUTATION, chunk_items, cap)

    def summary_roho(self, chunk_items: int = 0, cap: Optional[int] = None):
        """matUtils summary -R (summary.cpp:343-506, without dates): an SM_ROHO array, one record per reported (parent, mutation),
        ascending by the depth-first position of the parent; nodes are BFS indices, `entry` indexes the mutation CSR."""
        return self._sm_records(self._L.ugp_summary_roho_chunked, self.SM_ROHO, chunk_items, cap)

    def summary_clades(self, columns):
        """matUtils summary -c / -C (summary.cpp:88-137, 297-341): columns[c] = the nodes (BFS) with a non-empty annotation in column
        c.  Returns (per_node, leaf_clade): an SM_CLADE array in the order given -- the leaves strictly below each node and the
        leaves whose nearest annotated strict ancestor in that column it is -- and a uint32 array [n_columns, n_leaves]: that
        ancestor for every leaf in BFS order, 0xFFFFFFFF when there is none."""
        if not getattr(self, "_sm_ready", False):
            self.summary_attach()
        off, nodes = self._clades_csr(columns)
        n_leaves = self._t.n - len(np.unique(self._t.parent[1:]))
        per = np.zeros(len(nodes), self.SM_CLADE)
        per["column"] = np.repeat(np.arange(len(columns), dtype=np.uint32), np.diff(off).astype(np.int64))
        per["node"] = nodes
        incl = np.zeros(len(nodes), np.uint32); excl = np.zeros(len(nodes), np.uint32)
        leaf_clade = np.zeros((len(columns), n_leaves), np.uint32)
        self._ck(self._L.ugp_summary_clades(self._h, _ptr(off), _ptr(nodes), len(columns), _ptr(incl), _ptr(excl), _ptr(leaf_clade)))
        per["inclusive"] = incl
        per["exclusive"] = excl
        return per, leaf_clade

    def summary_time(self, reps: int = 5):
        """Bench hook: (sort_ms, roho_ms), the device time of the occurrence-list sort and of the RoHo kernel over every candidate."""
        if not getattr(self, "_sm_ready", False):
            self.summary_attach()
        a, b = C.c_double(0), C.c_double(0)
        self._ck(self._L.ugp_summary_time(self._h, int(reps), C.byref(a), C.byref(b)))
        return float(a.value), float(b.value)

    # ---- matUtils summary --translate (ugp_translate_attach / _codons / ugp_translate) ----------------------------------------
    TR_RECORD = np.dtype([("node", np.uint32), ("codon", np.uint32), ("before", np.uint8, (3,)), ("after", np.uint8, (3,)),
                          ("pad", np.uint8, (2,)), ("ent", np.uint32, (3,))])
    TR_INFO = np.dtype([("n_records", np.uint64), ("n_nodes", np.uint64), ("n_inconsistent", np.uint64), ("n_duplicate", np.uint64),
                        ("first_inconsistent", np.uint32), ("first_duplicate", np.uint32)])

    def translate_attach(self, arrays: Optional[Dict] = None):
        """ugp_translate_attach with the placer's own tree, or with other mutation arrays on the same topology (masked entries,
        ambiguous alleles, a position twice on one node: trees the placement tables refuse).  The depth-first tables are shared as
        genotypes_attach describes."""
        t = self._t if arrays is None else _TreeArrays(arrays)
        self._ck(self._L.ugp_translate_attach(self._h, C.byref(t.desc)))
        self._tr_ready = True

    def translate_codons(self, slot_pos, slot_init):
        """ugp_translate_codons: the codon table in the reference's creation order.  slot_pos [n, 3]: 1-based positions as mut_pos
        (descending for a '-' codon); slot_init [n, 3]: the letters before any mutation (bytes, or a str / bytes of 3 n letters).
        Replaces any earlier table."""
        if not getattr(self, "_tr_ready", False):
            self.translate_attach()
        pos = np.ascontiguousarray(slot_pos, dtype=np.int32).reshape(-1)
        if isinstance(slot_init, str):
            slot_init = slot_init.encode()
        init = (np.frombuffer(slot_init, np.uint8) if isinstance(slot_init, (bytes, bytearray))
                else np.ascontiguousarray(slot_init, dtype=np.uint8).reshape(-1))
        init = np.ascontiguousarray(init)
        if len(pos) % 3 or len(pos) != len(init):
            raise UgpError(-1, "slot_pos and slot_init hold three values per codon")
        self._ck(self._L.ugp_translate_codons(self._h, len(pos) // 3, _ptr(pos), _ptr(init)))

    def translate(self, chunk_items: int = 0, cap: Optional[int] = None):
        """matUtils summary --translate (translate.cpp, do_mutations in TSV mode): (records, info) -- a TR_RECORD array, one record per
        (node, codon its mutations touch), ascending by (depth-first position of the node, lowest mutated position of the codon on
        it, codon index), and a TR_INFO scalar.  A tree whose stored parent alleles disagree with the states above them, or with
        a coding position twice on one node, raises UgpError -2 (the serial walk is history dependent there); the TR_INFO of the
        last call, refused or not, stays in _tr_info.  chunk_items (test hook): work-items per launch window; cap (test hook):
        room for that many records only."""
        info = np.zeros(1, self.TR_INFO)
        self._tr_info = None
        n_out = C.c_uint64(0)
        fn = self._L.ugp_translate_chunked

        def call(buf, room):
            rc = fn(self._h, _ptr(buf) if room else None, int(room), C.byref(n_out), _ptr(info), int(chunk_items))
            if rc != -1:   # (an invalid call fills nothing)
                self._tr_info = info[0].copy()
            self._ck(rc)

        if cap is None:   # the two-call convention: the count, then the records
            call(None, 0)
            cap = int(n_out.value)
        out = np.zeros(int(cap), self.TR_RECORD)
        call(out, cap)
        self._tr_n_out = int(n_out.value)
        return out[:min(int(cap), self._tr_n_out)], info[0].copy()

    def translate_time(self, reps: int = 5) -> float:
        """Bench hook: milliseconds of device time of the passes of ugp_translate alone, no copy to the host."""
        ms = C.c_double(0)
        self._ck(self._L.ugp_translate_time(self._h, int(reps), C.byref(ms)))
        return float(ms.value)

    # ---- matUtils extract --closest-relatives / --within-distance (ugp_relatives_*) ---------------------------------------
    REL_INFO = np.dtype([("dist", np.uint32), ("count", np.uint32), ("levels", np.uint32), ("best", np.uint32)])
    REL_BLOCK = 16   # UGP_REL_BLOCK: leaves per block of the range minima (the tests aim at its edges)

    @staticmethod
    def name_ranks(names) -> np.ndarray:
        """The name_rank of relatives_attach: names[j]'s place in the order of std::string::operator<, which compares unsigned
        bytes (equal names, which a tree does not have, keep their index order)."""
        keys = [s if isinstance(s, bytes) else str(s).encode() for s in names]
        order = sorted(range(len(keys)), key=lambda j: (keys[j], j))
        rank = np.empty(len(keys), np.uint32)
        rank[order] = np.arange(len(keys), dtype=np.uint32)
        return rank

    def relatives_attach(self, name_rank=None, arrays: Optional[Dict] = None):
        """ugp_relatives_attach with the placer's own tree, or with other mutation arrays on the same topology: the leaf tables,
        range minima and (cum, leaf) order of the relatives calls.  name_rank [n] by BFS index (name_ranks(names)) lets
        relatives_closest report the relative with the smallest name; None: no ranks.  A later attach replaces the tables.  The
        depth-first tables are shared as genotypes_attach describes."""
        rank = None if name_rank is None else np.ascontiguousarray(name_rank, dtype=np.uint32)
        if rank is not None and len(rank) != self.n_nodes:
            raise UgpError(-1, "name_rank holds one rank per node")
        t = self._t if arrays is None else _TreeArrays(arrays)
        self._ck(self._L.ugp_relatives_attach(self._h, C.byref(t.desc), None if rank is None else _ptr(rank)))
        self._rel_ready = True

    def _relatives(self, call, nodes, lists, cap):
        if not getattr(self, "_rel_ready", False):
            self.relatives_attach()
        nodes = np.ascontiguousarray(nodes, dtype=np.uint32)
        n = len(nodes)
        info = np.zeros(n, self.REL_INFO)
        n_out = C.c_uint64(0)
        if not lists:
            self._ck(call(_ptr(nodes) if n else None, n, _ptr(info) if n else None, None, None, 0, C.byref(n_out)))
            self._rel_n_out = int(n_out.value)
            return info, None, None
        off = np.zeros(n + 1, np.uint64)
        room = int(cap) if cap is not None else max(4 * n, 1024)
        while True:   # grow and retry: the call reports the true total
            out = np.full(room, 0xFFFFFFFF, np.uint32)
            self._ck(call(_ptr(nodes) if n else None, n, _ptr(info) if n else None, _ptr(off), _ptr(out) if room else None, room, C.byref(n_out)))
            self._rel_n_out = int(n_out.value)
            if cap is not None or self._rel_n_out <= room:
                return info, off, out[:min(room, self._rel_n_out)]
            room = self._rel_n_out

    def relatives_closest(self, nodes, lists: bool = True, chunk_samples: int = 0, cap: Optional[int] = None):
        """matUtils extract --closest-relatives (get_closest_samples with fixed_k = false, select.cpp:577-714) for tree nodes given
        by BFS index.  Returns (info, off, nodes): info a REL_INFO array (dist, count, levels, best -- the closest relative with
        the smallest name rank, 0xFFFFFFFF without ranks or relatives); the relatives of sample i are nodes[off[i]:off[i + 1]]
        (BFS indices), level by level in depth-first order.  lists=False: only info (off and nodes are None).  chunk_samples
        (test hook): samples per workspace chunk; cap (test hook): room for that many list entries only, the true total is then
        in _rel_n_out.  The tables are made on the first call (relatives_attach without ranks)."""
        fn = self._L.ugp_relatives_closest_chunked
        return self._relatives(lambda nd, n, info, off, out, room, n_out: fn(self._h, n, nd, info, off, out, room, n_out, int(chunk_samples)),
                               nodes, lists, cap)

    def relatives_within(self, nodes, threshold: int, lists: bool = True, chunk_samples: int = 0, cap: Optional[int] = None):
        """matUtils extract --within-distance (get_closest_samples with fixed_k = true): the leaves within `threshold` mutation
        entries of each node, as relatives_closest returns them; dist is 0 and best 0xFFFFFFFF."""
        fn = self._L.ugp_relatives_within_chunked
        return self._relatives(lambda nd, n, info, off, out, room, n_out: fn(self._h, n, nd, int(threshold), info, off, out, room, n_out,
                                                                            int(chunk_samples)), nodes, lists, cap)

    def relatives_time(self, nodes, within: bool = False, threshold: int = 0, reps: int = 5):
        """Bench hook: (count_ms, fill_ms), the device time of the two passes alone over these nodes, no copy to the host."""
        nodes = np.ascontiguousarray(nodes, dtype=np.uint32)
        a, b = C.c_double(0), C.c_double(0)
        self._ck(self._L.ugp_relatives_time(self._h, len(nodes), _ptr(nodes), int(bool(within)), int(threshold), int(reps), C.byref(a), C.byref(b)))
        return float(a.value), float(b.value)

    # ---- matUtils extract's selectors as leaf-rank bitmaps (ugp_select_*) ----------------------------------------------------
    def select_attach(self, arrays: Optional[Dict] = None):
        """ugp_select_attach with the placer's own tree, or with other mutation arrays on the same topology: the leaf-rank tables
        of the select calls.  The depth-first tables are shared as genotypes_attach describes."""
        t = self._t if arrays is None else _TreeArrays(arrays)
        self._ck(self._L.ugp_select_attach(self._h, C.byref(t.desc)))
        n = C.c_uint64(0)
        self._ck(self._L.ugp_select_leaves(self._h, None, C.byref(n)))
        self._sel_leaves = int(n.value)

    def _sel_n(self) -> int:
        if getattr(self, "_sel_leaves", None) is None:
            self.select_attach()
        return self._sel_leaves

    @staticmethod
    def _sel_mask(words, n_leaves) -> np.ndarray:
        return np.unpackbits(words.view(np.uint8), bitorder="little")[:n_leaves].astype(bool)

    @staticmethod
    def _sel_words(mask, n_leaves) -> np.ndarray:
        mask = np.ascontiguousarray(mask, dtype=bool)
        if len(mask) != n_leaves:
            raise UgpError(-1, "mask holds one flag per leaf")
        bits = np.zeros(((n_leaves + 63) // 64) * 64, np.uint8)
        bits[:n_leaves] = mask
        return np.ascontiguousarray(np.packbits(bits, bitorder="little")).view(np.uint64)

    def select_leaves(self) -> np.ndarray:
        """The leaves in depth-first order, as BFS indices: leaf rank r of the select masks is select_leaves()[r]."""
        out = np.zeros(self._sel_n(), np.uint32)
        self._ck(self._L.ugp_select_leaves(self._h, _ptr(out) if len(out) else None, None))
        return out

    def select_mutations(self, pos, nuc, chunk_queries: int = 0):
        """get_mutation_samples (select.cpp:67-111) for the queries (pos[q], nuc[q]): (mask, counts) -- mask a bool array by leaf
        rank, the OR over the queries; counts[q] the leaves of query q alone.  A leaf has a mutation when the nearest node on its
        root path, itself included, with an entry at the position carries exactly that allele there.  chunk_queries (test hook):
        queries staged per launch.  The self._sel_words of the last call keep the raw words."""
        nl = self._sel_n()
        pos = np.ascontiguousarray(pos, dtype=np.int32)
        nuc = np.ascontiguousarray(nuc, dtype=np.uint8)
        if len(pos) != len(nuc):
            raise UgpError(-1, "pos and nuc hold one value per query")
        words = np.full((nl + 63) // 64, 0xA5A5A5A5A5A5A5A5, np.uint64)
        counts = np.zeros(len(pos), np.uint64)
        self._ck(self._L.ugp_select_mutations_chunked(self._h, len(pos), _ptr(pos) if len(pos) else None, _ptr(nuc) if len(pos) else None,
                                                      _ptr(words),
                                                      _ptr(counts) if len(pos) else None, int(chunk_queries)))
        self._sel_raw = words
        return self._sel_mask(words, nl), counts

    def select_subtrees(self, nodes, chunk_ranges: int = 0):
        """(mask, counts): the union of the leaves below the nodes (BFS indices; a leaf selects itself), counts[i] per node."""
        nl = self._sel_n()
        nodes = np.ascontiguousarray(nodes, dtype=np.uint32)
        words = np.full((nl + 63) // 64, 0xA5A5A5A5A5A5A5A5, np.uint64)
        counts = np.zeros(len(nodes), np.uint64)
        self._ck(self._L.ugp_select_subtrees_chunked(self._h, len(nodes), _ptr(nodes) if len(nodes) else None,
                                                     _ptr(words),
                                                     _ptr(counts) if len(nodes) else None, int(chunk_ranges)))
        self._sel_raw = words
        return self._sel_mask(words, nl), counts

    def select_mrca(self, mask):
        """(node, n_below): the deepest node (BFS index) whose subtree holds every leaf of `mask` (bool by leaf rank), and the
        leaves below it.  An empty mask raises UgpError -1."""
        nl = self._sel_n()
        words = self._sel_words(mask, nl)
        node, below = C.c_uint32(0), C.c_uint64(0)
        self._ck(self._L.ugp_select_mrca(self._h, _ptr(words), C.byref(node), C.byref(below)))
        return int(node.value), int(below.value)

    def select_time(self, pos, nuc, reps: int = 5) -> float:
        """Bench hook: milliseconds of device time of the mutation kernel alone over these queries."""
        self._sel_n()
        pos = np.ascontiguousarray(pos, dtype=np.int32)
        nuc = np.ascontiguousarray(nuc, dtype=np.uint8)
        ms = C.c_double(0)
        self._ck(self._L.ugp_select_time(self._h, len(pos), _ptr(pos), _ptr(nuc), int(reps), C.byref(ms)))
        return float(ms.value)

    # ---- matUtils mask in closed form (ugp_mask_*) -----------------------------------------------------------------------------
    def mask_attach(self, arrays: Optional[Dict] = None):
        """ugp_mask_attach with the placer's own tree, or with other mutation arrays on the same topology (masked entries, two
        entries at one position on a node).  The depth-first tables are shared as genotypes_attach describes."""
        t = self._t if arrays is None else _TreeArrays(arrays)
        self._ck(self._L.ugp_mask_attach(self._h, C.byref(t.desc)))
        self._msk_shape = (int(t.n), int(t.mut_off[t.n]))

    def _msk(self):
        if getattr(self, "_msk_shape", None) is None:
            self.mask_attach()
        return self._msk_shape

    def mask_restricted(self, leaves):
        """restrictSamples (mask.cpp:802-905) for named LEAVES (BFS indices): (roots, entry_masked) -- the restricted roots as BFS
        indices in depth-first order, and per entry of the mutation CSR whether the reference masks it.  A named internal node
        raises UgpError -2 (the caller walks); an empty list or a node out of range -1."""
        n_nodes, n_ent = self._msk()
        leaves = np.ascontiguousarray(leaves, dtype=np.uint32)
        masked = np.full(n_ent, 0xA5, np.uint8)
        roots = np.zeros(max(len(leaves), 1), np.uint32)   # disjoint roots, each with a named leaf below: never more than names
        nr, nm = C.c_uint64(0), C.c_uint64(0)
        self._ck(self._L.ugp_mask_restricted(self._h, len(leaves), _ptr(leaves) if len(leaves) else None, _ptr(masked) if n_ent else None,
                                             _ptr(roots), len(roots), C.byref(nr), C.byref(nm)))
        self._msk_n_masked = int(nm.value)
        return roots[:int(nr.value)], masked.astype(bool)

    @staticmethod
    def _msk_lines(pos, par, nuc, node, excl):
        pos = np.ascontiguousarray(pos, dtype=np.int32)
        par = np.ascontiguousarray(par, dtype=np.uint8)
        nuc = np.ascontiguousarray(nuc, dtype=np.uint8)
        node = np.ascontiguousarray(node, dtype=np.uint32)
        excl = [np.asarray(x, dtype=np.uint32).ravel() for x in (excl if excl is not None else [[]] * len(pos))]
        if not (len(pos) == len(par) == len(nuc) == len(node) == len(excl)):
            raise UgpError(-1, "pos, par, nuc, node and excl hold one value per line")
        off = np.zeros(len(pos) + 1, np.uint64)
        off[1:] = np.cumsum([len(x) for x in excl], dtype=np.uint64)
        flat = np.ascontiguousarray(np.concatenate(excl) if excl and int(off[-1]) else np.zeros(0, np.uint32), dtype=np.uint32)
        return pos, par, nuc, node, off, flat

    def mask_mutations(self, pos, par, nuc, node, excl=None, skip=None, chunk_lines: int = 0):
        """restrictMutationsLocally (mask.cpp:703-800) for the lines (pos, par, nuc, node, excl)[l]: par / nuc are 4-bit codes with 15
        for N, node a BFS index, excl[l] the excluded nodes of line l (BFS indices; anything out of range has no effect).  Returns
        (first_line, counts): per entry of the mutation CSR the first line that removes it (UINT32_MAX: none), and per line the
        entries it removes.  skip: per entry, set for entries that never match.  chunk_lines (test hook): lines per launch."""
        _, n_ent = self._msk()
        pos, par, nuc, node, off, flat = self._msk_lines(pos, par, nuc, node, excl)
        if skip is not None:
            skip = np.ascontiguousarray(skip, dtype=np.uint8)
            if len(skip) != n_ent:
                raise UgpError(-1, "skip holds one flag per mutation entry")
        first = np.full(n_ent, 0xA5A5A5A5, np.uint32)
        counts = np.zeros(len(pos), np.uint64)
        nl = len(pos)
        self._ck(self._L.ugp_mask_mutations_chunked(self._h, nl, _ptr(pos) if nl else None, _ptr(par) if nl else None,
                                                    _ptr(nuc) if nl else None, _ptr(node) if nl else None, _ptr(off),
                                                    _ptr(flat) if len(flat) else None, _ptr(skip) if skip is not None and n_ent else None,
                                                    _ptr(first) if n_ent else None, _ptr(counts) if nl else None, int(chunk_lines)))
        return first, counts

    def mask_time(self, leaves=None, pos=(), par=(), nuc=(), node=(), excl=None, reps: int = 5):
        """Bench hook: (restricted_ms, mutations_ms), milliseconds of device time of the passes alone (no copies) for the named
        leaves and for the lines; what is not given is not run and reads 0."""
        self._msk()
        leaves = np.ascontiguousarray(leaves if leaves is not None else [], dtype=np.uint32)
        pos, par, nuc, node, off, flat = self._msk_lines(pos, par, nuc, node, excl)
        nl = len(pos)
        a, b = C.c_double(0), C.c_double(0)
        self._ck(self._L.ugp_mask_time(self._h, len(leaves), _ptr(leaves) if len(leaves) else None, nl, _ptr(pos) if nl else None,
                                       _ptr(par) if nl else None, _ptr(nuc) if nl else None, _ptr(node) if nl else None, _ptr(off),
                                       _ptr(flat) if len(flat) else None, int(reps), C.byref(a), C.byref(b)))
        return float(a.value), float(b.value)

    # ---- the excess and imputed mutations of (sample, node) pairs (ugp_vectors_*) ---------------------------------------------------
    VEC_ENTRY = np.dtype([("pos", np.int32), ("ref", np.uint8), ("par", np.uint8), ("nuc", np.uint8), ("pad", np.uint8)])
    VEC_INFO = np.dtype([("n_excess", np.uint32), ("n_imputed", np.uint32), ("n_branch", np.uint32), ("set_difference", np.int32),
                         ("has_unique", np.uint8), ("eligible", np.uint8), ("refused", np.uint8), ("pad", np.uint8)])

    def vectors_attach(self, arrays: Optional[Dict] = None):
        """ugp_vectors_attach with the placer's own tree, or with other mutation arrays on the same topology: the stored parent
        alleles of the vectors calls.  The depth-first tables are shared as genotypes_attach describes."""
        t = self._t if arrays is None else _TreeArrays(arrays)
        self._ck(self._L.ugp_vectors_attach(self._h, C.byref(t.desc)))

    def _vec_pairs(self, queries, nodes, samples):
        nodes = np.ascontiguousarray(nodes, dtype=np.uint32)
        samples = None if samples is None else np.ascontiguousarray(samples, dtype=np.uint32)
        if samples is not None and len(samples) != len(nodes):
            raise UgpError(-1, "one sample per node")
        return nodes, samples

    def vectors(self, queries: QueryBatch, nodes, samples=None, chunk_pairs: int = 0, ex_cap: Optional[int] = None, im_cap: Optional[int] = None):
        """node_excess_mutations and node_imputed_mutations of mapper2_body (ugp_vectors) for the pairs (samples[i] -- an index into
        `queries`; None: i --, nodes[i] -- BFS).  Returns (info, ex_off, excess, im_off, imputed): info a VEC_INFO array; the excess
        entries of pair i are excess[ex_off[i]:ex_off[i + 1]] (VEC_ENTRY: pos, ref, par, nuc), the imputed ones likewise.  The tables
        are those of vectors_attach, which is not called here.  chunk_pairs (test hook): pairs per launch window; ex_cap / im_cap
        (test hooks): room for that many entries only, the true totals are then in _vec_totals."""
        nodes, samples = self._vec_pairs(queries, nodes, samples)
        n = len(nodes)
        info = np.zeros(n, self.VEC_INFO)
        ex_off, im_off = np.zeros(n + 1, np.uint64), np.zeros(n + 1, np.uint64)
        n_ex, n_im = C.c_uint64(0), C.c_uint64(0)
        room_ex = int(ex_cap) if ex_cap is not None else max(8 * n, 1024)
        room_im = int(im_cap) if im_cap is not None else max(2 * n, 1024)
        while True:   # grow and retry: the call reports the true totals
            ex, im = np.zeros(room_ex, self.VEC_ENTRY), np.zeros(room_im, self.VEC_ENTRY)
            self._ck(self._L.ugp_vectors_chunked(self._h, C.byref(queries.desc), n, None if samples is None or not n else _ptr(samples),
                                                 _ptr(nodes) if n else None, _ptr(info) if n else None, _ptr(ex_off), _ptr(ex) if room_ex else None,
                                                 room_ex, C.byref(n_ex), _ptr(im_off), _ptr(im) if room_im else None, room_im, C.byref(n_im),
                                                 int(chunk_pairs)))
            self._vec_totals = (int(n_ex.value), int(n_im.value))
            if (ex_cap is not None or self._vec_totals[0] <= room_ex) and (im_cap is not None or self._vec_totals[1] <= room_im):
                return info, ex_off, ex[:min(room_ex, self._vec_totals[0])], im_off, im[:min(room_im, self._vec_totals[1])]
            if ex_cap is None:
                room_ex = max(room_ex, self._vec_totals[0])
            if im_cap is None:
                room_im = max(room_im, self._vec_totals[1])

    def vectors_time(self, queries: QueryBatch, nodes, samples=None, reps: int = 5):
        """Bench hook: (count_ms, fill_ms), the device time of the two passes alone over these pairs, no copy to the host."""
        nodes, samples = self._vec_pairs(queries, nodes, samples)
        a, b = C.c_double(0), C.c_double(0)
        self._ck(self._L.ugp_vectors_time(self._h, C.byref(queries.desc), len(nodes), None if samples is None else _ptr(samples), _ptr(nodes),
                                          int(reps), C.byref(a), C.byref(b)))
        return float(a.value), float(b.value)

    # ---- the subtree induced by a selection, in closed form (ugp_subtree_*) ----------------------------------------------------------
    SUB_INFO = np.dtype([("n_selected", np.uint64), ("n_gathered", np.uint64), ("n_disagree", np.uint64), ("longest_chain", np.uint64),
                         ("first_disagree", np.uint32), ("pad", np.uint32)])

    def subtree_attach(self, arrays: Optional[Dict] = None):
        """ugp_subtree_attach with the placer's own tree, or with other mutation arrays on the same topology (masked entries, two
        entries at one position on a node).  The depth-first tables are shared as genotypes_attach describes."""
        t = self._t if arrays is None else _TreeArrays(arrays)
        self._ck(self._L.ugp_subtree_attach(self._h, C.byref(t.desc)))

    def subtree_nodes(self, nodes, chunk_items: int = 0, cap: Optional[int] = None):
        """get_subtree (mutation_annotated_tree.cpp:1577-1685) for the named nodes (BFS indices, leaf or internal): a dict with
        kept (BFS indices in depth-first order), parent (index into kept, UINT32_MAX for the root), ent_off (CSR offsets, one more
        than kept), pos / first_entry / nuc (the merged entries: position, the index in the mutation CSR of the entry that opened
        the state, the final allele) and info (a SUB_INFO scalar).  chunk_items (test hook): items per launch window; cap (test
        hook): room for that many kept nodes and merged entries only (ent_off then has as many values as kept)."""
        nodes = np.ascontiguousarray(nodes, dtype=np.uint32)
        info = np.zeros(1, self.SUB_INFO)
        nk, ne = C.c_uint64(0), C.c_uint64(0)

        def call(kept, par, off, room):
            self._ck(self._L.ugp_subtree_nodes_chunked(self._h, len(nodes), _ptr(nodes) if len(nodes) else None, _ptr(kept) if room else None,
                                                       _ptr(par) if room else None, _ptr(off) if room else None, int(room), C.byref(nk),
                                                       C.byref(ne), _ptr(info), int(chunk_items)))

        if cap is None:   # the two-call convention: the counts, then the lists
            call(None, None, None, 0)
            room = int(nk.value)
        else:
            room = int(cap)
        kept, par = np.full(room, 0xA5A5A5A5, np.uint32), np.full(room, 0xA5A5A5A5, np.uint32)
        off = np.full(room + 1, 0xA5A5A5A5A5A5A5A5, np.uint64)
        call(kept, par, off, room)
        w = min(room, int(nk.value))
        n_ent = int(ne.value)
        eroom = n_ent if cap is None else min(int(cap), n_ent)
        pos, first, nuc = np.zeros(eroom, np.int32), np.zeros(eroom, np.uint32), np.zeros(eroom, np.uint8)
        n_out = C.c_uint64(0)
        self._ck(self._L.ugp_subtree_entries(self._h, _ptr(pos) if eroom else None, _ptr(first) if eroom else None,
                                             _ptr(nuc) if eroom else None, eroom, C.byref(n_out)))
        if int(n_out.value) != n_ent:
            raise UgpError(-1, "ugp_subtree_entries and ugp_subtree_nodes disagree on the number of merged entries")
        if w == int(nk.value):
            off[w] = n_ent
            off = off[:w + 1]
        else:
            off = off[:w]
        return {"kept": kept[:w], "parent": par[:w], "ent_off": off, "pos": pos, "first_entry": first, "nuc": nuc, "info": info[0].copy(),
                "n_kept": int(nk.value), "n_entries": n_ent}

    def subtree_owner(self, nodes) -> np.ndarray:
        """Per node (BFS indices, any node) the index in the kept list of the last subtree_nodes call of the kept node whose chain
        holds it, or UINT32_MAX when no selected node lies at or below it."""
        nodes = np.ascontiguousarray(nodes, dtype=np.uint32)
        owner = np.full(len(nodes), 0xA5A5A5A5, np.uint32)
        self._ck(self._L.ugp_subtree_owner(self._h, len(nodes), _ptr(nodes) if len(nodes) else None, _ptr(owner) if len(nodes) else None))
        return owner

    def subtree_time(self, nodes, reps: int = 5):
        """Bench hook: (nodes_ms, merge_ms), milliseconds of device time of the passes alone for the named nodes."""
        nodes = np.ascontiguousarray(nodes, dtype=np.uint32)
        a, b = C.c_double(0), C.c_double(0)
        self._ck(self._L.ugp_subtree_time(self._h, len(nodes), _ptr(nodes) if len(nodes) else None, int(reps), C.byref(a), C.byref(b)))
        return float(a.value), float(b.value)

    # ---- many induced subtrees in one call (ugp_subtree_batch*) -------------------------------------------------------------------------
    SUB_BATCH_INFO = np.dtype([("n_selected", np.uint64), ("n_kept", np.uint64), ("n_entries", np.uint64), ("n_gathered", np.uint64),
                               ("n_disagree", np.uint64), ("longest_chain", np.uint64), ("first_disagree", np.uint32), ("lca", np.uint32)])

    @staticmethod
    def _selections(selections):
        sels = [np.ascontiguousarray(s, dtype=np.uint32).ravel() for s in selections]
        off = np.zeros(len(sels) + 1, np.uint64)
        off[1:] = np.cumsum([len(s) for s in sels], dtype=np.uint64)
        flat = np.concatenate(sels) if sels else np.zeros(0, np.uint32)
        return off, np.ascontiguousarray(flat, dtype=np.uint32)

    def subtree_batch(self, selections, group_positions: int = 0, chunk_items: int = 0):
        """get_subtree for every selection (lists of BFS indices) in one call: per selection the dict subtree_nodes returns, its kept
        nodes, parents and offsets sliced out of the batch's lists and rebased to the slice, and info a SUB_BATCH_INFO scalar.
        group_positions / chunk_items (test hooks): window positions per group, items per launch window; 0: the defaults."""
        off, flat = self._selections(selections)
        ns = len(off) - 1
        koff, eoff = np.zeros(ns + 1, np.uint64), np.zeros(ns + 1, np.uint64)
        info = np.zeros(max(ns, 1), self.SUB_BATCH_INFO)
        self._ck(self._L.ugp_subtree_batch_chunked(self._h, ns, _ptr(off), _ptr(flat) if len(flat) else None, _ptr(koff), _ptr(eoff), _ptr(info),
                                                   int(group_positions), int(chunk_items)))
        nk, ne = int(koff[ns]), int(eoff[ns])
        kept, par, ent = np.zeros(nk, np.uint32), np.zeros(nk, np.uint32), np.zeros(nk + 1, np.uint64)
        n_out = C.c_uint64(0)
        self._ck(self._L.ugp_subtree_batch_nodes(self._h, _ptr(kept) if nk else None, _ptr(par) if nk else None, _ptr(ent) if nk else None, nk,
                                                 C.byref(n_out)))
        if int(n_out.value) != nk:
            raise UgpError(-1, "ugp_subtree_batch_nodes and ugp_subtree_batch disagree on the number of kept nodes")
        ent[nk] = ne
        pos, first, nuc = np.zeros(ne, np.int32), np.zeros(ne, np.uint32), np.zeros(ne, np.uint8)
        self._ck(self._L.ugp_subtree_batch_entries(self._h, _ptr(pos) if ne else None, _ptr(first) if ne else None, _ptr(nuc) if ne else None, ne,
                                                   C.byref(n_out)))
        if int(n_out.value) != ne:
            raise UgpError(-1, "ugp_subtree_batch_entries and ugp_subtree_batch disagree on the number of merged entries")
        out = []
        for b in range(ns):
            k0, k1, e0, e1 = int(koff[b]), int(koff[b + 1]), int(eoff[b]), int(eoff[b + 1])
            out.append({"kept": kept[k0:k1].copy(), "parent": par[k0:k1].copy(), "ent_off": ent[k0:k1 + 1] - np.uint64(e0),
                        "pos": pos[e0:e1].copy(), "first_entry": first[e0:e1].copy(), "nuc": nuc[e0:e1].copy(), "info": info[b].copy(),
                        "n_kept": k1 - k0, "n_entries": e1 - e0})
        return out

    def subtree_batch_time(self, selections, reps: int = 5):
        """Bench hook: (nodes_ms, merge_ms), milliseconds of device time of the passes alone for the batch, summed over its groups."""
        off, flat = self._selections(selections)
        a, b = C.c_double(0), C.c_double(0)
        self._ck(self._L.ugp_subtree_batch_time(self._h, len(off) - 1, _ptr(off), _ptr(flat) if len(flat) else None, int(reps), C.byref(a),
                                                C.byref(b)))
        return float(a.value), float(b.value)

    # ---- matUtils summary --haplotype (ugp_haplotypes_attach / ugp_haplotype_groups / _sets) --------------------------------------
    HP_GROUP = np.dtype([("leaf", np.uint32), ("count", np.uint32), ("size", np.uint32), ("pad", np.uint32)])
    HP_INFO = np.dtype([("n_leaves", np.uint64), ("n_groups", np.uint64), ("n_collisions", np.uint64), ("n_duplicate", np.uint64),
                        ("n_visited", np.uint64), ("first_duplicate", np.uint32), ("pad", np.uint32)])

    def haplotypes_attach(self, arrays: Optional[Dict] = None):
        """ugp_haplotypes_attach with the placer's own tree, or with other mutation arrays on the same topology (masked entries,
        ambiguous alleles, a position twice on one node: trees the placement tables refuse).  The depth-first tables are shared as
        genotypes_attach describes."""
        t = self._t if arrays is None else _TreeArrays(arrays)
        self._ck(self._L.ugp_haplotypes_attach(self._h, C.byref(t.desc)))

    def haplotype_groups(self, hash_bits: int = 128, cap: Optional[int] = None, out: Optional[np.ndarray] = None):
        """matUtils summary -H (summary.cpp:182-264): (groups, info) -- an HP_GROUP array, one record per distinct haplotype of the
        leaves (the BFS index of its first leaf in depth-first order, its leaves, its pairs), ascending by the depth-first position
        of that leaf, and an HP_INFO scalar.  A tree with a position twice on one node, or a fingerprint that groups leaves the
        exact comparison tells apart, raises UgpError -2; the HP_INFO of the last call, refused or not, stays in _hp_info and the
        count it reported in _hp_n_out.  hash_bits (test hook): the low bits of the fingerprint that take part; cap (test hook):
        room for that many records only; out (test hook): the HP_GROUP buffer to write into (its length is the cap)."""
        info = np.zeros(1, self.HP_INFO)
        self._hp_info = None
        n_out = C.c_uint64(0)

        def call(buf, room):
            rc = self._L.ugp_haplotype_groups_hashed(self._h, _ptr(buf) if room else None, int(room), C.byref(n_out), _ptr(info), int(hash_bits))
            self._hp_n_out = int(n_out.value)
            if rc != -1:   # (an invalid call fills nothing)
                self._hp_info = info[0].copy()
            self._ck(rc)

        if out is not None:
            cap = len(out)
        elif cap is None:   # the two-call convention: the count, then the records
            call(None, 0)
            cap = int(n_out.value)
        if out is None:
            out = np.zeros(int(cap), self.HP_GROUP)
        call(out, cap)
        return out[:min(int(cap), self._hp_n_out)], info[0].copy()

    def haplotype_sets(self, leaves, chunk_leaves: int = 0, cap: Optional[int] = None):
        """ugp_haplotype_sets: (off, pos, nuc) -- the haplotypes of the given leaves (BFS) as a CSR: set i is pos / nuc[off[i] ..
        off[i + 1]), ascending by position, nuc the stored 4-bit code.  An internal node in the list raises UgpError -1.
        chunk_leaves (test hook): leaves per launch window; cap (test hook): room for that many pairs only, the true total is
        off[-1] and in _hp_n_out."""
        lv = np.ascontiguousarray(leaves, dtype=np.uint32)
        off = np.zeros(len(lv) + 1, np.uint64)
        n_out = C.c_uint64(0)
        fn = self._L.ugp_haplotype_sets_chunked
        if cap is None:   # the two-call convention: the offsets, then the pairs
            self._ck(fn(self._h, _ptr(lv) if len(lv) else None, len(lv), _ptr(off), None, None, 0, C.byref(n_out), int(chunk_leaves)))
            cap = int(n_out.value)
        pos = np.zeros(int(cap), np.int32)
        nuc = np.zeros(int(cap), np.uint8)
        self._ck(fn(self._h, _ptr(lv) if len(lv) else None, len(lv), _ptr(off), _ptr(pos) if cap else None, _ptr(nuc) if cap else None,
                    int(cap), C.byref(n_out), int(chunk_leaves)))
        self._hp_n_out = int(n_out.value)
        fill = min(int(cap), self._hp_n_out)
        return off, pos[:fill], nuc[:fill]

    def haplotype_time(self, reps: int = 5):
        """Bench hook: (scan_ms, sort_ms, verify_ms), milliseconds of device time of the passes of haplotype_groups alone."""
        a, b, c = C.c_double(0), C.c_double(0), C.c_double(0)
        self._ck(self._L.ugp_haplotype_time(self._h, int(reps), C.byref(a), C.byref(b), C.byref(c)))
        return float(a.value), float(b.value), float(c.value)

    RIPPLES_EVENT = np.dtype([("branch", np.uint64), ("i", np.uint32), ("j", np.uint32), ("donor", np.uint32), ("acceptor", np.uint32),
                              ("donor_count", np.uint32), ("acceptor_count", np.uint32), ("donor_score", np.int32),
                              ("acceptor_score", np.int32), ("donor_sibling", np.uint8), ("acceptor_sibling", np.uint8),
                              ("pad", np.uint8, 6)])

    def ripples_attach(self, name_rank, arrays: Optional[Dict] = None):
        """Advanced / test hook; ripples() attaches by itself.  ugp_ripples_attach with the placer's own tree, or with other
        mutation arrays on the same topology (trees the placement tables refuse: ambiguous alleles).  Arrays given here stay
        the searched tree for the life of the handle: ripples() keeps them when it attaches again for other ranks, and
        the placement calls go on using the handle's own tree."""
        rank = np.ascontiguousarray(name_rank, dtype=np.uint32)
        t = getattr(self, "_rip_t", self._t) if arrays is None else _TreeArrays(arrays)
        self._ck(self._L.ugp_ripples_attach(self._h, C.byref(t.desc), _ptr(rank)))
        self._rip_t = t
        self._rip_rank = rank.copy()

    def ripples(self, branches, name_rank, branch_len: int = 3, min_range: int = 1000, max_range: int = 10 ** 7,
                parsimony_improvement: int = 3, num_descendants: int = 10) -> np.ndarray:
        """RIPPLES' search (ugp_ripples, ripples/main.cpp:300-680 up to the interval refinement) for the branches given by BFS
        index: a structured array of raw events (RIPPLES_EVENT), in branch order, then pair order.  name_rank[k] = the rank of
        node k's name in byte order; the tables are made on the first call (ugp_ripples_attach) and kept for the same ranks."""
        rank = np.ascontiguousarray(name_rank, dtype=np.uint32)
        if getattr(self, "_rip_rank", None) is None or not np.array_equal(self._rip_rank, rank):
            self.ripples_attach(rank)
        br = np.ascontiguousarray(branches, dtype=np.uint32)
        opts = _lib.ugp_ripples_opts(int(branch_len), int(min_range), int(max_range), int(parsimony_improvement), int(num_descendants))
        n_out = C.c_uint64(0)
        cap = max(16, 4 * len(br))
        while True:
            out = np.zeros(cap, self.RIPPLES_EVENT)
            self._ck(self._L.ugp_ripples(self._h, C.byref(opts), _ptr(br), len(br), _ptr(out), cap, C.byref(n_out)))
            if n_out.value <= cap:
                return out[:n_out.value]
            cap = int(n_out.value)

    def node_order(self, order: str) -> np.ndarray:
        out = np.zeros(self.n_nodes, dtype=np.uint32)
        self._ck(self._L.ugp_node_order(self._h, {"bfs": 0, "dfs": 1}[order], _ptr(out)))
        return out

    def subtree_mask(self, root_j: int, max_levels: int, order: str = "bfs") -> np.ndarray:
        out = np.zeros(self.n_nodes, dtype=np.uint8)
        self._ck(self._L.ugp_subtree_mask(self._h, {"bfs": 0, "dfs": 1}[order], int(root_j), int(max_levels), _ptr(out)))
        return out

    # ---- add mode: records of the nodes created or rewritten since the tree was flattened -----------------------------
    def update(self, records: Sequence[Dict] = (), retired: Sequence[int] = ()) -> int:
        """ugp_mat_update.  A record is a dict: flat_j (index in the flattened tree, or None for a node created since), leaf, masked,
        path = [(pos, state, ref)] -- the parent's state wherever it is not the reference base --, own = [(pos, mut, prev, ref)].
        Returns the id of the first new record."""
        n = len(records)
        flat_j = np.array([0xFFFFFFFF if r.get("flat_j") is None else r["flat_j"] for r in records], np.uint32)
        flags = np.array([(1 if r.get("leaf") else 0) | (2 if r.get("masked") else 0) for r in records], np.uint8)
        n_path = np.array([len(r["path"]) for r in records], np.uint32)
        off = np.zeros(n + 1, np.uint64)
        pos, al, pv, rf = [], [], [], []
        for i, r in enumerate(records):
            for (p, a, f) in r["path"]:
                pos.append(p); al.append(a); pv.append(0); rf.append(f)
            for (p, m, pr, f) in r["own"]:
                pos.append(p); al.append(m); pv.append(pr); rf.append(f)
            off[i + 1] = len(pos)
        pos = np.array(pos, np.int32); al = np.array(al, np.uint8); pv = np.array(pv, np.uint8); rf = np.array(rf, np.uint8)
        t = _lib.ugp_touched(n, _ptr(flat_j), _ptr(flags), _ptr(n_path), _ptr(off), _ptr(pos), _ptr(al), _ptr(pv), _ptr(rf))
        ret = np.ascontiguousarray(list(retired), dtype=np.uint32)
        first = C.c_uint32()
        self._ck(self._L.ugp_mat_update(self._h, C.byref(t), _ptr(ret), len(ret), C.byref(first)))
        return int(first.value)

    def touched_open(self, batch: QueryBatch) -> None:
        self._ck(self._L.ugp_touched_open(self._h, C.byref(batch.desc)))

    def touched_score(self, first_id: int, first_sample: int) -> None:
        self._ck(self._L.ugp_touched_score(self._h, first_id, first_sample))

    def touched_rescore(self, sample: int) -> None:
        self._ck(self._L.ugp_touched_rescore(self._h, sample))

    def touched_fetch(self, first_sample: int, n: int, cap: int = 64):
        """(best [n] int32 -- INT32_MAX when no record is eligible --, count [n], ids [n][cap], has_unique [n][cap])"""
        best = np.zeros(n, np.int32); cnt = np.zeros(n, np.uint32)
        ids = np.zeros((n, max(cap, 1)), np.uint32); hu = np.zeros((n, max(cap, 1)), np.uint8)
        self._ck(self._L.ugp_touched_fetch(self._h, first_sample, n, cap, _ptr(best), _ptr(cnt), _ptr(ids), _ptr(hu)))
        return best, cnt, ids, hu

    # ---- device-resident path (bench / multi-GPU) ---------------------------
    def upload(self, batch: QueryBatch):
        h = C.c_void_p()
        self._ck(self._L.ugp_qset_upload(self._h, C.byref(batch.desc), C.byref(h)))
        return h

    def free_qset(self, h) -> None:
        self._L.ugp_qset_destroy(h)

    def coarse_pass(self, qset, method: str):
        """ugp_debug_coarse_pass (test hook): only the locality pre-pass of an uploaded batch, by method "walked" or "sparse" (UgpError
        where a call would not take the sparse one).  Returns (cost [Q], coarse node [Q], BFS indices of the coarse tree's nodes)."""
        Q = int(self._L.ugp_qset_size(qset))
        cost = np.zeros(Q, np.int32); node = np.zeros(Q, np.uint32); kept = np.zeros(self.n_nodes, np.uint32)
        n = C.c_uint64()
        self._ck(self._L.ugp_debug_coarse_pass(self._h, qset, {"walked": 0, "sparse": 1}[method], _ptr(cost), _ptr(node), _ptr(kept), len(kept), C.byref(n)))
        return cost, node, kept[:int(n.value)].copy()

    def bound3_build(self, useful: np.ndarray) -> Dict[str, np.ndarray]:
        """ugp_debug_bound3_build (test hook): the third bound's tables from useful[n_tiles][(n_sites + 7) // 8] (uint32, one nibble per
        site, as the tile builders leave them).  Returns over / under [n_tiles][n_blocks] and the maxima l1 / l2 / l3 (uint8)."""
        useful = np.ascontiguousarray(useful, np.uint32)
        n_tiles = useful.shape[0]
        if useful.ndim != 2 or useful.shape[1] != (int(self.info()["n_sites"]) + 7) // 8:
            raise ValueError("useful must be [n_tiles][(n_sites + 7) // 8]")
        n = C.c_uint64()
        self._ck(self._L.ugp_debug_bound3_build(self._h, None, n_tiles, None, None, None, None, None, C.byref(n)))
        sizes = [int(n.value)]
        for _ in range(3):
            sizes.append((sizes[-1] + 63) // 64)
        out = {k: np.zeros((n_tiles, s), np.uint8) for k, s in zip(("over", "under", "l1", "l2", "l3"), [sizes[0]] + sizes)}
        self._ck(self._L.ugp_debug_bound3_build(self._h, _ptr(useful), n_tiles, _ptr(out["over"]), _ptr(out["under"]), _ptr(out["l1"]), _ptr(out["l2"]),
                                                _ptr(out["l3"]), C.byref(n)))
        return out

    def last_prepass(self) -> str:
        """ugp_debug_last_prepass (test hook): the pre-pass the latest placement call took."""
        return ("none", "walked", "sparse")[int(self._L.ugp_debug_last_prepass(self._h))]

    def place_device(self, qset, d_out_ptr: int, stream: int = 0) -> None:
        """ugp_place_device: stream-ordered on `stream`, like a kernel launch."""
        self._ck(self._L.ugp_place_device(self._h, qset, C.c_void_p(d_out_ptr), C.c_void_p(stream)))

    def place_device_overlapped(self, qset, d_out_ptr: int, stream: int = 0) -> None:
        """ugp_place_device_overlapped: up to pipeline_depth() consecutive calls share the device; `stream` gets each call's completion;
        a call is ordered behind what was on `stream` pipeline_depth() - 1 calls ago (cycle through that many output buffers)."""
        self._ck(self._L.ugp_place_device_overlapped(self._h, qset, C.c_void_p(d_out_ptr), C.c_void_p(stream)))

    def pipeline_depth(self) -> int:
        """ugp_pipeline_depth: overlapped calls kept on the device at a time = output buffers to cycle through."""
        return int(self._L.ugp_pipeline_depth(self._h))

    def timing(self) -> Dict:
        out = _lib.ugp_timing()
        self._ck(self._L.ugp_get_timing(self._h, C.byref(out)))
        return {k: getattr(out, k) for k, _ in out._fields_}

    def timing_sum(self) -> Dict:
        """Durations summed over every call since the previous timing_sum() (waits for calls in flight); 'calls' = how many."""
        out = _lib.ugp_timing()
        n = C.c_uint32()
        self._ck(self._L.ugp_get_timing_sum(self._h, C.byref(out), C.byref(n)))
        d = {k: getattr(out, k) for k, _ in out._fields_}
        d["calls"] = int(n.value)
        return d


class MultiPlacer:
    """The same tree on several devices of one node (ugp_mat_create_multi: flattened once, uploaded n times).
    `place` shards a batch into contiguous blocks, one per device, each placed by its own host thread (ctypes
    releases the GIL for the duration of the call); the gather is a host-memory write.  This is the in-process
    form of the multi-GPU path (the reference simply loops over samples, usher_common.cpp:310); usher_amd.dist is
    the one-process-per-GPU form with an RCCL all-gather."""

    def __init__(self, arrays: Dict, devices: Sequence[int]):
        L = _lib.lib()
        self._t = _TreeArrays(arrays)
        self.n_nodes = self._t.n
        self.devices = list(devices)
        n = len(self.devices)
        devs = (C.c_int * n)(*self.devices)
        hs = (C.c_void_p * n)()
        _check(L.ugp_mat_create_multi(C.byref(self._t.desc), devs, n, hs))
        self._hs = [C.c_void_p(h) for h in hs]

    def close(self) -> None:
        for h in getattr(self, "_hs", []):
            if h.value:
                _lib.lib().ugp_mat_destroy(h)
        self._hs = []

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def place(self, batch: QueryBatch) -> np.ndarray:
        import threading
        from .dist import shard_bounds
        n = len(self._hs)
        out = np.zeros(len(batch), dtype=RESULT_DTYPE)
        errs: List[Optional[BaseException]] = [None] * n

        def work(d: int):
            try:
                lo, hi = shard_bounds(len(batch), n, d)
                if hi > lo:
                    part = batch.slice(lo, hi)
                    res = np.zeros(hi - lo, dtype=RESULT_DTYPE)
                    _check(_lib.lib().ugp_place_batch(self._hs[d], C.byref(part.desc), _ptr(res)))
                    out[lo:hi] = res
            except BaseException as e:   # noqa: BLE001 -- re-raised on the calling thread
                errs[d] = e

        ts = [threading.Thread(target=work, args=(d,)) for d in range(n)]
        for t in ts:
            t.start()
        for t in ts:
            t.join()
        for e in errs:
            if e is not None:
                raise e
        return out
