"""Symmetry-corrected ligand RMSD (reference utils/molecules_utils.py:3-18 -> vendored spyrmsd `rmsd.symmrmsd`,
spyrmsd/rmsd.py:116-203,209-303) for batches of poses on the MI355X.

Host: graph isomorphisms of the molecular graph (atomic numbers as node labels) with networkx, exactly the enumeration
spyrmsd's networkx back-end performs (spyrmsd/graphs/nx.py:52-100).  Device: for every pose the minimum over isomorphisms of
the summed squared displacement, then sqrt(min / n)  (`center=False, minimize=False`, the reference's call) -- `cbd_symm_rmsd`.
There is no CPU fallback for the reduction."""
from __future__ import annotations

import ctypes as C
from typing import List, Sequence, Tuple, Union

import numpy as np
import torch


class IsomorphismLimit(RuntimeError):
    """The enumeration of graph isomorphisms exceeded its time or count bound (highly symmetric ligand)."""


# The reference wraps the symmetry-corrected RMSD in `time_limit(10)` and falls back to the plain RMSD when it fires
# (inference.py:511-520, finetune_train.py:205-214).  The same bound here, plus a count cap so that the [K, N] index tables
# handed to the GPU stay small (ligands with factorially many automorphisms would otherwise exhaust host memory first).
MAX_ISOMORPHISMS = 100_000
ISOMORPHISM_TIME_LIMIT_S = 10.0


def graph_isomorphisms(atomicnums, adjacency, atomicnums2=None, adjacency2=None, max_isomorphisms=None,
                       time_limit_s=None) -> Tuple[np.ndarray, np.ndarray]:
    """All label-preserving isomorphisms between two molecular graphs as index arrays (idx1 [K,N], idx2 [K,N]) such that atom
    idx1[k, i] of molecule 1 corresponds to atom idx2[k, i] of molecule 2.  Raises ValueError if the graphs differ and
    IsomorphismLimit when more than `max_isomorphisms` exist or the enumeration takes longer than `time_limit_s` seconds
    (the callers then use the uncorrected RMSD, like the reference after its time_limit)."""
    import time
    import networkx as nx
    max_isomorphisms = MAX_ISOMORPHISMS if max_isomorphisms is None else max_isomorphisms
    time_limit_s = ISOMORPHISM_TIME_LIMIT_S if time_limit_s is None else time_limit_s
    a1, m1 = np.asarray(atomicnums), np.asarray(adjacency)
    a2 = a1 if atomicnums2 is None else np.asarray(atomicnums2)
    m2 = m1 if adjacency2 is None else np.asarray(adjacency2)
    G1, G2 = nx.Graph(m1), nx.Graph(m2)
    nx.set_node_attributes(G1, {i: v for i, v in enumerate(a1.tolist())}, "aprops")
    nx.set_node_attributes(G2, {i: v for i, v in enumerate(a2.tolist())}, "aprops")
    gm = nx.algorithms.isomorphism.GraphMatcher(G1, G2, lambda x, y: x["aprops"] == y["aprops"])
    if not gm.is_isomorphic():
        raise ValueError("Graphs are not isomorphic.")
    iso, t0 = [], time.monotonic()
    for m in gm.isomorphisms_iter():
        iso.append((list(m.keys()), list(m.values())))
        if len(iso) > max_isomorphisms:
            raise IsomorphismLimit(f"more than {max_isomorphisms} graph isomorphisms")
        if (len(iso) & 63) == 0 and time.monotonic() - t0 > time_limit_s:
            raise IsomorphismLimit(f"graph isomorphism enumeration exceeded {time_limit_s} s ({len(iso)} found)")
    idx1 = np.asarray([i for i, _ in iso], dtype=np.int32)
    idx2 = np.asarray([j for _, j in iso], dtype=np.int32)
    return idx1, idx2


# Isomorphisms of a ligand, enumerated once per process.  The fine-tuning loop measures the same ~100 ligands in every inference
# iteration of every epoch, and once per crystal pose; the enumeration above is Python and can take its whole 10 s.
#   * keyed on a digest of both graphs (atomic numbers, adjacency bits) and the count cap; not on names or object identity;
#   * an enumeration that raised (IsomorphismLimit, ValueError) is an entry too and is re-raised from it: a ligand that times out pays once;
#   * an entry also holds the device copies of its index tables (evaluation.pose_metrics_batch keeps them resident between calls),
#     and its size counts host and device bytes;
#   * least-recently-used entries are evicted by bytes (default limit 256 MB), never the whole cache at once;
#   * only `cached_isomorphisms` (and through it pose_metrics_batch) uses it: graph_isomorphisms / symmetry_rmsd / get_symmetry_rmsd enumerate as before.
_ISO_CACHE = __import__("collections").OrderedDict()      # key -> {"iso": (idx1, idx2) or None, "exc": (exception type, args) or None, "dev": {device key: (d1, d2)}, "bytes": int}
_ISO_CACHE_BYTES = [0]
_ISO_CACHE_CFG = {"enabled": True, "limit": 256 << 20}
_ISO_CACHE_COUNT = {"hits": 0, "misses": 0}
_ISO_ENTRY_OVERHEAD = 256      # bytes charged per entry on top of its tables (key, dict, a cached exception)


def iso_cache_configure(enabled=None, limit_bytes=None):
    if enabled is not None:
        _ISO_CACHE_CFG["enabled"] = bool(enabled)
        if not enabled:
            iso_cache_clear()
    if limit_bytes is not None:
        _ISO_CACHE_CFG["limit"] = int(limit_bytes)
        _iso_cache_evict(0)


def iso_cache_clear():
    _ISO_CACHE.clear()
    _ISO_CACHE_BYTES[0] = 0
    _ISO_CACHE_COUNT.update(hits=0, misses=0)


def iso_cache_stats():
    return {"entries": len(_ISO_CACHE), "bytes": _ISO_CACHE_BYTES[0], "hits": _ISO_CACHE_COUNT["hits"], "misses": _ISO_CACHE_COUNT["misses"]}


def _iso_cache_evict(incoming, keep=None):
    """drop least-recently-used entries (never `keep`) until `incoming` more bytes fit under the limit"""
    for key in list(_ISO_CACHE):
        if _ISO_CACHE_BYTES[0] + incoming <= _ISO_CACHE_CFG["limit"]:
            break
        if key != keep:
            _ISO_CACHE_BYTES[0] -= _ISO_CACHE.pop(key)["bytes"]


def isomorphism_key(atomicnums, adjacency, atomicnums2=None, adjacency2=None, max_isomorphisms=None):
    """digest of both molecular graphs: atomic numbers and adjacency bits (any non-zero entry is a bond), plus the count cap in force"""
    import hashlib
    h = hashlib.blake2b(digest_size=20)
    second = atomicnums2 is not None or adjacency2 is not None
    a1, m1 = np.asarray(atomicnums), np.asarray(adjacency)
    graphs = [(a1, m1)] + ([(a1 if atomicnums2 is None else np.asarray(atomicnums2), m1 if adjacency2 is None else np.asarray(adjacency2))]
                           if second else [])
    for nums, adj in graphs:
        nums = np.ascontiguousarray(nums, dtype=np.int64).reshape(-1)
        h.update(np.int64(len(nums)).tobytes())
        h.update(nums.tobytes())
        h.update(np.asarray(adj.shape, dtype=np.int64).tobytes())
        h.update(np.packbits(np.asarray(adj) != 0).tobytes())
    h.update(np.int64(MAX_ISOMORPHISMS if max_isomorphisms is None else max_isomorphisms).tobytes())
    return h.hexdigest()


def _iso_entry(atomicnums, adjacency, atomicnums2=None, adjacency2=None, max_isomorphisms=None, time_limit_s=None):
    """the cache entry of a pair of graphs (enumerating on a miss); with the cache off, a fresh entry that is not kept"""
    key = isomorphism_key(atomicnums, adjacency, atomicnums2, adjacency2, max_isomorphisms)
    entry = _ISO_CACHE.get(key) if _ISO_CACHE_CFG["enabled"] else None
    if entry is not None:
        _ISO_CACHE.move_to_end(key)
        _ISO_CACHE_COUNT["hits"] += 1
        return key, entry
    _ISO_CACHE_COUNT["misses"] += 1
    entry = {"iso": None, "exc": None, "dev": {}, "bytes": _ISO_ENTRY_OVERHEAD}
    try:
        idx1, idx2 = graph_isomorphisms(atomicnums, adjacency, atomicnums2, adjacency2, max_isomorphisms, time_limit_s)
        idx1.setflags(write=False)
        idx2.setflags(write=False)
        entry["iso"] = (idx1, idx2)
        entry["bytes"] += idx1.nbytes + idx2.nbytes
    except (IsomorphismLimit, ValueError) as e:
        entry["exc"] = (type(e), e.args)      # not the exception itself: it would keep the frames of the enumeration alive
    if _ISO_CACHE_CFG["enabled"] and entry["bytes"] <= _ISO_CACHE_CFG["limit"]:
        _iso_cache_evict(entry["bytes"])
        _ISO_CACHE[key] = entry
        _ISO_CACHE_BYTES[0] += entry["bytes"]
    return key, entry


def cached_isomorphisms(atomicnums, adjacency, atomicnums2=None, adjacency2=None, max_isomorphisms=None, time_limit_s=None):
    """graph_isomorphisms through the process-wide cache (policy: comment above): the same (idx1 [K,N], idx2 [K,N]) arrays, read-only
    and shared between callers; an IsomorphismLimit / ValueError of the first enumeration is raised again without enumerating."""
    _, entry = _iso_entry(atomicnums, adjacency, atomicnums2, adjacency2, max_isomorphisms, time_limit_s)
    if entry["exc"] is not None:
        raise entry["exc"][0](*entry["exc"][1])
    return entry["iso"]


def _identity_entry(n):
    """the identity mapping of n atoms (K = 1) as a cache entry, so that its device copy stays resident like any ligand's tables"""
    key = ("identity", int(n))
    entry = _ISO_CACHE.get(key) if _ISO_CACHE_CFG["enabled"] else None
    if entry is not None:
        _ISO_CACHE.move_to_end(key)
        return key, entry
    idx = np.arange(int(n), dtype=np.int32)[None]
    idx.setflags(write=False)
    entry = {"iso": (idx, idx), "exc": None, "dev": {}, "bytes": _ISO_ENTRY_OVERHEAD + 2 * idx.nbytes}
    if _ISO_CACHE_CFG["enabled"] and entry["bytes"] <= _ISO_CACHE_CFG["limit"]:
        _iso_cache_evict(entry["bytes"])
        _ISO_CACHE[key] = entry
        _ISO_CACHE_BYTES[0] += entry["bytes"]
    return key, entry


def _iso_device_tables(key, entry, device):
    """device copies (int32, contiguous) of an entry's index tables, uploaded on first use and kept in the entry: their bytes count
    towards the cache limit, and they go when the entry is evicted (the caching allocator keeps the memory valid for work already queued
    on the current stream)."""
    dev = torch.device(device)
    dkey = (dev.type, dev.index if dev.index is not None else (torch.cuda.current_device() if dev.type == "cuda" else 0))
    hit = entry["dev"].get(dkey)
    if hit is not None:
        return hit
    idx1, idx2 = entry["iso"]
    d1 = torch.from_numpy(np.array(idx1, dtype=np.int32, order="C")).to(dev)
    d2 = d1 if idx2 is idx1 else torch.from_numpy(np.array(idx2, dtype=np.int32, order="C")).to(dev)
    entry["dev"][dkey] = (d1, d2)
    if _ISO_CACHE.get(key) is entry:
        added = d1.numel() * 4 * (1 if d2 is d1 else 2)
        entry["bytes"] += added
        _ISO_CACHE_BYTES[0] += added
        _iso_cache_evict(0, keep=key)
    return d1, d2


def symmetry_rmsd(coords_ref, coords, atomicnums, adjacency, atomicnums2=None, adjacency2=None, device=None,
                  return_permutation=False, isomorphisms=None):
    """spyrmsd.rmsd.symmrmsd(coords_ref, coords, atomicnums, atomicnums2, adjacency, adjacency2) for one pose [N,3] or a
    batch / list of poses [B,N,3]: float or list of floats like the reference (+ the minimising (idx1, idx2) pairs)."""
    from .engine import load_library, _check, _dptr
    lib = load_library()
    single = not isinstance(coords, (list, tuple)) and np.asarray(coords if not torch.is_tensor(coords) else coords.cpu()).ndim == 2
    # default device: the tensors' own, else this process's CURRENT device (one process per GPU: never everybody's cuda:0)
    dev = torch.device(device) if device is not None else (coords.device if torch.is_tensor(coords) and coords.is_cuda
                                                            else torch.device("cuda", torch.cuda.current_device()))
    if dev.type != "cuda":
        raise RuntimeError("symmetry_rmsd runs on an MI355X (device type 'cuda' under ROCm)")
    to_t = lambda x: x.to(dev, torch.float32) if torch.is_tensor(x) else torch.as_tensor(np.asarray(x), dtype=torch.float32, device=dev)
    pos = to_t(coords[None] if single and torch.is_tensor(coords) else (np.asarray(coords)[None] if single else
               (torch.stack([to_t(c) for c in coords]) if isinstance(coords, (list, tuple)) else coords))).contiguous()
    ref = to_t(coords_ref).contiguous()
    if isomorphisms is None:
        isomorphisms = graph_isomorphisms(atomicnums, adjacency, atomicnums2, adjacency2)
    idx1, idx2 = isomorphisms
    B, N, K = pos.shape[0], pos.shape[1], idx1.shape[0]
    if ref.shape != (N, 3) or idx1.shape != (K, N):
        raise ValueError("coordinate / isomorphism shapes do not match")
    d1 = torch.as_tensor(idx1, dtype=torch.int32, device=dev).contiguous()
    d2 = torch.as_tensor(idx2, dtype=torch.int32, device=dev).contiguous()
    out = torch.empty(B, device=dev)
    arg = torch.empty(B, dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
        _check(lib.cbd_symm_rmsd(B, N, K, _dptr(pos), _dptr(ref), _dptr(d1), _dptr(d2), _dptr(out), _dptr(arg), stream))
    vals = out.cpu().tolist()
    res = vals[0] if single else vals
    if return_permutation:
        a = arg.cpu().tolist()
        perms = [(idx1[k].tolist(), idx2[k].tolist()) for k in a]
        return res, (perms[0] if single else perms)
    return res


def _graph_of(mol):
    """(atomicnums, adjacency) of a spyrmsd-Molecule-like object or an rdkit Mol (heavy atoms as given)."""
    if hasattr(mol, "atomicnums") and hasattr(mol, "adjacency_matrix"):
        return np.asarray(mol.atomicnums), np.asarray(mol.adjacency_matrix)
    if hasattr(mol, "GetAtoms") and hasattr(mol, "GetBonds"):
        nums = np.asarray([a.GetAtomicNum() for a in mol.GetAtoms()])
        am = np.zeros((len(nums), len(nums)), dtype=int)
        for b in mol.GetBonds():
            i, j = b.GetBeginAtomIdx(), b.GetEndAtomIdx()
            am[i, j] = am[j, i] = 1
        return nums, am
    raise TypeError("mol must provide atomicnums/adjacency_matrix (spyrmsd Molecule) or the rdkit Mol API")


class _HeavyAtomGraph:
    """what rdkit's RemoveAllHs leaves of a molecule, as far as the symmetry-corrected RMSD needs it: atomic numbers and adjacency"""

    def __init__(self, atomicnums, adjacency_matrix):
        self.atomicnums, self.adjacency_matrix = atomicnums, adjacency_matrix


def remove_all_hs(mol):
    """Heavy-atom graph of `mol` (the reference passes RemoveAllHs(orig_complex_graph.mol[0]) to get_symmetry_rmsd next to coordinates
    filtered with filterHs: utils/training.py:352, finetune_train.py:210).  A molecule without hydrogens comes back unchanged; None stays
    None (the callers then take their non-symmetry-corrected branch, as they do for any failure)."""
    if mol is None:
        return None
    nums, am = _graph_of(mol)
    keep = nums != 1
    if keep.all():
        return mol
    return _HeavyAtomGraph(nums[keep], am[np.ix_(keep, keep)])


def get_symmetry_rmsd(mol, coords1, coords2, mol2=None, return_permutation=False, device=None):
    """Same call as the reference (utils/molecules_utils.py:3): coords1 = reference pose, coords2 = pose or list of poses.
    `device` (extension): the GPU to reduce on; default = the poses' device or the process's current device."""
    n1, a1 = _graph_of(mol)
    n2, a2 = _graph_of(mol2) if mol2 is not None else (n1, a1)
    return symmetry_rmsd(coords1, coords2, n1, a1, n2, a2, device=device, return_permutation=return_permutation)
