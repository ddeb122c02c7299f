"""`NoiseTransform`: the forward-diffusion transform the fine-tuning DataLoader applies to every buffered pose
(reference datasets/pdbbind.py:25-133), with the reference's constructor arguments, RNG draw order and output fields:
  t ~ Beta(alpha, beta) (numpy global generator), sigma = t_to_sigma(t),
  tr_update ~ N(0, sigma_tr) (torch global generator, shape (1,3)), rot_update = so3.sample_vec(sigma_rot),
  torsion_updates ~ N(0, sigma_tor) (numpy, one per rotatable bond), pose moved by modify_conformer, and
  data.tr_score = -tr_update / sigma_tr^2, data.rot_score = so3.score_vec(...), data.tor_score = torus.score(...),
  data.tor_sigma_edge, complex_t / node_t set to t.
Host-side like the reference (it runs in the loader, one complex at a time, O(Nl) work); `time_independent`,
`crop_beyond_cutoff`, all-atom and asynchronous schedules are outside the hot path's scope and raise.

Opt-in device path for a whole batch: `NoiseTransform.draw` makes the draws and sets the targets of one item without moving its pose,
`NoiseTransform.apply_noise_batch` draws for every item of a list in order (so the generators advance exactly as under sequential
`__call__`s), packs the ragged batch -- different ligands, each with its own Nl, R and mask_rotate -- into one staging buffer, uploads
it once and moves all poses with one `cbd_noise_conformers` launch (csrc/noise_transform.hip); each item's `pos` becomes its slice
of the device output.
"""
from __future__ import annotations

import ctypes as C
import math
import random
from collections import OrderedDict

import numpy as np
import torch

from .. import so3, torus
from ..diffusion_utils import set_time
from ..sampling import _mask_rotate_of, modify_conformer_torsion_angles


MAX_ATOMS, MAX_TORSIONS = 512, 128      # capacity of cbd_noise_conformers per ligand (include/cbdock.h)


def pack_mask_rotate(mask_rotate) -> np.ndarray:
    """bool [R, Nl] -> uint32 [R, ceil(Nl / 32)], atom a at bit a % 32 of word a // 32 (the layout cbd_noise_conformers reads)."""
    m = np.asarray(mask_rotate, dtype=bool)
    m = m.reshape(0, 0) if m.ndim != 2 else m
    r, nl = m.shape
    words = (nl + 31) // 32
    padded = np.zeros((r, words * 32), dtype=bool)
    padded[:, :nl] = m
    return np.packbits(padded, axis=1, bitorder="little").view("<u4").reshape(r, words).astype(np.uint32, copy=False)


def unpack_mask_rotate(bits, nl) -> np.ndarray:
    """inverse of pack_mask_rotate -> bool [R, nl]"""
    b = np.ascontiguousarray(np.asarray(bits, dtype="<u4"))
    return np.unpackbits(b.view(np.uint8), axis=1, bitorder="little")[:, :nl].astype(bool)


def pack_ligand(data):
    """(rot_edge int32 [R, 2], mask_bits uint32 [R, ceil(Nl / 32)]) of one item: the ends (u, v) of its rotatable bonds in edge_mask
    order -- the rows modify_conformer hands to modify_conformer_torsion_angles -- and its packed mask_rotate."""
    lig = data["ligand"]
    nl = int(lig.pos.shape[0]) if torch.is_tensor(lig.pos) else int(lig.num_nodes)
    ei = data["ligand", "ligand"].edge_index.T[lig.edge_mask]
    edges = np.ascontiguousarray(ei.cpu().numpy().astype(np.int32)).reshape(-1, 2)
    mask = _mask_rotate_of(data)
    mask = mask.reshape(len(edges), nl) if mask.size else np.zeros((len(edges), nl), dtype=bool)
    if mask.shape != (len(edges), nl):
        raise ValueError(f"mask_rotate {mask.shape} does not match {len(edges)} rotatable bonds x {nl} atoms")
    return edges, pack_mask_rotate(mask)


def axis_angle_to_matrix(aa: torch.Tensor) -> torch.Tensor:
    """Rotation matrix of an axis-angle vector through the unit quaternion (reference utils/geometry.py:43-86, incl. the
    small-angle series of sin(x/2)/x below 1e-6)."""
    ang = torch.linalg.vector_norm(aa, dim=-1, keepdim=True)
    half = 0.5 * ang
    small = ang.abs() < 1e-6
    k = torch.where(small, 0.5 - ang * ang / 48, torch.sin(half) / torch.where(small, torch.ones_like(ang), ang))
    q = torch.cat([torch.cos(half), aa * k], dim=-1)
    r, i, j, kk = q.unbind(-1)
    two_s = 2.0 / (q * q).sum(-1)
    m = torch.stack([1 - two_s * (j * j + kk * kk), two_s * (i * j - kk * r), two_s * (i * kk + j * r),
                     two_s * (i * j + kk * r), 1 - two_s * (i * i + kk * kk), two_s * (j * kk - i * r),
                     two_s * (i * kk - j * r), two_s * (j * kk + i * r), 1 - two_s * (i * i + j * j)], dim=-1)
    return m.reshape(aa.shape[:-1] + (3, 3))


def kabsch(A: torch.Tensor, B: torch.Tensor):
    """R [3,3], t [3,1] minimising |R A + t - B| for 3xN point sets (reference utils/geometry.py:209-243).  The 3x3 SVD runs in
    numpy float64: torch's CPU LAPACK path spins up the whole thread pool for it (tens of ms per call on a many-core host)."""
    a, b_ = A.detach().cpu().numpy().astype(np.float64), B.detach().cpu().numpy().astype(np.float64)
    ca, cb = a.mean(axis=1, keepdims=True), b_.mean(axis=1, keepdims=True)
    U, S, Vt = np.linalg.svd((a - ca) @ (b_ - cb).T)
    R = Vt.T @ U.T
    if np.linalg.det(R) < 0:
        R = (Vt.T @ np.diag([1.0, 1.0, -1.0])) @ U.T
    assert math.fabs(np.linalg.det(R) - 1) < 3e-3
    t = -R @ ca + cb
    return torch.from_numpy(R).to(A.dtype), torch.from_numpy(t).to(A.dtype)


def modify_conformer(data, tr_update, rot_update, torsion_updates):
    """Rigid move about the centroid, torsion updates, Kabsch re-alignment onto the rigid pose
    (reference utils/diffusion_utils.py:33-58, pivot=None)."""
    pos = data["ligand"].pos
    center = torch.mean(pos, dim=0, keepdim=True)
    rot_mat = axis_angle_to_matrix(rot_update.squeeze())
    rigid = (pos - center) @ rot_mat.T + tr_update + center
    if torsion_updates is not None:
        ei = data["ligand", "ligand"].edge_index.T[data["ligand"].edge_mask]
        flex = modify_conformer_torsion_angles(rigid, ei, _mask_rotate_of(data), torsion_updates).to(rigid.device)
        R, t = kabsch(flex.T, rigid.T)
        data["ligand"].pos = flex @ R.T + t.T
    else:
        data["ligand"].pos = rigid
    return data


class NoiseTransform:
    def __init__(self, t_to_sigma, no_torsion, all_atom, alpha=1, beta=1, rot_alpha=1, rot_beta=1, tor_alpha=1, tor_beta=1,
                 separate_noise_schedule=False, asyncronous_noise_schedule=False, include_miscellaneous_atoms=False,
                 crop_beyond_cutoff=None, time_independent=False, rmsd_cutoff=0, minimum_t=0, sampling_mixing_coeff=0):
        if all_atom or asyncronous_noise_schedule or include_miscellaneous_atoms or time_independent or crop_beyond_cutoff is not None:
            raise NotImplementedError("all_atom / asynchronous / time_independent / crop_beyond_cutoff noise transforms are "
                                      "outside the score-model fine-tuning path")
        self.t_to_sigma, self.no_torsion, self.all_atom = t_to_sigma, no_torsion, all_atom
        self.minimum_t, self.mixing_coeff = minimum_t, sampling_mixing_coeff
        self.separate_noise_schedule = separate_noise_schedule
        self.alpha, self.beta = alpha, beta
        self.rot_alpha, self.rot_beta, self.tor_alpha, self.tor_beta = rot_alpha, rot_beta, tor_alpha, tor_beta

    def __call__(self, data):
        t_tr, t_rot, t_tor, t = self.get_time()
        return self.apply_noise(data, t_tr, t_rot, t_tor, t)

    def get_time(self):
        if self.separate_noise_schedule:
            return (np.random.beta(self.alpha, self.beta), np.random.beta(self.rot_alpha, self.rot_beta),
                    np.random.beta(self.tor_alpha, self.tor_beta), None)
        if self.mixing_coeff == 0:
            t = np.random.beta(self.alpha, self.beta)
            t = self.minimum_t + t * (1 - self.minimum_t)
        else:
            choice = np.random.binomial(1, self.mixing_coeff)
            t1 = np.random.beta(self.alpha, self.beta) * self.minimum_t
            t2 = self.minimum_t + np.random.beta(self.alpha, self.beta) * (1 - self.minimum_t)
            t = choice * t1 + (1 - choice) * t2
        return t, t, t, t

    def draw(self, data):
        """Everything apply_noise does except moving the pose: the time, the three updates from the same generators in the same order,
        set_time and the score targets.  -> (tr_update float32 [1, 3], rot_update float64 [3], torsion_updates float64 [R] or None)."""
        t_tr, t_rot, t_tor, t = self.get_time()
        if not torch.is_tensor(data["ligand"].pos):
            data["ligand"].pos = random.choice(data["ligand"].pos)
        tr_sigma, rot_sigma, tor_sigma = self.t_to_sigma(t_tr, t_rot, t_tor)
        set_time(data, t, t_tr, t_rot, t_tor, 1, self.all_atom, False, device=None)
        tr_update = torch.normal(mean=0, std=tr_sigma, size=(1, 3))
        rot_update = so3.sample_vec(eps=rot_sigma)
        n_tor = int(data["ligand"].edge_mask.sum())
        torsion_updates = np.random.normal(loc=0.0, scale=tor_sigma, size=n_tor)
        torsion_updates = None if self.no_torsion else torsion_updates
        data.tr_score = -tr_update / tr_sigma ** 2
        data.rot_score = torch.from_numpy(so3.score_vec(vec=rot_update, eps=rot_sigma)).float().unsqueeze(0)
        data.tor_score = None if self.no_torsion else torch.from_numpy(torus.score(torsion_updates, tor_sigma)).float()
        data.tor_sigma_edge = None if self.no_torsion else np.ones(n_tor) * tor_sigma
        if data["ligand"].pos.shape[0] == 1:
            data.rot_score = data.rot_score * 0   # a single atom has no orientation
        return tr_update, rot_update, torsion_updates

    _PACK_CACHE_ENTRIES = 4096

    def _packed(self, data):
        """pack_ligand(data), cached per ligand: the buffer hands out shallow copies, so the many poses of one ligand share the SAME
        mask_rotate / edge_index / edge_mask objects; an entry holds them (their ids cannot be recycled) and is checked by identity."""
        cache = self.__dict__.setdefault("_pack_cache", OrderedDict())
        lig, bonds = data["ligand"], data["ligand", "ligand"]
        refs = (lig.mask_rotate, bonds.edge_index, lig.edge_mask)
        key = tuple(id(r) for r in refs)
        hit = cache.get(key)
        if hit is not None and all(a is b for a, b in zip(hit[0], refs)):
            cache.move_to_end(key)
            return hit[1]
        packed = pack_ligand(data)
        cache[key] = (refs, packed)
        while len(cache) > self._PACK_CACHE_ENTRIES:
            cache.popitem(last=False)
        return packed

    def apply_noise_batch(self, data_list, device):
        """`__call__` for a list of items with the poses moved on the GPU: draws per item in list order, ONE upload of the packed
        ragged batch, ONE cbd_noise_conformers launch on the current stream; every item's `['ligand'].pos` is then its slice of the
        device output (fp32, on `device`).  An item over the kernel's capacity (Nl > 512 or R > 128) is moved by the host
        `modify_conformer` and stays on the host.  There is no CPU path: `device` must be a GPU.  -> data_list"""
        from .. import engine, staging
        dev = torch.device(device)
        if dev.type != "cuda":
            raise RuntimeError("apply_noise_batch moves the poses on the MI355X (cbd_noise_conformers); use __call__ per item on the host")
        lib = engine.load_library()
        fit = []
        for d in data_list:
            tr_u, rot_u, tor_u = self.draw(d)
            nl, n_tor = int(d["ligand"].pos.shape[0]), int(d["ligand"].edge_mask.sum())
            if nl > MAX_ATOMS or n_tor > MAX_TORSIONS:
                modify_conformer(d, tr_u, torch.from_numpy(rot_u).float(), tor_u)
            else:
                fit.append((d, tr_u, rot_u, tor_u, nl, n_tor) + self._packed(d))
        if not fit:
            return data_list
        nls, rs = np.asarray([f[4] for f in fit], dtype=np.int64), np.asarray([f[5] for f in fit], dtype=np.int64)
        lig_ptr = staging.ptr(nls)
        f32 = lambda arrays: np.concatenate([np.asarray(a, dtype=np.float32).reshape(-1) for a in arrays])
        staged, at = staging.upload(dict(
            lig_ptr=lig_ptr, rot_ptr=staging.ptr(rs), mask_ptr=staging.ptr(rs * ((nls + 31) // 32)),
            rot_edge=np.concatenate([f[6].reshape(-1) for f in fit]), mask_bits=np.concatenate([f[7].reshape(-1) for f in fit]),
            pos_in=f32(f[0]["ligand"].pos.detach().cpu().numpy() for f in fit), tr=f32(f[1].numpy() for f in fit),
            rot=f32(f[2] for f in fit), tor=None if self.no_torsion else f32(f[3] for f in fit)), dev)
        with torch.cuda.device(dev):
            out = torch.empty(int(lig_ptr[-1]), 3, dtype=torch.float32, device=dev)
            engine._check(lib.cbd_noise_conformers(len(fit), int(nls.max()), int(rs.max()), at("lig_ptr"), at("pos_in"), at("rot_ptr"),
                                                   at("rot_edge"), at("mask_ptr"), at("mask_bits"), at("tr"), at("rot"), at("tor"),
                                                   C.c_void_p(out.data_ptr()), C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)))
        # `staged` is read by the kernel just enqueued on the stream it was allocated on: the caching allocator orders its reuse behind it
        for f, a0, a1 in zip(fit, lig_ptr[:-1], lig_ptr[1:]):
            f[0]["ligand"].pos = out[int(a0):int(a1)]
        return data_list

    def apply_noise(self, data, t_tr, t_rot, t_tor, t, tr_update=None, rot_update=None, torsion_updates=None):
        if not torch.is_tensor(data["ligand"].pos):
            data["ligand"].pos = random.choice(data["ligand"].pos)
        tr_sigma, rot_sigma, tor_sigma = self.t_to_sigma(t_tr, t_rot, t_tor)
        set_time(data, t, t_tr, t_rot, t_tor, 1, self.all_atom, False, device=None)
        tr_update = torch.normal(mean=0, std=tr_sigma, size=(1, 3)) if tr_update is None else tr_update
        rot_update = so3.sample_vec(eps=rot_sigma) if rot_update is None else rot_update
        n_tor = int(data["ligand"].edge_mask.sum())
        torsion_updates = np.random.normal(loc=0.0, scale=tor_sigma, size=n_tor) if torsion_updates is None else torsion_updates
        torsion_updates = None if self.no_torsion else torsion_updates
        modify_conformer(data, tr_update, torch.from_numpy(rot_update).float(), torsion_updates)
        data.tr_score = -tr_update / tr_sigma ** 2
        data.rot_score = torch.from_numpy(so3.score_vec(vec=rot_update, eps=rot_sigma)).float().unsqueeze(0)
        data.tor_score = None if self.no_torsion else torch.from_numpy(torus.score(torsion_updates, tor_sigma)).float()
        data.tor_sigma_edge = None if self.no_torsion else np.ones(n_tor) * tor_sigma
        if data["ligand"].pos.shape[0] == 1:
            data.rot_score = data.rot_score * 0   # a single atom has no orientation
        return data
