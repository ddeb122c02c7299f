"""`sampling()` and `randomize_position()` with the reference's signatures and semantics
(reference utils/sampling.py:15-48, 59-274), driving the MI355X engine.

`batch_size` keeps its meaning for the order and sizes of the random draws, but consecutive loader batches of the same
complex are executed as ONE engine batch (up to the engine capacity, 64 poses): pose samples never interact, results are
unchanged, and e.g. the reference's default of 10 poses per batch no longer turns into four small GPU launches per layer.

What stays on the host (as in the reference): batching the data list, the schedule scalars of every step
(engine.make_steps), drawing the N(0,1) noise in the reference's order, writing poses back into `data_list`.
What moves to the GPU as ONE call per batch: the whole step loop (score model + perturbation + pose update),
`cbd_sample` in include/cbdock.h -- no per-step host round trips, no `.item()` syncs.

Differences from the reference that are deliberate and documented:
  * noise for a partial last batch is drawn with the batch's real size b (the reference draws min(batch_size, N)
    rows and fails on the shape mismatch, relying on the caller's halve-and-retry);
  * the noise is drawn on the CPU generator (torch.normal, same call order and sizes as the reference: tr (b,3),
    rot (b,3), tor (b*R) per step), so a seed reproduces the reference's CPU path draw for draw;
  * pivot, return_full_trajectory, return_features raise (they also raise in the reference); SVGD (experimental in the reference, off in
    the shipped configuration) runs step by step through _sample_svgd: engine scores + batched pairwise kernel terms on the device;
    crop_beyond of the SCORE model (not in the shipped yml) runs through _sample_cropped (a set-up per distinct crop mask and step).
Confidence scoring (reference utils/sampling.py:240-261): with `confidence_model` set, the final poses of every batch
are scored by the all-atom confidence engine (cbd_conf_score) -- crop_beyond per pose, t = 0 -- on the all-atom graphs
of `filtering_data_list` (or of `data_list` itself when it carries the 'atom' stores); returns the concatenated
confidences with NaN -> -1000 like the reference.
"""
from __future__ import annotations

import contextlib
from functools import partial
from types import SimpleNamespace

import numpy as np
import torch
from scipy.spatial.transform import Rotation as R

from .engine import make_steps, complex_fingerprint, _single_complex, _single_all_atom_complex
from .hostcfg import with_glue_threads
from .wave_pipeline import Group, LoaderBatch, WavePipeline, plan_waves, score_wave, switch_on_async_setup


# Test hook (tests/test_gpu_finetune_loop.py, tools/check_upload_ordering.py): False removes the ordering of the pipelined side-stream fills
# behind the caller's stream -- the state before round 6 -- to show that the hazard of ADVICE round 5 is real.  Never switched off in use.
# Read by every sampling() call and handed to its wave_pipeline.WavePipeline, where the ordering lives.
_ORDER_SIDE_FILLS = True
_STEPS_CACHE = __import__("weakref").WeakKeyDictionary()       # model -> {schedule / flag / embedding key: engine.make_steps(...)} (_cached_steps)

def _mask_rotate_of(graph):
    mr = graph["ligand"].mask_rotate
    while isinstance(mr, (list, tuple)):
        mr = mr[0]
    return np.asarray(mr)


def modify_conformer_torsion_angles(pos, edge_index, mask_rotate, torsion_updates, as_numpy=False):
    """Sequential torsion rotations on the host (reference utils/torsion.py:48-72); used by randomize_position only."""
    pos = pos.cpu().numpy().copy() if torch.is_tensor(pos) else np.array(pos, copy=True)
    edge_index = edge_index.cpu().numpy() if torch.is_tensor(edge_index) else np.asarray(edge_index)
    for idx_edge, (u, v) in enumerate(edge_index):
        if torsion_updates[idx_edge] == 0:
            continue
        rot_vec = pos[u] - pos[v]
        rot_vec = rot_vec * torsion_updates[idx_edge] / np.linalg.norm(rot_vec)
        rot_mat = R.from_rotvec(rot_vec).as_matrix()
        pos[mask_rotate[idx_edge]] = (pos[mask_rotate[idx_edge]] - pos[v]) @ rot_mat.T + pos[v]
    return pos if as_numpy else torch.from_numpy(pos.astype(np.float32))


def _pocket_center(data_list, pocket_knowledge=False, pocket_cutoff=7):
    """Where randomize_position puts the ligands of `data_list` (copies of one complex): the receptor's centroid, or with
    `pocket_knowledge` the centroid of the residues within `pocket_cutoff` of the crystal pose (the nearest residue if there is none)."""
    center_pocket = data_list[0]["receptor"].pos.mean(dim=0)
    if pocket_knowledge:
        cg = data_list[0]
        orig = cg["ligand"].orig_pos
        orig = orig[0] if isinstance(orig, (list, tuple)) else orig
        d = torch.cdist(cg["receptor"].pos, torch.from_numpy(np.asarray(orig)).float() - cg.original_center)
        label = torch.any(d < pocket_cutoff, dim=1)
        if torch.any(label):
            center_pocket = cg["receptor"].pos[label].mean(dim=0)
        else:
            center_pocket = cg["receptor"].pos[torch.argmin(torch.min(d, dim=1)[0])]
    return center_pocket


def randomize_position(data_list, no_torsion, no_random, tr_sigma_max, pocket_knowledge=False, pocket_cutoff=7):
    """In-place initial pose randomisation; RNG use identical to the reference (numpy global for torsions,
    scipy Rotation.random, torch global for the translation)."""
    center_pocket = _pocket_center(data_list, pocket_knowledge, pocket_cutoff)
    if not no_torsion:
        for g in data_list:
            n_tor = int(g["ligand"].edge_mask.sum())
            torsion_updates = np.random.uniform(low=-np.pi, high=np.pi, size=n_tor)
            g["ligand"].pos = modify_conformer_torsion_angles(
                g["ligand"].pos, g["ligand", "ligand"].edge_index.T[g["ligand"].edge_mask], _mask_rotate_of(g), torsion_updates)
    for g in data_list:
        molecule_center = torch.mean(g["ligand"].pos, dim=0, keepdim=True)
        random_rotation = torch.from_numpy(R.random().as_matrix()).float()
        g["ligand"].pos = (g["ligand"].pos - molecule_center) @ random_rotation.T + center_pocket
        if not no_random:
            g["ligand"].pos += torch.normal(mean=0, std=tr_sigma_max, size=(1, 3))


def draw_randomization(data_list, no_torsion, no_random, tr_sigma_max):
    """The draws of randomize_position(data_list, ...) without moving a pose, from the same global generators in the same order and
    sizes: every pose's torsion updates first, then a rotation per pose (both on numpy's global generator), then a translation per
    pose (torch's): afterwards both generators are where randomize_position leaves them.
    -> (tor: list of float64 [R] per pose, or None with no_torsion; rot_mat: float32 tensor [n, 3, 3], scipy's matrices cast the way
    randomize_position casts them; tr: float32 tensor [n, 1, 3], or None with no_random)"""
    tor = None
    if not no_torsion:
        tor = [np.random.uniform(low=-np.pi, high=np.pi, size=int(g["ligand"].edge_mask.sum())) for g in data_list]
    rot_mat = torch.stack([torch.from_numpy(R.random().as_matrix()).float() for _ in data_list]) if len(data_list) else torch.zeros(0, 3, 3)
    tr = None
    if not no_random:
        tr = torch.stack([torch.normal(mean=0, std=tr_sigma_max, size=(1, 3)) for _ in data_list]) if len(data_list) else torch.zeros(0, 1, 3)
    return tor, rot_mat, tr


def _randomize_with_draws(data_list, center_pocket, tor, rot_mat, tr):
    """randomize_position's arithmetic, statement for statement, with the draws of draw_randomization prescribed: the host route of
    randomize_position_batch for a complex over the kernel's capacity, and the host yardstick of tests/test_gpu_randomize_batch.py."""
    if tor is not None:
        for g, torsion_updates in zip(data_list, tor):
            g["ligand"].pos = modify_conformer_torsion_angles(
                g["ligand"].pos, g["ligand", "ligand"].edge_index.T[g["ligand"].edge_mask], _mask_rotate_of(g), torsion_updates)
    for k, g in enumerate(data_list):
        molecule_center = torch.mean(g["ligand"].pos, dim=0, keepdim=True)
        g["ligand"].pos = (g["ligand"].pos - molecule_center) @ rot_mat[k].T + center_pocket
        if tr is not None:
            g["ligand"].pos += tr[k]


RANDOMIZE_MAX_ATOMS, RANDOMIZE_MAX_TORSIONS = 512, 128      # capacity of cbd_randomize_poses per ligand (include/cbdock.h)


def _same_ligand(a, b):
    """do two graphs share start coordinates and torsion description (the copies of one complex do), so that one description serves both"""
    la, lb = a["ligand"], b["ligand"]
    ea, eb = a["ligand", "ligand"].edge_index, b["ligand", "ligand"].edge_index
    ma, mb = _mask_rotate_of(a), _mask_rotate_of(b)
    same = lambda x, y: x is y or (x.shape == y.shape and x.dtype == y.dtype and bool(torch.equal(x, y)))
    return (same(la.pos, lb.pos) and same(ea, eb) and same(la.edge_mask, lb.edge_mask)
            and (ma is mb or (ma.shape == mb.shape and np.array_equal(ma, mb))))


def _pack_randomization(groups, centers, draws):
    """The ragged batch cbd_randomize_poses reads, as host arrays.  `groups`: data_lists, one per complex (all within the capacity);
    `centers`: their pocket centres; `draws`: their draw_randomization results.  The graphs of a group that share start coordinates and
    torsion description (`_same_ligand` with the group's first graph) point at ONE ligand description, every other graph gets its own.
    -> dict: pose_lig, pose_cplx [P]; out_ptr, tor_ptr [P + 1]; lig_ptr, rot_ptr, mask_ptr [L + 1] (int32); rot_edge int32 [sum R, 2];
    mask_bits uint32 (flat); pos_in float32 [sum Nl, 3]; tor float64 [sum R over poses] or None; rot_mat float32 [P, 9]; tr float32
    [P, 3] or None; center float32 [C, 3]; max_nl, max_r."""
    from .datasets.pdbbind import pack_ligand
    from .staging import ptr
    pose_lig, pose_cplx, nl_of, r_of, descs = [], [], [], [], []
    for c, group in enumerate(groups):
        first = len(descs)                   # the description of the group's first graph
        for k, g in enumerate(group):
            lig = first
            if k == 0 or not _same_ligand(group[0], g):
                lig = len(descs)
                edges, bits = pack_ligand(g)
                descs.append((g["ligand"].pos.detach().cpu().numpy().astype(np.float32, copy=False).reshape(-1, 3), edges, bits))
            pose_lig.append(lig)
            pose_cplx.append(c)
            nl_of.append(descs[lig][0].shape[0])
            r_of.append(descs[lig][1].shape[0])

    def cat(arrays, dtype, shape):
        arrays = [np.asarray(a, dtype=dtype).reshape(shape) for a in arrays]
        return np.concatenate(arrays) if arrays else np.zeros(tuple(0 if s == -1 else s for s in shape), dtype=dtype)
    with_tor = bool(draws) and draws[0][0] is not None
    with_tr = bool(draws) and draws[0][2] is not None
    return dict(
        pose_lig=np.asarray(pose_lig, dtype=np.int32), pose_cplx=np.asarray(pose_cplx, dtype=np.int32), out_ptr=ptr(nl_of), tor_ptr=ptr(r_of),
        lig_ptr=ptr([d[0].shape[0] for d in descs]), rot_ptr=ptr([d[1].shape[0] for d in descs]), mask_ptr=ptr([d[2].size for d in descs]),
        rot_edge=cat([d[1] for d in descs], np.int32, (-1, 2)), mask_bits=cat([d[2] for d in descs], np.uint32, (-1,)),
        pos_in=cat([d[0] for d in descs], np.float32, (-1, 3)),
        tor=cat([t for d in draws for t in d[0]], np.float64, (-1,)) if with_tor else None,
        rot_mat=cat([d[1].numpy() for d in draws], np.float32, (-1, 9)),
        tr=cat([d[2].numpy() for d in draws], np.float32, (-1, 3)) if with_tr else None,
        center=cat([np.asarray(c) for c in centers], np.float32, (-1, 3)),
        max_nl=max(nl_of, default=0), max_r=max(r_of, default=0))


def randomize_position_batch(groups, no_torsion, no_random, tr_sigma_max, device, pocket_knowledge=False, pocket_cutoff=7):
    """randomize_position for the data_lists of several complexes (`groups`: one data_list per complex) with the poses moved on the
    GPU: draws per group in list order (draw_randomization: the generators advance as under randomize_position group after group),
    ONE upload of the packed ragged batch, ONE cbd_randomize_poses launch on the current stream, ONE download; every graph's
    `['ligand'].pos` is then an fp32 CPU tensor of its old shape.  A group with a ligand over the kernel's capacity (Nl > 512 or
    R > 128) is moved on the host with the draws already made.  There is no CPU path: `device` must be a GPU.  No reference counterpart."""
    import ctypes as C
    from . import engine, staging
    dev = torch.device(device)
    if dev.type != "cuda":
        raise RuntimeError("randomize_position_batch moves the poses on the MI355X (cbd_randomize_poses); use randomize_position on the host")
    lib = engine.load_library()
    fit, centers, draws = [], [], []
    for group in groups:
        center = _pocket_center(group, pocket_knowledge, pocket_cutoff)
        drawn = draw_randomization(group, no_torsion, no_random, tr_sigma_max)
        if any(int(g["ligand"].pos.shape[0]) > RANDOMIZE_MAX_ATOMS or int(g["ligand"].edge_mask.sum()) > RANDOMIZE_MAX_TORSIONS for g in group):
            _randomize_with_draws(group, center, *drawn)
            continue
        fit.append(group)
        centers.append(center)
        draws.append(drawn)
    if not fit:
        return groups
    pk = _pack_randomization(fit, centers, draws)
    staged, at = staging.upload({k: v for k, v in pk.items() if k not in ("max_nl", "max_r")}, dev)
    with torch.cuda.device(dev):
        out = torch.empty(int(pk["out_ptr"][-1]), 3, dtype=torch.float32, device=dev)
        engine._check(lib.cbd_randomize_poses(
            len(pk["pose_lig"]), len(pk["lig_ptr"]) - 1, len(fit), int(pk["max_nl"]), int(pk["max_r"]), at("pose_lig"), at("pose_cplx"),
            at("out_ptr"), at("tor_ptr"), at("lig_ptr"), at("pos_in"), at("rot_ptr"), at("rot_edge"), at("mask_ptr"), at("mask_bits"), at("tor"),
            at("rot_mat"), at("tr"), at("center"), C.c_void_p(out.data_ptr()), C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)))
        moved = out.cpu()      # the one download; it also orders `staged` behind the kernel
    graphs = [g for group in fit for g in group]
    for g, a0, a1 in zip(graphs, pk["out_ptr"][:-1], pk["out_ptr"][1:]):
        g["ligand"].pos = moved[int(a0):int(a1)].clone()
    return groups


def _draw_chunk_noise(b, R_, S, no_final_step_noise=False):
    """N(0,1) draws of one loader batch of b poses: per step tr (b,3), rot (b,3), tor (b*R) from the global CPU generator -- the
    order and sizes of the reference's torch.normal calls (utils/sampling.py:122-141)."""
    tr_l, rot_l, tor_l = [], [], []
    for s in range(S):
        last_quiet = no_final_step_noise and s == S - 1
        tr_l.append(torch.zeros(b, 3) if last_quiet else torch.normal(mean=0, std=1, size=(b, 3)))
        rot_l.append(torch.zeros(b, 3) if last_quiet else torch.normal(mean=0, std=1, size=(b, 3)))
        if R_ > 0:
            tor_l.append(torch.zeros(b * R_) if last_quiet else torch.normal(mean=0, std=1, size=(b * R_,)))
    return torch.stack(tr_l), torch.stack(rot_l), (torch.stack(tor_l) if R_ > 0 else None)


@with_glue_threads
def draw_noise_like_reference(N, R_, S, batch_size, no_final_step_noise=False):
    """The noise `sampling()` would draw for N poses of one complex (R_ rotatable bonds) walked in loader batches of `batch_size`,
    as a dict of 'tr' [S,N,3], 'rot' [S,N,3], 'tor' [S,N*R_] (None if R_ == 0) CPU tensors: `sampling(..., noise=this)` then equals
    `sampling(...)` under the same seed.  `sampling_distributed` draws it on every rank and slices, so results do not depend
    on the number of ranks.  (Under glue_threads like sampling() itself: with torch's default intra-op pool the first small randn
    after a thread-count change costs 2 .. 90 ms of pool start-up -- the run-to-run spread of bench.py's python_api leg in round 5.)"""
    parts = [_draw_chunk_noise(min(int(batch_size), N - start), R_, S, no_final_step_noise) for start in range(0, N, max(int(batch_size), 1))]
    return {"tr": torch.cat([p[0] for p in parts], 1), "rot": torch.cat([p[1] for p in parts], 1),
            "tor": torch.cat([p[2] for p in parts], 1) if R_ > 0 else None}


def _sample_cropped(eng, cplx, key, pos, steps, noise, crop):
    """Reverse diffusion with the score model's `crop_beyond` (reference utils/sampling.py:101-108 with utils/utils.py:395-420): before
    every step each pose's receptor is cropped to the residues within 3 sigma_tr(t) + crop_beyond of a ligand atom, and the model sees
    that smaller complex -- other residues, other C-alpha edges, another receptor embedding.  Not in the shipped yml; implemented on the
    existing entry points: per step the poses are grouped by their crop mask (early steps: everything is kept, late steps: the poses
    of a converged run share a pocket), each group's cropped complex goes through cbd_set_complex and ONE step of cbd_sample.  The
    arithmetic is the engine's; what this path adds is host orchestration (a set-up per distinct mask and step)."""
    from .utils import crop_beyond as crop_graph
    z_tr, z_rot, z_tor = noise
    B, Nl = pos.shape[0], pos.shape[1]
    R = eng.R
    rec_pos = cplx["receptor"].pos.float().cpu()
    base_R = int(cplx["ligand"].edge_mask.sum())
    graph_before = eng.get_option("graph", 1)      # the caller may have switched hipGraph replay off (debugging / profiling): restored as found
    eng.set_option("graph", 0)
    try:
        for i in range(len(steps)):
            cutoff = steps[i].tr_sigma * 3 + crop
            host = pos.detach().cpu()
            d2 = torch.sum((host.unsqueeze(1) - rec_pos.view(1, -1, 1, 3)) ** 2, -1)            # [B, Nr, Nl], the reference's formula
            keep = torch.any(d2 < cutoff ** 2, dim=2)
            groups = {}
            for b in range(B):
                groups.setdefault(keep[b].numpy().tobytes(), []).append(b)
            for mask_bytes, idx in groups.items():
                m = keep[idx[0]]
                if not bool(m.any()):
                    raise RuntimeError("crop_beyond left a pose without any receptor residue (the reference's model fails on an empty "
                                       "receptor graph as well)")
                g = cplx.shallow_copy()
                g["ligand"].pos = host[idx[0]]
                crop_graph(g, cutoff, False)
                eng.set_complex(g, (key, "crop", hash(mask_bytes)))
                sel = torch.as_tensor(idx, device=pos.device)
                p = pos.index_select(0, sel).contiguous()
                cols = (sel[:, None] * base_R + torch.arange(base_R, device=pos.device)[None, :]).reshape(-1)
                take = lambda z, c=None: None if z is None else z[i:i + 1].to(pos.device).index_select(1, sel if c is None else c).contiguous()
                eng.sample(p, (type(steps[i]) * 1)(steps[i]), take(z_tr), take(z_rot), take(z_tor, cols) if (R > 0 and z_tor is not None) else None)
                pos.index_copy_(0, sel, p)
    finally:
        eng.set_option("graph", graph_before)
        eng.complex_key = None          # the engine holds a cropped complex now


def get_dihedrals(data_list):
    """(c, a, b, d) atom quadruples of the rotatable bonds (reference utils/torsion.py:121-139): c / d = the first listed neighbour of
    a / b that is not the bond partner."""
    g = data_list[0]
    edge_index = torch.as_tensor(g["ligand", "ligand"].edge_index).cpu()
    edge_mask = torch.as_tensor(g["ligand"].edge_mask).cpu().bool()
    nbrs = [[] for _ in range(int(edge_index.max()) + 1)] if edge_index.numel() else []
    for u, v in edge_index.T.tolist():
        nbrs[u].append(v)
    quads = []
    for k, (a, b) in enumerate(edge_index.T.tolist()):
        if bool(edge_mask[k]):
            c = nbrs[a][0] if nbrs[a][0] != b else nbrs[a][1]
            d = nbrs[b][0] if nbrs[b][0] != a else nbrs[b][1]
            quads.append((c, a, b, d))
    return torch.tensor(quads, dtype=torch.long).reshape(-1, 4)


def _matrix_to_axis_angle(Rm):
    """Rotation matrices [..., 3, 3] -> rotation vectors (reference utils/geometry.py:100-205: through the best-conditioned quaternion
    candidate, small-angle branch sin(x/2)/x ~ 1/2 - x^2/48)."""
    m = Rm.reshape(Rm.shape[:-2] + (9,))
    m00, m01, m02, m10, m11, m12, m20, m21, m22 = torch.unbind(m, -1)
    q_abs = torch.sqrt(torch.clamp(torch.stack([1.0 + m00 + m11 + m22, 1.0 + m00 - m11 - m22, 1.0 - m00 + m11 - m22,
                                                1.0 - m00 - m11 + m22], -1), min=0.0))
    cand = torch.stack([torch.stack([q_abs[..., 0] ** 2, m21 - m12, m02 - m20, m10 - m01], -1),
                        torch.stack([m21 - m12, q_abs[..., 1] ** 2, m10 + m01, m02 + m20], -1),
                        torch.stack([m02 - m20, m10 + m01, q_abs[..., 2] ** 2, m12 + m21], -1),
                        torch.stack([m10 - m01, m20 + m02, m21 + m12, q_abs[..., 3] ** 2], -1)], -2)
    cand = cand / (2.0 * q_abs[..., None].clamp(min=0.1))
    best = q_abs.argmax(-1)
    q = torch.gather(cand, -2, best[..., None, None].expand(best.shape + (1, 4))).squeeze(-2)
    norms = torch.linalg.vector_norm(q[..., 1:], dim=-1, keepdim=True)
    half = torch.atan2(norms, q[..., :1])
    ang = 2 * half
    small = ang.abs() < 1e-6
    k = torch.where(small, 0.5 - ang * ang / 48, torch.sin(half) / torch.where(small, torch.ones_like(ang), ang))
    return q[..., 1:] / k


def _rigid_svgd_terms(P):
    """Pairwise rigid differences of the poses P [N, Nl, 3] (reference utils/torsion.py:171-185 over
    utils/geometry.py:279-314): translation between the centroids and the Kabsch rotation vector of every pair i < j, antisymmetric;
    all pairs as one batched 3 x 3 SVD instead of the reference's N (N - 1) / 2 sequential ones."""
    N = P.shape[0]
    c = P.mean(1)                                         # [N, 3]
    Pm = P - c[:, None, :]
    H = torch.einsum("ina,jnb->ijab", Pm, Pm)             # H[i, j] = Am_i Bm_j^T
    U, _, Vt = torch.linalg.svd(H)
    Rm = Vt.transpose(-1, -2) @ U.transpose(-1, -2)
    flip = torch.linalg.det(Rm) < 0
    D = torch.ones(N, N, 3, dtype=P.dtype, device=P.device)
    D[..., 2] = torch.where(flip, -1.0, 1.0)
    Rm = (Vt.transpose(-1, -2) * D[..., None, :]) @ U.transpose(-1, -2)
    rv = _matrix_to_axis_angle(Rm)                        # [N, N, 3]
    t = c[None, :, :] - c[:, None, :]                     # t[i, j] = -c_i + c_j
    upper = torch.triu(torch.ones(N, N, dtype=torch.bool, device=P.device), 1)[..., None]
    rot_diff = torch.where(upper, rv, torch.zeros_like(rv))
    rot_diff = rot_diff - rot_diff.transpose(0, 1)
    tr_diff = torch.where(upper, t, torch.zeros_like(t))
    tr_diff = tr_diff - tr_diff.transpose(0, 1)
    return (tr_diff ** 2).sum(-1, keepdim=True), (rot_diff ** 2).sum(-1, keepdim=True), tr_diff, rot_diff


def _torsion_svgd_terms(dihedral, P):
    """Torsion angles of the poses and their wrapped pairwise differences (reference utils/torsion.py:146-168)."""
    c, a, b, d = (dihedral[:, k] for k in range(4))
    bdot = lambda x, y: torch.sum(x * y, dim=-1, keepdim=True)
    ab = P[:, b] - P[:, a]
    c_proj = P[:, a] + bdot(P[:, c] - P[:, a], ab) / bdot(ab, ab) * ab
    d_proj = P[:, a] + bdot(P[:, d] - P[:, a], ab) / bdot(ab, ab) * ab
    dsh = P[:, d] - d_proj + c_proj
    u, v = dsh - c_proj, P[:, c] - c_proj
    cos = bdot(u, v) / (torch.linalg.vector_norm(u, dim=-1, keepdim=True) * torch.linalg.vector_norm(v, dim=-1, keepdim=True))
    cos = torch.clamp(cos, -1 + 1e-5, 1 - 1e-5)
    tau = (torch.acos(cos) * torch.sign(bdot(torch.linalg.cross(u, v), ab))).squeeze(-1)          # [N, R]
    diff = tau.unsqueeze(1) - tau.unsqueeze(0)
    diff = torch.fmod(diff + 3 * np.pi, 2 * np.pi) - np.pi
    return (diff ** 2).sum(-1, keepdim=True), diff


def _sample_svgd(eng, cplx, pos, steps, noise, sched, cfg, n_total):
    """Reverse diffusion with the reference's SVGD-style repulsion between the samples of a complex (utils/sampling.py:169-218,
    utils/torsion.py:121-185; experimental in the reference, off in the shipped configuration).  Per step: the engine's score
    (cbd_score), the pairwise kernel terms of all samples -- centroid translations, Kabsch rotation vectors, wrapped torsion differences
    -- as batched device tensors (the reference loops over the pairs on the host), the combined update, cbd_modify_conformer."""
    z_tr, z_rot, z_tor = noise
    N, dev = pos.shape[0], pos.device
    if N != n_total:
        raise ValueError("SVGD needs all samples of the complex in one batch (the reference reshapes the torsion scores to [1, N, R])")
    if z_tr is None:
        raise ValueError("SVGD sampling needs the stochastic sampler (not ode / no_random), as in the reference")
    S, Rn = len(steps), eng.R
    tr_s, rot_s, tor_s = sched
    dihedral = get_dihedrals([cplx]).to(dev) if Rn > 0 else None
    lin = lambda lo, hi, t, default: default if lo is None or hi is None else 10 ** (lo * t + hi * (1 - t))
    rot_w, tor_w = 10 ** cfg["rot_log_rel_weight"], 10 ** cfg["tor_log_rel_weight"]
    dt_of = lambda s, i: float(s[i] - s[i + 1]) if i < S - 1 else float(s[i])
    for i in range(S):
        t = i / S
        w = lin(cfg["weight_log_0"], cfg["weight_log_1"], t, 0.0)
        rep_w = lin(cfg["repulsive_weight_log_0"], cfg["repulsive_weight_log_1"], t, 1.0)
        st = steps[i]
        tr_score, rot_score, tor_score = eng.score(pos, st)
        zt, zr = z_tr[i].to(dev), z_rot[i].to(dev)
        zq = z_tor[i].to(dev) if (Rn > 0 and z_tor is not None) else None
        if not w > 0:
            tr_p = st.tr_score_coef * tr_score + st.tr_noise_coef * zt
            rot_p = st.rot_score_coef * rot_score + st.rot_noise_coef * zr
            tor_p = st.tor_score_coef * tor_score + st.tor_noise_coef * zq if Rn > 0 else None
        else:
            P = pos
            if cfg["use_x0"]:        # kernel terms on the one-step denoised poses (coefficient g^2 t instead of g^2 dt)
                adj = lambda coef, s, score: coef / dt_of(s, i) * float(s[i]) * score
                P = eng.modify_conformer(pos, adj(st.tr_score_coef, tr_s, tr_score), adj(st.rot_score_coef, rot_s, rot_score),
                                         adj(st.tor_score_coef, tor_s, tor_score) if Rn > 0 else None)
            tr_m, rot_m, tr_d, rot_d = _rigid_svgd_terms(P)
            tor_m, tor_d = _torsion_svgd_terms(dihedral, P) if Rn > 0 else (0.0, None)
            total = tr_m + rot_w * rot_m + tor_w * tor_m
            ks = lin(cfg["kernel_size_log_0"], cfg["kernel_size_log_1"], t, 1.0)
            lw = lin(cfg["langevin_weight_log_0"], cfg["langevin_weight_log_1"], t, 1.0)
            h = ks * torch.median(total, dim=1, keepdim=True)[0] / max(np.log(N), 1)
            k = torch.exp(-1 / h * total)
            tr_rep = torch.sum(2 / h * tr_d * k, dim=1)
            rot_rep = torch.sum(2 / h * rot_w * rot_d * k, dim=1)
            mix = lambda cs, cn, score, z, rep: 0.5 * cs * score + lw * (0.5 * cs * score + cn * z) + w * (cs * (score + rep_w * rep / N))
            tr_p = mix(st.tr_score_coef, st.tr_noise_coef, tr_score, zt, tr_rep)
            rot_p = mix(st.rot_score_coef, st.rot_noise_coef, rot_score, zr, rot_rep)
            tor_p = None
            if Rn > 0:
                tor_rep = torch.sum(2 / h * tor_w * tor_d * k, dim=1)                     # [N, R]
                tor_p = mix(st.tor_score_coef, st.tor_noise_coef, tor_score.reshape(N, Rn), zq.reshape(N, Rn), tor_rep).reshape(-1)
        pos.copy_(eng.modify_conformer(pos, tr_p, rot_p, tor_p))


def _check_arguments(N, model, model_args, conf_model, filtering_data_list, inference_steps, schedules, t_schedule, asyncronous_noise_schedule,
                     record, n_streams, svgd, ode, no_random, temp_sampling, pivot, return_features):
    """What sampling() refuses, before it touches an engine -> (does the model embed the common time, the three schedules as float64)"""
    assert not (return_features or pivot), "Not implemented yet in new inference version"
    score_crop = getattr(model_args, "crop_beyond", None)
    if record:
        why = ("n_streams > 1" if n_streams > 1 else "SVGD sampling" if svgd is not None
               else "the score model's crop_beyond" if score_crop is not None else None)
        if why is not None:
            raise NotImplementedError(f"return_full_trajectory is recorded by the one-launch step loop of a single engine; {why} "
                                      "steps on the host or over several streams and does not record")
    if svgd is not None:
        if ode or no_random:
            raise ValueError("SVGD sampling needs the stochastic sampler (the reference's SVGD branch reads the drawn noise)")
        if not all(float(x) == 1.0 for x in (temp_sampling if np.iterable(temp_sampling) else [temp_sampling])):
            raise NotImplementedError("SVGD together with low-temperature sampling: the reference's SVGD branch overwrites the temperature terms")
    # asyncronous_noise_schedule (inference.py:384-388, utils/diffusion_utils.py:172-175): the caller passes the common time grid as
    # `t_schedule`, the three component schedules are its beta-quantile images; what the flag changes is which time the MODEL embeds,
    # and that is a property of the model (score_model.py:85) -- a model built without it ignores complex_t['t'] in the reference too
    model_async = bool(getattr(getattr(model, "module", model), "asyncronous_noise_schedule", False))
    if model_async and (t_schedule is None or not asyncronous_noise_schedule):
        raise KeyError("'t': the model embeds the common diffusion time (asyncronous_noise_schedule) -- pass t_schedule and "
                       "asyncronous_noise_schedule=True, as inference.py does")
    if t_schedule is not None and len(t_schedule) != inference_steps:
        raise ValueError("t_schedule length != inference_steps")
    if score_crop is not None and getattr(model_args, "all_atoms", False):
        raise NotImplementedError("score-model crop_beyond is supported for the C-alpha score model (the shipped architecture)")
    if conf_model is not None and not hasattr(conf_model, "atom_confidence_predictor"):
        raise NotImplementedError("confidence scoring runs on the all-atom confidence engine (all_atom_score_model)")
    if filtering_data_list is not None and len(filtering_data_list) != N:
        raise ValueError("filtering_data_list must have one graph per pose")
    schedules = tuple(np.asarray(s, dtype=np.float64) for s in schedules)
    if not all(len(s) == inference_steps for s in schedules):
        raise ValueError("schedule length != inference_steps")
    return model_async, schedules


def _cached_steps(model, model_args, tr_schedule, rot_schedule, tor_schedule, common, ode=False, no_random=False, no_final_step_noise=False,
                  temp_sampling=1.0, temp_psi=0.0, temp_sigma_data=0.5):
    """engine.make_steps(...) through a cache.  --different_schedules (inference.py:375-383): rot / tor run on their own time grids;
    everything schedule-dependent is a host scalar of the step, the engine itself is agnostic.  The per-step scalars are a pure function
    of the schedules, six sigma limits, a few flags and the model's timestep embedding, and cost ~4 ms of host arithmetic (20 steps x
    torch scalar ops in the reference's own dtypes) -- 2 % of a one-complex call in the reference's inference.py loop, where every call
    passes the same schedules: cached per model, eight entries, the oldest evicted."""
    tkey = lambda v: tuple(float(x) for x in v) if np.iterable(v) else float(v)
    skey = (tr_schedule.tobytes(), rot_schedule.tobytes(), tor_schedule.tobytes(), None if common is None else common.tobytes(),
            tuple(float(getattr(model_args, k)) for k in ("tr_sigma_min", "tr_sigma_max", "rot_sigma_min", "rot_sigma_max", "tor_sigma_min", "tor_sigma_max")),
            bool(ode), bool(no_random), bool(no_final_step_noise), tkey(temp_sampling), tkey(temp_psi), float(temp_sigma_data),
            model.timestep_emb_func)        # the function itself, not its id(): the key keeps it alive, so no later one can take its place
    cache = _STEPS_CACHE.setdefault(model, {})          # beside the model, not on it: copy.deepcopy(model) must not meet ctypes arrays
    steps = cache.get(skey)
    if steps is None:
        steps = make_steps(tr_schedule, model_args, model.timestep_emb_func, ode=ode, no_random=no_random,
                           no_final_step_noise=no_final_step_noise, temp_sampling=temp_sampling, temp_psi=temp_psi,
                           temp_sigma_data=temp_sigma_data, rot_schedule=rot_schedule, tor_schedule=tor_schedule, common_t_schedule=common)
        if len(cache) >= 8:
            cache.pop(next(iter(cache)))
        cache[skey] = steps
    return steps


def _co_count(co_schedule, data_list, batch_size, n_streams=1, score_crop=None, svgd=None):
    """how many complexes advance in lockstep (the groups of a wave)"""
    if co_schedule is None:
        # aim at ~160 poses per merged launch -- 4 complexes of 40 samples, 8 of 8 (measured: 8-way is +6 % over 4-way at 8 samples per
        # complex and -1 % at 40).  Poses per complex = the leading run of equal names (the loader batches of a complex are merged).
        name0 = getattr(data_list[0], "name", None) if len(data_list) else None
        per = next((i for i, d in enumerate(data_list) if getattr(d, "name", None) != name0), len(data_list)) if name0 is not None else int(batch_size)
        co_schedule = -(-160 // max(per, 1))
    if svgd is not None and score_crop is not None:
        raise NotImplementedError("SVGD together with the score model's crop_beyond")
    # one complex at a time: over several streams; with crop_beyond, where the cropped receptor differs from pose to pose and step to
    # step (_sample_cropped); with SVGD, where the samples of ONE complex interact, step by step on the host (_sample_svgd)
    alone = n_streams != 1 or score_crop is not None or svgd is not None
    return 1 if alone else max(1, min(int(co_schedule), 8))


def _walk(data_list, batch_size, max_batch, n_co, no_torsion, S, noise, use_noise, no_final_step_noise):
    """`data_list` in loader batches of `batch_size` -> the waves of wave_pipeline.Group that run together (wave_pipeline.plan_waves).
    The reference collates every chunk with torch_geometric's Batch (utils/sampling.py:78); only the ligand coordinates of the poses and
    ONE copy of the complex are needed here, so the chunks are walked without collating (for a 40-pose complex the collation of the
    1281-wide receptor features alone costs more host time than the GPU work).  The noise of a chunk is drawn (or sliced from `noise`)
    as the walk reaches it: the order of the draws on the global generator is the reference's."""
    batches, keys, offset = [], [], 0
    for start in range(0, len(data_list), max(int(batch_size), 1)):
        chunk = data_list[start:start + max(int(batch_size), 1)]
        b = len(chunk)
        if b > max_batch:
            raise RuntimeError(f"batch of {b} exceeds the engine capacity {max_batch}")
        if any(getattr(d, "num_graphs", 1) != 1 for d in chunk):
            raise ValueError("data_list elements must be single graphs (as inference.py builds them)")
        batch = chunk[0]
        Nl = batch["ligand"].pos.shape[0]
        key = complex_fingerprint(batch)
        for d in chunk[1:]:
            if complex_fingerprint(d) != key:
                raise NotImplementedError("all poses of one batch must belong to the same complex (as modify_conformer_batch assumes)")
        R_ = int(batch["ligand"].edge_mask.sum()) if not no_torsion else 0
        z = (None, None, None)
        if use_noise and noise is not None:
            z = (noise["tr"][:, offset:offset + b], noise["rot"][:, offset:offset + b],
                 noise["tor"][:, offset * R_:(offset + b) * R_] if R_ > 0 else None)
        elif use_noise:
            z = _draw_chunk_noise(b, R_, S, no_final_step_noise)
        lig_pos = torch.stack([d["ligand"].pos.detach().cpu().float().reshape(Nl, 3) for d in chunk])
        batches.append(LoaderBatch(offset, lig_pos, z, batch))
        keys.append(key)
        offset += b
    plan = plan_waves(keys, [b.pos.shape[0] for b in batches], max_batch, n_co)
    return [[Group(_single_complex(batches[g[0]].graph)[0], keys[g[0]], [batches[c] for c in g]) for g in wave] for wave in plan]


@contextlib.contextmanager
def _call_scope():
    """End-of-call duties of sampling().  The pipelined set-up is a property of THIS call, not of the model's cached engines:
    "async_setup" goes back to what it was.  The confidence engine's capacity flag is sticky and lives on the (cached) engine: if the
    call ends by an exception before the final check(), the flag must not survive into the next, unrelated call.
    -> scope.async_before: engines whose "async_setup" this call switched on -> previous value; scope.conf_used: the confidence
    engines this call scored on"""
    scope = SimpleNamespace(async_before={}, conf_used=set())
    try:
        yield scope
    except BaseException:
        for ceng in scope.conf_used:
            try:
                ceng.check()
            except RuntimeError:
                pass
        raise
    finally:
        for e, was in scope.async_before.items():
            e.set_option("async_setup", was)


def _engine_sets(model, eng, waves, look_ahead, scope):
    """The two engine sets the waves alternate between (the same set twice without look-ahead): `eng` and as many partners sharing its
    weights as the widest wave of each parity needs, running with `eng`'s options (operand precision, graph replay, ...)."""
    need_a = max((len(w) for w in waves[0::2]), default=1)
    need_b = max((len(w) for w in waves[1::2]), default=0) if look_ahead else 0
    partners = model.co_engines(need_a - 1 + need_b, eng) if need_a - 1 + need_b > 0 else []
    for e in partners:
        for name, val in getattr(eng, "_options", {}).items():
            if name != "async_setup" and e.get_option(name) != val:
                e.set_option(name, val)
    if need_b:
        switch_on_async_setup([eng] + partners, scope.async_before)
    set_a = [eng] + partners[:need_a - 1]
    return [set_a, partners[need_a - 1:] if need_b else set_a]


def _score_confidence(staged, conf_model, max_batch, filtering_data_list, crop, used, out):
    """Confidence [b] of every group's final poses, appended to `out`, on the confidence model's engine and its partners: the k-th
    complex of a launch runs on the k-th of them.  `filtering_data_list`: the all-atom graphs per pose (None: the sampled graphs
    carry the 'atom' stores).  No host sync: the engines go into `used`, sampling() checks their sticky capacity flags at the end."""
    main = conf_model.engine(max_batch=max_batch)      # looked up here, behind the wave's launch: the look-up checksums weights on the device
    items = []
    for s in staged:
        fbatch = filtering_data_list[s.group.first] if filtering_data_list is not None else s.group.batches[0].graph
        fg, _, fNl = _single_all_atom_complex(fbatch)
        if fNl != s.pos.shape[1]:
            raise RuntimeError("filtering graphs hold a different ligand than the sampled ones")
        items.append((fg, complex_fingerprint(fbatch) + (fg["atom"].pos.shape[0],), s.pos))
    n = min(len(items), 4)
    cengs = [main] + (conf_model.co_engines(n - 1, main) if n > 1 else [])
    used.update(cengs)
    out.extend(score_wave(cengs, items, crop, check=False, skip_same_key=True))


def _finish_wave(staged, trajs, data_list, trajectory, score=None):
    """the wave's results back into the caller's lists: recorded frames (one download for the wave: the groups' [S,b,Nl,3] blocks back
    to back), final poses (views of the device batch), confidences (`score`: _score_confidence with the call's constants bound)"""
    if trajs is not None:
        host = torch.cat([t.reshape(-1) for t in trajs]).cpu()
        lo = 0
        for s, t in zip(staged, trajs):
            block = host[lo:lo + t.numel()].reshape(t.shape)
            lo += t.numel()
            first = s.group.first
            for i in range(s.pos.shape[0]):
                trajectory[first + i] = block[:, i].clone()
    for s in staged:
        first, B, Nl = s.group.first, s.pos.shape[0], s.pos.shape[1]
        flat = s.pos.reshape(B * Nl, 3)
        for i in range(B):
            data_list[first + i]["ligand"].pos = flat[i * Nl:(i + 1) * Nl]
    if score is not None:
        score(staged)


def _run_waves(pipe, waves, finish, look_ahead, **launch_kw):
    """launch k, stage k + 1 on the other engine set under its step loop (`look_ahead`; otherwise after finish k), finish k"""
    ahead = None
    for k, wave in enumerate(waves):
        staged = ahead if ahead is not None else pipe.stage(wave, k % 2, ahead=k > 0, skip_same_key=True)
        trajs = pipe.launch(staged, **launch_kw)
        ahead = pipe.stage(waves[k + 1], (k + 1) % 2, ahead=True, skip_same_key=True) if look_ahead and k + 1 < len(waves) else None
        finish(staged, trajs)


@with_glue_threads
def sampling(data_list, model, inference_steps, tr_schedule, rot_schedule, tor_schedule, device, t_to_sigma, model_args,
             no_random=False, ode=False, visualization_list=None, confidence_model=None, filtering_data_list=None,
             filtering_model_args=None, asyncronous_noise_schedule=False, t_schedule=None, batch_size=32,
             no_final_step_noise=False, pivot=None, return_full_trajectory=False, temp_sampling=1.0, temp_psi=0.0,
             temp_sigma_data=0.5, return_features=False, svgd_weight_log_0=None, svgd_repulsive_weight_log_0=None,
             svgd_weight_log_1=None, svgd_repulsive_weight_log_1=None, svgd_kernel_size_log_0=None,
             svgd_kernel_size_log_1=None, svgd_langevin_weight_log_0=None, svgd_langevin_weight_log_1=None,
             svgd_rot_log_rel_weight=0.0, svgd_tor_log_rel_weight=0.0, svgd_use_x0=False, noise=None, n_streams=1, co_schedule=None):
    """Reverse diffusion of every pose in `data_list`; returns (data_list, confidence) like the reference.
    `noise` (optional, extension): dict of pre-drawn 'tr' [S,N,3], 'rot' [S,N,3], 'tor' [S,N*R] CPU tensors.
    `n_streams` (extension): each batch is split over this many concurrent HIP streams (identical results).
    `co_schedule` (extension): when `data_list` holds poses of several complexes, up to this many (<= 8) complexes are advanced in
    lockstep with merged tensor-product launches (identical results; 1 = one complex at a time like the reference; default: as many
    as bring a launch to ~160 poses).
    `return_full_trajectory`: returns (data_list, confidence, trajectory) like the reference (utils/sampling.py:267-268): trajectory[i]
    is a CPU float32 tensor [inference_steps, Nl_i, 3], frame k the pose of data_list[i] after step k in the ligand-centred frame of
    data["ligand"].pos (the last frame is the final pose).  The pose-update kernel records the frames on the device
    (cbd_sample_traj) and they are downloaded once per co-scheduled wave.  With a `visualization_list` every frame is added as
    add(frame + original_center, part=1, order=k + 2) -- what the reference's commented-out per-step add intended -- in place of the
    single final order=2 frame.  Not implemented (NotImplementedError) for the host-stepped, non-default samplers: n_streams > 1,
    SVGD and the score model's crop_beyond.
    The waves (co-scheduled groups of complexes) run on wave_pipeline.WavePipeline: the next wave is set up under the current one."""
    N, S, record = len(data_list), inference_steps, bool(return_full_trajectory)
    svgd = None
    if svgd_weight_log_0 is not None and svgd_weight_log_1 is not None:
        svgd = dict(weight_log_0=svgd_weight_log_0, weight_log_1=svgd_weight_log_1, repulsive_weight_log_0=svgd_repulsive_weight_log_0,
                    repulsive_weight_log_1=svgd_repulsive_weight_log_1, kernel_size_log_0=svgd_kernel_size_log_0,
                    kernel_size_log_1=svgd_kernel_size_log_1, langevin_weight_log_0=svgd_langevin_weight_log_0,
                    langevin_weight_log_1=svgd_langevin_weight_log_1, rot_log_rel_weight=svgd_rot_log_rel_weight,
                    tor_log_rel_weight=svgd_tor_log_rel_weight, use_x0=bool(svgd_use_x0))
    conf_model = getattr(confidence_model, "module", confidence_model)
    model_async, schedules = _check_arguments(N, model, model_args, conf_model, filtering_data_list, inference_steps,
                                              (tr_schedule, rot_schedule, tor_schedule), t_schedule, asyncronous_noise_schedule, record,
                                              n_streams, svgd, ode, no_random, temp_sampling, pivot, return_features)
    device = torch.device(device)
    model = getattr(model, "module", model)
    score_crop = getattr(model_args, "crop_beyond", None)
    eng = model.engine_pool(n_streams=n_streams, max_batch=max(int(batch_size), 1)) if n_streams > 1 else model.engine()
    steps = _cached_steps(model, model_args, *schedules, np.asarray(t_schedule, dtype=np.float64) if model_async else None, ode, no_random,
                          no_final_step_noise, temp_sampling, temp_psi, temp_sigma_data)
    n_co = _co_count(co_schedule, data_list, batch_size, n_streams, score_crop, svgd)
    # the host-stepped samplers (and a CPU device) run their waves one after the other, without a side stream
    look_ahead = svgd is None and score_crop is None and n_streams == 1 and device.type == "cuda"
    host_step = None
    if svgd is not None:
        host_step = lambda s: _sample_svgd(s.engine, s.group.cplx, s.pos, steps, s.noise, schedules, svgd, N)
    elif score_crop is not None:
        host_step = lambda s: _sample_cropped(s.engine, s.group.cplx, s.group.key, s.pos, steps, s.noise, float(score_crop))
    trajectory, confidence = [None] * N, []
    with torch.no_grad(), _call_scope() as scope:
        waves = _walk(data_list, batch_size, eng.max_batch, n_co, model_args.no_torsion, S, noise, not (no_random or ode), no_final_step_noise)
        if waves:
            score = None
            if conf_model is not None:
                crop = getattr(filtering_model_args, "crop_beyond", None) if filtering_data_list is not None else None
                score = partial(_score_confidence, conf_model=conf_model, max_batch=eng.max_batch, filtering_data_list=filtering_data_list,
                                crop=crop, used=scope.conf_used, out=confidence)
            pipe = WavePipeline(device, _engine_sets(model, eng, waves, look_ahead, scope), side_fills=look_ahead, order_fills=_ORDER_SIDE_FILLS)
            _run_waves(pipe, waves, partial(_finish_wave, data_list=data_list, trajectory=trajectory, score=score), look_ahead,
                       steps=steps, trajectory=record, host_step=host_step)
        for idx, visualization in enumerate(visualization_list or []):
            center = data_list[idx].original_center.detach().cpu()
            if record:
                for t_idx in range(S):
                    visualization.add(trajectory[idx][t_idx] + center, part=1, order=t_idx + 2)
            else:
                visualization.add(data_list[idx]["ligand"].pos.detach().cpu() + center, part=1, order=2)
    for ceng in scope.conf_used:
        ceng.check()          # raises if any of the batches above exceeded a per-atom edge capacity
    confidence = torch.nan_to_num(torch.cat(confidence, dim=0), nan=-1000) if conf_model is not None else None
    return (data_list, confidence, trajectory) if record else (data_list, confidence)

