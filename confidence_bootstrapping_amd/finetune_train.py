"""The confidence-bootstrapping loop (reference finetune_train.py:133-349): alternate
  (1) `inference_epoch`: for every target complex sample `inference_samples` poses by reverse diffusion (the fused MI355X
      engine), score them with the confidence model (all-atom engine), compute symmetry-corrected RMSDs when the crystal pose is
      known, and keep the poses whose confidence exceeds `confidence_cutoff`;
  (2) push them into the `CBBuffer`, and
  (3) `train_epoch` on the buffer through `NoiseTransform` (differentiable HIP path), with EMA weights used for inference.
Same function names, argument meaning and metric keys as the reference; checkpoints / wandb / dataset construction (which need
rdkit, PyG datasets and the MOAD files) are the caller's business here: `inference_finetune` takes the complexes directly.
"""
from __future__ import annotations

import copy
import traceback
from functools import partial

import numpy as np
import torch

from .diffusion_utils import get_inverse_schedule, get_t_schedule
from .hetero import Batch
from .molecules_utils import get_symmetry_rmsd, remove_all_hs
from .sampling import randomize_position, randomize_position_batch, sampling
from .training import loss_function, train_epoch
from .hostcfg import with_glue_threads


def _copy(g):
    """the reference deep-copies the complex once per pose (finetune_train.py:169); poses only re-bind `pos`, so sharing the
    tensors is equivalent and 100x cheaper"""
    return g.shallow_copy() if hasattr(g, "shallow_copy") else copy.deepcopy(g)


def _as_batch1(g):
    return g if isinstance(g, Batch) else Batch.from_data_list([g])


def _crystal_inputs(orig, predictions_list, ligand_pos):
    """What the RMSD of a complex's poses is measured on: (heavy-atom poses [P, N, 3], crystal poses [Q, N, 3] in the frame of the poses,
    heavy-atom graph or None); None when the crystal pose is not known."""
    orig_pos = getattr(orig["ligand"], "orig_pos", None)
    if orig_pos is None:
        return None
    if isinstance(orig_pos, list):
        orig_pos = orig_pos[0]
    orig_pos = np.asarray(orig_pos, dtype=np.float32)
    orig_pos = orig_pos[None] if orig_pos.ndim == 2 else orig_pos
    filterHs = torch.not_equal(predictions_list[0]["ligand"].x[:, 0], 0).cpu().numpy()
    lp = ligand_pos[:, filterHs]
    ref = orig_pos[:, filterHs] - orig.original_center.cpu().numpy()
    mol = getattr(orig, "mol", None)
    mol = mol[0] if isinstance(mol, (list, tuple)) else mol
    mol = remove_all_hs(mol)          # RemoveAllHs(orig_complex_graph.mol[0]) in the reference; the coordinates are filtered with filterHs
    return lp, ref, mol


def _valid_poses(results, positions, device, group):
    """args.keep_valid: per complex a bool [n] -- evaluation.pose_checks' `valid` of each sampled pose (bond lengths, 1-3 distances,
    internal and receptor clashes on heavy atoms).  The receptor atoms come from the complex's all-atom graph: the first graph of
    `filtering_data_list` when it has an 'atom' store, else `orig`, shifted into the frame of the poses if the two `original_center`s
    differ; without an 'atom' store only the internal checks run.  ONE evaluation.pose_checks_batch call per `group` consecutive complexes
    on a GPU `device`, the host route on any other."""
    from .evaluation import ligand_check_tables, pose_checks, pose_checks_batch, receptor_check_atoms
    on_gpu = torch.device(device).type == "cuda"
    cpu = lambda t: t.detach().cpu().numpy() if torch.is_tensor(t) else np.asarray(t)
    valid = []
    for k in range(0, len(results), group):
        items = []
        for ((orig, _, filtering_data_list), (predictions_list, _)), ligand_pos in zip(results[k:k + group], positions[k:k + group]):
            filterHs = torch.not_equal(predictions_list[0]["ligand"].x[:, 0], 0).cpu().numpy()
            mol = getattr(orig, "mol", None)
            mol = mol[0] if isinstance(mol, (list, tuple)) else mol
            tables = None if mol is None else ligand_check_tables(mol)
            if tables is not None and len(tables[3]) != int(filterHs.sum()):
                print("pose checks: the molecule does not match the poses; no internal checks for this complex")
                tables = None
            receptor = None
            for graph in ([filtering_data_list[0]] if filtering_data_list else []) + [orig]:
                receptor = receptor_check_atoms(graph)
                if receptor is not None:
                    shift = (cpu(graph.original_center).reshape(1, 3) - cpu(orig.original_center).reshape(1, 3)).astype(np.float32)
                    if np.any(shift != 0):
                        receptor = (receptor[0] + shift, receptor[1])
                    break
            items.append((ligand_pos[:, filterHs], tables, receptor))
        found = pose_checks_batch(items, device) if on_gpu else [pose_checks(*item) for item in items]
        valid.extend(np.asarray(f.valid, dtype=bool) for f in found)
    return valid


def _keep_distinct(candidates, results, positions, confidence_cutoff, cutoff_rmsd, device, group, valid=None):
    """args.keep_distinct_rmsd: of each complex's poses above `confidence_cutoff`, only the heads of its binding modes -- the poses are
    clustered in descending confidence (evaluation.cluster_poses: symmetry-corrected heavy-atom RMSD in the receptor frame, cutoff
    `cutoff_rmsd`), ONE evaluation.cluster_poses_batch call per `group` consecutive complexes on a GPU `device`, the host route on any
    other.  `candidates`: [(index into results, predictions_list, final confidences float64 [n]), ...] in the order of `results`.
    `valid`: the per-complex masks of _valid_poses (args.keep_valid), or None: only valid poses are clustered.
    -> [(graph, confidence), ...] in the order the unfiltered list has."""
    from .evaluation import cluster_poses, cluster_poses_batch
    on_gpu = torch.device(device).type == "cuda"
    kept = []
    for k in range(0, len(candidates), group):
        chunk, items, picks = candidates[k:k + group], [], []
        for i, predictions_list, conf in chunk:
            above = np.flatnonzero(conf > confidence_cutoff if valid is None else (conf > confidence_cutoff) & valid[i])
            ranked = above[np.argsort(-conf[above], kind="stable")]          # descending confidence, ties in sampling order
            orig = results[i][0][0]
            filterHs = torch.not_equal(predictions_list[0]["ligand"].x[:, 0], 0).cpu().numpy()
            mol = getattr(orig, "mol", None)
            mol = remove_all_hs(mol[0] if isinstance(mol, (list, tuple)) else mol)
            picks.append(ranked)
            items.append((positions[i][ranked][:, filterHs], mol))
        live = [j for j, ranked in enumerate(picks) if len(ranked)]
        found = {}
        if live and on_gpu:
            found = dict(zip(live, cluster_poses_batch([items[j] for j in live], device, cutoff=cutoff_rmsd)))
        elif live:
            found = {j: cluster_poses(*items[j], cutoff=cutoff_rmsd) for j in live}
        for j, (i, predictions_list, conf) in enumerate(chunk):
            if j not in found:
                continue
            head = found[j][1]
            heads = set(int(picks[j][r]) for r in range(len(head)) if head[r] == r)
            kept.extend((predictions_list[i_], float(conf[i_])) for i_ in range(len(predictions_list)) if i_ in heads)
    return kept


def summarize_inference(results, args, filtering_args, confidence_cutoff, device, group=1):
    """The post-processing of inference_epoch (reference finetune_train.py:198-245): `results` = [((orig, data_list, filtering_data_list),
    (predictions_list, confidences)), ...] in sampling order -> (losses, [(graph, confidence), ...] above the cutoff, top-confidence
    RMSDs).  With `args.device_metrics` (opt-in) the RMSDs of each `group` consecutive complexes come from one
    evaluation.pose_metrics_batch call (cached isomorphisms, one upload / launch / download) instead of one get_symmetry_rmsd call per
    complex and crystal pose; everything else, and the order of every list, is the same.  With `args.keep_distinct_rmsd` = a cutoff in
    Angstrom (opt-in, default None) only the heads of each complex's binding modes among the poses above the cutoff are kept
    (_keep_distinct); `losses` and the top-confidence RMSDs do not change.  With `args.keep_valid` (opt-in, default absent / False) a pose is
    kept only if evaluation.pose_checks calls it valid (_valid_poses: one pose_checks_batch call per `group` on a GPU device); validity is
    decided first, so with `keep_distinct_rmsd` the modes are formed among the valid poses; `losses` and the top-confidence RMSDs do not
    change either."""
    rmsds, min_rmsds, top_rmsds, confidences_list, complexes_to_keep = [], [], [], [], []
    positions = [np.asarray([g["ligand"].pos.cpu().numpy() for g in predictions_list]) for _, (predictions_list, _) in results]
    inputs = [_crystal_inputs(orig, predictions_list, ligand_pos)
              for ((orig, _, _), (predictions_list, _)), ligand_pos in zip(results, positions)]
    device_rmsd = {}
    keep_distinct, candidates = getattr(args, "keep_distinct_rmsd", None), []
    valid = _valid_poses(results, positions, device, max(int(group), 1)) if getattr(args, "keep_valid", False) else None
    if getattr(args, "device_metrics", False):
        from .evaluation import pose_metrics_batch
        for k in range(0, len(results), max(int(group), 1)):
            ids = [i for i in range(k, min(k + max(int(group), 1), len(results))) if inputs[i] is not None]
            if ids:
                for i, out in zip(ids, pose_metrics_batch([inputs[i] for i in ids], device)):
                    device_rmsd[i] = out[0].astype(np.float64)
    for i, ((orig, _, _), (predictions_list, confidences)) in enumerate(results):
        if confidences is not None and isinstance(getattr(filtering_args, "rmsd_classification_cutoff", None), list):
            confidences = confidences[:, 0]
        if inputs[i] is not None:   # crystal pose known: RMSD metrics
            lp, ref, mol = inputs[i]
            if i in device_rmsd:
                rmsd = device_rmsd[i]
            else:
                per_ref = []
                for r in ref:
                    try:
                        per_ref.append(np.asarray(get_symmetry_rmsd(mol, r, [l for l in lp], device=device)))
                    except Exception as e:
                        print("Using non corrected RMSD because of the error:", e)
                        per_ref.append(np.sqrt(((lp - r) ** 2).sum(axis=2).mean(axis=1)))
                rmsd = np.min(np.asarray(per_ref), axis=0)
            rmsds.extend(rmsd.tolist())
            min_rmsds.append(rmsd.min())
            if confidences is not None:
                top_rmsds.append(rmsd[int(np.argmax(np.asarray([float(c) for c in confidences])))])
            if getattr(args, "oracle_confidence", False):
                confidences = -4 * np.tanh(2 * rmsd / 3 - 2)
        if confidences is None:
            continue
        confidences_list.extend(float(c) for c in confidences)
        if keep_distinct is not None:      # opt-in: decided after the loop, one launch per `group` of complexes
            candidates.append((i, predictions_list, np.asarray([float(c) for c in confidences], dtype=np.float64)))
            continue
        complexes_to_keep.extend((predictions_list[i_], float(confidences[i_])) for i_ in range(len(predictions_list))
                                 if float(confidences[i_]) > confidence_cutoff and (valid is None or valid[i][i_]))
    if keep_distinct is not None:
        complexes_to_keep = _keep_distinct(candidates, results, positions, confidence_cutoff, float(keep_distinct), device, max(int(group), 1),
                                           valid=valid)
    rmsds, min_rmsds, top_rmsds, conf = (np.asarray(x, dtype=np.float64) for x in (rmsds, min_rmsds, top_rmsds, confidences_list))
    pct = lambda a, thr, n: float(100 * (a < thr).sum() / n) if n else None
    losses = {"rmsds_lt2": pct(rmsds, 2, len(rmsds)), "rmsds_lt5": pct(rmsds, 5, len(rmsds)),
              "filtered_rmsds_lt2": pct(top_rmsds, 2, len(min_rmsds)), "filtered_rmsds_lt5": pct(top_rmsds, 5, len(min_rmsds)),
              "min_rmsds_lt2": pct(min_rmsds, 2, len(min_rmsds)), "min_rmsds_lt5": pct(min_rmsds, 5, len(min_rmsds)),
              "avg_confidence": float(conf.mean()) if len(conf) else None,
              "median_confidence": float(np.median(conf)) if len(conf) else None}
    return losses, complexes_to_keep, top_rmsds


@with_glue_threads
def inference_epoch(model, filtering_model, complex_graphs, filtering_complex_dict, device, t_to_sigma, args, filtering_args,
                    confidence_cutoff):
    """Sample + score every complex; returns (metrics, [(graph, confidence), ...] above the cutoff, top-confidence RMSDs)
    (reference finetune_train.py:133-245)."""
    t_schedule = get_t_schedule(sigma_schedule="expbeta", inference_steps=args.inference_steps, inf_sched_alpha=1, inf_sched_beta=1)
    asyn = bool(getattr(args, "asyncronous_noise_schedule", False))
    if asyn:      # finetune_train.py:137-140: every component runs on its own Beta quantile of the common time grid
        tr_schedule = get_inverse_schedule(t_schedule, args.sampling_alpha, args.sampling_beta)
        rot_schedule = get_inverse_schedule(t_schedule, args.rot_alpha, args.rot_beta)
        tor_schedule = get_inverse_schedule(t_schedule, args.tor_alpha, args.tor_beta)
    else:
        tr_schedule = rot_schedule = tor_schedule = t_schedule
    model.eval()
    n = args.inference_samples

    def run(items, bs):
        """one sampling() call over the poses of all `items` (complexes): consecutive complexes are co-scheduled on the GPU"""
        flat = [g for it in items for g in it[1]]
        filt = [g for it in items for g in it[2]] if items[0][2] is not None else None
        preds, conf = sampling(data_list=flat, model=model, inference_steps=args.inference_steps, tr_schedule=tr_schedule,
                               rot_schedule=rot_schedule, tor_schedule=tor_schedule, device=device, t_to_sigma=t_to_sigma, model_args=args,
                               confidence_model=filtering_model, filtering_data_list=filt, filtering_model_args=filtering_args,
                               asyncronous_noise_schedule=asyn, t_schedule=t_schedule, batch_size=bs)
        return [(preds[k * n:(k + 1) * n], None if conf is None else conf[k * n:(k + 1) * n]) for k in range(len(items))]

    prepared = []
    device_randomize = bool(getattr(args, "device_randomize", False))
    pocket = dict(pocket_knowledge=getattr(args, "inf_pocket_knowledge", False), pocket_cutoff=getattr(args, "inf_pocket_cutoff", 7))
    for orig in complex_graphs:
        orig = _as_batch1(orig)
        name = orig.name[0] if isinstance(orig.name, (list, tuple)) else orig.name
        filtering_data_list = None
        if filtering_model is not None and filtering_complex_dict is not None:
            if name not in filtering_complex_dict:
                print(f"HAPPENING | The filtering dataset did not contain {name}. We are skipping this complex.")
                continue
            filtering_data_list = [_copy(filtering_complex_dict[name]) for _ in range(n)]
        data_list = [_copy(orig) for _ in range(n)]
        if not device_randomize:
            randomize_position(data_list, args.no_torsion, False, args.tr_sigma_max, **pocket)
        prepared.append((orig, data_list, filtering_data_list))

    results = []
    group = 8 if n % max(args.inference_batch_size, 1) == 0 else 1      # loader batches must not straddle complexes
    if device_randomize:      # opt-in: the starting poses of each group of co-scheduled complexes in one launch, same draws in the same order
        for k in range(0, len(prepared), group):
            randomize_position_batch([it[1] for it in prepared[k:k + group]], args.no_torsion, False, args.tr_sigma_max, device, **pocket)
    for k in range(0, len(prepared), group):
        items = prepared[k:k + group]
        try:
            results.extend(zip(items, run(items, args.inference_batch_size)))
            continue
        except Exception as e:
            print("Exception while running inference on a group of complexes, retrying one by one:", e)
        for it in items:           # the reference's per-complex halve-and-retry protocol (finetune_train.py:176-196)
            out, failed, bs = None, 0, args.inference_batch_size
            while out is None and failed <= 5:
                try:
                    out = run([it], bs)[0]
                except Exception as e:
                    failed += 1
                    bs = max(bs // 2, 1)
                    print("Exception while running inference on complex:", e)
                    traceback.print_exc()
            if out is None:
                print("failed 5 times - skipping the complex")
                continue
            results.append((it, out))

    return summarize_inference(results, args, filtering_args, confidence_cutoff, device, group=group)


class _Loader:
    """DataListLoader stand-in: shuffled lists of `batch_size` transformed buffer items per epoch.  With `batch_transform` the loader
    fetches the UN-transformed items (`dataset.get`) and hands each batch's list to it once -- NoiseTransform.apply_noise_batch, which
    noises the whole batch on the GPU; same shuffle, same item order."""

    def __init__(self, dataset, batch_size, shuffle=True, drop_last=False, batch_transform=None):
        self.dataset, self.batch_size, self.shuffle, self.drop_last = dataset, batch_size, shuffle, drop_last
        self.batch_transform = batch_transform

    def __iter__(self):
        n = len(self.dataset)
        order = np.random.permutation(n) if self.shuffle else np.arange(n)
        for i in range(0, n, self.batch_size):
            idx = order[i:i + self.batch_size]
            if self.drop_last and len(idx) < self.batch_size:
                break
            if self.batch_transform is None:
                yield [self.dataset[int(k)] for k in idx]
            else:
                yield self.batch_transform([self.dataset.get(int(k)) for k in idx])

    def __len__(self):
        n = len(self.dataset)
        return n // self.batch_size if self.drop_last else (n + self.batch_size - 1) // self.batch_size


def inference_finetune(args, model, filtering_model, filtering_args, filtering_complex_dict, confidence_cutoff, optimizer, ema_weights,
                       finetune_dataset, target_complexes, t_to_sigma, device, log=print):
    """The outer loop (reference finetune_train.py:248-349).  `finetune_dataset` is a CBBuffer whose transform is a NoiseTransform,
    `target_complexes` the graphs of the target cluster.  Returns the per-epoch logs."""
    loss_fn = partial(loss_function, tr_weight=args.tr_weight, rot_weight=args.rot_weight, tor_weight=args.tor_weight,
                      no_torsion=args.no_torsion)
    history, loader = [], None
    for epoch in range(args.n_epochs):
        logs = {}
        ema_weights.store(model.parameters())
        if args.use_ema:
            ema_weights.copy_to(model.parameters())    # inference with the EMA weights
        if epoch % args.cb_inference_freq == 0:
            inf_dataset = list(target_complexes)[:args.num_inference_complexes]
            iterations = args.initial_iterations if epoch == 0 else args.inference_iterations
            complexes, metrics = [], None
            for _ in range(iterations):
                m, kept, _ = inference_epoch(model, filtering_model, inf_dataset, filtering_complex_dict, device, t_to_sigma, args,
                                             filtering_args, confidence_cutoff)
                metrics = metrics or {k: [] for k in m}
                for k in m:
                    if m[k] is not None:
                        metrics[k].append(m[k])
                complexes.extend(kept)
            finetune_dataset.add_complexes(complexes)
            batch_transform = None
            if getattr(args, "device_noise", False):       # opt-in: noise each batch with one launch instead of item by item on the host
                batch_transform = partial(finetune_dataset.transform.apply_noise_batch, device=device)
            loader = _Loader(finetune_dataset, args.batch_size, shuffle=True, drop_last=getattr(args, "dataloader_drop_last", False),
                             batch_transform=batch_transform)
            logs.update({"targetinf_" + k: (float(np.mean(v)) if v else None) for k, v in metrics.items()})
            logs["kept"] = len(complexes)
            logs["buffer"] = len(finetune_dataset.complexes)
        ema_weights.restore(model.parameters())
        if loader is not None and len(finetune_dataset.complexes) > 1:
            train_losses = train_epoch(model, loader, optimizer, device, t_to_sigma, loss_fn, ema_weights)
            logs.update({"train_" + k: v for k, v in train_losses.items()})
        log(f"Epoch {epoch}: " + ", ".join(f"{k} {v:.4f}" if isinstance(v, float) else f"{k} {v}" for k, v in logs.items()
                                         if k in ("kept", "buffer", "train_loss", "targetinf_avg_confidence")))
        history.append(logs)
    return history
