"""Reverse-diffusion trajectories recorded by the pose-update kernel (cbd_sample_traj) up to the files tools/dock.py writes.

The step loop is deterministic and the existing tests require replay = eager = separate calls bitwise, so every equality here is
torch.equal unless a tolerance is named:
  * 1e-3 A RMSD against the CPU oracle / the reference's golden trajectory: the tolerance of tests/test_gpu_parity.py's trajectory tests
  * 6e-5 A for a coordinate read back from an SDF (four decimals + the fp32 half-ulp below 128 A), 5.1e-4 A from a PDB (three decimals)
"""
import copy
import glob
import os
import re
from functools import partial

import numpy as np
import pytest
import torch

from tests.helpers import to_cx, rmsd

pytestmark = pytest.mark.gpu
T = torch.from_numpy
HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def model(dev):
    from confidence_bootstrapping_amd.utils import make_score_model
    return make_score_model(device=dev, seed=0)


def _steps(model, S):
    from confidence_bootstrapping_amd.engine import make_steps
    from confidence_bootstrapping_amd.diffusion_utils import get_t_schedule
    m, args = model
    return make_steps(get_t_schedule("expbeta", S), args, m.timestep_emb_func)


def _head(steps, n):
    from confidence_bootstrapping_amd.engine import cbd_step
    return (cbd_step * n)(*[steps[i] for i in range(n)])


def _inputs(cplx, B, S, seed, dev):
    """B start poses around the complex and explicit noise, on the device"""
    g = torch.Generator().manual_seed(seed)
    R = int(cplx["ligand"].edge_mask.sum())
    pos0 = cplx["ligand"].pos[None].repeat(B, 1, 1) + torch.randn(B, 1, 3, generator=g) * 5
    nz = [torch.randn(S, B, 3, generator=g).to(dev), torch.randn(S, B, 3, generator=g).to(dev), torch.randn(S, B * R, generator=g).to(dev)]
    return pos0.to(dev).contiguous(), nz


def _assert_prefix(eng, pos0, steps, nz, traj, ks):
    """traj[k] == the final pose of a call over the steps 0..k alone"""
    for k in ks:
        q = pos0.clone()
        eng.sample(q, _head(steps, k + 1), *[None if z is None else z[:k + 1].contiguous() for z in nz])
        assert torch.equal(traj[k], q), f"frame {k}"


@pytest.fixture(scope="module")
def tiny(dev, model):
    """the tiny complex (Nl 12, Nr 40, R 2) on an engine of its own, B = 3 / S = 4 inputs built as
    test_gpu_parity.py::test_config_c1_1a0q_single_sample_trajectory builds them (seeded randomize_position, torch.normal draws in the
    reference's order)"""
    from confidence_bootstrapping_amd import Batch
    from confidence_bootstrapping_amd.engine import DockEngine
    from confidence_bootstrapping_amd.synthetic import make_workload
    from confidence_bootstrapping_amd.sampling import randomize_position
    m, args = model
    cplx = make_workload("tiny")
    eng = DockEngine.from_model(m, dev, max_batch=8)
    eng.set_complex(cplx)
    assert (eng.Nl, eng.Nr, eng.R) == (12, 40, 2)
    B, S = 3, 4
    torch.manual_seed(3)
    np.random.seed(3)
    dl = [Batch.from_data_list([copy.deepcopy(cplx)]) for _ in range(B)]
    randomize_position(dl, False, False, args.tr_sigma_max)
    pos0 = torch.stack([d["ligand"].pos for d in dl]).float().contiguous()
    torch.manual_seed(4)
    noise = {"tr": [], "rot": [], "tor": []}
    for _ in range(S):
        noise["tr"].append(torch.normal(0, 1, (B, 3)))
        noise["rot"].append(torch.normal(0, 1, (B, 3)))
        noise["tor"].append(torch.normal(0, 1, (B * eng.R,)))
    noise = {k: torch.stack(v) for k, v in noise.items()}
    return dict(eng=eng, cplx=cplx, pos0=pos0, noise=noise, S=S, B=B)


@pytest.mark.parametrize("graph", [0, 1])
def test_prefix_property(tiny, model, dev, graph):
    eng, S = tiny["eng"], tiny["S"]
    eng.set_option("graph", graph)
    steps = _steps(model, S)
    pos0 = tiny["pos0"].to(dev)
    nz = [tiny["noise"][k].to(dev) for k in ("tr", "rot", "tor")]
    p = pos0.clone()
    traj = eng.sample(p, steps, *nz, trajectory=True)
    assert traj.shape == (S, tiny["B"], 12, 3) and traj.is_cuda and traj.dtype == torch.float32
    assert torch.equal(traj[S - 1], p)
    plain = pos0.clone()
    assert eng.sample(plain, steps, *nz) is None
    assert torch.equal(plain, p)
    _assert_prefix(eng, pos0, steps, nz, traj, range(S))
    # with the per-step scores as well: the same frames, the same scores as the scores-only call
    q = pos0.clone()
    scores, traj2 = eng.sample(q, steps, *nz, return_scores=True, trajectory=True)
    assert torch.equal(traj2, traj) and torch.equal(scores, eng.sample(pos0.clone(), steps, *nz, return_scores=True))
    eng.set_option("graph", 0)


def test_against_the_cpu_oracle(tiny, model, dev, tables):
    from confidence_bootstrapping_amd.diffusion_utils import get_t_schedule
    from oracle import score_ref as sr, pose_ref as pr
    m, _ = model
    eng, S = tiny["eng"], tiny["S"]
    so3, torus = tables
    sched = get_t_schedule("expbeta", S)
    _, trace = pr.sampling_ref({k: v.cpu() for k, v in m.state_dict().items()}, to_cx(tiny["cplx"]), tiny["pos0"], sched, sr.ScoreConfig(),
                               so3, torus, noise=tiny["noise"], record=True)
    for graph in (0, 1):
        eng.set_option("graph", graph)
        traj = eng.sample(tiny["pos0"].to(dev), _steps(model, S), *[tiny["noise"][k].to(dev) for k in ("tr", "rot", "tor")], trajectory=True).cpu()
        for k in range(S):
            err = float(rmsd(traj[k], trace[k]["pos"]).max())
            print(f"graph {graph} frame {k}: max RMSD vs oracle {err:.2e} A")
            assert err < 1e-3
    eng.set_option("graph", 0)


def _rigid_exit(eng, cplx, model, dev):
    S, B = 3, 2
    steps = _steps(model, S)
    pos0, nz = _inputs(cplx, B, S, 11, dev)
    if eng.R == 0:
        nz[2] = None
    for graph in (0, 1):
        eng.set_option("graph", graph)
        p = pos0.clone()
        traj = eng.sample(p, steps, *nz, trajectory=True)
        assert torch.equal(traj[-1], p)
        assert all(not torch.equal(traj[k], pos0) for k in range(S))
        assert all(not torch.equal(traj[k], traj[k + 1]) for k in range(S - 1))
        _assert_prefix(eng, pos0, steps, nz, traj, range(S))


def test_rigid_early_return(model, dev):
    """the exit of the pose update that skips torsions and Kabsch: a ligand without rotatable bonds, and a no_torsion model"""
    from confidence_bootstrapping_amd.engine import DockEngine
    from confidence_bootstrapping_amd.synthetic import make_complex, make_workload
    from confidence_bootstrapping_amd.utils import make_score_model, load_model_args
    rigid = make_complex(Nl=9, Nr=40, R=0, knn=8, seed=5)
    eng = DockEngine.from_model(model[0], dev, max_batch=4)
    eng.set_complex(rigid)
    assert eng.R == 0
    _rigid_exit(eng, rigid, model, dev)
    args = load_model_args()
    args.no_torsion = True
    nt = make_score_model(device=dev, seed=3, args=args)
    eng = DockEngine.from_model(nt[0], dev, max_batch=4)
    eng.set_complex(make_workload("tiny"))
    assert eng.R == 2 and eng.cfg.no_torsion == 1
    _rigid_exit(eng, make_workload("tiny"), nt, dev)


def test_lane_and_batch_strides(model, dev):
    from confidence_bootstrapping_amd.engine import DockEngine
    from confidence_bootstrapping_amd.synthetic import make_complex, make_workload
    eng = DockEngine.from_model(model[0], dev, max_batch=4)
    # (b) more atoms than lanes: every lane-strided loop of the kernel runs twice; (c) B below max_batch: the rows stride by B
    for cplx, S in ((make_complex(Nl=70, Nr=40, R=2, knn=8), 2), (make_workload("tiny"), 3)):
        eng.set_complex(cplx)
        steps = _steps(model, S)
        pos0, nz = _inputs(cplx, 2, S, 21, dev)
        for graph in (0, 1):
            eng.set_option("graph", graph)
            p = pos0.clone()
            traj = eng.sample(p, steps, *nz, trajectory=True)
            assert traj.shape == (S, 2, eng.Nl, 3) and torch.equal(traj[-1], p)
            _assert_prefix(eng, pos0, steps, nz, traj, range(S))


@pytest.mark.parametrize("graph", [0, 1])
def test_coscheduling_replay_and_stale_pointer(model, dev, graph):
    """graph = 1 is the case the captured loop replays; graph = 0 is the one where the descriptor points at the CALLER's buffer, so a
    pointer that survived into a later plain call would show as a changed (still live) trajectory tensor."""
    from confidence_bootstrapping_amd.engine import DockEngine
    from confidence_bootstrapping_amd.synthetic import make_complex, make_workload
    S = 3
    steps = _steps(model, S)
    ca, cb = make_workload("tiny"), make_complex(Nl=20, Nr=48, R=3, knn=8)
    e0 = DockEngine.from_model(model[0], dev, max_batch=4)
    e1 = DockEngine(dev, max_batch=4)
    e1.share_weights_from(e0)
    e0.set_complex(ca)
    e1.set_complex(cb)
    engines = [e0, e1]
    for e in engines:
        e.set_option("graph", graph)

    def separate(inputs):
        out = []
        for e, (p0, nz) in zip(engines, inputs):
            p = p0.clone()
            out.append((e.sample(p, steps, *nz, trajectory=True), p))
        return out
    first = [_inputs(ca, 3, S, 31, dev), _inputs(cb, 2, S, 32, dev)]
    ref = separate(first)
    # (i) record one, the other, both
    for want in ([True, False], [False, True], [True, True]):
        poses = [p0.clone() for p0, _ in first]
        trajs = DockEngine.sample_multi(engines, poses, steps, [nz for _, nz in first], trajectory=want)
        for k in range(2):
            assert torch.equal(poses[k], ref[k][1])
            assert (trajs[k] is None) == (not want[k])
            if want[k]:
                assert torch.equal(trajs[k], ref[k][0])
    # (ii) the same call (the same cached graph) on other inputs with fresh output buffers
    second = [_inputs(ca, 3, S, 41, dev), _inputs(cb, 2, S, 42, dev)]
    poses2 = [p0.clone() for p0, _ in second]
    trajs2 = DockEngine.sample_multi(engines, poses2, steps, [nz for _, nz in second], trajectory=True)
    for k, e in enumerate(engines):
        assert trajs2[k].data_ptr() != trajs[k].data_ptr() and not torch.equal(trajs2[k], trajs[k])
        _assert_prefix(e, second[k][0], steps, second[k][1], trajs2[k], [0])
        assert torch.equal(trajs2[k][-1], poses2[k])
    # (iii) later calls that do not record leave the recorded tensors (kept alive here) alone
    torch.cuda.synchronize()
    kept = [t.clone() for t in trajs2]
    poses3 = [p0.clone() for p0, _ in first]
    assert DockEngine.sample_multi(engines, poses3, steps, [nz for _, nz in first]) is None
    for k, e in enumerate(engines):
        assert torch.equal(poses3[k], ref[k][1])
        B = first[k][0].shape[0]
        g = torch.Generator().manual_seed(50 + k)
        e.modify_conformer(first[k][0], torch.randn(B, 3, generator=g), 0.3 * torch.randn(B, 3, generator=g), torch.randn(B * e.R, generator=g))
        e.sample(first[k][0].clone(), steps, *first[k][1])
    torch.cuda.synchronize()
    for k in range(2):
        assert torch.equal(trajs2[k], kept[k])


class _Recorder:
    def __init__(self):
        self.calls = []

    def add(self, coords, order, part=0, repeat=1):
        self.calls.append((part, order, coords.clone()))


def test_python_api(golden, model, dev):
    from confidence_bootstrapping_amd import Batch
    from confidence_bootstrapping_amd.synthetic import make_workload, make_complex
    from confidence_bootstrapping_amd.sampling import sampling
    from confidence_bootstrapping_amd.diffusion_utils import t_to_sigma
    g = golden("g6_sampling.npz")
    m, args = model
    cplx = make_workload("tiny")
    pos0 = T(g["pos0"])
    center = torch.tensor([[10.5, -20.25, 30.125]])

    def data_list(extra=None):
        out = []
        for i in range(pos0.shape[0]):
            d = Batch.from_data_list([copy.deepcopy(cplx)])
            d["ligand"].pos = pos0[i].clone()
            d.original_center = center.clone()
            out.append(d)
        if extra is not None:
            for i in range(2):
                d = Batch.from_data_list([copy.deepcopy(extra)])
                d["ligand"].pos = extra["ligand"].pos + torch.tensor([[2.0 * i, 1.0, -1.0]])
                d.original_center = center.clone()
                out.append(d)
        return out

    def run(dl, **kw):
        torch.manual_seed(42)   # the seed oracle/make_golden.py set before the reference's sampling()
        return sampling(dl, m, 20, g["schedule"], g["schedule"], g["schedule"], dev, partial(t_to_sigma, args=args), args, **kw)
    eng = m.engine()
    try:
        for bs, graph in ((3, 0), (2, 1)):
            eng.set_option("graph", graph)
            plain_vis = [_Recorder() for _ in range(3)]
            plain, conf = run(data_list(), batch_size=bs, visualization_list=plain_vis)
            assert conf is None
            vis = [_Recorder() for _ in range(3)]
            out, conf, trajectory = run(data_list(), batch_size=bs, return_full_trajectory=True, visualization_list=vis)
            assert conf is None and len(trajectory) == 3
            # The golden trajectory was drawn with ONE loader batch of 3 poses: the seeded call reproduces its draws at batch_size=3
            # only (at 2 the per-batch draw order differs, in the reference as well).  With the golden run's own noise handed in, the
            # comparison holds at both batch sizes.
            given, _, given_traj = run(data_list(), batch_size=bs, return_full_trajectory=True,
                                       noise={k: T(g["noise_" + k]) for k in ("tr", "rot", "tor")})
            for res, tr_ in ((given, given_traj),) + (((out, trajectory),) if bs == 3 else ()):
                got = torch.stack([d["ligand"].pos.cpu() for d in res])
                err = float(rmsd(got, T(g["final_pos"])).max())
                print(f"batch_size {bs}: final poses vs the reference's, max RMSD {err:.2e} A")
                assert err < 1e-3
                assert all(torch.equal(tr_[i][-1], got[i]) for i in range(3))
            for i in range(3):
                t = trajectory[i]
                assert t.shape == (20, 12, 3) and t.dtype == torch.float32 and not t.is_cuda
                assert torch.equal(t[-1], out[i]["ligand"].pos.cpu())
                assert torch.equal(out[i]["ligand"].pos.cpu(), plain[i]["ligand"].pos.cpu())
                assert [(p, o) for p, o, _ in vis[i].calls] == [(1, k + 2) for k in range(20)]
                assert all(torch.equal(c, t[k] + center) for k, (_, _, c) in enumerate(vis[i].calls))
                assert [(p, o) for p, o, _ in plain_vis[i].calls] == [(1, 2)]
                assert torch.equal(plain_vis[i].calls[0][2], plain[i]["ligand"].pos.cpu() + center)
        eng.set_option("graph", 0)
        # a second complex of another size in the same call (two co-scheduled groups in one wave)
        other = make_complex(Nl=17, Nr=60, R=3, knn=10, seed=77, name="other")
        plain, _ = run(data_list(other), batch_size=3)
        out, _, trajectory = run(data_list(other), batch_size=3, return_full_trajectory=True)
        assert [t.shape for t in trajectory] == [(20, 12, 3)] * 3 + [(20, 17, 3)] * 2
        for i in range(5):
            assert torch.equal(trajectory[i][-1], out[i]["ligand"].pos.cpu())
            assert torch.equal(out[i]["ligand"].pos.cpu(), plain[i]["ligand"].pos.cpu())
        assert not torch.equal(trajectory[3], trajectory[4])
        with pytest.raises(NotImplementedError):
            run(data_list(), batch_size=3, return_full_trajectory=True, n_streams=2)
    finally:
        eng.set_option("graph", 0)


def _pdb_models(path):
    models = []
    for line in open(path):
        if line.startswith("MODEL"):
            models.append([])
        elif line.startswith("HETATM"):
            models[-1].append((float(line[30:38]), float(line[38:46]), float(line[46:54])))
    return [np.asarray(m) for m in models]


def test_front_door(tmp_path, dev):
    from confidence_bootstrapping_amd.datasets import process_mols as pm
    from tools import dock
    D = os.path.join(HERE, "golden", "1a0q")
    out = str(tmp_path / "docked")
    order, data_list, confidence = dock.main(["--protein", os.path.join(D, "1a0q_protein_processed.pdb.gz"),
                                              "--ligand", os.path.join(D, "1a0q_ligand.sdf"), "--out", out, "--samples", "4", "--steps", "4",
                                              "--save-visualisation"])
    assert os.path.exists(os.path.join(out, "rank1.sdf"))
    confs = []
    for k in range(1, 5):
        files = glob.glob(os.path.join(out, f"rank{k}_confidence*.sdf"))
        assert len(files) == 1
        confs.append(float(re.fullmatch(rf"rank{k}_confidence(-?\d+\.\d\d)\.sdf", os.path.basename(files[0])).group(1)))
        assert len(_pdb_models(os.path.join(out, f"rank{k}_reverseprocess.pdb"))) == 4 + 3
    assert len(glob.glob(os.path.join(out, "*"))) == 1 + 4 + 4
    assert all(confs[k] >= confs[k + 1] for k in range(3))
    best = int(torch.argmax(confidence))
    assert order[0] == best and abs(confs[0] - float(confidence[best])) <= 0.005 + 1e-6
    want = data_list[best]["ligand"].pos.cpu().double().numpy() + data_list[best].original_center.cpu().double().numpy()
    back = pm.read_molecule(os.path.join(out, "rank1.sdf"))
    assert back.GetNumAtoms() == 23
    assert np.abs(back.pos - want).max() <= 6e-5
    assert np.abs(_pdb_models(os.path.join(out, "rank1_reverseprocess.pdb"))[-1] - want).max() <= 5.1e-4
