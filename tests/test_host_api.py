"""Host-side logic without a GPU: the C-ABI library loads and exports every declared symbol, the Python shim
mirrors the reference's interfaces, and the product fails loudly (no CPU fallback) when no GPU is present."""
import copy
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_library_exports_every_declared_symbol():
    from confidence_bootstrapping_amd import engine
    lib = engine.load_library()
    hdr = open(os.path.join(ROOT, "include", "cbdock.h")).read()
    declared = set(re.findall(r"\b(cbd_[a-z_0-9]+)\s*\(", hdr))
    assert declared == set(engine.SYMBOLS), declared ^ set(engine.SYMBOLS)
    for name in declared:
        assert getattr(lib, name) is not None
    assert b"gfx950" in lib.cbd_version()


def test_product_library_holds_only_correct_kernels():
    """the timing-only kernel variants with WRONG results (CBD_CONV_VARIANT 9-13, CBD_BF16_DIAG bits), the phase-stamp
    builds and the losing role-split experiment are compiled into experiments/libcbdock_diag.so only (tools/diag_lib.py).  The product
    library exports no non-zero VAR / DIAG instantiation of a tensor-product kernel, does not contain the persistent role-split kernel
    and never reads the diagnostic environment variables; the package does not import experiments/ or a library GEMM for the TP op."""
    import subprocess
    lib = os.path.join(ROOT, "confidence_bootstrapping_amd", "libcbdock.so")
    names = subprocess.run(["nm", "-C", "--defined-only", lib], capture_output=True, text=True, check=True).stdout
    seen = 0
    for m in re.finditer(r"__device_stub__(tp_conv_kernel|tp_conv64_kernel|tp_conv64s_kernel)<([^>]*)>", names):
        args = [a.strip() for a in m.group(2).split(",")]
        var = args[0] if m.group(1) == "tp_conv64s_kernel" else args[2]
        assert var == "0", m.group(0)
        seen += 1
    assert seen >= 13, seen          # 4 levels x (fp32, bf16x3, bf16 streaming) + the register-stationary kernel
    assert "tp_conv64p" not in names and "bf16p" not in names
    raw = open(lib, "rb").read()
    for env in (b"CBD_CONV_VARIANT", b"CBD_BF16_DIAG", b"CBD_BF16_ROLES", b"CBD_BF16P_WGS", b"CBD_DIAG_MIN_ROLES", b"CBD_S_WEIGHTS", b"CBD_S_EQUAL_UNITS"):
        assert env not in raw, env
    pkg = os.path.join(ROOT, "confidence_bootstrapping_amd")
    for dp, _, fs in os.walk(pkg):
        for f in fs:
            if f.endswith(".py"):
                txt = open(os.path.join(dp, f)).read()
                assert not re.search(r"^\s*(from|import)\s+experiments\b", txt, re.M), f
    ops = open(os.path.join(pkg, "train_ops.py")).read()
    assert "torch.mm(" not in ops and "torch.bmm(" not in ops and "GH_KERNEL" not in ops


def test_product_does_not_import_oracle():
    pkg = os.path.join(ROOT, "confidence_bootstrapping_amd")
    for dp, _, fs in os.walk(pkg):
        for f in fs:
            if f.endswith((".py", ".hip", ".h")):
                txt = open(os.path.join(dp, f)).read()
                assert not re.search(r"^\s*(from|import)\s+oracle\b", txt, re.M), f


def test_no_cpu_fallback_without_gpu(score_model):
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    from confidence_bootstrapping_amd import Batch
    from confidence_bootstrapping_amd.synthetic import make_workload
    from confidence_bootstrapping_amd.diffusion_utils import set_time
    model, args = score_model
    b = Batch.from_data_list([make_workload("tiny")])
    set_time(b, None, 0.5, 0.5, 0.5, 1, False, False, torch.device("cpu"))
    with pytest.raises(RuntimeError):
        model(b)


def test_state_dict_layout_matches_reference_shapes(score_model):
    model, _ = score_model
    sd = model.state_dict()
    assert sum(p.numel() for p in model.parameters()) == 4084564
    assert len(sd) == 215
    assert sd["conv_layers.0.fc.3.3.weight"].shape == (1660, 96) and "conv_layers.4.fc.2.0.weight" not in sd
    assert sd["rec_node_embedding.additional_features_embedder.weight"].shape == (32, 1312)
    assert sd["final_conv.batch_norm.bias"].shape == (0,) and sd["final_conv.fc.3.weight"].shape == (124, 64)
    assert sd["tor_bond_conv.fc.3.weight"].shape == (384, 96) and sd["tor_final_layer.0.weight"].shape == (32, 64)
    # e3nn persistent buffers in a real checkpoint are accepted and ignored
    extra = dict(sd)
    extra["final_conv.tp.output_mask"] = torch.ones(12)
    extra["final_tp_tor.output_mask"] = torch.ones(20)
    model.load_state_dict(extra, strict=True)


def test_unsupported_architectures_raise():
    from confidence_bootstrapping_amd.utils import load_model_args, get_model
    from functools import partial
    from confidence_bootstrapping_amd.diffusion_utils import t_to_sigma
    a = load_model_args()
    a.sh_lmax = 2
    with pytest.raises(NotImplementedError):
        get_model(a, torch.device("cpu"), partial(t_to_sigma, args=a), no_parallel=True)


def test_randomize_position_matches_reference(golden):
    from confidence_bootstrapping_amd import Batch
    from confidence_bootstrapping_amd.synthetic import make_workload
    from confidence_bootstrapping_amd.sampling import randomize_position
    g = golden("g7_randomize.npz")
    for wl in ("tiny", "c2_dockgen_median"):
        cplx = make_workload(wl)
        dl = [Batch.from_data_list([copy.deepcopy(cplx)]) for _ in range(4)]
        np.random.seed(7)
        torch.manual_seed(7)
        randomize_position(dl, False, False, 19.0)
        got = torch.stack([d["ligand"].pos for d in dl])
        torch.testing.assert_close(got, torch.from_numpy(g[f"{wl}_pos"]), rtol=0, atol=2e-5)


def test_make_steps_matches_oracle_scalars(score_model, tables):
    from confidence_bootstrapping_amd.engine import make_steps
    from oracle import pose_ref as pr, score_ref as sr
    model, args = score_model
    sched = pr.get_t_schedule(20)
    steps = make_steps(sched, args, model.timestep_emb_func)
    cfg = sr.ScoreConfig()
    so3, torus = tables
    for i in (0, 7, 19):
        ts, dts, sig, g = pr.sde_coefficients(i, sched, cfg)
        t, dt = ts[0], dts[0]
        assert steps[i].tr_score_coef == pytest.approx(float(g[0] ** 2 * dt), rel=1e-6)
        assert steps[i].tor_noise_coef == pytest.approx(float(g[2] * np.sqrt(dt)), rel=1e-6)
        ct = float(t) * torch.ones(1)
        s_t = sr.t_to_sigma(ct, ct, ct, cfg)
        assert steps[i].cross_cutoff == float((s_t[0] * 3 + 20)[0])
        assert steps[i].rot_score_norm == float(sr.so3_score_norm(so3, s_t[1].numpy())[0])
        emb = sr.sinusoidal_embedding(1000.0 * ct, 32)[0]
        assert [steps[i].sigma_emb[k] for k in range(32)] == [float(x) for x in emb]
    last = make_steps(sched, args, model.timestep_emb_func, no_final_step_noise=True)[19]
    assert last.tr_noise_coef == 0.0 and last.tr_score_coef == steps[19].tr_score_coef
    ode = make_steps(sched, args, model.timestep_emb_func, ode=True)[3]
    assert ode.tr_score_coef == pytest.approx(0.5 * steps[3].tr_score_coef, rel=1e-6) and ode.rot_noise_coef == 0.0
    # --different_schedules: every component on its own grid (the translation grid drives the embedding and the cross cutoff)
    rot_s, tor_s = sched ** 2, np.sqrt(sched)
    diff = make_steps(sched, args, model.timestep_emb_func, rot_schedule=rot_s, tor_schedule=tor_s)
    for i in (0, 5, 19):
        ts, dts, sig, g = pr.sde_coefficients(i, sched, cfg, rot_s, tor_s)
        assert diff[i].tr_score_coef == steps[i].tr_score_coef and diff[i].cross_cutoff == steps[i].cross_cutoff
        assert [diff[i].sigma_emb[k] for k in range(32)] == [steps[i].sigma_emb[k] for k in range(32)]
        assert diff[i].rot_score_coef == pytest.approx(float(g[1] ** 2 * dts[1]), rel=1e-6)
        assert diff[i].tor_noise_coef == pytest.approx(float(g[2] * np.sqrt(dts[2])), rel=1e-6)
        s_t = sr.t_to_sigma(float(ts[0]) * torch.ones(1), float(ts[1]) * torch.ones(1), float(ts[2]) * torch.ones(1), cfg)
        assert diff[i].rot_score_norm == float(sr.so3_score_norm(so3, s_t[1].numpy())[0])


def test_bench_refuses_to_report_a_smaller_run():
    """`python bench.py --gpus 2` on a box with fewer than 2 GPUs (here: none) exits non-zero and prints no JSON line -- it must never
    report `n_gpus: 1` for a multi-GPU request; a rank whose WORLD_SIZE disagrees with --gpus fails the same way."""
    import json
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK")}
    r = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "2"], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode != 0 and "GPU" in r.stderr
    assert not any(l.strip().startswith("{") for l in r.stdout.splitlines())
    env2 = dict(env, RANK="0", WORLD_SIZE="1", LOCAL_RANK="0")
    r = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "2"], capture_output=True, text=True, env=env2, timeout=300)
    assert r.returncode != 0 and "WORLD_SIZE" in r.stderr and not r.stdout.strip()


def test_embedding_table_offsets_are_keyed_by_content_not_by_object_identity():
    """train_forward.atom_encoder_index caches the row offsets of an encoder's concatenated embedding tables.  Keyed by id(encoder)
    (round 3, first version) a NEW encoder could inherit the offsets of a garbage-collected one of another shape: wrong embedding rows
    or indices beyond the table (a GPU memory fault in 1 of 10 runs of the training tests).  The key is the tuple of table sizes."""
    import gc
    import torch
    from confidence_bootstrapping_amd.score_model import AtomEncoder
    from confidence_bootstrapping_amd import train_forward as tf
    for rep in range(50):
        dims = ([3 + rep % 4, 5, 2 + rep % 3], 0) if rep % 2 else ([7 + rep % 5], 0)
        enc = AtomEncoder(8, dims, 0)
        x = torch.stack([torch.randint(0, d, (11,)) for d in dims[0]], 1).float()
        idx = tf.atom_encoder_index(enc, x)
        offs = torch.tensor([0] + list(torch.tensor(dims[0]).cumsum(0)[:-1]))
        assert idx.shape == (11 * len(dims[0]),) and torch.equal(idx.view(11, -1), x.long() + offs)
        assert int(idx.max()) < sum(dims[0])
        del enc
        gc.collect()


def test_glue_threads_is_reference_counted_and_gpu_only():
    """hostcfg: nested / overlapping users restore the saved thread count only when the last one leaves; the decorator
    leaves torch's threads alone when the wrapped call runs on the CPU."""
    import threading
    import torch
    from confidence_bootstrapping_amd import hostcfg
    before = torch.get_num_threads()
    if before < 2:
        torch.set_num_threads(2)
    base = torch.get_num_threads()
    try:
        with hostcfg.glue_threads(1):
            assert torch.get_num_threads() == 1
            with hostcfg.glue_threads(1):
                assert torch.get_num_threads() == 1
            assert torch.get_num_threads() == 1          # the inner exit must not restore
        assert torch.get_num_threads() == base
        # two host threads entering and leaving out of order
        inside, leave_a = threading.Event(), threading.Event()
        def a():
            with hostcfg.glue_threads(1):
                inside.set(); leave_a.wait(5)
        t = threading.Thread(target=a); t.start(); inside.wait(5)
        with hostcfg.glue_threads(1):
            leave_a.set(); t.join()
            assert torch.get_num_threads() == 1          # thread a left first: still limited for this user
        assert torch.get_num_threads() == base
        seen = {}
        @hostcfg.with_glue_threads
        def step(model, device, x=0):
            seen[str(device)] = torch.get_num_threads()
        step(None, "cpu"); step(None, device="cuda:0")
        assert seen["cpu"] == base and seen["cuda:0"] == 1
        assert hostcfg.dev_key("cpu") == "cpu" and hostcfg.dev_key("cuda:1") == "cuda:1"
    finally:
        torch.set_num_threads(before)


def test_remove_all_hs_gives_the_heavy_atom_graph():
    """the reference passes RemoveAllHs(mol) to get_symmetry_rmsd next to filterHs-filtered coordinates
    (utils/training.py:352, finetune_train.py:210); a molecule that still carries hydrogens must be reduced the same way."""
    from confidence_bootstrapping_amd.molecules_utils import remove_all_hs, _graph_of

    class Mol:          # methanol with explicit hydrogens: C O H H H H
        atomicnums = np.array([6, 8, 1, 1, 1, 1])
        adjacency_matrix = np.zeros((6, 6), dtype=int)
    for i, j in ((0, 1), (0, 2), (0, 3), (0, 4), (1, 5)):
        Mol.adjacency_matrix[i, j] = Mol.adjacency_matrix[j, i] = 1
    nums, am = _graph_of(remove_all_hs(Mol))
    assert nums.tolist() == [6, 8] and am.tolist() == [[0, 1], [1, 0]]
    heavy = remove_all_hs(remove_all_hs(Mol))
    assert _graph_of(heavy)[0].tolist() == [6, 8]       # idempotent: no hydrogens left -> returned as is
    assert remove_all_hs(None) is None


def test_timed_region_stats_cuts_the_trace_between_the_markers(tmp_path):
    """tools/timed_region_stats.py (round 6): from a rocprofv3 kernel trace keep only the dispatches between the two marker kernels of
    `bench.py --mark-timed-region` and recompute roofline.frac from them.  Synthetic trace: 3 warm-up tp_conv launches in front of the
    first marker, 4 timed ones (1 ms each) + another kernel between the markers, 2 launches behind the second marker."""
    import csv
    import json
    import subprocess
    import sys
    d = tmp_path / "trace" / "sub"
    d.mkdir(parents=True)
    rows, t = [], 1000
    def add(name, dur):
        nonlocal t
        rows.append({"Kernel_Name": name, "Start_Timestamp": t, "End_Timestamp": t + dur})
        t += dur + 500
    conv = "void cbd::tp_conv_kernel<3, 3, 0, cbd::OpsF32>(cbd::ConvArgs)"
    mark = "void at::native::vectorized_elementwise_kernel<4, at::native::CUDAFunctorOnSelf_add<short>, std::array<char*, 2ul> >(int, ...)"
    for _ in range(3):
        add(conv, 2_000_000)
    add(mark, 3000)
    for _ in range(4):
        add(conv, 1_000_000)
    add("cbd::node_proj_kernel(cbd::ProjArgs)", 50_000)
    add(mark, 3000)
    for _ in range(2):
        add(conv, 1_000_000)
    with open(d / "p_kernel_trace.csv", "w", newline="") as f:
        w = csv.DictWriter(f, fieldnames=["Kernel_Name", "Start_Timestamp", "End_Timestamp"])
        w.writeheader()
        w.writerows(rows)
    rf = {"frac": 0.5, "peak": 100.0, "launches": 4, "executed_gflop_per_launch": 50.0, "executed_tflop_total": 0.2, "tp_conv_ms_total": 4.0}
    line = {"metric": "m", "value": 1.0, "ms_per_step": 1.0, "steps": 4, "warmup": 3, "roofline": rf}
    lf = tmp_path / "line.json"
    lf.write_text(json.dumps({"leg": "headline_detail", "roofline": rf}) + "\n" + json.dumps(line) + "\n")
    out = str(tmp_path / "rX")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "timed_region_stats.py"), str(tmp_path / "trace"), str(lf), out],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    rec = json.load(open(out + "_timed_recompute.json"))
    assert rec["tp_conv_launches_in_trace"] == 4 and rec["dispatches_in_region"] == 5 and rec["kernels_in_region"] == 2
    assert abs(rec["tp_conv_ms_total_trace"] - 4.0) < 1e-9
    assert abs(rec["frac_recomputed_from_trace"] - 0.2 / 4e-3 / 100.0) < 1e-4          # 0.2 TFLOP / 4 ms / 100 TFLOP/s = 0.5
    stats = list(csv.DictReader(open(out + "_timed_kernel_stats.csv")))
    assert stats[0]["Name"] == conv and stats[0]["Calls"] == "4" and stats[0]["TotalDurationNs"] == "4000000"


def test_diagnostic_library_still_builds():
    """The diagnostic twin is not linked into the product, so nothing else notices when a change breaks its #ifdef CBD_DIAG code.
    Incremental build of the twin (tools/diag_lib.py: the product sources with -DCBD_DIAG); it must export the whole C ABI too, and
    it holds no kernel that computes wrong results: the only diagnostic instantiations are the phase stamps / non-temporal gathers of
    tp_conv_kernel (VAR 8, 14) and the phase stamps of tp_conv64_kernel (DIAG 4)."""
    import ctypes
    import subprocess
    sys_path = os.path.join(ROOT)
    import sys
    if sys_path not in sys.path:
        sys.path.insert(0, sys_path)
    from tools import diag_lib
    from confidence_bootstrapping_amd import engine
    path = diag_lib.build()
    lib = ctypes.CDLL(path)
    for name in engine.SYMBOLS:
        assert getattr(lib, name) is not None
    names = subprocess.run(["nm", "-C", "--defined-only", path], capture_output=True, text=True, check=True).stdout
    seen = set()
    for m in re.finditer(r"__device_stub__(tp_conv_kernel|tp_conv64_kernel)<([^>]*)>", names):
        var = m.group(2).split(",")[2].strip()
        assert var in (("0", "8", "14") if m.group(1) == "tp_conv_kernel" else ("0", "4")), m.group(0)
        seen.add((m.group(1), var))
    assert {("tp_conv_kernel", "0"), ("tp_conv_kernel", "8"), ("tp_conv_kernel", "14"), ("tp_conv64_kernel", "0"), ("tp_conv64_kernel", "4")} <= seen, seen
