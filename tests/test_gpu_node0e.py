"""Node-major 0e path of the fp32 74 -> 74 layers (csrc/tp_node0e.hip) against the per-edge chain of tp_conv_kernel, layer by layer, on
the headline complex (C2 DockGen median).  The two differ only by the reassociation of fp32 sums.  Needs an MI355X:  pytest -m gpu"""
import numpy as np
import pytest
import torch

from tests.helpers import rel_err

pytestmark = pytest.mark.gpu
SCORE_TOL = 2e-5


def _layers(eng, pos, st):
    eng.debug(True)
    try:
        tr, rot, tor = eng.score(pos, st)
        out = {f"conv_{l}": eng.fetch(f"conv_{l}").reshape(-1, 80)[:, :74] for l in range(5)}
        out.update({f"conv_{l}_rec": eng.fetch(f"conv_{l}_rec").reshape(-1, 80)[:, :74] for l in range(4)})
        out.update(tr=tr.cpu().numpy(), rot=rot.cpu().numpy(), tor=tor.cpu().numpy())
        return out
    finally:
        eng.debug(False)


def test_node0e_matches_per_edge_chain_layer_by_layer(score_model):
    from confidence_bootstrapping_amd.engine import DockEngine, make_steps
    from confidence_bootstrapping_amd.synthetic import make_workload
    dev = torch.device("cuda:0")
    model, args = score_model
    cplx = make_workload("c2_dockgen_median")
    eng = DockEngine(dev, max_batch=8)
    eng.load_state_dict(model.state_dict())
    eng.set_complex(cplx)
    gen = torch.Generator().manual_seed(5)
    B = 6
    pos = (cplx["ligand"].pos[None].repeat(B, 1, 1) - cplx["ligand"].pos.mean(0) + torch.randn(B, 1, 3, generator=gen) * 4).to(dev)
    for t in (0.8, 0.2):
        st = make_steps(np.array([t]), args, model.timestep_emb_func)[0]
        eng.set_option("node0e", 0)
        old = _layers(eng, pos, st)
        eng.set_option("node0e", 1)
        new = _layers(eng, pos, st)
        again = _layers(eng, pos, st)
        for k in old:
            assert rel_err(torch.from_numpy(new[k]), torch.from_numpy(old[k])) < SCORE_TOL, (t, k)
            assert np.array_equal(new[k], again[k]), (t, k)   # repeat = repeat, bitwise
        # the option really switched paths: the reassociated sums differ in the last bits somewhere
        assert any(not np.array_equal(new[k], old[k]) for k in old if k.startswith("conv_")), t
