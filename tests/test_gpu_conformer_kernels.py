"""The conformer-embedding and torsion-matching kernels (csrc/conformer_embed.hip, csrc/torsion_match.hip) against the float64 references
and a-priori fp32 bounds of tests/conformer_kernel_helpers.py (its docstring derives every count), through `embed_conformers_batch(...,
iters=...)`, `match_score`, `match_torsions` and the C ABI.  tests/test_conformer_kernel_refs.py checks the references themselves.

Embedding: iters = (0, 0, 0) returns the start and its stage-4 objective; (0, 0, 1), (1, 0, 0) and (0, 1, 0) one FIRE step of the 3-D, the
weak and the strong 4-D stage from that start, so the difference of the returned coordinates is the clamped dt^2 F.  Only xyz is returned:
the w4 term's own gradient component is not covered (in the 4-D stages it is seen only through the clamp's norm).  Every test re-asserts
the branch margins on the coordinates the kernel returned before it compares; no element is left out.

Every test prints its largest error / bound ratio; DESIGN.md section 9 records the values measured on an MI355X."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import conformer_kernel_helpers as H

pytestmark = pytest.mark.gpu
SETTINGS = {"start": (0, 0, 0), **{k: v[0] for k, v in H.STAGES.items()}}


def _embed(cases, iters):
    from confidence_bootstrapping_amd.datasets import conformer_embedding as ce
    res = ce.embed_conformers_batch([c["bounds"] for c in cases], 1, seed=H.EMBED_SEED, conf_ids=[[c["conf_id"]] for c in cases],
                                    mol_ids=[c["mol_id"] for c in cases], iters=iters)
    return [(pos[0], float(err[0])) for pos, _, err in res]


@pytest.fixture(scope="module")
def embedded():
    """every case in one launch per setting of iters: name -> list of (pos [N, 3] float64 of the fp32 output, err); and the inferred starts"""
    cases = H.embed_cases()
    runs = {name: _embed(cases, iters) for name, iters in SETTINGS.items()}
    units = [H.embed_units(H.EMBED_SEED, c["mol_id"], c["conf_id"], c["N"]) for c in cases]
    return {"cases": cases, "runs": runs, "units": units}


def _start_of(embedded, k):
    c = embedded["cases"][k]
    x4 = H.infer_start(embedded["runs"]["start"][k][0], embedded["units"][k], c["N"])
    assert x4 is not None, f"{c['id']}: no box of 3 (cbrt(N) +- {H.CBRT_ULPS} ulp) reproduces the returned start"
    return x4


def test_start_is_the_restated_hash(embedded):
    worst = 0.0
    for k, c in enumerate(embedded["cases"]):
        pos = embedded["runs"]["start"][k][0]
        ulps = H.start_ulps(pos, embedded["units"][k], c["N"])
        worst = max(worst, ulps)
        assert ulps <= H.START_ULPS, (c["id"], ulps)
        _start_of(embedded, k)                                    # and one fp32 box gives every coordinate bitwise
    print(f"start: largest distance from the exact restatement {worst:.2f} ulp (allowed {H.START_ULPS})")


def test_objective_matches_float64_at_the_returned_start(embedded):
    worst, each = {}, []
    for k, c in enumerate(embedded["cases"]):
        x3 = _start_of(embedded, k)
        x3[:, 3] = 0.0
        ev = H.embed_eval(x3, c["lower"], c["upper"], c["cons"], 0.0, 1.0, 1.0)
        assert ev["margin"] >= H.MARGIN, (c["id"], ev["margin"])
        r = H.ratio(abs(embedded["runs"]["start"][k][1] - ev["E"]), ev["bE"])
        worst[c["S"]] = max(worst.get(c["S"], 0.0), r)
        each.append(f"{c['id']} {r:.3f}")
        assert r <= 1.0, (c["id"], embedded["runs"]["start"][k][1], ev["E"], ev["bE"])
    print("objective: |err_out - E64| / bound per case: " + ", ".join(each))
    print("objective: largest |err_out - E64| / bound per S: " + ", ".join(f"S={s}: {v:.3f}" for s, v in sorted(worst.items())))


@pytest.mark.parametrize("stage", list(H.STAGES))
def test_one_fire_step_is_the_clamped_float64_force(embedded, stage):
    four = H.STAGES[stage][4]
    worst = {"clamped": 0.0, "unclamped": 0.0}
    seen = {"clamped": 0, "unclamped": 0, "still": 0}
    each = []
    for k, c in enumerate(embedded["cases"]):
        x = _start_of(embedded, k)
        if not four:
            x[:, 3] = 0.0
        st = H.embed_step(x, c["lower"], c["upper"], c["cons"], stage)
        assert st["margin"] >= H.MARGIN and st["ftol_ratio"] >= 2, (c["id"], st["margin"], st["fm"])
        assert not st["moves"] or (st["clamp_margin"] >= H.CLAMP_MARGIN and st["clamp_bound_ok"]), (c["id"], st["clamp_margin"])
        before, after = embedded["runs"]["start"][k][0], embedded["runs"][stage][k][0]
        still = ~np.any(st["bound"], axis=1)
        assert np.array_equal(after[still], before[still]), c["id"]               # zero force, zero bound: bitwise where it was
        err = np.abs((after - before) - st["delta"])
        for name, sel in (("clamped", st["clamped"]), ("unclamped", ~st["clamped"] & ~still)):
            worst[name] = max(worst[name], H.ratio(err[sel], st["bound"][sel]))
            seen[name] += int(sel.sum())
        seen["still"] += int(still.sum())
        each.append(f"{c['id']} {H.ratio(err, st['bound']):.3f}")
        assert H.ratio(err, st["bound"]) <= 1.0, (c["id"], H.ratio(err, st["bound"]))
        if c["flavour"] in ("satisfied", "below_ftol") and not (four and c["flavour"] == "below_ftol"):
            assert np.array_equal(after, before), c["id"]
    assert min(seen.values()) > 0, seen
    print(f"{stage}: largest |step - clamp(dt^2 F64)| / bound per case: " + ", ".join(each))
    print(f"{stage}: largest |step - clamp(dt^2 F64)| / bound: clamped {worst['clamped']:.3f} ({seen['clamped']} atoms), "
          f"unclamped {worst['unclamped']:.3f} ({seen['unclamped']} atoms); {seen['still']} atoms must not move")


@pytest.mark.parametrize("setting", list(SETTINGS))
def test_a_molecule_alone_is_bitwise_what_it_is_in_the_batch(embedded, setting):
    for k, c in enumerate(embedded["cases"]):
        pos, err = _embed([c], SETTINGS[setting])[0]
        assert np.array_equal(pos, embedded["runs"][setting][k][0]) and err == embedded["runs"][setting][k][1], c["id"]


# ---------------------------------------------------------------------------------------------------------------------- matching
@pytest.fixture(scope="module")
def scored():
    """every case, plain and relabelled, in ONE launch (max_nl = 256, max_r = 32: most problems have nl < max_nl and r < max_r)"""
    from confidence_bootstrapping_amd.datasets import conformer_matching as cm
    cases = H.match_cases()
    problems = [c[which] for c in cases for which in ("plain", "permuted")]
    thetas = [c["theta"] for c in cases for _ in range(2)]
    assert any(len(p[0]) < 256 and len(p[2]) < 32 for p in problems)
    return {"cases": cases, "problems": problems, "thetas": thetas, "got": cm.match_score(problems, thetas)}


def test_score_at_slot_and_angle_edges(scored):
    from confidence_bootstrapping_amd.datasets import conformer_matching as cm
    for i, c in enumerate(scored["cases"]):
        r2, b = H.match_expected(i)
        worst = {}
        for j, which in enumerate(("plain", "permuted")):
            got = scored["got"][2 * i + j].astype(np.float64)
            assert np.isfinite(got).all() and got.shape == (H.N_THETA,)
            worst[which] = H.ratio(np.abs(got * got - r2), b)
            assert worst[which] <= 1.0, (c["id"], which, got, np.sqrt(np.maximum(r2, 0)))
            # theta = phi + 2 pi m: the untouched probe's aligned RMSD, up to the fp32 rounding of the angle itself
            pos, target, quads, mask = c[which]
            aligned = cm.rigid_align(pos.astype(np.float64), target.astype(np.float64))[1]
            for row in range(4):
                th = c["theta"][row]
                _, b0, _ = H.match_ref(pos, target, th, quads, mask, extra_angle=2 * H.U * float(np.abs(th).max()))
                assert abs(got[row] ** 2 - aligned ** 2) <= b0, (c["id"], which, row)
        print(f"{c['id']}: r^2 in [{r2.min():.3e}, {r2.max():.3e}] A^2; largest |gpu^2 - ref| / bound: plain {worst['plain']:.4f}, "
              f"relabelled {worst['permuted']:.4f}; bound as an RMSD " + (f"{np.sqrt(b[9]):.2e} A where the target is reached" if c["exact"] else f"{(b / (2 * np.sqrt(r2))).max():.2e} A"))


def test_each_problem_alone_is_bitwise_what_it_is_in_the_mixed_launch(scored):
    from confidence_bootstrapping_amd.datasets import conformer_matching as cm
    for k, (prob, th) in enumerate(zip(scored["problems"], scored["thetas"])):
        assert np.array_equal(cm.match_score([prob], [th])[0], scored["got"][k]), k


def test_a_single_atom_is_refused():
    """Nl = 1 with R >= 1: a dihedral needs four atoms, every index check fails and the score is not a number"""
    from confidence_bootstrapping_amd import engine
    lib = engine.load_library()
    dev = torch.device("cuda")
    i32 = lambda a: torch.tensor(a, dtype=torch.int32, device=dev)
    nl, r = i32([1, 4]), i32([1, 1])
    pos = torch.tensor([[[0.0, 0, 0]] * 4, [[0.0, 0, 0], [1.5, 0, 0], [1.5, 1.5, 0], [1.5, 1.5, 1.5]]], device=dev)
    quads = i32([[[0, 0, 0, 0]], [[0, 1, 2, 3]]])
    mask = torch.tensor([[[0, 0, 0, 0]], [[0, 0, 1, 1]]], dtype=torch.uint8, device=dev)
    theta, out = torch.zeros(2, 1, 1, device=dev), torch.full((2, 1), 7.0, device=dev)
    p = lambda t: C.c_void_p(t.data_ptr())
    assert lib.cbd_match_score(2, 4, 1, 1, p(nl), p(r), p(pos), p(pos), p(quads), p(mask), p(theta), p(out), None) == 0
    torch.cuda.synchronize()
    assert torch.isnan(out[0, 0]) and torch.isfinite(out[1, 0])


# ---------------------------------------------------------------------------------------------------------------------- evolution
@pytest.mark.parametrize("k", range(len(H.DE_SHAPES)), ids=[f"P{max(ps * R, 5)}_R{R}" for ps, R, _ in H.DE_SHAPES])
def test_start_population_and_best_index(k):
    from confidence_bootstrapping_amd.datasets import conformer_matching as cm
    popsize, R, _ = H.DE_SHAPES[k]
    prob = H.de_problems()[k]
    theta, fit, gens = cm.match_torsions([prob], seed=H.DE_SEED, popsize=popsize, maxiter=0, problem_ids=[3])[0]
    assert gens == 0 and theta.shape == (R,)
    pop = H.de_population(H.DE_SEED, 3, popsize, R)
    tol = H.DE_ULPS * float(np.spacing(H.PI32))
    dist = np.abs(pop.astype(np.float64) - theta.astype(np.float64)[None, :]).max(1)
    star = int(dist.argmin())
    assert dist[star] <= tol and (dist <= tol).sum() == 1, (dist[star], tol)
    scores = cm.match_score([prob], [np.concatenate([theta[None, :], pop])])[0].astype(np.float64)
    ref, b, r2 = H.match_ref(*prob[:2], theta, *prob[2:], extra_angle=tol)
    tol_r = b / ref                                                  # |got - ref| <= b / (got + ref) <= b / ref: the target is noisy, ref > 0.1 A
    assert ref > 0.1 and abs(fit - ref) <= tol_r and abs(fit - scores[0]) <= tol_r, (fit, ref, scores[0], tol_r)
    under = np.nonzero(scores[1:] < fit)[0]
    for i in under:                                                  # only a member that scores lower can undercut
        ref_i, b_i, _ = H.match_ref(*prob[:2], pop[i], *prob[2:], extra_angle=tol)
        assert fit - scores[1 + i] <= 2 * max(tol_r, b_i / ref_i), (i, fit, scores[1 + i])
    print(f"P = {len(pop)}, R = {R}: best member {star}, theta within {dist[star] / float(np.spacing(H.PI32)):.2f} ulp of pi of the restatement; "
          f"|fitness - ref64| / bound {abs(fit - ref) / tol_r:.4f}; {len(under)} members score lower on the device")


def test_generation_bookkeeping():
    from confidence_bootstrapping_amd.datasets import conformer_matching as cm
    probs = [H.de_problems()[k] for k in (0, 1, 3)]
    kw = dict(seed=H.DE_SEED, popsize=4)
    f0 = [f for _, f, _ in cm.match_torsions(probs, maxiter=0, **kw)]
    one = cm.match_torsions(probs, maxiter=1, tol=0.0, **kw)
    assert all(f1 <= f for (_, f1, _), f in zip(one, f0)) and all(g == 1 for _, _, g in one)
    for maxiter in (1, 7):                                           # std <= tol |mean| must hold: the first generation is the last
        assert all(g == 1 for _, _, g in cm.match_torsions(probs, maxiter=maxiter, tol=1e30, **kw))
    assert all(g == 3 for _, _, g in cm.match_torsions(probs, maxiter=3, tol=0.0, **kw))
