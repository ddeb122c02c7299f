"""CPU checks of the references, bounds and case tables in tests/conformer_kernel_helpers.py, which tests/test_gpu_conformer_kernels.py holds
the conformer-embedding and torsion-matching kernels to.  Nothing here runs a kernel:

  * the restated start is self-consistent (exact units, the box candidates, the inference of the box from returned coordinates);
  * the case table reaches every S of {256, 128, 64, 51, 4, 3, 2, 1}, every nc of {0, 1, S-1, S, S+1, 257, 1024}, both distance branches,
    every outcome of every constraint kind, clamped and unclamped atoms in every stage, and every margin of every case holds for the
    committed conformer ids (a case whose margins fail is an error);
  * the analytic float64 gradient agrees with central differences of the float64 objective;
  * the two float64 statements of the matching objective agree, on the plain and on the relabelled molecules, and the relabelled cases
    put the axis atoms into every pair of lane slots;
  * keyed_perm is a bijection and the restated start population is a Latin hypercube;
  * each deliberate mistake moves the expected output of a committed case by more than ten times that case's bound."""
import numpy as np
import pytest

from tests import conformer_kernel_helpers as H


def _start(c):
    return H.restated_start(H.EMBED_SEED, c["mol_id"], c["conf_id"], c["N"])


def _flat(x4):
    x3 = x4.copy()
    x3[:, 3] = 0.0
    return x3


def test_restated_start_is_self_consistent():
    for n in H.EMBED_NS:
        units = H.embed_units(H.EMBED_SEED, 3, 7, n)
        assert units.shape == (n, 4) and (units >= -0.5).all() and (units < 0.5).all()
        assert np.array_equal(units * 2.0 ** 24, np.round(units * 2.0 ** 24)) and np.array_equal(units.astype(np.float32).astype(np.float64), units)
        cands = H.box_candidates(n)
        assert float(np.float32(3.0) * np.float32(float(n) ** (1 / 3))) in cands and 1 <= len(cands) <= 2 * H.CBRT_ULPS + 1
        x = H.restated_start(H.EMBED_SEED, 3, 7, n)
        assert H.start_ulps(x[:, :3].astype(np.float32), units, n) <= H.START_ULPS
        assert np.array_equal(H.infer_start(x[:, :3].astype(np.float32), units, n), x)
        moved = x[:, :3].astype(np.float32)
        moved[0, 0] = np.nextafter(moved[0, 0], np.float32(np.inf)) * np.float32(1.001)
        assert H.infer_start(moved, units, n) is None
    assert 12.0 in H.box_candidates(64) and 3.0 in H.box_candidates(1)
    # different ids, different draws
    assert not np.array_equal(H.embed_units(1, 0, 0, 4), H.embed_units(1, 0, 1, 4)) and not np.array_equal(H.embed_units(1, 0, 0, 4), H.embed_units(1, 1, 0, 4))


def test_case_table_reaches_every_path_and_every_margin_holds():
    cases = H.embed_cases()
    assert {c["N"] for c in cases} == set(H.EMBED_NS) and {c["S"] for c in cases} == {256, 128, 64, 51, 4, 3, 2, 1}
    assert any(256 % c["N"] for c in cases)                                         # idle threads
    for n in H.EMBED_NS:
        if n >= 4:
            S = 256 // n
            assert {0, 1, S - 1, S, S + 1, 257, 1024} - {-1} == {c["nc"] for c in cases if c["N"] == n and c["flavour"] == "random"}
    total = {}
    for c in cases:
        x4 = _start(c)
        ok, why = H.embed_checks(c, x4)
        assert ok, (c["id"], why)
        for stage, (_, _, _, _, four) in H.STAGES.items():
            st = H.embed_step(x4 if four else _flat(x4), c["lower"], c["upper"], c["cons"], stage)
            for k, v in st["counts"].items():
                total[stage, k] = total.get((stage, k), 0) + v
            total[stage, "clamped"] = total.get((stage, "clamped"), 0) + int(st["clamped"].sum())
            total[stage, "unclamped"] = total.get((stage, "unclamped"), 0) + int((st["moves"] & ~st["clamped"] & (np.abs(st["delta"]).sum(1) > 0)).sum())
            if c["flavour"] == "satisfied":
                assert not np.any(st["delta"]) and not np.any(st["bound"]), c["id"]
            if c["flavour"] == "below_ftol" and stage == "3d":
                assert not st["moves"] and 0 < st["fm"] < H.FTOL / 2
    for stage in H.STAGES:
        for k in ("upper", "lower", "inside", "volume_under", "volume_over", "volume_inside", "abs_under", "abs_over", "abs_inside", "abs_negative",
                  "planar", "clamped", "unclamped"):
            assert total[stage, k] > 0, (stage, k)
    print({f"{s}:{k}": v for (s, k), v in sorted(total.items()) if k in ("clamped", "unclamped")})
    # every atom role of every kind: a constraint's four atoms are its four roles, and every atom's step is compared
    for kind in (H.KIND_VOLUME, H.KIND_ABS, H.KIND_PLANAR):
        assert any((c["cons"]["kind"] == kind).any() for c in cases)


@pytest.mark.parametrize("stage", list(H.STAGES))
def test_analytic_gradient_matches_central_differences(stage):
    _, w4, wv, wp, four = H.STAGES[stage]
    worst = 0.0
    for c in H.embed_cases():
        if c["N"] > 5 and c["id"] not in ("n64_c5", "n85_c4"):
            continue
        x = _start(c) if four else _flat(_start(c))
        ev = H.embed_eval(x, c["lower"], c["upper"], c["cons"], w4, wv, wp)
        fd = np.zeros_like(x)
        for i in range(c["N"]):
            for k in range(4 if four else 3):
                h = 1e-5
                xp, xm = x.copy(), x.copy()
                xp[i, k] += h
                xm[i, k] -= h
                fd[i, k] = (H.embed_eval(xp, c["lower"], c["upper"], c["cons"], w4, wv, wp)["E"]
                            - H.embed_eval(xm, c["lower"], c["upper"], c["cons"], w4, wv, wp)["E"]) / (2 * h)
        g = ev["grad"] if four else ev["grad"] * [1, 1, 1, 0]
        scale = max(1.0, float(np.abs(g).max()))
        worst = max(worst, float(np.abs(fd - g).max()) / scale)
        assert np.abs(fd - g).max() <= 1e-6 * scale, (c["id"], stage)
        assert (ev["bG"] >= 0).all() and ev["bE"] >= 0
    print(f"{stage}: largest |central difference - analytic| / max(1, |gradient|_max) = {worst:.2e}")


def test_the_two_matching_references_agree():
    from confidence_bootstrapping_amd.datasets import conformer_matching as cm
    seen, sides = set(), set()
    for i, c in enumerate(H.match_cases()):
        r2, b = H.match_expected(i)
        pos, target, quads, mask = (np.asarray(a, dtype=np.float64) if a.dtype == np.float32 else a for a in c["plain"])
        other = np.array([cm.score_conformation(pos, target, t.astype(np.float64), quads, mask) for t in c["theta"]])
        perm = np.array([H.match_ref(*c["permuted"][:2], t, *c["permuted"][2:], want_bound=False)[2] for t in c["theta"]])
        # 1e-9 A^2: float64 cancellation of sums of some 1e5 A^2
        assert np.abs(other ** 2 - r2).max() < 1e-9 and np.abs(perm - r2).max() < 1e-9, c["id"]
        aligned = cm.rigid_align(pos, target)[1]
        assert np.abs(r2[:4] - aligned ** 2).max() < 1e-4 * max(aligned, 1e-3), c["id"]          # theta = phi (+ 2 pi m), rounded to fp32
        assert (b > 0).all() and np.isfinite(b).all()
        if c["exact"]:
            assert r2[9] < 1e-9, c["id"]                                                   # the target is reached (up to its fp32 rounding)
        else:
            assert r2.min() > 0.01, c["id"]
        if c["nl"] == 256 and c["R"] == 32:
            assert {(su, sv) for su, sv, _ in H.slot_pairs(c, "permuted")} == {(a, b_) for a in range(4) for b_ in range(4)}
        seen |= {(su, sv) for su, sv, _ in H.slot_pairs(c, "permuted")} | {(su, sv) for su, sv, _ in H.slot_pairs(c, "plain")}
        sides |= {turn for _, _, turn in H.slot_pairs(c, "plain")}
    assert len(seen) == 16 and sides == {True, False}
    assert {c["nl"] for c in H.match_cases()} == {4, 63, 64, 65, 128, 129, 192, 193, 256} and {c["R"] for c in H.match_cases()} == {1, 2, 31, 32}


def test_keyed_perm_is_a_bijection_and_the_start_a_latin_hypercube():
    for P in (5, 15, 17, 64, 65, 480, 512):
        bits = H.de_bits(P)
        assert (1 << bits) >= P > (1 << (bits - 1)) or P <= 2
        for seed, dim in ((0, 0), (H.DE_SEED, 1), (12345, 31)):
            key = H.de_key(seed, 3)
            assert sorted(H.keyed_perm(i, P, bits, key, dim) for i in range(P)) == list(range(P)), (P, seed, dim)
    assert sorted(max(ps * R, 5) for ps, R, _ in H.DE_SHAPES) == [5, 15, 17, 64, 65, 480, 512] and {R for _, R, _ in H.DE_SHAPES} == {1, 3, 32}
    for (ps, R, nl), (pos, target, quads, mask) in zip(H.DE_SHAPES, H.de_problems()):
        assert pos.shape == target.shape == (nl, 3) and quads.shape == (R, 4) and mask.shape == (R, nl)
        assert H.match_ref(pos, target, np.zeros(R), quads, mask)[0] > 0.1                       # a noisy target: the optimum is not zero
    for ps, R, _ in H.DE_SHAPES[:5]:
        pop = H.de_population(H.DE_SEED, 3, ps, R)
        P = len(pop)
        assert pop.dtype == np.float32 and (pop >= -H.PI32).all() and (pop < H.PI32).all()
        strata = np.floor((pop.astype(np.float64) + np.pi) / (2 * np.pi) * P + 1e-4).astype(int).clip(0, P - 1)
        assert all(sorted(strata[:, j].tolist()) == list(range(P)) for j in range(R)), (ps, R)


@pytest.mark.parametrize("mut", H.EMBED_MUTATIONS)
def test_embedding_mistakes_move_an_expected_output(mut):
    for c in H.embed_cases():
        if c["N"] > 64:
            continue
        x4 = _start(c)
        ev, bad = (H.embed_eval(_flat(x4), c["lower"], c["upper"], c["cons"], 0.0, 1.0, 1.0, mut=m) for m in (None, mut))
        moved = abs(bad["E"] - ev["E"]) / max(ev["bE"], 1e-300) if bad["E"] != ev["E"] else 0.0
        for stage, (_, _, _, _, four) in H.STAGES.items():
            st, sb = (H.embed_step(x4 if four else _flat(x4), c["lower"], c["upper"], c["cons"], stage, mut=m) for m in (None, mut))
            moved = max(moved, H.ratio(np.abs(sb["delta"] - st["delta"]), st["bound"]))
        if moved > 10:
            print(f"{mut}: moves {c['id']} by {moved:.3g} bounds")
            return
    raise AssertionError(f"{mut} moves no case by more than ten bounds")


@pytest.mark.parametrize("mut", H.MATCH_MUTATIONS)
def test_matching_mistakes_move_an_expected_output(mut):
    for i, c in enumerate(H.match_cases()):
        r2, b = H.match_expected(i)
        bad = np.array([H.match_ref(*c["permuted"][:2], t, *c["permuted"][2:], mut=mut, want_bound=False)[2] for t in c["theta"]])
        moved = float(np.where(np.isfinite(bad), np.abs(bad - r2) / b, np.inf).max())
        if moved > 10:
            print(f"{mut}: moves {c['id']} by {moved:.3g} bounds")
            return
    raise AssertionError(f"{mut} moves no case by more than ten bounds")
