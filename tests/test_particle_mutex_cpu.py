"""Mutual exclusion for contested landmarks (slamgpu_set_particle_mutex), the parts that need no GPU: the numpy model of the contract
(tests/mutex_model.py) on the four constructed cases of tests/test_gpu_particle_mutex.py and on random inputs, and the entry points in
the library and the Python wrapper."""
import numpy as np
import pytest

from mutex_model import COUNTERS, DISCARD, NEW, mutex_model

GATE = 4.0
R = np.diag([0.01, (np.pi / 180) ** 2])


def gates(slots, obs):
    """float64 (nis, nd) of observations (range, bearing) against slots (range, bearing) opened from the origin by one observation each:
    the record is the observation's point, Pf = Gz R Gz^T, so S = Hf Pf Hf^T + R = 2 R seen from the origin"""
    S = 2.0 * R
    nis = np.zeros((len(obs), len(slots)))
    for q, (zr, zb) in enumerate(obs):
        for j, (r, b) in enumerate(slots):
            v = np.array([zr - r, (zb - b + np.pi) % (2 * np.pi) - np.pi])
            nis[q, j] = v @ np.linalg.solve(S, v)
    return nis, nis + np.log(np.linalg.det(S))


A, B = 0, 1
NEAR = [(10.0, 0.0), (10.0, 0.03)]
FAR = [(10.0, 0.0), (10.0, 0.3)]
# name: slots, observations, L0, wanted F, (contested, lost, rematched, overturned)
CASES = {
    "overturn and re-match": (NEAR, [(10.0, 0.012), (10.0, 0.002)], [A, A], [B, A], (1, 1, 1, 1)),
    "incumbent keeps, loser re-matched": (NEAR, [(10.0, 0.002), (10.0, 0.012)], [A, A], [A, B], (1, 1, 1, 0)),
    "no alternative": (NEAR, [(10.0, -0.03), (10.0, 0.002)], [A, A], [DISCARD, A], (1, 1, 0, 1)),
    "gated claim beats a rule claim": (FAR, [(10.5, 0.0), (10.0, 0.002)], [A, A], [DISCARD, A], (1, 1, 0, 1)),
}


@pytest.mark.parametrize("name", list(CASES))
def test_constructed_cases(name):
    slots, obs, L0, want, counts = CASES[name]
    nis, nd = gates(slots, obs)
    F, cnt = mutex_model(L0, nis, nd, [True, True], GATE)
    print(name, "nis", nis.round(3).tolist(), "nd", nd.round(3).tolist(), "F", F.tolist(), cnt)
    assert F.tolist() == want
    assert tuple(cnt[k] for k in COUNTERS) == (1,) + counts


def test_the_margins_the_issue_quotes():
    nis, nd = gates(NEAR, [(10.0, 0.012), (10.0, 0.002), (10.0, -0.03)])
    assert abs((nd[0, A] - nd[1, A]) - 0.230) < 1e-3 and abs(nis[0, B] - 0.53) < 5e-3
    assert abs(nis[2, A] - 1.48) < 5e-3 and abs(nis[2, B] - 5.91) < 5e-3 and nis[2, B] > GATE
    nis, nd = gates(FAR, [(10.5, 0.0), (10.0, 0.002)])
    assert abs(nis[0, A] - 12.5) < 1e-9 and nis[0, A] > GATE > nis[1, A]  # the class decides, not nd


def _random_case(rng):
    nz, nf = int(rng.integers(1, 9)), int(rng.integers(1, 7))
    nis = rng.uniform(0.0, 8.0, (nz, nf))
    nd = nis + rng.uniform(-8.0, -6.0, (1, nf))  # (ln det S is the slot's)
    if rng.random() < 0.3:  # exact ties and a NaN now and then
        nd = np.round(nd)
        nis[rng.integers(nz), rng.integers(nf)] = np.nan
    usable = rng.random(nf) < 0.8
    L0 = np.where(rng.random(nz) < 0.7, rng.integers(0, nf, nz), rng.choice([NEW, DISCARD], nz))
    return L0, nis, nd, usable


def test_random_inputs_keep_the_invariants():
    rng = np.random.default_rng(11)
    seen = dict.fromkeys(COUNTERS, 0)
    for _ in range(3000):
        L0, nis, nd, usable = _random_case(rng)
        F, cnt = mutex_model(L0, nis, nd, usable, GATE)
        slots = F[F >= 0]
        assert len(set(slots.tolist())) == len(slots), "a slot twice in F"
        contested = [l for l in set(L0[L0 >= 0].tolist()) if (L0 == l).sum() > 1]
        keepers = 0
        for l in contested:
            kept = [q for q in np.nonzero(L0 == l)[0] if F[q] == l]
            assert len(kept) == 1, "a contested slot is held by exactly one of its claimants"
            keepers += 1
        losers = np.array([L0[q] in contested and F[q] != L0[q] for q in range(len(L0))], bool)
        assert np.array_equal(F != L0, losers), "F differs from L0 only at losers"
        assert np.all(F[losers] != NEW) and np.all(F[(L0 == NEW) | (L0 == DISCARD)] == L0[(L0 == NEW) | (L0 == DISCARD)])
        for q in np.nonzero(losers)[0]:
            if F[q] >= 0:  # a re-match is a usable slot inside the gate that nobody named
                assert usable[F[q]] and nis[q, F[q]] < GATE and F[q] not in L0.tolist()
        assert cnt["contested"] == len(contested) and cnt["lost"] == int(losers.sum()) == sum(int((L0 == l).sum()) - 1 for l in contested)
        assert cnt["rematched"] == int((F[losers] >= 0).sum()) and cnt["overturned"] <= cnt["contested"] <= cnt["lost"]
        assert cnt["overturned"] == sum(1 for l in contested if F[np.nonzero(L0 == l)[0][0]] != l)
        for k in COUNTERS:
            seen[k] += cnt[k]
    assert all(v > 100 for v in seen.values()), seen


def test_order_matters_only_among_losers():
    """the contest does not depend on the order of the observations: with the two observations swapped the same observation keeps A"""
    slots, obs, L0, _, _ = CASES["overturn and re-match"]
    nis, nd = gates(slots, obs)
    F, _ = mutex_model(L0, nis, nd, [True, True], GATE)
    Fs, _ = mutex_model(L0, nis[::-1], nd[::-1], [True, True], GATE)
    assert F.tolist() == Fs[::-1].tolist()


def test_entry_points_exist():
    import slam_amd
    lib = slam_amd.load_library()
    for sym in ("slamgpu_set_particle_mutex", "slamgpu_particle_mutex_stats"):
        assert sym in slam_amd.DECLARED_SYMBOLS and hasattr(lib, sym), sym
    assert callable(getattr(slam_amd.SlamGpu, "set_particle_mutex", None)) and callable(getattr(slam_amd.SlamGpu, "particle_mutex_stats", None))
