"""Three relations with three noise models in one engine, on both iteration paths: a Gaussian relation with a sampled alpha, a
censored one and a logit one, none of the last two the first relation.  The two paths must agree bit for bit, and both with the
chain recorded before the relations' device state got its one builder (tests/golden/mixed_relations_parent.npz)."""
import os
import textwrap

import numpy as np
import pytest

from both_paths import child

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "mixed_relations_parent.npz")

# argv: the .npz to write, the repository root to import from
CHILD = textwrap.dedent('''
    import sys
    import numpy as np
    sys.path.insert(0, sys.argv[2])
    import bdf_amd as B
    rng = np.random.default_rng(4)
    Na, Nb, Nc, D = 40, 30, 24, 8
    U = [rng.standard_normal((n, 3)) for n in (Na, Nb, Nc)]

    def cells(n1, n2, n):
        """n distinct cells, shared out evenly over the rows of the first mode, in a shuffled order"""
        ij = [(i + 1, j + 1) for i in range(n1) for j in rng.choice(n2, n // n1 + (i < n % n1), replace=False)]
        return np.asarray(ij)[rng.permutation(n)]

    a, b, c = B.Entity("a"), B.Entity("b"), B.Entity("c")
    ids = cells(Na, Nb, 500)
    y = np.sum(U[0][ids[:, 0] - 1] * U[1][ids[:, 1] - 1], axis=1) + 0.3 * rng.standard_normal(500) + 2.0
    ab = B.Relation({"a": ids[:, 0], "b": ids[:, 1], "y": y}, "ab", [a, b], dims=[Na, Nb])
    ab.model.alpha_sample = True
    B.assignToTest(ab, np.arange(1, 61))
    ids = cells(Na, Nc, 400)
    y = np.sum(U[0][ids[:, 0] - 1] * U[2][ids[:, 1] - 1], axis=1) + 0.5 * rng.standard_normal(400)
    flags = np.where(y > 1.0, 1, np.where(y < -1.0, -1, 0))
    ac = B.Relation({"a": ids[:, 0], "c": ids[:, 1], "y": np.clip(y, -1.0, 1.0)}, "ac", [a, c], dims=[Na, Nc])
    B.setPrecision(ac, 2.0)
    B.setCensored(ac, flags)
    ids = cells(Nb, Nc, 300)
    psi = np.sum(U[1][ids[:, 0] - 1] * U[2][ids[:, 1] - 1], axis=1)
    bc = B.Relation({"b": ids[:, 0], "c": ids[:, 1], "y": (rng.random(300) < 1.0 / (1.0 + np.exp(-psi))).astype(float)}, "bc", [b, c], dims=[Nb, Nc])
    B.setLogit(bc, offset=0.25)
    rd = B.RelationData()
    for r in (ab, ac, bc):
        B.addRelation(rd, r)
    deg = [np.zeros(en.count, dtype=np.int64) for en in rd.entities]
    for r in rd.relations:
        for k, en in enumerate(r.entities):
            j = [e is en for e in rd.entities].index(True)
            deg[j] += np.bincount(np.asarray(r.data.ids[:, k], dtype=np.int64) - 1, minlength=en.count)
    d = {"min_degree": np.array(min(int(x.min()) for x in deg)), "flag_kinds": np.unique(flags)}
    res = B.macau(rd, num_latent=D, burnin=2, psamples=2, verbose=False, seed=77)
    eng = rd._engine
    d["native"], d["pred"], d["alpha"] = np.array(int(eng.native)), res["predictions"]["pred"].to_numpy(), np.array(ab.model.alpha)
    d["ac_linear"] = eng.rel[1].linear.cpu().numpy()
    d["bc_omega"], d["bc_linear"] = eng.rel[2].omega.cpu().numpy(), eng.rel[2].linear.cpu().numpy()
    d["k1"] = np.array([eng.rows_dispatch(j)["k1"] for j in range(3)])
    for k, en in enumerate(rd.entities):
        d["S%d" % k], d["mu%d" % k], d["Lam%d" % k] = en.model.sample.T, en.model.mu, en.model.Lambda
    eng.close()
    np.savez(sys.argv[1], **d)
''')

ARRAYS = ["pred", "alpha", "ac_linear", "bc_omega", "bc_linear"] + [f"{n}{k}" for k in range(3) for n in ("S", "mu", "Lam")]


@pytest.fixture(scope="module")
def chains():
    """2 + 2 iterations of macau() on the three relations, on the native and on the step-by-step path: one child process per path"""
    return child(CHILD, ROOT, no_native=False), child(CHILD, ROOT, no_native=True)


def test_the_case_is_what_it_says(chains):
    nat = chains[0]
    assert nat["min_degree"] >= 15                          # no entity has an empty row, or a nearly empty one
    assert np.array_equal(nat["flag_kinds"], [-1, 0, 1])
    assert np.array_equal(nat["k1"], [40, 30, 24])          # entities of two relations: every row by the general row kernel
    assert nat["pred"].shape == (60,) and nat["S0"].shape == (40, 8) and nat["ac_linear"].shape == (400,) and nat["bc_omega"].shape == (300,)


def test_both_paths_agree_bit_for_bit(chains):
    nat, step = chains
    assert nat["native"] == 1 and step["native"] == 0
    assert sorted(nat) == sorted(step) and set(ARRAYS) <= set(nat)
    for k in ARRAYS:
        assert np.array_equal(nat[k], step[k]), k


def test_both_paths_agree_with_the_recorded_chain(chains):
    """the fixture: this module's CHILD run on the commit named in its key `parent_commit`, on an MI355X.  The expected difference
    is zero; the tolerance allows for another machine's math library"""
    gold = dict(np.load(GOLDEN))
    assert str(gold["parent_commit"])
    for ch in chains:
        for k in ARRAYS:
            np.testing.assert_allclose(ch[k], gold[k], rtol=1e-6, atol=1e-6, err_msg=k)


def test_the_models_buffers_were_written(chains):
    for ch in chains:
        assert np.ptp(ch["ac_linear"]) > 0.0 and np.ptp(ch["bc_omega"]) > 0.0
        assert np.all(np.isfinite(ch["bc_omega"])) and np.all(ch["bc_omega"] > 0.0)
