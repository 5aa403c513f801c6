"""noise_kind and check_model (relation_data.py) on the host (no GPU): one small relation per noise model."""
import numpy as np
import pytest


def _relation(B, kind):
    rng = np.random.default_rng(3)
    n = 40
    ids = np.stack([rng.integers(1, 9, n), rng.integers(1, 7, n)], axis=1)
    y = rng.standard_normal(n)
    if kind in ("probit", "logit"):
        y = (y > 0).astype(np.float64)
    elif kind == "counts":
        y = rng.poisson(3.0, n).astype(np.float64)
    elif kind == "ordinal":
        y = rng.integers(1, 6, n).astype(np.float64)
    rel = B.Relation({"u": ids[:, 0], "v": ids[:, 1], "y": y}, "ratings", [B.Entity("u"), B.Entity("v")], alpha=2.0, dims=[8, 6])
    {"gauss": lambda: None,
     "probit": lambda: B.setProbit(rel),
     "censored": lambda: B.setCensored(rel, rng.integers(-1, 2, n)),
     "interval": lambda: B.setInterval(rel, y - 0.5, y + 0.5),
     "ordinal": lambda: B.setOrdinal(rel, n_levels=5),
     "weights": lambda: B.setWeights(rel, rng.uniform(0.5, 2.0, n)),
     "robust": lambda: B.setRobust(rel, nu=4.0),
     "logit": lambda: B.setLogit(rel, offset=0.25),
     "counts": lambda: B.setCounts(rel, 3)}[kind]()
    return rel


# the sentences GibbsEngine.__init__ held, one block per model, before check_model (the ordinal block had none of its own: an
# ordinal relation is refused through its interval bounds; a Gaussian relation is not refused)
ONE_RANK = {
    "gauss": None,
    "probit": "Relation ratings has the probit noise model: one rank only",
    "censored": "Relation ratings has censoring flags: one rank only",
    "interval": "Relation ratings has interval bounds: one rank only",
    "ordinal": "Relation ratings has interval bounds: one rank only",
    "weights": "Relation ratings has observation weights: one rank only",
    "robust": "Relation ratings has the robust noise model: one rank only",
    "logit": "Relation ratings has the logit noise model: one rank only",
    "counts": "Relation ratings has the counts noise model: one rank only",
}


@pytest.mark.parametrize("kind", list(ONE_RANK))
def test_noise_kind_and_the_one_rank_refusal(B, kind):
    from bdf_amd.relation_data import check_model, noise_kind
    rel = _relation(B, kind)
    assert noise_kind(rel) == kind
    assert check_model(rel) is None and check_model(rel, world=1) is None
    assert noise_kind(rel) == kind                      # (the checks rebuild some fields; the kind stays)
    if ONE_RANK[kind] is None:
        assert check_model(rel, world=2) is None
    else:
        with pytest.raises(B.ArgumentError) as e:
            check_model(rel, world=2)
        assert str(e.value) == ONE_RANK[kind]


def _raised(B, check, rel):
    with pytest.raises(B.ArgumentError) as e:
        check(rel)
    return str(e.value)


def test_check_model_raises_what_the_models_own_check_raises(B):
    """relations changed by hand after their setter"""
    from bdf_amd.relation_data import check_censored, check_interval, check_model, check_pg, check_probit, check_robust
    rel = _relation(B, "probit")
    rel.data.values[3] = 2.0
    assert _raised(B, check_model, rel) == _raised(B, check_probit, rel) == "Relation ratings must hold only the values 0 and 1 for the probit noise model."
    rel = _relation(B, "censored")
    rel.model.censor = rel.model.censor[:-1]
    assert _raised(B, check_model, rel) == _raised(B, check_censored, rel)
    assert "40 training rows but (39,) censoring flags" in _raised(B, check_model, rel)
    rel = _relation(B, "interval")
    rel.model.interval = rel.model.interval[:, 0]
    assert _raised(B, check_model, rel) == _raised(B, check_interval, rel)
    rel = _relation(B, "robust")
    rel.model.robust = {"nu": 0.5}
    assert _raised(B, check_model, rel) == _raised(B, check_robust, rel)
    rel = _relation(B, "logit")
    rel.model.alpha = 3.0
    assert _raised(B, check_model, rel) == _raised(B, check_pg, rel)
    # the check comes before the refusal of several ranks, as in the engine's constructor
    rel = _relation(B, "probit")
    rel.data.values[3] = 2.0
    with pytest.raises(B.ArgumentError, match="must hold only the values 0 and 1"):
        check_model(rel, world=2)


def test_check_model_checks_an_ordinal_relation_before_its_bounds(B):
    """check_ordinal rebuilds the bounds from the levels, then check_interval reads them: bounds spoilt by hand are put right, levels
    spoilt by hand are refused by the ordinal check"""
    from bdf_amd.relation_data import check_model, check_ordinal
    rel = _relation(B, "ordinal")
    keep = rel.model.interval.copy()
    rel.model.interval = keep[:-1]
    assert check_model(rel) is None and np.array_equal(rel.model.interval, keep)
    rel.data.values[0] = 9.0
    assert _raised(B, check_model, rel) == _raised(B, check_ordinal, rel)
