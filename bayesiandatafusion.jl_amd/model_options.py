"""Which model options go together: one registry of the options and one table of the pairs that are refused.

Host only.  Every setter of relation_data.py calls refuse(subject, its key) once, and the checks a sampler runs before it is built
(check_model, check_spike, check_nonneg, check_new_rows) call refuse(..., build=True) for every option that is present.  What is
about an option's own values -- 0/1 values, positive weights, k in 1..64 -- stays with its setter.
"""
from collections import namedtuple

from . import features as feat
from ._lib import ArgumentError

RELATION, ENTITY, RUN = "relation", "entity", "run"

# key
# scope     set on a relation, on an entity, or asked of one macau() run (never "present": it only comes)
# field     the attribute of RelationModel / Entity / Relation that holds it (None: it leaves none)
# present   present(x): whether relation or entity x has it
# phrase    what every message calls it
# trainer   why bpmf_vb and macau_hmc refuse it (None: they take it)
# one_rank  None: it runs on several ranks; True: it does not; a string: it does not, and what that refusal calls it
# has       how a message says that a relation has it, where "has <phrase>" would not do
Option = namedtuple("Option", "key scope field present phrase trainer one_rank has", defaults=(None, None, None))


def _never(x):
    return False


def _pg(model):
    return lambda r: r.model.pg is not None and r.model.pg["model"] == model


_GAUSS_ONLY, _MEASURED, _NW_ONLY = "has Gaussian noise only", "takes every value as a measurement", "has the Normal-Wishart prior only"

OPTIONS = (
    Option("dense", RELATION, "dense", lambda r: r.model.dense, "a dense matrix (setDense)", "reads the listed cells", "a dense matrix (setDense)",
           "is dense (setDense)"),
    # the noise models, in the order noise_kind() asks for them (an ordinal relation has interval bounds too)
    Option("probit", RELATION, "probit", lambda r: r.model.probit, "the probit noise model (setProbit)", _GAUSS_ONLY, "the probit noise model"),
    Option("censored", RELATION, "censor", lambda r: r.model.censor is not None, "censoring flags (setCensored)", _MEASURED, "censoring flags"),
    Option("ordinal", RELATION, "ordinal", lambda r: r.model.ordinal is not None, "the ordinal noise model (setOrdinal)", _MEASURED, "interval bounds"),
    Option("interval", RELATION, "interval", lambda r: r.model.interval is not None and r.model.ordinal is None,
           "interval bounds (setInterval / setBinned)", _MEASURED, "interval bounds"),
    Option("robust", RELATION, "robust", lambda r: r.model.robust is not None, "the robust noise model (setRobust)", _GAUSS_ONLY, "the robust noise model"),
    Option("weights", RELATION, "weights", lambda r: r.model.weights is not None, "observation weights (setWeights)", "weighs every value alike",
           "observation weights"),
    Option("entity_noise", RELATION, "entity_noise", lambda r: r.model.entity_noise is not None, "a noise precision per row (setEntityNoise)",
           "has one noise precision for every cell", "a noise precision per row"),
    Option("logit", RELATION, "pg", _pg("logit"), "the logit noise model (setLogit)", _GAUSS_ONLY, "the logit noise model"),
    Option("counts", RELATION, "pg", _pg("counts"), "the count noise model (setCounts)", _GAUSS_ONLY, "the counts noise model"),
    Option("background", RELATION, "background", lambda r: r.model.background is not None, "a background (setBackground)", "fits the listed cells only",
           "a background"),
    Option("recommend", RELATION, "recommend", lambda r: r.model.recommend is not None, "top-k lists (setRecommend)", "keeps no sum of scores over draws",
           True),
    Option("acquire", RELATION, "acquire", lambda r: r.model.acquire is not None, "acquisition lists (setAcquire)",
           "keeps no moments of scores over draws", True),
    Option("bias", RELATION, "bias", lambda r: bool(r.model.bias), "biases (setBias)", "models a cell as mean + u.v", True),
    Option("new_test", RELATION, "new_test", lambda r: r.model.new_test is not None, "cells of new rows (setNewTest)", None, True),
    Option("new_observed", RELATION, "new_observed", lambda r: r.model.new_observed is not None, "known cells of new rows (setNewObserved)", None, True),
    Option("waic", RELATION, "waic", lambda r: r.model.waic is not None, "WAIC on its training cells (setWaic)", None, True),
    Option("diagnostics", RELATION, "diagnostics", lambda r: r.model.diagnostics is not None, "convergence diagnostics (setDiagnostics)",
           "keeps no draws of the predictions", True),
    Option("features", RELATION, "F", lambda r: not feat.isempty(r.F), "features (relation-level side information)"),
    Option("alpha_sample", RELATION, "alpha_sample", lambda r: r.model.alpha_sample, "a sampled precision (alpha_sample)"),
    # read by macau(lpd=True) alone, which checks them then: no other option's setter or check looks at them
    Option("test_interval", RUN, "test_interval", _never, "test bounds (setTestInterval)"),
    Option("test_ordinal", RUN, "test_ordinal", _never, "test levels (setTestOrdinal)"),
    Option("precision", RUN, None, _never, "a precision of its own (setPrecision)"),
    Option("lpd", RUN, None, _never, "lpd = true", None, True),
    Option("rmse_train", RUN, None, _never, "rmse_train = true"),
    Option("full_prediction", RUN, None, _never, "full_prediction = true (the prediction of all elements)"),
    Option("entity_features", ENTITY, "F", lambda e: not feat.isempty(e.F), "features"),
    Option("spike", ENTITY, "spike", lambda e: e.spike is not None, "the spike-and-slab prior (setSpikeAndSlab)", _NW_ONLY, True),
    Option("nonneg", ENTITY, "nonneg", lambda e: e.nonneg is not None, "the non-negative prior (setNonNegative)", _NW_ONLY, True),
    Option("new_rows", ENTITY, "new_rows", lambda e: e.new_rows is not None, "new rows (setNewRows)"),
)
OPTION = {o.key: o for o in OPTIONS}

NOISE = ("probit", "censored", "ordinal", "interval", "robust", "weights", "entity_noise", "logit", "counts")
_PG = ("logit", "counts")
_LATENT = ("probit", "censored", "ordinal", "interval")        # a latent value per observation
_PRIORS = ("spike", "nonneg")
_GRAM = "a Gram matrix is folded into the prior precision"
_NO_CLOSED_FORM = "the marginal over a new row's factor has no closed form, which rules out {incoming}"
_OMEGA = "every cell's precision is its sampled omega"

# The table.  A row is (an option, the options it does not go with, the reason or None); the pair is refused in both orders.
# A message reads "Relation R has <what is there>: it does not take <what comes>[, <reason>]."; a reason that names {incoming}
# itself stands in place of "it does not take ...".  A reason is looked up in the order (there, comes) first, so a pair written in
# both orders is worded per order.  Options of which a relation takes one are a group: every pair inside it is refused.
_GROUPS = ((NOISE, "a relation has one noise model"),)
_ROWS = (
    ("interval", ("ordinal",), "an ordinal relation's bounds follow its edges"),
    ("features", NOISE + ("dense", "background", "recommend", "acquire", "new_test"), None),
    ("features", ("bias",), "both write the rows' base"),
    ("alpha_sample", ("probit",), "the probit latent has unit variance"),
    ("alpha_sample", _PG, _OMEGA),
    ("precision", ("probit",), "its latent has unit variance, there is no precision to set"),
    ("precision", _PG, _OMEGA + ", there is no precision to set"),
    ("bias", NOISE, "biases are sampled under plain Gaussian noise"),
    ("bias", ("background",), "the unlisted cells would need them too"),
    ("bias", ("dense",), "no cell is listed to the rows"),
    ("bias", ("recommend", "acquire"), "the score is u.v + mean alone"),
    ("bias", ("new_test",), "a new row has no bias"),
    ("bias", _PRIORS, None),
    ("background", _LATENT + _PG + ("robust", "entity_noise"), None),
    ("background", ("dense",), "a dense relation leaves no cell unlisted"),
    ("background", _PRIORS, _GRAM),
    ("dense", NOISE + ("recommend", "acquire", "new_test"), None),
    ("dense", _PRIORS, _GRAM),
    ("recommend", ("probit",) + _PG, "its prediction is not u.v + mean"),
    # acquisition lists: the moments of u.v + mean over the draws, the noise of one precision alpha per draw
    ("acquire", ("probit",) + _PG, "its prediction is not u.v + mean"),
    ("acquire", ("robust", "weights", "entity_noise"), "an unlisted cell's precision is not one alpha"),
    ("acquire", ("ordinal",), "a level is not on the latent's scale"),
    ("acquire", ("recommend",), "a relation keeps one ranked list"),
    ("waic", ("robust", "weights", "entity_noise", "background") + _PG, "a cell's density under it is not scored yet"),
    ("lpd", ("robust", "weights") + _PG, "a held-out cell's density under it is not scored yet"),
    ("rmse_train", ("censored",), "its training values are bounds, not measurements"),
    ("rmse_train", ("ordinal", "interval"), "its training values stand for intervals, not measurements"),
    ("full_prediction", ("probit",) + _PG, "its prediction is not u.v + mean"),
    ("new_test", ("robust",) + _PG, _NO_CLOSED_FORM),
    ("new_test", ("weights",), "the weight of a new cell is unknown, which rules out {incoming}"),
    ("new_test", ("entity_noise",), "the precision of a new row is unknown, which rules out {incoming}"),
    ("new_test", ("acquire",), "no list is ranked for a new row"),
    ("new_test", ("ordinal",), "a held-out level is not a measurement, which rules out {incoming}"),
    # the fold-in: a new row's known cells enter its conditional as u.v + mean under one precision alpha
    ("new_observed", NOISE, "a new row is conditioned on its known cells under plain Gaussian noise, which rules out {incoming}"),
    ("new_observed", ("background",), "a new row's unlisted cells are unknown, not background"),
    ("new_observed", ("dense",), "a new row's known cells are a list"),
    ("new_observed", ("bias",), "a new row has no bias"),
    ("new_observed", ("recommend",), "no list is ranked for a new row"),
    ("new_observed", ("features",), "a new cell has no relation features"),
    ("new_observed", _PRIORS, "a new row is conditioned under the Normal-Wishart prior, which rules out {incoming}"),
    ("test_interval", ("probit",), "its test values are scored as 0/1 values"),
    ("entity_features", _PRIORS, "{incoming} does not take side information"),
    ("spike", ("nonneg",), None),
    ("new_rows", _PRIORS, "{incoming} does not take them"),
    ("spike", ("new_rows",), "it takes no side information and no {incoming}"),
    ("nonneg", ("new_rows",), "it takes no side information and no {incoming}"),
)

REFUSED = {(a, b): why for group, why in _GROUPS for a in group for b in group if a != b}      # (A, B) as written -> the reason or None
REFUSED.update({(a, b): why for a, others, why in _ROWS for b in others})

# (present, incoming): pairs of the table that the incoming option's setter accepts and only the build-time pass refuses; the other
# order is refused at once.  Nobody chose these: they are how the guards happened to be written before the table, kept so that
# the table changed no behaviour.  Closing them (refusing at once in both orders) is a follow-up: DESIGN.md section 28.
_REFUSED_ONLY_AT_BUILD = frozenset(
    [("background", b) for b in _LATENT + _PG + ("robust", "waic")]
    + [("recommend", b) for b in ("probit",) + _PG]
    + [("new_test", b) for b in ("ordinal", "robust", "weights", "entity_noise") + _PG]
    + [("spike", "background")])


def refused(there, comes):
    """(whether the table refuses the two options together, the reason or None in the wording for this order)"""
    for pair in ((there, comes), (comes, there)):
        if pair in REFUSED:
            return True, REFUSED[pair]
    return False, None


# an option that ranks a list as another one does: where the table has no row for it, refuse() reads the other one's.  The fold-in's
# row (new_observed) names setRecommend alone, and what it says of a ranked list holds for an acquisition list as well
_AS_FOR = {"acquire": "recommend"}


def _refused_as(there, comes):
    """refused(there, comes), or what the table says of the options that these two stand where (_AS_FOR)"""
    no, why = refused(there, comes)
    a, b = _AS_FOR.get(there, there), _AS_FOR.get(comes, comes)
    if not no and a != b and (a, b) != (there, comes):
        no, why = refused(a, b)
    return no, why


def present(x, scope):
    """the options of that scope that relation or entity x has, in the registry's order"""
    return [o for o in OPTIONS if o.scope == scope and o.present(x)]


def _around(subject):
    """(option, its owner) of everything present on subject and on what it is tied to: a relation's entities, an entity's relations"""
    own, tied, theirs = (RELATION, subject.entities, ENTITY) if hasattr(subject, "entities") else (ENTITY, subject.relations, RELATION)
    return [(o, subject) for o in present(subject, own)] + [(o, t) for t in tied for o in present(t, theirs)]


def _kind(x):
    return "Relation" if hasattr(x, "entities") else "Entity"


def refuse(subject, incoming, build=False):
    """raises if relation or entity `subject`, one of its entities or one of its relations has an option that does not go with the
    option `incoming`.  build: the pass before a sampler is built, which also refuses the pairs of _REFUSED_ONLY_AT_BUILD"""
    phrase = OPTION[incoming].phrase
    for opt, owner in _around(subject):
        no, why = _refused_as(opt.key, incoming)
        if opt.key == incoming or not no or (not build and (opt.key, incoming) in _REFUSED_ONLY_AT_BUILD):
            continue
        if why is None or "{incoming}" not in why:
            who = "it" if owner is subject else f"its {_kind(subject).lower()} {subject.name}"
            why = f"{who} does not take {{incoming}}" + (f", {why}" if why else "")
        raise ArgumentError(f"{_kind(owner)} {owner.name} {opt.has or 'has ' + opt.phrase}: {why.format(incoming=phrase)}.")


def refuse_ranks(subject, key, world):
    opt = OPTION[key]
    if world > 1 and opt.one_rank:
        raise ArgumentError(f"{_kind(subject)} {subject.name} has {opt.phrase if opt.one_rank is True else opt.one_rank}: one rank only")


def noise_kind(r):
    """which noise model relation r has: the key of the one option of NOISE that is present, or "gauss".  The table admits one per
    relation."""
    return next((o.key for o in present(r, RELATION) if o.key in NOISE), "gauss")
