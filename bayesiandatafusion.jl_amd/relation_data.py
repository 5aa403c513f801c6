"""Entity / Relation / RelationData -- host mirror of src/RelationData.jl of the reference.

Only the data model lives here (what the user builds before calling macau); every numeric step of the Gibbs
sweep is done by libbdf_hip.so through engine.GibbsEngine.  Names follow the reference with the trailing `!`
dropped (assignToTest!, setTest!, setPrecision!, addRelation!, normalizeFeatures!, normalizeRows!).
Entity and mode numbers in accessors are 1-based as in the reference.
"""
import math

import numpy as np

from . import features as feat
from ._lib import ArgumentError
from .indexed_df import IndexedDF, _split_table
from .model_options import OPTION, RELATION, noise_kind, present, refuse, refuse_ranks  # noqa: F401  (noise_kind is imported from here)


class EntityModel:
    """EntityModel (RelationData.jl:14-40).  Arrays live on the device once macau() has initialised the model;
    the attributes below return host copies in the reference's orientation (sample is D x N)."""

    def __init__(self):
        self._dev = None          # engine.EntityState

    def _get(self, name):
        if self._dev is None:
            raise AttributeError("model not initialised: call macau() (reset!) first")
        return self._dev.host(name)

    sample = property(lambda self: self._get("sample"))
    mu = property(lambda self: self._get("mu"))
    Lambda = property(lambda self: self._get("Lambda"))
    beta = property(lambda self: self._get("beta"))
    uhat = property(lambda self: self._get("uhat"))
    mu0 = property(lambda self: self._get("mu0"))
    WI = property(lambda self: self._get("WI"))
    b0 = property(lambda self: self._dev.b0)
    nu0 = property(lambda self: self._dev.nu0)


class Entity:
    """Entity(name; F=zeros(0,0), lambda_beta=1.0) (RelationData.jl:42-63)"""

    def __init__(self, name, F=None, lambda_beta=1.0):
        self.F = F
        self.FF = None
        self.use_FF = False
        self.relations = []
        self.count = 0
        self.name = str(name)
        self.modes = []
        self.modes_other = []
        self.lambda_beta = float(lambda_beta)
        self.lambda_beta_sample = True
        self.mu = 1.0          # hyper-prior for lambda_beta
        self.nu = 1e-3
        self.spike = None      # setSpikeAndSlab: {"incl_a", "incl_b", "shape", "rate"}; None: the Normal-Wishart prior
        self.nonneg = None     # setNonNegative: {"shape", "rate"}; None: the Normal-Wishart prior
        self.new_rows = None   # setNewRows: the features (n* x numF) of instances that are not among the entity's rows
        self.model = None

    def __repr__(self):
        s = f"[Entity] {self.name}: {self.count:6d} "
        if hasFeatures(self):
            lam = "sample" if self.lambda_beta_sample else f"{self.lambda_beta:1.1f}"
            return s + f"with {feat.feature_shape(self.F)[1]} features (λ = {lam})"
        return s + "with no features"


def hasFeatures(x):
    return not feat.isempty(x.F)


def toStr(x):
    if isinstance(x, Entity):
        if x.model is None or x.model._dev is None:
            return x.name[:3] + "[]"
        st = x.model._dev            # device state: the norms are reduced there (bdf_norm2), not on a host copy
        s = f"U:{st.norm('sample'):6.2f}"
        if hasFeatures(x):
            s += f" β:{st.norm('beta'):3.2f}"
            if x.lambda_beta_sample:
                s += f" λ={x.lambda_beta:1.1f}"
        if x.spike is not None and st.spike_state is not None:
            s += f" on:{st.spike_active()}"
        if x.nonneg is not None:
            s += " nn"
        return f"{x.name[:3]}[{s}]"
    m = x.model
    if m.pg is not None:
        return f"{x.name[:4]}[{'logit' if m.pg['model'] == 'logit' else 'nb:%s' % m.pg['r']}]"
    s = "probit" if m.probit else f"α={m.alpha:2.1f}"
    if hasFeatures(x) and m.beta is not None and len(m.beta):
        s += f" β:{np.linalg.norm(m.beta):2.1f}"
    s += "".join(show(x) for key, show in _SHOWN.items() if OPTION[key].present(x))
    return f"{x.name[:4]}[{s}]"


def _open_rows(x):
    return f" intv:{int(np.count_nonzero(x.model.interval[:, 0] < x.model.interval[:, 1]))}"


# what toStr adds for an option that is present, in the order it is shown
_SHOWN = {
    "censored": lambda x: f" cens:{int(np.count_nonzero(x.model.censor))}",
    "interval": _open_rows,
    "ordinal": lambda x: _open_rows(x) + f" ord:{x.model.ordinal['K']}",
    "robust": lambda x: f" t:{x.model.robust['nu']:g}",
    "weights": lambda x: " wts",
    "entity_noise": lambda x: f" τ:{x.entities[x.model.entity_noise['mode'] - 1].name[:3]}",
    "bias": lambda x: " b:" + ",".join(x.entities[k - 1].name[:3] for k in sorted(x.model.bias)),
    "background": lambda x: f" bg:{x.model.background['weight']:g}",
    "recommend": lambda x: f" rec:{x.model.recommend['k']}",
    "acquire": lambda x: f" acq:{x.model.acquire['k']}",
    "dense": lambda x: " dense",
}


class RelationModel:
    """RelationModel (RelationData.jl:107-119)"""

    def __init__(self, alpha=1.0, lambda_beta=1.0):
        self.alpha_sample = False
        self.alpha_nu0 = 2.0
        self.alpha_lambda0 = 1.0
        self.lambda_beta = float(lambda_beta)
        self.alpha = float(alpha)
        self.beta = np.zeros(0)
        self.mean_value = 0.0
        self.probit = False       # setProbit: 0/1 values with the probit noise model instead of Gaussian noise of precision alpha
        self.censor = None        # setCensored: int8 per training row, 0 a measurement, +1 "at least the value", -1 "at most the value"
        self.interval = None      # setInterval / setBinned: float64 (n, 2), per training row the bounds lower <= upper of its value
        self.test_interval = None # setTestInterval / setTestBinned: float64 (numTest, 2), the same per row of test_vec (macau(lpd=True))
        self.ordinal = None       # setOrdinal: {"K", "step", "sample_edges"}; the training values are levels 1 .. K
        self.ordinal_codes = None # ... int8 per training row, its level
        self.ordinal_edges = None # ... float64 (K - 1): the edges e_1 .. e_{K-1}, k + 1/2 until macau() has drawn them (then the last draw)
        self.test_ordinal = None  # setTestOrdinal: int8 per row of test_vec, its level (macau(lpd=True))
        self.waic = None          # setWaic: {"pointwise"}; macau() scores the training cells by WAIC
        self.robust = None        # setRobust: {"nu"}; Student-t noise with nu degrees of freedom and scale alpha^-1/2
        self.weights = None       # setWeights: float64 per training row, its known precision weight (> 0)
        self.pg = None            # setLogit / setCounts: {"model": "logit" | "counts", "r", "offset"}; Polya-Gamma augmentation
        self.background = None    # setBackground: {"weight", "value"}; every cell that is not listed observes `value` with precision alpha weight
        self.recommend = None     # setRecommend: {"k", "rows", "exclude_listed", "batch"}; macau() returns a top-k list per row of the first entity
        self.acquire = None       # setAcquire: {"k", "rule", "kappa", "threshold", "rows", "exclude_listed", "batch"}; macau() returns a top-k list by an acquisition score
        self.diagnostics = None   # setDiagnostics: {"pointwise", "rhat_cut", "ess_cut"}; macau() keeps every draw of the test cells' predictions and returns their split R-hat and effective sample size
        self.entity_noise = None  # setEntityNoise: {"mode" (1-based), "shape", "rate"}; a sampled noise precision per row of that entity
        self.dense = False        # setDense: all N M cells of the two-mode relation are kept as a matrix on the device, none is listed to the row kernels
        self.bias = {}            # setBias: {mode (1-based): {"shape", "rate"}}; a sampled bias per row of every listed entity
        self.new_test = None      # setNewTest: {"mode" (1-based: the entity with new rows), "ids" (n, 2), "values" (NaN: unknown)}; cells of new rows
        self.new_observed = None  # setNewObserved: {"mode" (1-based), "ids" (k, 2), "values", "n_rows"}; cells of the new rows that are known


class RelationTemp:
    def __init__(self):
        self.linear_values = None
        self.FF = None


class TestVec:
    """Relation.test_vec: the held-out rows of the table (ids 1-based)."""

    def __init__(self, ids, values, names):
        self.ids = np.asarray(ids)
        self.values = np.asarray(values, dtype=np.float64)
        self.names = list(names)

    def __len__(self):
        return len(self.values)

    @property
    def shape(self):
        return (len(self.values), self.ids.shape[1] + 1)

    def to_frame(self, **extra):
        import pandas as pd
        d = {self.names[k]: self.ids[:, k] for k in range(self.ids.shape[1])}
        d[self.names[-1]] = self.values
        d.update(extra)
        return pd.DataFrame(d)


def _table_from_sparse(M):
    """findnz(::SparseMatrixCSC) order: column-major (RelationData.jl:165-171, 299-305)"""
    csc = M.tocsc(copy=True)
    csc.sum_duplicates()
    csc.sort_indices()
    cols = np.repeat(np.arange(csc.shape[1], dtype=np.int64), np.diff(csc.indptr)) + 1
    rows = csc.indices.astype(np.int64) + 1
    return np.stack([rows, cols], axis=1), np.asarray(csc.data, dtype=np.float64)


class Relation:
    """Relation(data, name, entities=[]; class_cut=0.0, dims=...) (RelationData.jl:128-171).

    data: IndexedDF | pandas DataFrame / dict / (ids, values) table | scipy sparse matrix."""

    def __init__(self, data, name, entities=None, class_cut=0.0, alpha=1.0, dims=None):
        entities = list(entities) if entities is not None else []
        self.F = None
        self.name = str(name)
        self.class_cut = float(class_cut)
        self.model = RelationModel(alpha)
        self.temp = RelationTemp()
        self.test_F = None
        if isinstance(data, IndexedDF):
            self.data = data
            self.entities = entities
        else:
            if hasattr(data, "tocsc"):
                if len(entities) != 2:
                    raise ArgumentError("For matrix relation the number of entities has to be 2.")
                ids, vals = _table_from_sparse(data)
                names = ["E1", "E2", "values"]
                dims = [int(data.shape[0]), int(data.shape[1])]
            else:
                ids, vals, names = _split_table(data)
                if dims is None:
                    dims = [int(ids[:, i].max()) if len(ids) else 0 for i in range(ids.shape[1])]
                dims = [int(d) for d in dims]
            if entities:
                if ids.shape[1] != len(entities):
                    raise ArgumentError(f"data has {ids.shape[1] + 1} columns but needs to have {len(entities) + 1} "
                                        "which is number of entities + 1")
                for i, en in enumerate(entities):
                    if en.count == 0:
                        en.count = dims[i]
                    elif en.count > dims[i]:
                        dims[i] = en.count
                    elif en.count < dims[i]:
                        raise ArgumentError(f"Entity {en.name} has smaller count {en.count} than the largest id in the data "
                                            f"{dims[i]}. Set entity.count manually before creating the relation.")
            self.data = IndexedDF((ids, vals), dims, names=names)
            self.entities = entities
        self.test_vec = TestVec(self.data.ids[:0, :], self.data.values[:0], self.data.names)
        self.test_label = np.zeros(0, dtype=bool)
        self._dev = None          # engine.RelationState

    def size(self, d=None):
        return self.data.size(d)

    def __repr__(self):
        a = "sample" if self.model.alpha_sample else f"{self.model.alpha:.2f}"
        s = (f"[Relation] {self.name}: {'--'.join(e.name for e in self.entities)}, #known = {numData(self)}, "
             f"#test = {numTest(self)}, α = {a}")
        if hasFeatures(self):
            s += f", #feat = {feat.feature_shape(self.F)[1]}"
        return s


def numData(r):
    return r.data.nnz()


def numTest(r):
    return len(r.test_vec)


def setPrecision(r, precision):
    refuse(r, "precision")
    r.model.alpha = float(precision)


def _number(x):
    """whether x is a finite real number (no bool, no string)"""
    return not isinstance(x, (bool, np.bool_)) and isinstance(x, (int, float, np.integer, np.floating)) and bool(np.isfinite(x))


def _is_binary(values):
    values = np.asarray(values)
    return bool(np.all((values == 0) | (values == 1)))


def setProbit(r):
    """Probit noise model for a relation of 0/1 values (the reference has Gaussian noise only): y = 1[z > 0] with a latent
    z ~ N(u'v, 1) that macau() samples beside the rows.  Predictions become probabilities Phi(u'v), class_cut 0.5.  Works before
    or after assignToTest / setTest; every training and test value must be exactly 0 or 1."""
    check_probit(r, build=False)
    r.model.probit = True
    r.model.alpha = 1.0
    r.model.alpha_sample = False
    r.model.mean_value = 0.0
    r.class_cut = 0.5
    r.test_label = r.test_vec.values < r.class_cut
    r._dev = None
    return None


def check_probit(r, build=True):
    """what a probit relation must still satisfy when a sampler is built on it (it may have been changed since setProbit)"""
    refuse(r, "probit", build)
    if not _is_binary(r.data.values) or not _is_binary(r.test_vec.values):
        raise ArgumentError(f"Relation {r.name} must hold only the values 0 and 1 for the probit noise model.")


def setCensored(r, censor):
    """Censored (Tobit) noise model for a Gaussian relation (the reference takes every value as a measurement): censor[k] says
    what training row k of r.data, in its current order, is -- 0 the measurement, +1 "the true value is at least this"
    (right-censored), -1 "at most this" (left-censored).  macau() then samples a latent value for every flagged row beside the
    rows: z ~ N(u'v + mean, 1 / alpha) truncated to the bound's side.  Predictions, the test set and alpha (fixed, setPrecision or
    alpha_sample) stay what they are.  Call it AFTER the test split (assignToTest removes training rows; setTest does not)."""
    refuse(r, "censored")
    r.model.censor = _censor_flags(r, censor)
    r._dev = None
    return None


def _pg_r(r, disp):
    if not _number(disp) or disp != int(disp) or disp < 1 or disp > COUNT_MAX:
        raise ArgumentError(f"Relation {r.name}: r = {disp} must be an integer, at least 1.")
    return int(disp)


COUNT_MAX = 2 ** 31


def _is_count(values):
    v = np.asarray(values, dtype=np.float64)
    return bool(np.all(np.isfinite(v) & (v >= 0) & (v <= COUNT_MAX) & (v == np.floor(v))))


def setLogit(r, offset=0.0):
    """Logit noise model for a relation of 0/1 values (the reference has Gaussian noise only): P(y = 1) = 1 / (1 + e^-psi),
    psi = u'v + offset.  macau() samples a Polya-Gamma variable omega ~ PG(1, psi) for every training row beside the rows (Polson,
    Scott & Windle 2013), which makes the row a Gaussian pseudo-observation (y - 1/2) / omega of psi with precision omega.
    Predictions become probabilities, class_cut 0.5.  Works before or after assignToTest / setTest; every training and test value
    must be exactly 0 or 1."""
    refuse(r, "logit")
    if not _is_binary(r.data.values) or not _is_binary(r.test_vec.values):
        raise ArgumentError(f"Relation {r.name} must hold only the values 0 and 1 for the logit noise model.")
    r.model.pg = {"model": "logit", "r": 0, "offset": _finite(r, "offset", offset)}
    r.model.alpha = 1.0
    r.model.alpha_sample = False
    r.model.mean_value = r.model.pg["offset"]
    r.class_cut = 0.5
    r.test_label = r.test_vec.values < r.class_cut
    r._dev = None
    return None


def setCounts(rel, r, offset=0.0):
    """Count noise model (the reference has Gaussian noise only): the values are the integers 0, 1, 2, ... (at most 2^31, stored as
    floats), negative binomial with the fixed integer dispersion r >= 1 and mean r e^psi, psi = u'v + offset: pmf proportional to
    p^y (1 - p)^r at p = 1 / (1 + e^-psi).  macau() samples omega ~ PG(y + r, psi) for every training row beside the rows, which
    makes the row a Gaussian pseudo-observation (y - r) / (2 omega) of psi with precision omega (exact up to y + r = 170, a
    moment-matched normal above).  Predictions are the mean r e^psi.  Works before or after assignToTest / setTest."""
    refuse(rel, "counts")
    disp, off = _pg_r(rel, r), _finite(rel, "offset", offset)
    if not _is_count(rel.data.values) or not _is_count(rel.test_vec.values):
        raise ArgumentError(f"Relation {rel.name} must hold only the integers 0 ... 2^31 for the count noise model.")
    rel.model.pg = {"model": "counts", "r": disp, "offset": off}
    rel.model.alpha = 1.0
    rel.model.alpha_sample = False
    rel.model.mean_value = off
    rel._dev = None
    return None


def check_pg(r):
    """what a logit or count relation must still satisfy when a sampler is built on it (it may have been changed since)"""
    pg = r.model.pg
    refuse(r, pg["model"], build=True)
    if r.model.alpha != 1.0:
        raise ArgumentError(f"Relation {r.name} has {OPTION[pg['model']].phrase}: every cell's precision is its sampled omega, alpha stays 1.")
    off = _finite(r, "offset", pg.get("offset"))
    if pg["model"] == "logit":
        if not _is_binary(r.data.values) or not _is_binary(r.test_vec.values):
            raise ArgumentError(f"Relation {r.name} must hold only the values 0 and 1 for the logit noise model.")
        r.model.pg = {"model": "logit", "r": 0, "offset": off}
    else:
        disp = _pg_r(r, pg.get("r"))
        if not _is_count(r.data.values) or not _is_count(r.test_vec.values):
            raise ArgumentError(f"Relation {r.name} must hold only the integers 0 ... 2^31 for the count noise model.")
        r.model.pg = {"model": "counts", "r": disp, "offset": off}
    r.model.mean_value = off


def setRobust(r, nu=4.0):
    """Robust noise model for a Gaussian relation (the reference weighs every training cell alike): Student-t noise with nu
    degrees of freedom and scale alpha^-1/2, as the scale mixture y ~ N(u'v + mean, 1 / (alpha omega)), omega ~ Gamma(nu / 2,
    rate nu / 2).  macau() samples omega for every training row beside the rows, so that a gross outlier counts with a small
    precision instead of dragging the factors; result["robust"]["weights"] is the posterior mean of omega per training row (small:
    an outlier).  nu >= 1; nu = 1 is Cauchy noise, a large nu approaches the Gaussian model.  Predictions, the test set and alpha
    (fixed, setPrecision or alpha_sample) stay what they are."""
    refuse(r, "robust")
    r.model.robust = {"nu": _robust_nu(r, nu)}
    r._dev = None
    return None


def _robust_nu(r, nu):
    if not _number(nu) or nu < 1.0:
        raise ArgumentError(f"Relation {r.name}: nu = {nu} must be a finite number, at least 1.")
    return float(nu)


def setWeights(r, weights):
    """Known observation weights for a Gaussian relation: training row k of r.data, in its current order, counts with precision
    alpha weights[k] (replicate counts, reported standard errors as 1 / se^2 relative to 1 / alpha, down-weighted imputed cells).
    Every weight is finite and strictly positive.  A sampled alpha is drawn from its conditional under the weights.  Call it AFTER
    the test split (assignToTest removes training rows; setTest does not)."""
    refuse(r, "weights")
    r.model.weights = _obs_weights(r, weights)
    r._dev = None
    return None


def _obs_weights(r, weights):
    try:
        w = np.asarray(weights, dtype=np.float64)
    except (TypeError, ValueError):
        raise ArgumentError(f"Relation {r.name}: observation weights must be numbers.") from None
    if w.ndim != 1 or len(w) != r.data.nnz():
        raise ArgumentError(f"Relation {r.name} has {r.data.nnz()} training rows but {w.shape} observation weights were given.")
    if not bool(np.all(np.isfinite(w) & (w > 0.0))):
        raise ArgumentError(f"Relation {r.name}: observation weights must be finite and strictly positive.")
    return np.ascontiguousarray(w)


def check_robust(r):
    """what a robust or weighted relation must still satisfy when a sampler is built on it (it may have been changed since)"""
    if r.model.robust is not None:
        refuse(r, "robust", build=True)
        r.model.robust = {"nu": _robust_nu(r, r.model.robust.get("nu"))}
    if r.model.weights is not None:
        refuse(r, "weights", build=True)
        r.model.weights = _obs_weights(r, r.model.weights)


def setEntityNoise(r, entity, shape=2.0, rate=2.0):
    """A noise precision per row of one entity of a Gaussian relation (the reference has one alpha for every cell): a cell whose id
    in that entity's mode is j is observed with precision alpha tau_j, tau_j ~ Gamma(shape, rate) a priori (mean shape / rate), and
    macau() samples tau_j beside the rows from Gamma(shape + n_j / 2, rate + alpha S_j / 2), S_j the row's sum of squared
    residuals -- so that one noisy assay column or one erratic rater pools the evidence of all its cells and stops dragging every
    other row's factors towards its noise.  entity: an Entity of the relation, its name, or its 1-based mode.  alpha (fixed,
    setPrecision or alpha_sample) stays the overall scale.  result["noise"]["precision"] is the posterior mean tau per row of the
    entity.  Predictions and the test set stay what they are; macau(lpd=True) scores a held-out cell with alpha tau of its row.
    Works before or after the test split."""
    refuse(r, "entity_noise")
    r.model.entity_noise = _entity_noise_spec(r, entity, shape, rate)
    r._dev = None
    return None


def _entity_noise_spec(r, entity, shape, rate):
    n_modes = len(r.entities)
    if isinstance(entity, Entity):
        hit = [k for k, e in enumerate(r.entities) if e is entity]
    elif isinstance(entity, str):
        hit = [k for k, e in enumerate(r.entities) if e.name == entity]
    elif isinstance(entity, (int, np.integer)) and not isinstance(entity, (bool, np.bool_)):
        hit = [int(entity) - 1] if 1 <= int(entity) <= n_modes else []
    else:
        hit = []
    if len(hit) != 1:
        raise ArgumentError(f"Relation {r.name}: entity = {entity!r} must be one of its entities ({', '.join(e.name for e in r.entities)}), "
                            f"by object, by name or by its mode 1 ... {n_modes}.")
    for name, x in (("shape", shape), ("rate", rate)):
        if not _number(x) or x <= 0:
            raise ArgumentError(f"Relation {r.name}: {name} = {x} must be a finite number above 0.")
    return {"mode": hit[0] + 1, "shape": float(shape), "rate": float(rate)}


def check_entity_noise(r):
    """what a relation with a noise precision per row must still satisfy when a sampler is built on it (it may have been changed since)"""
    refuse(r, "entity_noise", build=True)
    m = r.model.entity_noise
    r.model.entity_noise = _entity_noise_spec(r, m.get("mode"), m.get("shape"), m.get("rate"))


def setBias(r, entity, shape=1.0, rate=1.0):
    """A bias per row of one entity of a Gaussian relation (the reference has one mean_value per relation; its successor SMURFF and
    every practical recommender have these): y_ij = mean + a_i + b_j + u_i.v_j + noise -- a harsh rater, a popular film or an assay
    with an offset shifts every cell of its row by the same amount, and the factors need not spend components on it.  Call it once
    per entity that gets biases: entity is an Entity of the relation, its name, or its 1-based mode.  b_j ~ N(0, 1 / lambda) with
    lambda ~ Gamma(shape, rate) (rate parametrisation), one lambda per biased entity; macau() samples the biases and lambda beside
    the rows and returns result["bias"][relation name][entity name] = {"mean": the posterior mean bias per
    row, "precision": the posterior mean lambda}.  mean_value stays the mean of the training values, which is why the prior mean
    is zero.  Predictions, the test set, lpd, setWaic, rmse_train and full_prediction include the biases; alpha is fixed, set by
    setPrecision, or sampled.  Plain Gaussian noise only: no other noise model, observation weights, relation features,
    setBackground, setDense, setRecommend or setNewTest on the relation, no spike-and-slab or non-negative entity in it; one rank."""
    refuse(r, "bias")
    mode, spec = _bias_spec(r, entity, shape, rate)
    if mode in r.model.bias:
        raise ArgumentError(f"Relation {r.name} already has biases for its entity {r.entities[mode - 1].name} (setBias): once per entity.")
    r.model.bias = dict(r.model.bias)
    r.model.bias[mode] = spec
    r._dev = None
    return None


def _bias_spec(r, entity, shape, rate):
    m = _entity_noise_spec(r, entity, shape, rate)        # (the same resolution of `entity` and the same numbers)
    return m["mode"], {"shape": m["shape"], "rate": m["rate"]}


def check_bias(r):
    """what a relation with biases must still satisfy when a sampler is built on it (it may have been changed since setBias)"""
    refuse(r, "bias", build=True)
    out = {}
    for mode, spec in r.model.bias.items():
        m, sp = _bias_spec(r, mode, spec.get("shape"), spec.get("rate"))
        out[m] = sp
    r.model.bias = out


def setSpikeAndSlab(entity, incl_a=1.0, incl_b=1.0, shape=1.0, rate=1.0):
    """A spike-and-slab prior for the rows of `entity` in place of the Normal-Wishart one (the reference has none; its successor SMURFF
    does): loading d of row i is u_id = s_id w_id with s_id ~ Bernoulli(pi_d), w_id ~ N(0, 1 / tau_d), pi_d ~ Beta(incl_a, incl_b) and
    tau_d ~ Gamma(shape, rate) (rate parametrisation).  A component can be switched off for the whole entity -- with one column entity
    per view this is the group sparsity of group factor analysis -- and a single loading can be exactly zero.  macau() samples
    (s_id, w_id) one component after the other from their exact conditional and returns, under
    result["spike"][entity.name], the posterior means "inclusion" (pi_d), "precision" (tau_d), "activity" (the share of rows with a
    nonzero loading) per component and "row_inclusion" (N x D).  The verbose line's " on:<k>" for such an entity is the number of
    components with a nonzero loading in the current draw (a count, not their list).  The entity takes no side information, none of its relations a
    background (setBackground); one rank only.  The other entities keep their prior; every noise model composes."""
    if not isinstance(entity, Entity):
        raise ArgumentError(f"setSpikeAndSlab takes an Entity, not {type(entity).__name__}.")
    spec = _spike_spec(entity, incl_a, incl_b, shape, rate)
    refuse(entity, "spike")
    entity.spike = spec
    return None


def _spike_spec(entity, incl_a, incl_b, shape, rate):
    for name, x in (("incl_a", incl_a), ("incl_b", incl_b), ("shape", shape)):
        if not _number(x) or x < 0.5:
            raise ArgumentError(f"Entity {entity.name}: {name} = {x} must be a finite number, at least 0.5 (setSpikeAndSlab).")
    if not _number(rate) or rate <= 0:
        raise ArgumentError(f"Entity {entity.name}: rate = {rate} must be a finite number above 0 (setSpikeAndSlab).")
    return {"incl_a": float(incl_a), "incl_b": float(incl_b), "shape": float(shape), "rate": float(rate)}


def check_spike(entity, world=1):
    """what an entity with the spike-and-slab prior must still satisfy when a sampler is built on it"""
    m = entity.spike
    entity.spike = _spike_spec(entity, m.get("incl_a"), m.get("incl_b"), m.get("shape"), m.get("rate"))
    refuse(entity, "spike", build=True)
    refuse_ranks(entity, "spike", world)


def setNonNegative(entity, shape=1.0, rate=1.0):
    """Non-negative factors for the rows of `entity` in place of the Normal-Wishart prior (the reference has none): loading d of row i
    is u_id ~ N(0, 1 / tau_d) truncated to u_id >= 0 (a half-normal) with tau_d ~ Gamma(shape, rate) (rate parametrisation) -- Bayesian
    non-negative matrix factorisation (Schmidt, Winther & Hansen 2009): with one entity of a relation constrained semi-NMF, with all of
    them NMF proper.  macau() samples a row one component after the other from its truncated-normal conditional by inversion (DESIGN.md
    section 26) and returns, under result["nonneg"][entity.name], the posterior means "precision" (tau_d) and "factors" (N x D, all
    >= 0).  The per-component precision switches surplus components off by itself.  Centring: a Gaussian-kind relation ALL of whose
    entities are non-negative is NOT centred -- its model is u.v itself, which is >= 0, so mean_value is 0 instead of the mean of its
    values; every other relation keeps its centring (with one free entity the centred model is the right semi-NMF).  The verbose
    line marks such an entity with " nn".  The entity takes no side information and no new rows (setNewRows), not the spike-and-slab
    prior (setSpikeAndSlab), none of its relations a background (setBackground) or the dense path (setDense); one rank only; bpmf_vb and
    macau_hmc do not take it.  The other entities keep their prior; every noise model composes."""
    if not isinstance(entity, Entity):
        raise ArgumentError(f"setNonNegative takes an Entity, not {type(entity).__name__}.")
    spec = _nonneg_spec(entity, shape, rate)
    refuse(entity, "nonneg")
    entity.nonneg = spec
    return None


def _nonneg_spec(entity, shape, rate):
    if not _number(shape) or shape < 0.5:
        raise ArgumentError(f"Entity {entity.name}: shape = {shape} must be a finite number, at least 0.5 (setNonNegative).")
    if not _number(rate) or rate <= 0:
        raise ArgumentError(f"Entity {entity.name}: rate = {rate} must be a finite number above 0 (setNonNegative).")
    return {"shape": float(shape), "rate": float(rate)}


def check_nonneg(entity, world=1):
    """what an entity with the non-negative prior must still satisfy when a sampler is built on it"""
    m = entity.nonneg
    entity.nonneg = _nonneg_spec(entity, m.get("shape"), m.get("rate"))
    refuse(entity, "nonneg", build=True)
    refuse_ranks(entity, "nonneg", world)


def setBackground(r, weight, value=0.0):
    """Implicit feedback (Hu, Koren & Volinsky 2008; the one-class factorisation of Pan et al., here in its Bayesian form): every
    cell of a two-mode relation that is NOT among its training rows is an observation of `value` (in the relation's raw units) with
    precision alpha weight.  The listed cells keep precision alpha omega_k, omega_k their setWeights weight or 1, so 0 < weight <
    min omega_k.  The N M - nnz background cells are never listed: they enter every row's conditional through the Gram matrix of
    the other entity's rows, which all rows share, and an iteration costs what the listed cells cost.
    mean_value becomes the mean over ALL cells, as valueMean of the dense listing would be.  A sampled alpha is drawn from its
    conditional over all N M cells.  noise_kind stays "gauss" or "weights".  Held-out cells (assignToTest / setTest) that are not
    listed are background cells during training: the usual protocol for implicit data.  rmse_train covers the listed cells.
    Works before or after setWeights and the test split."""
    refuse(r, "background")
    _background_cells(r)
    w, v = _finite(r, "weight", weight), _finite(r, "value", value)
    _background_weight(r, w)
    r.model.background = {"weight": w, "value": v}
    r._dev = None
    return None


def _finite(r, name, x):
    if not _number(x):
        raise ArgumentError(f"Relation {r.name}: {name} = {x} must be a finite number.")
    return float(x)


def _background_weight(r, w):
    """0 < w < the smallest listed weight (1 without setWeights): a listed cell then counts with omega_k - w > 0 beside the Gram term"""
    least = float(np.min(r.model.weights)) if (r.model.weights is not None and len(r.model.weights)) else 1.0
    if not (0.0 < w < least):
        raise ArgumentError(f"Relation {r.name}: weight = {w} must lie strictly between 0 and the smallest weight of a listed cell ({least}).")


def _two_modes(r, key, takes):
    if len(r.data.dims) != 2:
        raise ArgumentError(f"Relation {r.name} has {len(r.data.dims)} modes: {OPTION[key].phrase} {takes} a two-mode relation.")


def _listed_once(r, key, why):
    ids = np.asarray(r.data.ids).reshape(r.data.nnz(), 2)
    if len(np.unique(ids, axis=0)) != len(ids):
        raise ArgumentError(f"Relation {r.name} lists a cell more than once: {OPTION[key].phrase} {why}.")
    return ids


def _background_cells(r):
    _two_modes(r, "background", "takes")
    _listed_once(r, "background", "would subtract it from the Gram term twice")


def check_background(r):
    """what a background relation must still satisfy when a sampler is built on it (setWeights, a noise model or setWaic may have
    come since setBackground)"""
    refuse(r, "background", build=True)
    _background_cells(r)
    b = r.model.background
    w, v = _finite(r, "weight", b.get("weight")), _finite(r, "value", b.get("value"))
    _background_weight(r, w)
    r.model.background = {"weight": w, "value": v}


def background_mean(r):
    """mean_value of a background relation: the mean over all N M cells, the unlisted ones at the background value"""
    cells = float(r.data.dims[0]) * float(r.data.dims[1])
    nn = r.data.nnz()
    return (float(np.sum(np.asarray(r.data.values, dtype=np.float64))) + (cells - nn) * r.model.background["value"]) / cells if cells else 0.0


def setDense(r, on=True):
    """A two-mode Gaussian relation whose N x M cells are (nearly) all observed: an expression panel, a fully screened plate, a
    feature block taken as a relation.  macau() then keeps the values as one N x M matrix on the device and lists no cell to the row
    kernels: every row's conditional reads the relation through the Gram matrix of the other entity's rows, which all rows share,
    and its own row of R V, two products on the matrix cores per iteration.  Nothing is approximated: the
    chain is the explicit listing's up to rounding.  Cells that are not listed -- held out by assignToTest, or NaN in
    denseRelation's array -- are holes: they are imputed before every iteration, r_ij = u_i.v_j + z / sqrt(alpha), which is exact
    Gibbs sampling on the augmented model; at least half of the cells must be listed (the sparse path is the right one otherwise).
    noise_kind stays "gauss"; alpha is fixed, set by setPrecision, or sampled over all N M cells.  Entity side information, the
    test set, lpd, rmse_train, setWaic and further relations (sparse, dense or with a background) on the same entities all work.
    setDense(r, False) takes it back.  Works before or after the test split."""
    if not on:
        r.model.dense = False
        r._dev = None
        return None
    check_dense(r, build=False)
    r.model.dense = True
    r._dev = None
    return None


def denseRelation(Y, name, entities, class_cut=0.0, alpha=1.0):
    """Relation(...) from a 2-D array of values, NaN where a cell is not observed, with setDense.  (A bare 2-D array handed to
    Relation itself is a table of ids and values.)"""
    Y = np.asarray(Y, dtype=np.float64)
    if Y.ndim != 2:
        raise ArgumentError(f"denseRelation takes a 2-D array of values, not {Y.ndim} dimensions.")
    if len(entities) != 2:
        raise ArgumentError("For matrix relation the number of entities has to be 2.")
    ii, jj = np.nonzero(~np.isnan(Y))                   # row by row
    r = Relation((np.stack([ii + 1, jj + 1], axis=1).astype(np.int64), Y[ii, jj]), name, entities, class_cut=class_cut, alpha=alpha,
                 dims=[int(Y.shape[0]), int(Y.shape[1])])
    setDense(r)
    return r


def check_dense(r, build=True):
    """what a dense relation must still satisfy when a sampler is built on it (a noise model, a background or a test split may have
    come since setDense)"""
    what = OPTION["dense"].phrase
    refuse(r, "dense", build)
    _two_modes(r, "dense", "takes")
    ids = _listed_once(r, "dense", "keeps one value per cell")
    cells = int(r.data.dims[0]) * int(r.data.dims[1])
    if cells == 0 or 2 * len(ids) < cells:
        raise ArgumentError(f"Relation {r.name} lists {len(ids)} of its {cells} cells: {what} takes a relation with at least half of them "
                            "listed (the sparse path is the right one for this one).")


def dense_matrix(r):
    """(Y, holes) of a dense relation: its values as an N x M array, NaN at the holes, and the holes' (i, j), 0-based, row by row"""
    N, M = int(r.data.dims[0]), int(r.data.dims[1])
    Y = np.full((N, M), np.nan)
    ids = np.asarray(r.data.ids, dtype=np.int64).reshape(r.data.nnz(), 2)
    Y[ids[:, 0] - 1, ids[:, 1] - 1] = np.asarray(r.data.values, dtype=np.float64)
    return Y, np.argwhere(np.isnan(Y))


RECOMMEND_MAX_K = 64          # BDF_REC_MAX_K, BDF_REC_MAX_BATCH (csrc/recommend.h)
RECOMMEND_MAX_BATCH = 32


def setRecommend(r, k, rows=None, exclude_listed=True, batch=8):
    """macau() returns, for rows of this relation's FIRST entity, the k (1 .. 64) best items of the second by the posterior mean
    score mean_value + E[u.v]: result["recommend"] = {"k", "rows", "items", "scores"} and, when the relation has test cells,
    recall@k, NDCG@k and the hit rate on them ("recall", "ndcg", "hit_rate", "rows_scored").  The sum of u.v over the draws is kept
    on the device (rows x M doubles), `batch` (1 .. 32) draws' factors buffered per pass over it; only the lists come back.
    rows: None, every row; else distinct 1-based ids of the first entity, the only rows that get a sum and a list.
    exclude_listed: a row's training cells never appear in its list.  Lists are ordered by falling score, equal scores by rising
    item id; a list is padded with item 0 and score NaN behind the row's last candidate.  The first relation of its RelationData,
    two modes, no relation features, a noise model whose prediction is u.v + mean (not probit, logit or counts), one rank.
    Nothing of the chain changes."""
    refuse(r, "recommend")
    _two_modes(r, "recommend", "take")
    r.model.recommend = _recommend_spec(r, k, rows, exclude_listed, batch)
    r._dev = None
    return None


def _recommend_int(r, name, x, top, setter="setRecommend"):
    if isinstance(x, (bool, np.bool_)) or not isinstance(x, (int, np.integer)) or not (1 <= int(x) <= top):
        raise ArgumentError(f"Relation {r.name}: {name} = {x} must be an integer in 1 ... {top} ({setter}).")
    return int(x)


def _recommend_spec(r, k, rows, exclude_listed, batch, setter="setRecommend"):
    """k, rows, exclude_listed and batch of a ranked list, checked; setter: who the messages name (setRecommend, setAcquire)"""
    k, batch = _recommend_int(r, "k", k, RECOMMEND_MAX_K, setter), _recommend_int(r, "batch", batch, RECOMMEND_MAX_BATCH, setter)
    if not isinstance(exclude_listed, (bool, np.bool_)):
        raise ArgumentError(f"Relation {r.name}: exclude_listed = {exclude_listed} must be true or false ({setter}).")
    if rows is not None:
        N = int(r.data.dims[0])
        try:
            a = np.asarray(rows)
        except (TypeError, ValueError):
            a = np.asarray(0.5)
        if a.ndim != 1 or a.dtype == np.bool_ or not np.issubdtype(a.dtype, np.integer):
            raise ArgumentError(f"Relation {r.name}: rows must be a list of integer ids of {r.entities[0].name} ({setter}).")
        a = a.astype(np.int64)
        if len(a) and (a.min() < 1 or a.max() > N):
            raise ArgumentError(f"Relation {r.name}: rows holds an id outside 1 ... {N} ({setter}).")
        if len(np.unique(a)) != len(a):
            raise ArgumentError(f"Relation {r.name}: rows holds an id more than once ({setter}).")
        rows = a
    return {"k": k, "rows": rows, "exclude_listed": bool(exclude_listed), "batch": batch}


def check_recommend(r):
    """what a relation with setRecommend must still satisfy when a sampler is built on it (a noise model may have come since)"""
    refuse(r, "recommend", build=True)
    _two_modes(r, "recommend", "take")
    m = r.model.recommend
    r.model.recommend = _recommend_spec(r, m.get("k"), m.get("rows"), m.get("exclude_listed"), m.get("batch"))


ACQUIRE_RULES = ("ucb", "sd", "prob_above")


def setAcquire(r, k, rule="ucb", kappa=1.0, threshold=None, rows=None, exclude_listed=True, batch=8):
    """macau() returns, for rows of this relation's FIRST entity, the k (1 .. 64) unlisted items of the second with the largest
    acquisition score, computed from the post-burn-in draws: which cell to measure next, which cell is likely above a threshold.
    With m the posterior mean of u.v + mean_value and sd the sample standard deviation (n - 1) of u.v over the n draws:
    rule "ucb": m + kappa sd, kappa >= 0 and finite (kappa = 0 ranks by the mean); "sd": sd alone (uncertainty sampling);
    "prob_above": the posterior probability that a measurement of the cell exceeds `threshold` (required, finite), the noise
    integrated out per draw: (1/n) sum_b Phi(sqrt(alpha_b) (u_b.v_b + mean_value - threshold)), alpha_b the draw's precision, fixed
    or sampled (alpha_sample); under setBackground alpha_b is the LISTED cells' precision.
    result["acquire"] = {"k", "rule", "kappa", "threshold", "rows", "items", "scores", "mean", "sd"} and, for prob_above, "prob":
    n_rows x k each, the moments read at the listed items on the device.  The running mean and sum of squared deviations (Welford)
    of u.v -- and the sum of the probabilities -- are kept on the device (rows x M doubles each), `batch` (1 .. 32) draws' factors
    buffered per pass over them; only the lists come back.  With fewer than 2 draws ucb and sd have no candidates, with none
    prob_above has none.  rows, exclude_listed, the order and the padding of a list: as for setRecommend, which the relation cannot
    have as well.  The first relation of its RelationData, two modes, no relation features, Gaussian noise of one precision
    (censored and interval values are taken), one rank.  Nothing of the chain changes.  k = None clears it."""
    if k is None:
        r.model.acquire = None
        r._dev = None
        return None
    refuse(r, "acquire")
    _two_modes(r, "acquire", "take")
    r.model.acquire = _acquire_spec(r, k, rule, kappa, threshold, rows, exclude_listed, batch)
    r._dev = None
    return None


def _acquire_spec(r, k, rule, kappa, threshold, rows, exclude_listed, batch):
    spec = _recommend_spec(r, k, rows, exclude_listed, batch, "setAcquire")

    def number(x):
        return isinstance(x, (int, float, np.integer, np.floating)) and not isinstance(x, (bool, np.bool_)) and math.isfinite(x)
    if not isinstance(rule, str) or rule not in ACQUIRE_RULES:
        raise ArgumentError(f"Relation {r.name}: rule = {rule!r} must be one of {', '.join(repr(x) for x in ACQUIRE_RULES)} (setAcquire).")
    if not number(kappa) or kappa < 0:
        raise ArgumentError(f"Relation {r.name}: kappa = {kappa} must be a finite number, not negative (setAcquire).")
    if rule == "prob_above":
        if threshold is None or not number(threshold):
            raise ArgumentError(f"Relation {r.name}: rule 'prob_above' needs a finite threshold, not {threshold} (setAcquire).")
    elif threshold is not None:
        raise ArgumentError(f"Relation {r.name}: a threshold goes with rule 'prob_above', not with {rule!r} (setAcquire).")
    spec.update({"rule": rule, "kappa": float(kappa), "threshold": None if threshold is None else float(threshold)})
    return spec


def check_acquire(r):
    """what a relation with setAcquire must still satisfy when a sampler is built on it (its model may have been changed since)"""
    refuse(r, "acquire", build=True)
    _two_modes(r, "acquire", "take")
    m = r.model.acquire
    r.model.acquire = _acquire_spec(r, m.get("k"), m.get("rule"), m.get("kappa"), m.get("threshold"), m.get("rows"), m.get("exclude_listed"), m.get("batch"))


def setNewRows(entity, F_new):
    """Features of instances of `entity` that are NOT among its rows -- a compound nobody has assayed, a user who has rated nothing:
    F_new (n* x numF; dense, scipy sparse, SparseMatrixCSR or SparseBinMatrix) has the columns of entity.F.  macau() predicts the
    cells that setNewTest lists for them from every posterior draw of the link matrix beta: given the draw, the factor of a new row
    with features f is N(mu + beta' f, Lambda^-1), which is integrated out of the cell's prediction in closed form (DESIGN.md
    section 24).  F_new must carry the normalisation that was applied to entity.F (normalizeFeatures / normalizeRows work on
    entity.F alone: scale the new rows with the SAME column norms, or normalise their rows the same way, before passing them).
    The entity must have features and keep the Normal-Wishart prior (not setSpikeAndSlab).  None clears it."""
    if not isinstance(entity, Entity):
        raise ArgumentError(f"setNewRows takes an Entity, not {type(entity).__name__}.")
    if F_new is None:
        entity.new_rows = None
        return None
    _new_rows_guards(entity, F_new)
    entity.new_rows = F_new
    return None


def _new_rows_guards(entity, F_new, build=False):
    if not hasFeatures(entity):
        raise ArgumentError(f"Entity {entity.name} has no features: new rows (setNewRows) are predicted from their features through beta.")
    refuse(entity, "new_rows", build)
    if feat.isempty(F_new):
        raise ArgumentError(f"Entity {entity.name}: F_new is empty (setNewRows takes a matrix with one row per new instance; None clears it).")
    have, want = feat.feature_shape(F_new)[1], feat.feature_shape(entity.F)[1]
    if have != want:
        raise ArgumentError(f"Entity {entity.name}: F_new has {have} columns but the entity's features have {want} (setNewRows).")


def setNewTest(r, entity, table):
    """Cells of relation r in the rows that setNewRows gave `entity`: a table shaped like setTest's, in the relation's column order,
    where the id in `entity`'s column is 1 ... n* into F_new, the other id is an existing instance of the other entity and the last
    column is the held-out value -- NaN where it is unknown: such a cell is predicted and left out of every score.  macau() then
    returns result["new_rows"] = {"entity", "n_rows", "predictions" (the ids, value, pred, stdev and, with lpd = true, lpd),
    "RMSE", "ROC", "accuracy", "n_scored", "factors" (n* x D: the posterior mean of mu + beta' f) and, with lpd = true, "LPD"}; stdev
    is the posterior sd of the cell's noise-free value, new row's factor included (probit: of its probability).  The first relation
    of its RelationData, two modes, no relation features, one rank; Gaussian noise (fixed or sampled alpha; also with setCensored,
    setInterval / setBinned and setBackground: a held-out value is a measurement) or setProbit (values 0 / 1 or NaN).  None clears it."""
    if table is None:
        r.model.new_test = None
        return None
    if not isinstance(entity, Entity):
        raise ArgumentError(f"setNewTest takes an Entity, not {type(entity).__name__}.")
    hit = [k for k, e in enumerate(r.entities) if e is entity]
    if not hit:
        raise ArgumentError(f"Relation {r.name} has no entity {entity.name} (setNewTest).")
    _new_test_guards(r, entity, build=False)
    ids, vals, _ = _split_table(table)
    ids, vals = np.asarray(ids), np.asarray(vals, dtype=np.float64).reshape(-1)
    if ids.ndim != 2 or ids.shape[1] != 2 or len(ids) != len(vals):
        raise ArgumentError(f"Relation {r.name}: the table of new cells must have two id columns and a value column (setNewTest).")
    if not np.issubdtype(ids.dtype, np.integer):
        if ids.size and not (np.all(np.isfinite(ids)) and np.all(ids == np.floor(ids))):
            raise ArgumentError(f"Relation {r.name}: the ids of new cells must be integers (setNewTest).")
        ids = ids.astype(np.int64)
    r.model.new_test = _new_test_spec(r, hit[0] + 1, ids.astype(np.int64), vals)
    return None


def _folds_in(r, entity):
    """whether setNewObserved named `entity` on relation r: its new rows are then conditioned on cells of their own"""
    m = r.model.new_observed
    return m is not None and 1 <= m.get("mode", 0) <= len(r.entities) and r.entities[m["mode"] - 1] is entity


def _new_test_guards(r, entity, build):
    refuse(r, "new_test", build)
    _two_modes(r, "new_test", "take")
    if entity.new_rows is None:
        # (an entity without features has new rows only through their known cells)
        if not _folds_in(r, entity):
            raise ArgumentError(f"Entity {entity.name} has no new rows: call setNewRows(entity, F_new) before setNewTest.")
        return
    _new_rows_guards(entity, entity.new_rows, build)


def _new_test_spec(r, mode, ids, vals):
    entity = r.entities[mode - 1]
    n_new = feat.feature_shape(entity.new_rows)[0] if entity.new_rows is not None else int(r.model.new_observed["n_rows"])
    other = 2 - mode                                       # 0-based column of the other entity
    n_other = int(r.data.dims[other])
    if len(ids) and (ids[:, mode - 1].min() < 1 or ids[:, mode - 1].max() > n_new):
        rows = "the rows of F_new" if entity.new_rows is not None else "the new rows of setNewObserved"
        raise ArgumentError(f"Relation {r.name}: a new cell's id of {entity.name} is outside 1 ... {n_new}, {rows} (setNewTest).")
    if len(ids) and (ids[:, other].min() < 1 or ids[:, other].max() > n_other):
        raise ArgumentError(f"Relation {r.name}: a new cell's id of {r.entities[other].name} is outside 1 ... {n_other} (setNewTest).")
    if r.model.probit and not _is_binary(vals[~np.isnan(vals)]):
        raise ArgumentError(f"Relation {r.name} has the probit noise model: the values of its new cells must be 0, 1 or NaN (setNewTest).")
    if np.any(np.isinf(vals)):
        raise ArgumentError(f"Relation {r.name}: the value of a new cell must be finite, or NaN where it is unknown (setNewTest).")
    return {"mode": int(mode), "ids": np.ascontiguousarray(ids, dtype=np.int64), "values": np.ascontiguousarray(vals, dtype=np.float64)}


def setNewObserved(r, entity, table, n_rows=None):
    """Cells of the NEW rows of `entity` in relation r that are known -- the ten films a new user has rated, the three assays a new
    compound was measured in: a table shaped like setNewTest's, where the id in `entity`'s column is 1 ... n*, the other id is an
    existing instance of the other entity and the value is finite.  macau() then predicts the cells of setNewTest from every
    posterior draw CONDITIONED on them: given the draw (mu, Lambda, beta, V, alpha), a new row i with prior mean mu_i (mu + beta' f_i
    for an entity with setNewRows, mu otherwise) and known cells K_i has u* ~ N(uhat_i, P_i^-1) with P_i = Lambda + alpha sum_K v v'
    and uhat_i = P_i^-1 (Lambda mu_i + alpha sum_K (y - mean) v), which is integrated out of a cell in closed form (DESIGN.md section
    29).  The known cells do not feed back into the other entity's factors: this is the standard fold-in, p(u* | y*, draw), not a
    refit.  A row without a known cell is predicted as setNewTest alone predicts it.  A cell of setNewTest may also be a known
    cell: it is then predicted with its own value in the conditional.
    n*: the rows of F_new for an entity with setNewRows; for an entity WITHOUT features n_rows, by default the largest new id of the
    table.  An entity with features but without setNewRows is refused: its new rows' prior mean needs their features.  An entity
    without features takes setNewTest only after setNewObserved has named it.  result["new_rows"]["factors"] is then the posterior
    mean of uhat_i and result["new_rows"]["n_known"] the known cells per new row.  An empty table is legal: every row is cold.  The
    first relation of its RelationData, two modes, plain Gaussian noise (fixed or sampled alpha), the Normal-Wishart prior, one
    rank; no relation features, setBackground, setDense, setBias or setRecommend.  None clears it."""
    if table is None:
        r.model.new_observed = None
        return None
    if not isinstance(entity, Entity):
        raise ArgumentError(f"setNewObserved takes an Entity, not {type(entity).__name__}.")
    hit = [k for k, e in enumerate(r.entities) if e is entity]
    if not hit:
        raise ArgumentError(f"Relation {r.name} has no entity {entity.name} (setNewObserved).")
    _new_observed_guards(r, entity, build=False)
    ids, vals, _ = _split_table(table)
    ids, vals = np.asarray(ids), np.asarray(vals, dtype=np.float64).reshape(-1)
    if ids.size == 0:
        ids = np.zeros((0, 2), dtype=np.int64)
    if ids.ndim != 2 or ids.shape[1] != 2 or len(ids) != len(vals):
        raise ArgumentError(f"Relation {r.name}: the table of known cells must have two id columns and a value column (setNewObserved).")
    if not np.issubdtype(ids.dtype, np.integer):
        if ids.size and not (np.all(np.isfinite(ids)) and np.all(ids == np.floor(ids))):
            raise ArgumentError(f"Relation {r.name}: the ids of known cells must be integers (setNewObserved).")
        ids = ids.astype(np.int64)
    r.model.new_observed = _new_observed_spec(r, hit[0] + 1, ids.astype(np.int64), vals, n_rows)
    return None


def _new_observed_guards(r, entity, build):
    refuse(r, "new_observed", build)
    _two_modes(r, "new_observed", "take")
    if entity.new_rows is not None:
        _new_rows_guards(entity, entity.new_rows, build)
    elif hasFeatures(entity):
        # (mu_i of such a row would be mu + beta' f_i: without f_i it would be conditioned on mu alone, beta silently left out)
        raise ArgumentError(f"Entity {entity.name} has features but no new rows: call setNewRows(entity, F_new) before setNewObserved, "
                            "the prior mean of a new row is mu + beta' f.")


def _new_observed_spec(r, mode, ids, vals, n_rows):
    entity = r.entities[mode - 1]
    other = 2 - mode
    n_other = int(r.data.dims[other])
    if n_rows is not None and (isinstance(n_rows, bool) or not isinstance(n_rows, (int, np.integer)) or n_rows < 1):
        raise ArgumentError(f"Relation {r.name}: n_rows must be a positive integer (setNewObserved).")
    if entity.new_rows is not None:
        n_new = feat.feature_shape(entity.new_rows)[0]
        if n_rows is not None and int(n_rows) != n_new:
            raise ArgumentError(f"Relation {r.name}: n_rows is {int(n_rows)} but F_new of {entity.name} has {n_new} rows (setNewObserved).")
        rows = "the rows of F_new"
    else:
        if n_rows is None and not len(ids):
            raise ArgumentError(f"Relation {r.name}: an empty table of known cells needs n_rows, {entity.name} has no F_new to count the new rows by (setNewObserved).")
        n_new = int(n_rows) if n_rows is not None else int(ids[:, mode - 1].max())
        rows = "n_rows"
    if len(ids) and (ids[:, mode - 1].min() < 1 or ids[:, mode - 1].max() > n_new):
        raise ArgumentError(f"Relation {r.name}: a known cell's id of {entity.name} is outside 1 ... {n_new}, {rows} (setNewObserved).")
    if len(ids) and (ids[:, other].min() < 1 or ids[:, other].max() > n_other):
        raise ArgumentError(f"Relation {r.name}: a known cell's id of {r.entities[other].name} is outside 1 ... {n_other} (setNewObserved).")
    if not np.all(np.isfinite(vals)):
        raise ArgumentError(f"Relation {r.name}: the value of a known cell must be finite (setNewObserved).")
    if len(ids) and len(np.unique(ids[:, 0] * (int(ids[:, 1].max()) + 1) + ids[:, 1])) != len(ids):
        raise ArgumentError(f"Relation {r.name}: a known cell is listed twice (setNewObserved).")
    return {"mode": int(mode), "ids": np.ascontiguousarray(ids, dtype=np.int64), "values": np.ascontiguousarray(vals, dtype=np.float64),
            "n_rows": n_new}


def _check_new_observed(r, world):
    """setNewObserved at build time: the same guards on the relation as it is now, and cells of setNewTest on the same entity"""
    m = r.model.new_observed
    entity = r.entities[m["mode"] - 1] if 1 <= m.get("mode", 0) <= len(r.entities) else None
    if entity is None:
        raise ArgumentError(f"Relation {r.name}: the entity of its known cells is not among its entities (setNewObserved).")
    _new_observed_guards(r, entity, build=True)
    r.model.new_observed = _new_observed_spec(r, m["mode"], np.asarray(m["ids"], dtype=np.int64).reshape(-1, 2),
                                              np.asarray(m["values"], dtype=np.float64), m.get("n_rows") if entity.new_rows is None else None)
    if r.model.new_test is not None and r.model.new_test.get("mode") != m["mode"]:
        raise ArgumentError(f"Relation {r.name}: its known cells (setNewObserved) are {entity.name}'s but its new cells (setNewTest) are another entity's.")
    refuse_ranks(r, "new_observed", world)


def check_new_rows(data, world=1):
    """what setNewRows / setNewTest / setNewObserved must still satisfy when macau() runs (models and features may have changed
    since); returns the relation whose new cells are predicted -- the first one -- or None"""
    for r in data.relations[1:]:
        if r.model.new_test is not None:
            raise ArgumentError(f"Relation {r.name} lists cells of new rows (setNewTest) but is not the first relation: macau() predicts new "
                                "rows for the first relation only.")
        if r.model.new_observed is not None:
            raise ArgumentError(f"Relation {r.name} lists known cells of new rows (setNewObserved) but is not the first relation: macau() "
                                "predicts new rows for the first relation only.")
    r = data.relations[0] if data.relations else None
    if r is not None and r.model.new_observed is not None:
        _check_new_observed(r, world)
    if r is None or r.model.new_test is None:
        return None
    m = r.model.new_test
    entity = r.entities[m["mode"] - 1] if 1 <= m.get("mode", 0) <= len(r.entities) else None
    if entity is None:
        raise ArgumentError(f"Relation {r.name}: the entity of its new cells is not among its entities (setNewTest).")
    _new_test_guards(r, entity, build=True)
    r.model.new_test = _new_test_spec(r, m["mode"], np.asarray(m["ids"], dtype=np.int64).reshape(-1, 2), np.asarray(m["values"], dtype=np.float64))
    refuse_ranks(r, "new_test", world)
    return r


def _censor_flags(r, censor):
    c = np.asarray(censor)
    if c.ndim != 1 or len(c) != r.data.nnz():
        raise ArgumentError(f"Relation {r.name} has {r.data.nnz()} training rows but {c.shape} censoring flags were given.")
    if not (np.issubdtype(c.dtype, np.integer) or c.dtype == np.bool_) or not bool(np.all((c == 0) | (c == 1) | (c == -1))):
        raise ArgumentError(f"Relation {r.name}: censoring flags must be the integers -1, 0 or +1.")
    return np.ascontiguousarray(c, dtype=np.int8)


def check_censored(r):
    """what a censored relation must still satisfy when a sampler is built on it (it may have been changed since setCensored)"""
    refuse(r, "censored", build=True)
    r.model.censor = _censor_flags(r, r.model.censor)


def setInterval(r, lower, upper):
    """Interval-censored noise model for a Gaussian relation (the reference takes every value as a measurement): training row k of
    r.data, in its current order, says only that the true value lies in [lower[k], upper[k]].  Either bound may be infinite;
    (-inf, +inf) says nothing.  lower[k] == upper[k] keeps the row a measurement.  macau() then samples a latent value for every
    row with lower < upper beside the rows: z ~ N(u'v + mean, 1 / alpha) truncated to the interval.  The stored value is where the
    latent starts, so it must lie inside its bounds.  Predictions, the test set and alpha (fixed, setPrecision or alpha_sample)
    stay what they are.  Call it AFTER the test split (assignToTest removes training rows; setTest does not)."""
    refuse(r, "interval")
    r.model.interval = _interval_bounds(r, lower, upper)
    r._dev = None
    return None


def setBinned(r, edges):
    """Values reported in bins: `edges` are the strictly increasing finite interior edges e_1 < ... < e_{K-1} of K bins, the first
    and the last of which are open (e_0 = -inf, e_K = +inf).  A stored value v lies in bin j when e_j <= v < e_{j+1}; every training
    row gets its bin's bounds (setInterval).  setBinned(rel, [1.5, 2.5, 3.5, 4.5]) is a 1 ... 5 rating."""
    e = _bin_edges(r, edges)
    full = np.concatenate([[-np.inf], e, [np.inf]])
    v = np.asarray(r.data.values, dtype=np.float64)
    if bool(np.any(np.isnan(v))):
        raise ArgumentError(f"Relation {r.name}: a NaN value lies in no bin.")
    j = np.searchsorted(e, v, side="right")          # the number of edges <= v: e_j <= v < e_{j+1}
    return setInterval(r, full[j], full[j + 1])


def setTestInterval(r, lower, upper):
    """What the held-out rows are records of, for the held-out log predictive density (macau(lpd=True)): row k of r.test_vec, in its
    current order, says that the true value lies in [lower[k], upper[k]], and is scored by the mass the model gives that interval.
    Either bound may be infinite (a censored test record is an interval with one infinite bound); lower[k] == upper[k] marks an
    exact cell, scored by the Gaussian density at its stored value.  The stored test value must lie inside its bounds.  Nothing
    but the LPD reads the bounds: predictions, RMSE and ROC stay what they are.  setTest and assignToTest replace the test
    table and drop the bounds: call this after them.  Not on a probit relation, whose 0/1 test values are scored by the probit
    likelihood."""
    refuse(r, "test_interval")
    r.model.test_interval = _interval_bounds(r, lower, upper, test=True)
    r.model.test_ordinal = None
    return None


def setTestBinned(r, edges):
    """Held-out values reported in bins: setBinned's edge rule (a stored value v lies in bin j when e_j <= v < e_{j+1}, the first
    and the last bin open) applied to the rows of r.test_vec (setTestInterval)."""
    e = _bin_edges(r, edges)
    full = np.concatenate([[-np.inf], e, [np.inf]])
    v = np.asarray(r.test_vec.values, dtype=np.float64)
    if bool(np.any(np.isnan(v))):
        raise ArgumentError(f"Relation {r.name}: a NaN test value lies in no bin.")
    j = np.searchsorted(e, v, side="right")
    return setTestInterval(r, full[j], full[j + 1])


ORDINAL_MIN_LEVELS, ORDINAL_MAX_LEVELS = 4, 16


def _ordinal_codes(r, values, K, what):
    v = np.asarray(values, dtype=np.float64)
    if not bool(np.all(np.isfinite(v))) or not bool(np.all(v == np.round(v))) or (len(v) and (v.min() < 1 or v.max() > K)):
        raise ArgumentError(f"Relation {r.name}: the {what} values of an ordinal relation must be the integers 1 ... {K}.")
    return np.ascontiguousarray(v, dtype=np.int8)


def _ordinal_bounds(codes, edges):
    """(n, 2) bounds of the levels `codes` under the interior edges e_1 .. e_{K-1}: setBinned's rule applied to the levels"""
    e = np.asarray(edges, dtype=np.float64)
    full = np.concatenate([[-np.inf], e, [np.inf]])
    j = np.searchsorted(e, np.asarray(codes, dtype=np.float64), side="right")
    return np.ascontiguousarray(np.stack([full[j], full[j + 1]], axis=1))


def setOrdinal(r, n_levels=None, step=0.1, sample_edges=True):
    """Ordinal probit noise model (Albert & Chib 1993; the cutpoint step of Cowles 1996): the training values are levels 1 ... K,
    4 <= K <= 16 (n_levels; by default the largest value), y = k iff e_{k-1} <= z < e_k for the latent z ~ N(u'v + mean, 1 / alpha)
    of the interval model.  e_1 = 1.5 and e_{K-1} = K - 1/2 are fixed, so that the mean, alpha and the predictions stay on the
    scale of the levels; the K - 3 edges between them start at k + 1/2 and macau() samples them, one Metropolis step per iteration
    with step size `step` adapted during the burn-in.  sample_edges=False keeps them where they start: setBinned(rel, [1.5, ...,
    K - 1/2]) exactly.  Everything the interval model refuses is refused here (relation features, rmse_train, more than one rank),
    and so are setProbit, setCensored and a setInterval / setBinned of the relation's own.  Call it AFTER the test split.  The
    edges' trace and the step size's burn-in belong to one macau() run: macau(engine=..., reset_model=False) does not continue a
    chain whose edges have moved, it is refused."""
    refuse(r, "ordinal")
    v = np.asarray(r.data.values, dtype=np.float64)
    if n_levels is None:
        if len(v) == 0 or not bool(np.all(np.isfinite(v))):
            raise ArgumentError(f"Relation {r.name}: the training values of an ordinal relation must be the integers 1 ... K.")
        n_levels = v.max()
    if not _number(n_levels) or n_levels != int(n_levels):
        raise ArgumentError(f"Relation {r.name}: n_levels must be an integer.")
    K = int(n_levels)
    if K == 3:
        raise ArgumentError(f"Relation {r.name}: with 3 levels both edges are fixed and nothing is left to sample: use setBinned(rel, [1.5, 2.5]).")
    if K < ORDINAL_MIN_LEVELS or K > ORDINAL_MAX_LEVELS:
        raise ArgumentError(f"Relation {r.name}: an ordinal relation has {ORDINAL_MIN_LEVELS} ... {ORDINAL_MAX_LEVELS} levels, not {K}.")
    step = float(step)
    if not (1e-8 <= step <= 10.0):
        raise ArgumentError(f"Relation {r.name}: step = {step} must lie in [1e-8, 10].")
    codes = _ordinal_codes(r, v, K, "training")
    edges = np.arange(1, K, dtype=np.float64) + 0.5
    b = _ordinal_bounds(codes, edges)
    r.model.interval = _interval_bounds(r, b[:, 0], b[:, 1])
    r.model.ordinal = {"K": K, "step": step, "sample_edges": bool(sample_edges)}
    r.model.ordinal_codes, r.model.ordinal_edges = codes, edges
    r.model.test_ordinal = None
    r._dev = None
    return None


def setTestOrdinal(r):
    """The held-out rows of an ordinal relation are levels too, for the held-out log predictive density (macau(lpd=True)): row k of
    r.test_vec is scored by the mass of its level's bin, between the edges of every posterior draw (with sample_edges=False: the
    fixed ones).  setTest and assignToTest replace the test table and drop this: call it after them, and after setOrdinal."""
    if r.model.ordinal is None:
        raise ArgumentError(f"Relation {r.name} is not ordinal: call setOrdinal first (or setTestBinned for fixed bins).")
    r.model.test_ordinal = _ordinal_codes(r, r.test_vec.values, r.model.ordinal["K"], "test")
    r.model.test_interval = None
    return None


def check_ordinal(r):
    """what an ordinal relation must still satisfy when a sampler is built on it (it may have been changed since setOrdinal); the
    chain starts from the edges k + 1/2"""
    refuse(r, "ordinal", build=True)
    o = r.model.ordinal
    K = int(o["K"])
    if K < ORDINAL_MIN_LEVELS or K > ORDINAL_MAX_LEVELS or not (1e-8 <= float(o["step"]) <= 10.0):
        raise ArgumentError(f"Relation {r.name}: an ordinal relation has {ORDINAL_MIN_LEVELS} ... {ORDINAL_MAX_LEVELS} levels and a step in [1e-8, 10].")
    r.model.ordinal_codes = _ordinal_codes(r, r.data.values, K, "training")
    r.model.ordinal_edges = np.arange(1, K, dtype=np.float64) + 0.5
    b = _ordinal_bounds(r.model.ordinal_codes, r.model.ordinal_edges)
    r.model.interval = _interval_bounds(r, b[:, 0], b[:, 1])
    if r.model.test_ordinal is not None:
        r.model.test_ordinal = _ordinal_codes(r, r.test_vec.values, K, "test")


def setWaic(r, on=True, pointwise=False):
    """macau() scores the TRAINING cells of this relation (the first of its RelationData) by the widely applicable information
    criterion: result["WAIC"] = {"waic", "elpd", "lppd", "p_waic", "se", "n_high", "n"}, an estimate of the expected log predictive
    density that needs no held-out cells.  Every training row is scored as the kind of record its noise model says it is (a
    measurement, a 0/1 value, a censored or interval value, a level between this draw's edges).  pointwise=True also returns
    result["WAIC"]["pointwise"], the training ids with every cell's lppd and p_waic.  on=False takes it back.  Nothing of the chain
    changes; call it at any time before macau()."""
    if not isinstance(on, (bool, np.bool_)) or not isinstance(pointwise, (bool, np.bool_)):
        raise ArgumentError(f"Relation {r.name}: setWaic takes on = true / false and pointwise = true / false.")
    if pointwise and not on:
        raise ArgumentError(f"Relation {r.name}: setWaic(on = false) returns no pointwise table.")
    if on:
        refuse(r, "waic")
    r.model.waic = {"pointwise": bool(pointwise)} if on else None
    return None


def setDiagnostics(r, on=True, pointwise=False, rhat_cut=1.1, ess_cut=100.0):
    """macau() keeps every posterior draw of the predictions of this relation's TEST cells (the first relation of its RelationData) on
    the device and says whether the draws can be trusted: per test cell, and for the draw's sum of squared test errors ("sse") and
    a sampled precision ("alpha"), the split R-hat, the effective sample size by Geyer's initial monotone sequence and the Monte Carlo
    standard error of the posterior mean.  result["diagnostics"] = {"n_draws", "max_rhat", "min_ess",
    "n_rhat_high" (cells with R-hat > rhat_cut), "n_ess_low" (cells with ESS < ess_cut), "n_constant" (cells whose draws do not vary:
    they have no figures and are in no other count), "rhat_cut", "ess_cut", "scalars": {"sse": {"rhat", "ess", "mcse"}, ...}}.
    pointwise=True also adds the columns rhat, ess and mcse to result["predictions"].  The plane takes psamples x numTest doubles of
    device memory.  on=False takes it back.  Nothing of the chain changes; call it at any time before macau()."""
    if not isinstance(on, (bool, np.bool_)) or not isinstance(pointwise, (bool, np.bool_)):
        raise ArgumentError(f"Relation {r.name}: setDiagnostics takes on = true / false and pointwise = true / false.")
    if pointwise and not on:
        raise ArgumentError(f"Relation {r.name}: setDiagnostics(on = false) returns no pointwise columns.")
    cuts = []
    for name, cut, least in (("rhat_cut", rhat_cut, 1.0), ("ess_cut", ess_cut, 0.0)):
        if isinstance(cut, (bool, np.bool_)) or not isinstance(cut, (int, float, np.integer, np.floating)) or not np.isfinite(cut) or cut < least:
            raise ArgumentError(f"Relation {r.name}: {name} = {cut} must be a finite number, at least {least:g} (setDiagnostics).")
        cuts.append(float(cut))
    if on:
        refuse(r, "diagnostics")
    r.model.diagnostics = {"pointwise": bool(pointwise), "rhat_cut": cuts[0], "ess_cut": cuts[1]} if on else None
    return None


def _waic_bounds(r):
    """the bounds (lo, hi) of every training row by its kind of record, for WAIC: None for a Gaussian and for a probit relation (the
    density at the stored value; the probit link); censoring flags 0 -> (y, y), +1 -> (y, +inf), -1 -> (-inf, y); interval bounds
    as they stand (lo == hi a measurement); an ordinal relation's levels between the edges k + 1/2 (sampled edges: where every
    chain starts; macau() then refreshes them with every draw).  The relation's own checks run first."""
    m, kind = r.model, noise_kind(r)
    if kind == "censored":
        check_censored(r)
        y = np.asarray(r.data.values, dtype=np.float64)
        return np.ascontiguousarray(np.stack([np.where(m.censor < 0, -np.inf, y), np.where(m.censor > 0, np.inf, y)], axis=1))
    if kind == "ordinal":
        check_ordinal(r)
        check_interval(r)
        return _ordinal_bounds(m.ordinal_codes, np.arange(1, m.ordinal["K"]) + 0.5)
    if kind == "interval":
        check_interval(r)
        return np.ascontiguousarray(m.interval, dtype=np.float64)
    return None


def _bin_edges(r, edges):
    e = np.asarray(edges, dtype=np.float64)
    if e.ndim != 1 or len(e) == 0 or not bool(np.all(np.isfinite(e))) or not bool(np.all(np.diff(e) > 0)):
        raise ArgumentError(f"Relation {r.name}: bin edges must be a non-empty list of finite, strictly increasing numbers.")
    return e


def check_test_interval(r):
    """what the test bounds must still satisfy when macau(lpd=True) reads them (they may have been changed since setTestInterval)"""
    b = np.asarray(r.model.test_interval)
    if b.ndim != 2 or b.shape[1] != 2:
        raise ArgumentError(f"Relation {r.name}: test bounds must be a (numTest, 2) array, not {b.shape}.")
    refuse(r, "test_interval", build=True)
    r.model.test_interval = _interval_bounds(r, b[:, 0], b[:, 1], test=True)


def _interval_bounds(r, lower, upper, test=False):
    """(n, 2) float64 bounds of the training rows (test: of the rows of test_vec) after the checks they must pass"""
    n = len(r.test_vec) if test else r.data.nnz()
    what = "test" if test else "training"
    try:
        lo, hi = np.asarray(lower, dtype=np.float64), np.asarray(upper, dtype=np.float64)
    except (TypeError, ValueError):
        raise ArgumentError(f"Relation {r.name}: interval bounds must be numbers.")
    if lo.ndim != 1 or hi.ndim != 1 or len(lo) != n or len(hi) != n:
        raise ArgumentError(f"Relation {r.name} has {n} {what} rows but {lo.shape} lower and {hi.shape} upper bounds were given.")
    if bool(np.any(np.isnan(lo))) or bool(np.any(np.isnan(hi))):
        raise ArgumentError(f"Relation {r.name}: an interval bound is NaN (use -inf / +inf for an open side).")
    if bool(np.any(lo > hi)):
        raise ArgumentError(f"Relation {r.name}: a lower bound is above its upper bound (row {int(np.argmax(lo > hi)) + 1}).")
    v = np.asarray(r.test_vec.values if test else r.data.values, dtype=np.float64)
    out = ~((lo <= v) & (v <= hi))
    if bool(np.any(out)):
        if test:
            raise ArgumentError(f"Relation {r.name}: the stored value of test row {int(np.argmax(out)) + 1} lies outside its bounds.")
        raise ArgumentError(f"Relation {r.name}: the stored value of row {int(np.argmax(out)) + 1} lies outside its bounds; it is where "
                            "the latent value starts.")
    return np.ascontiguousarray(np.stack([lo, hi], axis=1))


def check_interval(r):
    """what an interval relation must still satisfy when a sampler is built on it (it may have been changed since setInterval)"""
    refuse(r, "interval" if r.model.ordinal is None else "ordinal", build=True)       # (an ordinal relation has bounds too)
    b = np.asarray(r.model.interval)
    if b.ndim != 2 or b.shape[1] != 2:
        raise ArgumentError(f"Relation {r.name}: interval bounds must be an (n, 2) array, not {b.shape}.")
    r.model.interval = _interval_bounds(r, b[:, 0], b[:, 1])


# what a sampler checks on a relation before it is built, per option that is present, in the registry's order (the ordinal check
# rebuilds the bounds)
_CHECKS = {"dense": check_dense, "probit": check_probit, "censored": check_censored, "ordinal": check_ordinal, "interval": check_interval,
           "robust": check_robust, "weights": check_robust, "entity_noise": check_entity_noise, "logit": check_pg, "counts": check_pg,
           "background": check_background, "recommend": check_recommend, "acquire": check_acquire, "bias": check_bias}


def check_model(r, world=1):
    """every check_* that relation r's options ask for; world > 1: none of them runs on several ranks"""
    for opt in present(r, RELATION):
        if opt.key in _CHECKS:
            _CHECKS[opt.key](r)
            refuse_ranks(r, opt.key, world)


def assignToTest(r, test, rng=None):
    """assignToTest!(r, ntest::Int) / assignToTest!(r, test_id::Vector) (RelationData.jl:191-212); ids 1-based"""
    if r.model.interval is not None:
        raise ArgumentError(f"Relation {r.name} has interval bounds, one pair per training row: call assignToTest before setInterval.")
    if r.model.censor is not None:
        raise ArgumentError(f"Relation {r.name} has censoring flags, one per training row: call assignToTest before setCensored.")
    if r.model.weights is not None:
        raise ArgumentError(f"Relation {r.name} has observation weights, one per training row: call assignToTest before setWeights.")
    if np.isscalar(test):
        rng = rng if rng is not None else np.random.default_rng()
        test_id = rng.choice(r.data.nnz(), size=int(test), replace=False) + 1
    else:
        test_id = np.asarray(test, dtype=np.int64)
    rows0 = test_id - 1
    r.test_vec = TestVec(r.data.ids[rows0, :], r.data.values[rows0], r.data.names)
    r.data = r.data.removeSamples(test_id)
    r.test_label = r.test_vec.values < r.class_cut
    r.model.test_interval = None
    r.model.test_ordinal = None
    if hasFeatures(r):
        r.test_F = feat.take_rows(r.F, rows0)
        train = np.ones(feat.feature_shape(r.F)[0], dtype=bool)
        train[rows0] = False
        r.F = feat.subset_rows(r.F, train)
    r._dev = None
    return None


def setTest(r, test, test_feat=None):
    """setTest!(r, test_df[, test_feat]) / setTest!(r, test_mat::SparseMatrixCSC) (RelationData.jl:214-252)"""
    if hasattr(test, "tocsc"):
        if hasFeatures(r):
            raise ArgumentError("Cannot add test set using SparseMatrixCSC when relation has features. Use DataFrame instead.")
        if r.data.ids.shape[1] != 2:
            raise ArgumentError("Relation must have 2 entities if using SparseMatrixCSC for test set.")
        ids, vals = _table_from_sparse(test)
    else:
        ids, vals, _ = _split_table(test)
        if hasFeatures(r) and test_feat is None:
            raise ArgumentError("Relation has features, please supply features with test data:\nsetTest(rel, test_df, test_features")
        if hasFeatures(r) and feat.feature_shape(r.F)[1] != feat.feature_shape(test_feat)[1]:
            raise ArgumentError("The test_feat must have the same number of columns as relation.F.")
        if hasFeatures(r) and feat.feature_shape(test_feat)[0] != len(vals):
            raise ArgumentError("The test_feat must have the same number of rows as test_df.")
        if ids.shape[1] + 1 != r.data.ids.shape[1] + 1:
            raise ArgumentError("The number of columns in test_df must be the same as in relation.data.df.")
    if r.model.probit and not _is_binary(vals):
        raise ArgumentError(f"Relation {r.name} has the probit noise model: its test values must be 0 or 1.")
    if r.model.pg is not None and r.model.pg["model"] == "logit" and not _is_binary(vals):
        raise ArgumentError(f"Relation {r.name} has the logit noise model: its test values must be 0 or 1.")
    if r.model.pg is not None and r.model.pg["model"] == "counts" and not _is_count(vals):
        raise ArgumentError(f"Relation {r.name} has the count noise model: its test values must be the integers 0 ... 2^31.")
    r.test_vec = TestVec(ids, vals, r.data.names)
    r.test_label = r.test_vec.values < r.class_cut
    r.model.test_interval = None
    r.model.test_ordinal = None
    if hasFeatures(r):
        r.test_F = test_feat
    r._dev = None
    return None


class RelationData:
    """RelationData (RelationData.jl:254-311).

    RelationData()                         empty
    RelationData(relation)                 one relation with entities already attached (:307-311)
    RelationData(M; feat1, feat2, ...)     two-entity matrix relation from a scipy sparse matrix or an IndexedDF (:260-274, 293-305)
    RelationData(table; rname, ...)        N-mode relation from a table, one entity per id column (:276-286)
    """

    def __init__(self, data=None, feat1=None, feat2=None, entity1="E1", entity2="E2", relation="Rel", ntest=0,
                 class_cut=math.log10(200), alpha=5.0, alpha_sample=False, lambda_beta=1.0, rname="R1"):
        self.entities = []
        self.relations = []
        if data is None:
            return
        if isinstance(data, Relation):
            addRelation(self, data)
            return
        if hasattr(data, "tocsc"):
            ids, vals = _table_from_sparse(data)
            data = IndexedDF((ids, vals), [int(data.shape[0]), int(data.shape[1])], names=["row", "col", "value"])
        if isinstance(data, IndexedDF):
            if len(data.dims) != 2:
                raise ArgumentError("RelationData(::IndexedDF) builds a two-entity relation")
            r = Relation(data, relation, [], class_cut, 1.0 if alpha_sample else alpha)
            r.model.alpha_sample = bool(alpha_sample)
            e1 = Entity(entity1, F=feat1, lambda_beta=lambda_beta)
            e2 = Entity(entity2, F=feat2, lambda_beta=lambda_beta)
            e1.relations, e1.count = [r], r.size(1)
            e2.relations, e2.count = [r], r.size(2)
            if not feat.isempty(feat1) and feat.feature_shape(feat1)[0] != r.size(1):
                raise ArgumentError(f"Number of rows in feat1 {feat.feature_shape(feat1)[0]} must equal number of rows in the relation {r.size(1)}")
            if not feat.isempty(feat2) and feat.feature_shape(feat2)[0] != r.size(2):
                raise ArgumentError(f"Number of rows in feat2 {feat.feature_shape(feat2)[0]} must equal number of columns in the relation {r.size(2)}")
            r.entities = [e1, e2]
            self.entities = [e1, e2]
            self.relations = [r]
            if ntest:
                assignToTest(r, int(ntest))
            return
        # generic table: one entity per id column, named after the column
        ids, vals, names = _split_table(data)
        dims = [int(ids[:, i].max()) for i in range(ids.shape[1])]
        names = names or [f"E{i + 1}" for i in range(ids.shape[1])] + ["value"]
        idf = IndexedDF((ids, vals), dims, names=names)
        r = Relation(idf, rname, [], class_cut, alpha)
        self.relations.append(r)
        for d in range(len(dims)):
            en = Entity(names[d])
            en.relations, en.count = [r], idf.size(d + 1)
            self.entities.append(en)
            r.entities.append(en)

    def __repr__(self):
        out = ["[Relations]"]
        for r in self.relations:
            a = "sample" if r.model.alpha_sample else f"{r.model.alpha:.2f}"
            s = f"{r.name:>10s}: {'--'.join(e.name for e in r.entities)}, #known = {numData(r)}, #test = {numTest(r)}, α = {a}"
            if hasFeatures(r):
                s += f", #feat = {feat.feature_shape(r.F)[1]}"
            out.append(s)
        out.append("[Entities]")
        for en in self.entities:
            out.append(f"{en.name:>10s}: " + repr(en).split(": ", 1)[1])
        return "\n".join(out)


def addRelation(rd, r):
    """addRelation!(rd, r) (RelationData.jl:387-409).

    The reference registers r on an entity only when `! any(en.relations .!= r)` (:404), which drops every relation
    after the first on a shared entity although sample_user2 (sampling.jl:270-283) sums over all of them; the evident
    intent (register unless already present) is implemented here -- see DESIGN.md note N1."""
    if len(r.size()) != len(r.entities):
        raise ArgumentError(f"Relation has {len(r.entities)} entities but its data implies {r.size()}.")
    rd.relations.append(r)
    for i, en in enumerate(r.entities):
        if en.count == 0:
            en.count = r.size(i + 1)
        elif en.count != r.size(i + 1):
            raise ArgumentError(f"Entity {en.name} has {en.count} instances, relation {r.name} has data for {r.size(i + 1)}.")
        if not any(e is en for e in rd.entities):
            rd.entities.append(en)
        if not any(x is r for x in en.relations):
            en.relations.append(r)
    return None


def normalizeFeatures(entity):
    """normalizeFeatures!(entity) (RelationData.jl:450-454): unit column norms"""
    F = entity.F
    if hasattr(F, "tocsc"):
        import scipy.sparse as sp
        d = np.sqrt(np.asarray(F.multiply(F).sum(axis=0)).ravel())
        entity.F = (F @ sp.diags(1.0 / d)).tocsr()
    else:
        F = np.asarray(F, dtype=np.float64)
        entity.F = F / np.sqrt((F ** 2).sum(axis=0))[None, :]


def normalizeRows(entity):
    """normalizeRows!(entity) (RelationData.jl:456-459): unit row norms"""
    F = entity.F
    if hasattr(F, "tocsc"):
        import scipy.sparse as sp
        d = np.sqrt(np.asarray(F.multiply(F).sum(axis=1)).ravel())
        entity.F = (sp.diags(1.0 / d) @ F).tocsr()
    else:
        F = np.asarray(F, dtype=np.float64)
        entity.F = F / np.sqrt((F ** 2).sum(axis=1))[:, None]
