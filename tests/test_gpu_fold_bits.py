"""The fold of background cells and dense relations into the prior (DESIGN.md sections 20 and 25; csrc/prior_fold.h) is written once for
both families.  Sharing it may not move a bit: the refined solve, the padding and the fixed order of every sum are why these kernels give
the same bits on a rerun, and the tests beside this one compare against numpy and math.fsum with tolerances, which a reordered sum
passes.  Here the tolerance is 0.

The reference is tests/golden/fold_bits.npz: the build BEFORE the fold was shared, run on the inputs below and recorded by
`python tests/test_gpu_fold_bits.py --record` on an MI355X.  Only the public ABI and macau() are used, so the same file runs on either
build.  Every case also records a digest of its generated inputs, and the test refuses a fixture that does not match them.  Inputs are
made with elementwise operations alone (no BLAS), so that they are the same bits wherever they are generated.  A case's outputs are
stored whole for D <= 17, where a difference needs to be read, and as their SHA-256 digest above.  Of the prior pack the fixture keeps
the D doubles that are computed (Lambda_eff mu_eff) and the digest of the whole: the rest is a rearranged image of Lambda_out.

Cases:
  bdf_background_prior   D in 3, 16, 17, 32, 33, 64 (every DP instantiation, both sides of its edge) x one and three terms (the second of
                         three reads its alpha through alpha_dev) x a shared mean with the prior pack (Lambda_out, mu_out, the pack,
                         alpha_rows_out) and per-row means at N = 19, two 16-row tiles with the second partial (Lambda_out, mu_out,
                         alpha_rows_out)
  bdf_dense_prior        the same D, N = 19 x dense, dense + background, background + dense + dense (the last term's alpha through
                         alpha_dev) x shared and per-row mu: Lambda_out, mu_out, alpha_rows_out
  bdf_background_sse     D in 7, 32, 64 x 9 pairs (one workgroup) and 8 * 32 * 5 + 3 pairs (six workgroups) x with and without weights
  bdf_dense_sse          D in 7, 32, 64 at N = 37 x with and without holes_r2: the one double
  whole chains           macau() with burnin 3, psamples 3 on a 23 x 17 relation, D in 5 and 32, natively and step by step
                         (BDF_NO_NATIVE), alpha sampled: (a) setBackground; (b) setDense with holes; (c) an entity that is mode 0 of a
                         dense and of a background relation; (d) setBackground on an entity with features, so per-row means.  Every
                         entity's final sample and every relation's final alpha.
"""
import ctypes as C
import hashlib
import os
import sys
import textwrap

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
GOLDEN = os.path.join(HERE, "golden", "fold_bits.npz")
SEED = 1234
DS = [3, 16, 17, 32, 33, 64]
SSE_DS = [7, 32, 64]
N_ROWS = 19
FULL_UP_TO = 17                      # outputs are stored whole up to this D, as a digest above
DENSE_LISTS = ["dense", "dense+background", "background+dense+dense"]
BG_SSE_PAIRS = [9, 8 * 32 * 5 + 3]
CHAIN_CONFIGS = ["background", "holes", "shared", "features"]
CHAIN_DS = [5, 32]


def _p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _sha(arrays):
    h = hashlib.sha256()
    for a in arrays:
        a = np.ascontiguousarray(a)
        h.update(str(a.dtype).encode() + str(a.shape).encode())
        h.update(a.tobytes())
    return np.frombuffer(h.digest(), dtype=np.uint8).copy()


def _pack(D, outputs, prior_pack=None):
    """what the fixture keeps of a case: the outputs end to end, or their digest"""
    outputs = [np.ascontiguousarray(o, dtype=np.float64) for o in outputs]
    if prior_pack is not None:
        outputs += [prior_pack] if D > FULL_UP_TO else [prior_pack[:D], _sha([prior_pack]).astype(np.float64)]
    assert all(np.isfinite(o).all() for o in outputs), "an output is not finite"
    if D <= FULL_UP_TO:
        return np.concatenate([o.ravel() for o in outputs])
    return _sha(outputs)


def _spd(rng, D):
    """a prior precision, diagonally dominant, from elementwise operations alone"""
    A = rng.random((D, D)) - 0.5
    return (A + A.T) * (0.5 / D) + np.diag(2.0 + rng.random(D))


def _sums(c2, D, F_t):
    """bdf_hyper_sums of F's rows -> (s, G)"""
    from bdf_amd._lib import check, lib
    s_t, G_t = c2.zeros(D), c2.zeros(D, D)
    check(lib().bdf_hyper_sums(c2.handle, D, F_t.shape[0], _p(F_t), None, _p(s_t), _p(G_t)))
    return s_t, G_t


# ---- the two priors ------------------------------------------------------------------------------------------------------------------------
def _prior_inputs(seed, D, kinds):
    rng = np.random.default_rng(seed)
    inp = {"Lam": _spd(rng, D), "mu": rng.standard_normal(D), "mus": rng.standard_normal((N_ROWS, D))}
    for k, kind in enumerate(kinds):
        inp["V%d" % k] = 0.5 * rng.standard_normal((11 + 6 * k, D))
        inp["alpha%d" % k] = np.array(1.7 - 0.4 * k)
        if kind == "dense":
            inp["C%d" % k] = rng.standard_normal((N_ROWS, D))
        else:
            inp["c0%d" % k], inp["rb%d" % k] = np.array(0.3 - 0.05 * k), np.array(-0.5 + 0.2 * k)
    return inp


def _background_prior(B, c2, D, n_terms, per_row):
    from bdf_amd._lib import BackgroundTerm, check, lib
    kinds = ["background"] * n_terms
    inp = _prior_inputs(5000 + 10 * D + n_terms, D, kinds)
    keep, bg = [], (BackgroundTerm * n_terms)()
    for k in range(n_terms):
        s_t, G_t = _sums(c2, D, c2.tensor(inp["V%d" % k]))
        bg[k].sum, bg[k].gram, bg[k].weight, bg[k].resid = s_t.data_ptr(), G_t.data_ptr(), float(inp["c0%d" % k]), float(inp["rb%d" % k])
        bg[k].alpha = float(inp["alpha%d" % k])
        if k == 1:                                       # read through alpha_dev: the argument is then not looked at
            a_t = c2.tensor([float(inp["alpha%d" % k])])
            bg[k].alpha, bg[k].alpha_dev = 123.0, a_t.data_ptr()
            keep.append(a_t)
        keep += [s_t, G_t]
    Lam_t, mu_t = c2.tensor(inp["Lam"]), c2.tensor(inp["mus"] if per_row else inp["mu"])
    Le_t, me_t, ar_t = c2.zeros(D, D), (c2.zeros(N_ROWS, D) if per_row else c2.zeros(D)), c2.zeros(n_terms)
    pk_t = None if per_row else c2.zeros(lib().bdf_prior_pack_doubles(D))
    check(lib().bdf_background_prior(c2.handle, D, N_ROWS, n_terms, bg, _p(mu_t), int(per_row), _p(Lam_t), _p(Le_t), _p(me_t), _p(pk_t), _p(ar_t)))
    c2.sync()
    return _pack(D, [t.cpu().numpy() for t in (Le_t, me_t, ar_t)], None if per_row else pk_t.cpu().numpy()), _sha([inp[k] for k in sorted(inp)])


def _dense_prior(B, c2, D, kinds, per_row):
    from bdf_amd._lib import DenseTerm, check, lib
    kinds = kinds.split("+")
    inp = _prior_inputs(6000 + 10 * D + len(kinds), D, kinds)
    keep, dt = [], (DenseTerm * len(kinds))()
    for k, kind in enumerate(kinds):
        s_t, G_t = _sums(c2, D, c2.tensor(inp["V%d" % k]))
        dt[k].gram, dt[k].alpha = G_t.data_ptr(), float(inp["alpha%d" % k])
        if kind == "dense":
            C_t = c2.tensor(inp["C%d" % k])
            dt[k].C, dt[k].weight = C_t.data_ptr(), 1.0
            keep.append(C_t)
        else:
            dt[k].sum, dt[k].weight, dt[k].resid = s_t.data_ptr(), float(inp["c0%d" % k]), float(inp["rb%d" % k])
        if k == len(kinds) - 1 and k > 0:
            a_t = c2.tensor([float(inp["alpha%d" % k])])
            dt[k].alpha, dt[k].alpha_dev = 123.0, a_t.data_ptr()
            keep.append(a_t)
        keep += [s_t, G_t]
    Lam_t, mu_t = c2.tensor(inp["Lam"]), c2.tensor(inp["mus"] if per_row else inp["mu"])
    Le_t, me_t, ar_t = c2.zeros(D, D), c2.zeros(N_ROWS, D), c2.zeros(len(kinds))
    check(lib().bdf_dense_prior(c2.handle, D, N_ROWS, len(kinds), dt, _p(mu_t), int(per_row), _p(Lam_t), _p(Le_t), _p(me_t), _p(ar_t)))
    c2.sync()
    return _pack(D, [t.cpu().numpy() for t in (Le_t, me_t, ar_t)]), _sha([inp[k] for k in sorted(inp)])


# ---- the two sums over all cells -------------------------------------------------------------------------------------------------------
def _background_sse(B, c2, D, n_pairs, weights):
    from bdf_amd._lib import check, lib
    N, M = 37, 41
    rng = np.random.default_rng(7000 + 10 * D + n_pairs)
    ids = np.stack([rng.integers(1, N + 1, n_pairs), rng.integers(1, M + 1, n_pairs)], axis=1).astype(np.int64)
    y, w = rng.standard_normal(n_pairs), 0.5 + rng.random(n_pairs)
    U, V = 0.5 * rng.standard_normal((N, D)), 0.5 * rng.standard_normal((M, D))
    mean, value, c0 = 0.25, -0.5, 0.3
    ft = [c2.tensor(U), c2.tensor(V)]
    pairs = B.DevicePairs(c2, ids, y)
    sU, gU = _sums(c2, D, ft[0])
    sV, gV = _sums(c2, D, ft[1])
    w_t = c2.tensor(w) if weights else None
    out = c2.tensor([np.nan])
    facs = (C.c_void_p * 2)(*[t.data_ptr() for t in ft])
    check(lib().bdf_background_sse(c2.handle, pairs.handle, D, facs, mean, _p(w_t), value, c0, _p(sU), _p(gU), _p(sV), _p(gV), N, M, _p(out)))
    c2.sync()
    got = out.cpu().numpy()
    pairs.close()
    return _pack(0, [got]), _sha([ids, y, w, U, V])


def _dense_sse(B, c2, D, holes):
    from bdf_amd._lib import check, lib
    N, M = 37, 29
    rng = np.random.default_rng(8000 + D)
    U, V, Cm = 0.5 * rng.standard_normal((N, D)), 0.5 * rng.standard_normal((M, D)), rng.standard_normal((N, D))
    r2, h2 = 1000.0 + rng.random(), 10.0 * rng.random()
    U_t, C_t = c2.tensor(U), c2.tensor(Cm)
    _, gU = _sums(c2, D, U_t)
    _, gV = _sums(c2, D, c2.tensor(V))
    h_t = c2.tensor([h2, 0.0, 0.0, 0.0]) if holes else None
    out = c2.tensor([np.nan])
    check(lib().bdf_dense_sse(c2.handle, D, N, _p(U_t), _p(C_t), _p(gU), _p(gV), r2, _p(h_t), _p(out)))
    c2.sync()
    return _pack(0, [out.cpu().numpy()]), _sha([U, V, Cm, np.array([r2, h2])])


# ---- whole chains ------------------------------------------------------------------------------------------------------------------------
CHILD = textwrap.dedent('''
    import sys
    import numpy as np
    sys.path.insert(0, %r); sys.path.insert(0, %r)
    import bdf_amd as B
    from test_gpu_fold_bits import chain_inputs
    out, d = sys.argv[1], {}
    for config in %r:
        for D in %r:
            inp = chain_inputs(config)
            N, M, W = 23, 17, 11
            F = inp["F"] if config == "features" else None
            u, v = B.Entity("u", F=F), B.Entity("v")
            rels = []
            if config in ("holes", "shared"):
                rel = B.denseRelation(inp["Y"], "panel", [u, v], alpha=2.0)
                if config == "holes":
                    B.assignToTest(rel, inp["held"])
            else:
                ids, y = inp["ids"], inp["y"]
                rel = B.Relation({"u": ids[:, 0], "v": ids[:, 1], "y": y}, "plays", [u, v], alpha=2.0, dims=[N, M])
                B.setBackground(rel, 0.3, -0.5)
            rels.append(rel)
            rd = B.RelationData(rel)
            if config == "shared":
                ids, y = inp["ids2"], inp["y2"]
                r2 = B.Relation({"u": ids[:, 0], "w": ids[:, 1], "y": y}, "side", [u, B.Entity("w")], alpha=1.5, dims=[N, W])
                B.setBackground(r2, 0.3, -0.5)
                B.addRelation(rd, r2)
                rels.append(r2)
            for r in rels:
                r.model.alpha_sample = True
            B.macau(rd, num_latent=D, burnin=3, psamples=3, verbose=False, seed=91)
            key = "%%s_D%%d_" %% (config, D)
            d[key + "native"] = np.array(int(rd._engine.native))
            for k, en in enumerate(rd.entities):
                d[key + "S%%d" %% k] = np.ascontiguousarray(en.model.sample.T)
            d[key + "alpha"] = np.array([r.model.alpha for r in rels])
            rd._engine.close()
    np.savez(out, **d)
''') % (ROOT, HERE, CHAIN_CONFIGS, CHAIN_DS)


def _table(rng, N, M):
    """a rank-3 table plus noise, the rank-one pieces added one after the other (no BLAS)"""
    a, b = rng.standard_normal((N, 3)), rng.standard_normal((M, 3))
    Y = 0.3 * rng.standard_normal((N, M)) + 0.7
    for k in range(3):
        Y = Y + a[:, k, None] * b[None, :, k]
    return Y


def _listing(rng, N, M, n):
    cells = np.sort(rng.choice(N * M, size=n, replace=False))
    return np.stack([cells // M + 1, cells % M + 1], axis=1).astype(np.int64), 1.0 + 4.0 * rng.random(n)


def chain_inputs(config):
    rng = np.random.default_rng(9000 + CHAIN_CONFIGS.index(config))
    N, M, W = 23, 17, 11
    inp = {}
    if config in ("holes", "shared"):
        inp["Y"] = _table(rng, N, M)
        if config == "holes":
            inp["held"] = np.sort(rng.choice(N * M, size=78, replace=False)) + 1
        else:
            inp["ids2"], inp["y2"] = _listing(rng, N, W, 60)
    else:
        inp["ids"], inp["y"] = _listing(rng, N, M, 90)
        if config == "features":
            inp["F"] = rng.standard_normal((N, 4))
    return inp


def _chain_outputs(ch, config, D):
    key = "%s_D%d_" % (config, D)
    names = sorted(k for k in ch if k.startswith(key + "S")) + [key + "alpha"]
    return int(ch[key + "native"]), _pack(D, [ch[k] for k in names]), _sha([v for _, v in sorted(chain_inputs(config).items())])


# ---- the cases, by key ------------------------------------------------------------------------------------------------------------------
def _direct_cases():
    """key -> (runner, arguments) of every case that is one call of the C ABI"""
    cases = {}
    for D in DS:
        for n in (1, 3):
            for per_row in (False, True):
                cases["bgprior_D%d_%dterms_%s" % (D, n, "rowmeans" if per_row else "shared")] = (_background_prior, (D, n, per_row))
        for kinds in DENSE_LISTS:
            for per_row in (False, True):
                cases["denseprior_D%d_%s_%s" % (D, kinds, "rowmeans" if per_row else "shared")] = (_dense_prior, (D, kinds, per_row))
    for D in SSE_DS:
        for n in BG_SSE_PAIRS:
            for weights in (False, True):
                cases["bgsse_D%d_%dpairs_%s" % (D, n, "weights" if weights else "unit")] = (_background_sse, (D, n, weights))
        for holes in (False, True):
            cases["densesse_D%d_%s" % (D, "holes" if holes else "full")] = (_dense_sse, (D, holes))
    return cases


DIRECT = _direct_cases()


@pytest.fixture(scope="module")
def golden():
    with np.load(GOLDEN) as z:
        g = {k: z[k] for k in z.files}
    return g, {k.decode(): d for k, d in zip(g["input_keys"], g["input_digests"])}


@pytest.fixture(scope="module")
def c2(B):
    c = B.Context(seed=SEED)
    yield c
    c.close()


def _compare(golden, key, got, digest):
    g, inputs = golden
    assert np.array_equal(inputs[key], digest), "the generated inputs are not the recorded ones: the fixture does not apply"
    exp = g[key]
    if got.dtype == np.float64:
        print("%s: %d doubles, max |difference| %.3e" % (key, got.size, float(np.max(np.abs(got - exp))) if got.shape == exp.shape else np.inf))
    assert got.dtype == exp.dtype and got.shape == exp.shape and np.array_equal(got, exp), key


@pytest.mark.parametrize("key", sorted(DIRECT))
def test_fold_keeps_the_bits(B, c2, golden, key):
    run, args = DIRECT[key]
    got, digest = run(B, c2, *args)
    _compare(golden, key, got, digest)


@pytest.fixture(scope="module")
def chains():
    from both_paths import child
    return child(CHILD, no_native=False), child(CHILD, no_native=True)


@pytest.mark.parametrize("no_native", [0, 1])
@pytest.mark.parametrize("D", CHAIN_DS)
@pytest.mark.parametrize("config", CHAIN_CONFIGS)
def test_chains_keep_the_bits(chains, golden, config, D, no_native):
    native, got, digest = _chain_outputs(chains[no_native], config, D)
    assert native == 1 - no_native
    _compare(golden, "chain_%s_D%d_%s" % (config, D, "step" if no_native else "native"), got, digest)


def _record():
    sys.path.insert(0, ROOT)
    sys.path.insert(0, HERE)
    import bdf_amd as B
    from both_paths import child
    c = B.Context(seed=SEED)
    out, digests = {}, {}
    for key in sorted(DIRECT):
        run, args = DIRECT[key]
        out[key], digests[key] = run(B, c, *args)
    c.close()
    for no_native in (0, 1):
        ch = child(CHILD, no_native=bool(no_native))
        for config in CHAIN_CONFIGS:
            for D in CHAIN_DS:
                key = "chain_%s_D%d_%s" % (config, D, "step" if no_native else "native")
                native, out[key], digests[key] = _chain_outputs(ch, config, D)
                assert native == 1 - no_native, key
    keys = sorted(digests)
    out["input_keys"], out["input_digests"] = np.array(keys, dtype="S"), np.stack([digests[k] for k in keys])
    dst = sys.argv[2] if len(sys.argv) > 2 else GOLDEN
    np.savez(dst, **out)
    print("recorded %d cases, %d bytes -> %s" % (len(keys), os.path.getsize(dst), dst))


if __name__ == "__main__" and len(sys.argv) > 1 and sys.argv[1] == "--record":
    _record()
