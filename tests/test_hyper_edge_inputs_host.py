"""Host checks of tests/hyper_edge_inputs.py and tests/hyper_restatement.py: every case sits on the edge its name promises, the
inputs let the double-precision oracle reach 1e-12 of the long-double restatement (the condition the GPU tests' bound of
1000 E_D rests on), the prior pack round-trips and the restated random part is the one the oracle consumes.  No GPU."""
import numpy as np
import pytest

import hyper_edge_inputs as I
import hyper_restatement as R


def test_partial_caps_of_the_chain():
    want = {range(1, 16): 14, range(16, 23): 13, range(23, 28): 12, range(28, 32): 11, range(32, 36): 10, range(36, 39): 9, range(39, 65): 8}
    for Ds, cap in want.items():
        assert all(R.max_partials(D) == cap for D in Ds), cap
    assert sum(len(r) for r in want) == 64
    # the random part's workgroups, the partial sums' and the draw's fit the sixteen nominal slots wherever the cap is not the floor of 8
    for D in range(1, 39):
        assert -(-(D * D + D) // 256) + R.max_partials(D) + 1 <= R.CHAIN_SLOTS


def test_sums_cases_sit_on_their_edges():
    assert set(I.SUMS_ROWS) == {1, 3, 4, 5, 127, 128, 129, 1920, 2048, 2049, 4097}
    for N, (_, nblocks, per, last) in I.SUMS_ROWS.items():
        assert R.unfused_partition(N) == (nblocks, per, last), N
    # N = 0: one workgroup with no row
    assert R.unfused_partition(0) == (1, 1, 0)
    # the 16 interleaved chains of the final sum: 15, 16, 17 and 33 partials
    assert [I.SUMS_ROWS[N][1] for N in (1920, 2048, 2049, 4097)] == [15, 16, 17, 33]
    assert sorted(I.SUMS_LARGE) == [(17, 524_417, True), (32, 262_145, False), (33, 262_145, False)]
    for (D, N, with_uhat), (_, nblocks, per, last) in I.SUMS_LARGE.items():
        assert N > R.UNFUSED_WORKGROUPS * R.HS_ROWS and R.unfused_partition(N) == (nblocks, per, last)
        assert N * D * 8 * (2 if with_uhat else 1) < 145e6                       # device memory of the case
    # the paired loop (widths 16 and 32) with an even and an odd number of chunks, the unpaired one (width 64) with two
    assert [(R.width(D), I.SUMS_LARGE[D, N, u][2]) for D, N, u in sorted(I.SUMS_LARGE)] == [(32, 3), (32, 2), (64, 2)]
    # the lone tail chunk of the odd case is run by its last workgroup too: 257 rows are two chunks and a row
    assert I.SUMS_LARGE[17, 524_417, True][3] == 2 * R.HS_ROWS + 1


def test_chain_cases_sit_on_their_edges():
    assert len(I.CHAIN_CASES) == 10
    for name, ((D, Nu, Nv, feats, no_poll), promised) in I.CHAIN_CASES.items():
        assert (R.chain_partition(D, Nu), R.chain_partition(D, Nv)) == promised, name
    cap = R.max_partials
    for name in ("cap14_16wide", "cap13_16wide", "cap10_fused_head", "cap10_generic_head", "cap8", "no_poll"):
        (D, Nu, Nv, _, _), ((nb_u, per_u, _), (nb_v, per_v, _)) = I.CHAIN_CASES[name]
        # u: exactly the cap of one-chunk partials (the unfused partition, so the sums are the unfused sums' bits); v: one row more,
        # two chunks per workgroup
        assert Nu == R.HS_ROWS * cap(D) and Nv == Nu + 1 and (nb_u, per_u, per_v) == (cap(D), 1, 2)
        assert R.chain_partition(D, Nu) == R.unfused_partition(Nu) and R.chain_partition(D, Nv) != R.unfused_partition(Nv)
    for name in ("cap10_fused_head", "largest_fused_32", "no_poll", "with_uhat", "cap14_16wide", "cap13_16wide"):
        assert I.CHAIN_CASES[name][0][0] <= 32           # the head that takes the partials in one pass
    for name in ("cap10_generic_head", "cap8", "largest_fused_64"):
        assert I.CHAIN_CASES[name][0][0] > 32
    # the largest fused entities: an odd number of chunks in the paired loop (a lone tail), sixteen in the unpaired one
    assert I.CHAIN_CASES["largest_fused_32"][1][0][:2] == (10, 13) and I.CHAIN_CASES["largest_fused_64"][1][0][:2] == (8, 16)
    assert I.CHAIN_CASES["largest_fused_32"][0][1] == R.CHAIN_ROWS == I.CHAIN_CASES["one_past_the_limit"][0][1] - 1
    # one row past the limit: the unfused sums, more partials than the chain's last workgroup could add
    assert I.CHAIN_CASES["one_past_the_limit"][1][0] == R.unfused_partition(R.CHAIN_ROWS + 1) == (129, 1, 1)


def test_draws_cases_cross_the_launch_edges():
    Ds = sorted({D for D, _, _ in I.DRAWS_CASES})
    assert Ds == [1, 7, 8, 15, 16, 64]
    total = lambda D: D * D + D
    assert total(7) <= 64 < total(8) and total(15) <= 256 < total(16)
    for D in Ds:
        mine = [(N, nu) for d, N, nu in I.DRAWS_CASES if d == D]
        assert any(nu != int(nu) for _, nu in mine)                              # a non-integer nu
        assert any(nu == D and N == 0 for N, nu in mine)                         # nu = D: the last row's gamma has shape 1/2


def test_seeds_are_distinct():
    keys = [(D, N) for D in I.WIDTHS_D for N in list(I.SUMS_ROWS) + list(I.DRAW_ROWS)] + [(D, N) for D, N, _ in I.SUMS_LARGE]
    keys = sorted(set(keys))
    assert len({I.seed_of(D, N) for D, N in keys}) == len(keys)


@pytest.mark.parametrize("D", I.WIDTHS_D)
def test_oracle_reaches_the_restatement_on_the_draw_inputs(D):
    """conditions on the inputs, not measurements: within 1e-12 for mu_N, W, Lambda and mu (both mean maps), cond(W) < 1e3"""
    for N in I.DRAW_ROWS:
        d = I.oracle_distances(D, N)
        print("D %2d N %3d " % (D, N) + " ".join("%s %.2e" % kv for kv in sorted(d.items())))
        assert d["cond_W"] < I.COND_MAX, (N, d)
        assert all(v <= I.ORACLE_TOL for k, v in d.items() if k != "cond_W"), (N, d)
    print("E_%d = %.2e, device bound %.2e" % (D, I.E(D), I.device_bound(D)))
    # the GPU tests' bound: far above the rounding of one double, far below the 1e-7 the draw was held to before
    assert 2.0 ** -53 < I.E(D) <= I.ORACLE_TOL and I.device_bound(D) <= 1e-9


def test_sums_restatement_against_numpy():
    S, uh = I.sums_inputs(17, 2049, True)
    sumU, UUt, bU, bUU = R.sums(S, uh, block=500)                               # (five blocks, the last one short)
    U = S - uh
    assert np.all(np.abs(U.sum(0) - sumU) <= bU) and np.all(np.abs(U.T @ U - UUt) <= bUU)
    assert np.array_equal(UUt, UUt.T) and bUU.min() > 0
    # the bound is tight where it matters: an off-diagonal entry that cancels keeps a bound from its terms' sizes, not from its own
    assert np.all(bUU * (1 + 1e-12) >= 2049 * 2.0 ** -52 * np.abs(UUt.astype(np.float64)))
    z = R.sums(np.zeros((0, 5)))
    assert all(not a.any() for a in z)


def test_linear_algebra_written_out():
    rng = np.random.default_rng(3)
    for n in (1, 2, 17, 64):
        Q = rng.standard_normal((n, n))
        M = Q @ Q.T / n + np.eye(n)
        L = R.chol_lower(M)
        assert np.allclose(L.astype(float), np.linalg.cholesky(M), rtol=0, atol=1e-14)
        assert np.abs(L @ R.lower_inverse(L) - np.eye(n)).max() < 1e-17
        assert np.abs(R.spd_inverse(M) @ M.astype(R.LD) - np.eye(n)).max() < 1e-16
        z = rng.standard_normal(n)
        assert np.abs(L.T @ R.solve_upper(L.T, z) - z).max() < 1e-17
    with pytest.raises(np.linalg.LinAlgError):
        R.chol_lower(-np.eye(2))


@pytest.mark.parametrize("D", [1, 15, 16, 17, 33, 64])
def test_pack_image_round_trips(D):
    rng = np.random.default_rng(D)
    Q = rng.standard_normal((D, D))
    Lam, mu = Q @ Q.T + np.eye(D), rng.standard_normal(D)
    pack = R.pack_image(Lam, mu, D)
    assert len(pack) == R.pack_doubles(D) == D + {16: 1, 32: 3, 64: 10}[R.width(D)] * 256
    head, Lt = R.unpack_image(pack, D)
    np.testing.assert_allclose(head, Lam @ mu, rtol=1e-13, atol=1e-13)
    assert not np.isnan(Lt).any()
    assert np.array_equal(Lt[:D, :D], Lam[::-1, ::-1])                          # Lambda reversed ...
    DP = R.width(D)
    assert np.array_equal(Lt[D:, D:], np.eye(DP - D)) and not Lt[D:, :D].any() and not Lt[:D, D:].any()      # ... identity on the padding
    # every image element names one entry of the lower block-triangle, each exactly once
    rows, cols = R._image_index(D)
    assert len(set(zip(rows.tolist(), cols.tolist()))) == len(rows) and np.all(rows // 16 >= cols // 16)


@pytest.mark.parametrize("D,N,nu", [(1, 0, 1.0), (2, 5, 5.0), (17, 129, 19.5), (64, 5, 67.0)])
def test_restated_random_part_is_what_the_oracle_consumes(O, D, N, nu):
    """draw() fed with draws() reproduces oracle.hyper_draw's (mu, Lambda) from the SAME parameters, for both mean maps: the indexing of
    (row, entry, purpose, tag) and the layout are the oracle's"""
    S, mu0, Tinv, b0, _ = I.draw_inputs(D, N)
    mu_N, beta_N, T_N, nu_N = O.hyper_params(S, mu0, b0, Tinv, nu)
    rand = R.draws(D, nu_N, 99, 3, 8)
    A = rand[:D * D].reshape(D, D)
    assert not np.triu(A, 1).any() and np.all(np.diag(A) > 0) and np.all(np.tril(A, -1)[np.tril_indices(D, -1)] != 0)
    W = R.spd_inverse(T_N)
    for mm in ("factor", "reference"):
        mu, Lam, _ = R.draw(W, mu_N, beta_N, A, rand[D * D:], mm)
        mu_o, Lam_o = O.hyper_draw(mu_N, beta_N, T_N, nu_N, 99, 3, 8, mean_map=mm)
        assert I.rel_distance(Lam_o, Lam) < 1e-12 and I.rel_distance(mu_o, mu, 1.0) < 1e-12, mm
    # another tag, sweep or seed is another random part
    for other in (R.draws(D, nu_N, 99, 3, 9), R.draws(D, nu_N, 99, 4, 8), R.draws(D, nu_N, 98, 3, 8)):
        assert not np.any(other[rand != 0] == rand[rand != 0])
