"""Host checks of the inputs of tests/test_gpu_feature_edges.py (tests/feature_edge_inputs.py): the row-length histograms the sparse
cases promise, the condition numbers its tolerances rest on, and the two shortcuts against their literal numpy forms.  No GPU."""
import numpy as np

import feature_edge_inputs as I


def test_edge_matrix_has_the_promised_row_lengths():
    rows, cols, vals, A, Abin = I.edge_sparse()
    m, n = I.EDGE_SHAPE
    assert all(m % k and n % k for k in (8, 16, 32))
    lens = np.bincount(rows, minlength=m)
    assert np.array_equal(lens, I.edge_row_lengths())
    assert set(lens) == set(I.EDGE_ROW_LENGTHS) and lens[0] == 33 and lens[-1] == 17
    # neighbouring rows differ, so the four rows of a wave end at different chunks of sixteen
    assert np.all(lens[1:] != lens[:-1])
    # exactly the three duplicated entries, summed in the dense statement
    pairs = rows.astype(np.int64) * n + cols
    uniq, cnt = np.unique(pairs, return_counts=True)
    assert sorted(uniq[cnt == 2] // n) == list(I.EDGE_DUPLICATE_ROWS) and cnt.max() == 2
    assert Abin.sum() == len(rows) and (Abin == 2).sum() == 3
    assert np.isclose(A.sum(), vals.sum())
    # the input order is shuffled: the library sorts by row itself
    assert np.any(np.diff(rows) < 0)


def test_panel_matrix_has_the_promised_rows():
    rows, cols, lens, empty, panel_of = I.panel_sparse()
    m, n = I.PANEL_SHAPE
    assert m % 16 == 3 and -(-n // I.PANEL_WIDTH) == 4 and -(-m // I.PANEL_WIDTH) == 4
    assert np.array_equal(np.bincount(rows, minlength=m), lens)
    assert len(empty) == 101 and empty[0] == 0 and not lens[empty].any()
    assert len(panel_of) == 101 and (m - 1) in panel_of and set(panel_of.values()) == {0, 1, 2, 3}
    start = np.concatenate([[0], np.cumsum(lens)])
    for i, p in panel_of.items():
        c = cols[start[i]:start[i + 1]]
        assert len(c) == I.PANEL_DENSE_PER_ROW > 32 and np.all(c // I.PANEL_WIDTH == p)
    others = np.setdiff1d(np.arange(m), np.concatenate([empty, list(panel_of)]))
    assert np.all(lens[others] == I.PANEL_PER_ROW)
    # every row in strictly increasing column order (the library panels nothing else), all columns inside the matrix
    same_row = rows[1:] == rows[:-1]
    assert np.all(np.diff(cols)[same_row] > 0) and cols.min() >= 0 and cols.max() < n
    # the gathered operands are above the 8 MiB of the panel path at 30 and 32 columns, below it at 2
    assert min(m, n) * 30 * 8 >= 8 << 20 and max(m, n) * 2 * 8 < 8 << 20


def test_shortcuts_match_their_literal_forms():
    rng = np.random.default_rng(1)
    for rows, numF in ((40, 25), (25, 40), (30, 30)):
        A = I.dense_features(rows, numF, rows)
        lb = 0.7
        np.testing.assert_allclose(I.cond_AtA(A, lb), np.linalg.cond(A.T @ A + lb * np.eye(numF)), rtol=1e-10)
    # the rows x rows form of the solve, used above WOODBURY_ABOVE columns, against the literal one just below
    _, _, _, A = I.sparse_features(300, 2600, I.CG_SPARSE_PER, 3)
    A = A.toarray()
    rhs = rng.standard_normal((2600, 3))
    lit = np.linalg.solve(A.T @ A + 1.3 * np.eye(2600), rhs)
    wood = (rhs - A.T @ np.linalg.solve(A @ A.T + 1.3 * np.eye(300), A @ rhs)) / 1.3
    np.testing.assert_allclose(wood, lit, rtol=0, atol=1e-13 * np.abs(lit).max())
    assert I.WOODBURY_ABOVE >= 2600
    np.testing.assert_array_equal(I.direct_solve(A, 1.3, rhs), lit)


def test_every_solve_case_is_well_conditioned():
    worst = 0.0
    for numF, D, _ in I.DIRECT_CASES:
        lb = I.lb_of(numF, D)
        assert 0.5 <= lb <= 2.5
        worst = max(worst, I.cond_AtA(I.dense_features(I.DIRECT_ROWS, numF, 400 + numF), lb))
    for rows, numF, D in I.CG_DENSE_CASES:
        worst = max(worst, I.cond_AtA(I.dense_features(rows, numF, 500 + numF + rows), I.lb_of(numF, D)))
    for rows, numF, D, kind in I.CG_SPARSE_CASES:
        A = I.sparse_features(rows, numF, I.CG_SPARSE_PER, 550 + numF + D, binary=kind == "bin")[3]
        worst = max(worst, I.cond_AtA(A, I.lb_of(numF, D)))
    for N, numF, D in I.RESIDENT_CASES + [I.RESIDENT_REFUSED]:
        worst = max(worst, I.cond_AtA(I.dense_features(N, numF, N + numF + D), I.RESIDENT_LB))
    for numF in I.REL_NUMF:
        worst = max(worst, I.cond_AtA(I.dense_features(500, numF, 451 + numF), (0.8 + numF / 100.0) / 1.7))
    _, _, _, A, Abin = I.edge_sparse()
    for M in (A, Abin):
        for D in (2, 33):
            worst = max(worst, I.cond_AtA(M, I.lb_of(M.shape[1], D)))
    print(f"feature edge inputs: largest cond(A'A + lb I) over all solve cases {worst:.1f}")
    assert worst < 1e4


def test_solver_and_dimension_coverage_of_the_direct_cases():
    """every solver of the direct path sees D = 1, a D in 17 .. 32 and a D above 32"""
    def solver(numF, no_eig):
        if numF <= 64:
            return 16 if numF <= 16 else 32 if numF <= 32 else 64
        return "eig" if numF <= 640 and not no_eig else ("chol-forced" if no_eig else "chol")
    seen = {}
    for numF, D, no_eig in I.DIRECT_CASES:
        seen.setdefault(solver(numF, no_eig), set()).add(D)
    assert set(seen) == {16, 32, 64, "eig", "chol", "chol-forced"}
    for s, ds in seen.items():
        assert 1 in ds and any(17 <= d <= 32 for d in ds) and any(d > 32 for d in ds), (s, ds)
    assert {d for _, d, _ in I.DIRECT_CASES} == {1, 16, 17, 33, 64}
