"""Build facts of EVERY instantiation of K1c, the ones that gather from the gather image included (k_rows_col.hip: k_rows_col and
k_rows_col_img): at most 208 vector registers, no scratch, two waves per SIMD, and a wave of the prediction update still fits beside
two of them -- 2 x R_rows + R_update <= 512.  Read from the resource remarks the Makefile leaves beside every
object, as tests/test_fit_registers.py reads them."""
from test_fit_registers import FILE, _alloc, _resources


def test_every_column_kernel_fits_beside_the_update():
    rows = {k: v for k, v in _resources("k_rows_col").items() if "k_rows_col" in k}
    img = [k for k in rows if "k_rows_col_img" in k]
    assert len(img) == 2 and len(rows) == 7, sorted(rows)         # the full and the pair image | DR 20, 24, 28, 32 and 32-FULL
    upd = [v for k, v in _resources("k_update_runs").items() if "k_update_runs" in k]
    assert len(upd) == 1, upd
    for k, v in rows.items():
        assert v["VGPRs"] + v["AGPRs"] <= 208, (k, v)
        assert v["ScratchSize"] == 0, (k, v)
        assert v["Occupancy"] >= 2, (k, v)
        assert 2 * _alloc(v) + _alloc(upd[0]) <= FILE, (k, v, upd[0])
