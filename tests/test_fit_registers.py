"""Build facts of the register split between the row kernel K1c and the sweep's prediction update: a wave of
the update fits beside two row waves on a SIMD -- 2 x R_rows + R_update <= 512 -- and neither side pays for it with scratch.
Read from the resource remarks the Makefile leaves beside every object (*.o.res); no assembly is searched."""
import glob
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GRANULE = 8                        # vector registers are allocated in blocks of 8 per lane
FILE = 512                         # per SIMD lane


def _resources(unit):
    path = os.path.join(ROOT, "bayesiandatafusion.jl_amd", "csrc", unit + ".o.res")
    assert glob.glob(path), "no csrc/%s.o.res: build with __graft_entry__.build() (make)" % unit
    res, name = {}, None
    for line in open(path):
        m = re.search(r"remark: \s*(Function Name|VGPRs|AGPRs|ScratchSize \[bytes/lane\]|Occupancy \[waves/SIMD\]): (\S+)", line)
        if not m:
            continue
        if m.group(1) == "Function Name":
            name = m.group(2)
            res[name] = {}
        elif name is not None:
            res[name][m.group(1).split(" ")[0]] = int(m.group(2))
    return res


def _alloc(r):
    return (r["VGPRs"] + r["AGPRs"] + GRANULE - 1) // GRANULE * GRANULE


def test_update_fits_beside_two_row_waves():
    rows = {k: v for k, v in _resources("k_rows_col").items() if "10k_rows_colILi" in k}
    assert len(rows) == 5, sorted(rows)                    # DR 20, 24, 28, 32 and 32-FULL: any of them may run beside the update
    for k, v in rows.items():
        assert v["ScratchSize"] == 0, (k, v)
        assert v["Occupancy"] >= 2, (k, v)
    upd = [v for k, v in _resources("k_update_runs").items() if "k_update_runs" in k]
    assert len(upd) == 1, upd
    assert upd[0]["ScratchSize"] == 0, upd
    r_rows = max(_alloc(v) for v in rows.values())
    assert 2 * r_rows + _alloc(upd[0]) <= FILE, (r_rows, upd[0])


def test_the_sorted_predict_kernel_uses_no_scratch():
    # k_predict_runs keeps the sorted pairs' raw predictions and per-pair baselines (not in the sweep)
    runs = [v for k, v in _resources("k_predict").items() if "k_predict_runs" in k]
    assert len(runs) == 1 and runs[0]["ScratchSize"] == 0, runs
