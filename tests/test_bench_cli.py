"""CPU: bench.py's argument checks and its output dump (no device is touched: the checks run
before the first HIP call, dump_outputs takes host data)."""
import types

import numpy as np
import pandas as pd
import pytest


@pytest.mark.parametrize("argv", [["--steps", "0"], ["--cpu-full-ask", "x.json"], ["--no-such-option"]])
def test_rejected_arguments(monkeypatch, argv):
    import bench

    monkeypatch.setattr("sys.argv", ["bench.py"] + argv)
    with pytest.raises(SystemExit) as e:
        bench.main()
    assert e.value.code == 2


@pytest.mark.parametrize("rank, sfx", [(0, ""), (3, "_rank3")])
def test_dump_outputs_writes_float64_npy(tmp_path, rank, sfx):
    import bench

    cand = pd.DataFrame({"x_0": [0.25, 1.0], "x_1": [0.5, 0.0], "f_0_pred": np.float32([1.5, -2.0]), "f_0_des": [3, 4]})
    stats = types.SimpleNamespace(best_value=np.float64(0.125))
    info = bench.dump_outputs(str(tmp_path / "a" / "b"), cand, stats, rank)
    c = np.load(tmp_path / "a" / "b" / f"candidate{sfx}.npy")
    v = np.load(tmp_path / "a" / "b" / f"acq_value{sfx}.npy")
    assert c.dtype == np.float64 and v.dtype == np.float64
    assert np.array_equal(c, [[0.25, 0.5, 1.5, 3.0], [1.0, 0.0, -2.0, 4.0]]) and np.array_equal(v, [0.125])
    assert info == {"files": {f"candidate{sfx}.npy": [2, 4], f"acq_value{sfx}.npy": [1]},
                    "candidate_columns": ["x_0", "x_1", "f_0_pred", "f_0_des"]}
