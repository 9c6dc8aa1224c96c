"""bench.py's options and the helpers behind --dump-outputs, without a GPU: a plain run switches every side leg off, --full
switches them back on, and the dumped arrays stay within their budget and are the same sample in every run."""
import importlib.util
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("bench_under_test", os.path.join(ROOT, "bench.py"))
bench = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(bench)

SIDE = ("no_cpu_baseline", "no_records_leg", "no_overlap_leg", "no_hits_only_leg", "no_copy_ref", "no_configs_leg")
HIT = np.dtype([("seq_id", "<u8"), ("i", "<u4"), ("power_db", "<f4"), ("freq_hz", "<u8")], align=True)


def test_plain_run_has_no_side_legs_and_full_has_them():
    a = bench.parse(["--gpus", "1", "--steps", "7", "--warmup", "3"])
    assert a.steps == 7 and a.warmup == 3 and not a.full and a.dump_outputs is None
    assert all(getattr(a, k) for k in SIDE)
    f = bench.parse(["--full"])
    assert f.full and not any(getattr(f, k) for k in SIDE)
    assert bench.parse(["--full", "--no-overlap-leg"]).no_overlap_leg


def test_sample_rows_is_fixed_and_within_budget():
    assert bench.sample_rows(512, 4096 * 4, 40 << 20) is None
    r = bench.sample_rows(8192, 4096 * 4, 40 << 20)
    assert np.array_equal(r, bench.sample_rows(8192, 4096 * 4, 40 << 20))
    assert len(r) == (40 << 20) // (4096 * 4) and np.all(np.diff(r) > 0) and 0 <= r[0] and r[-1] < 8192


def test_write_outputs_float_types_and_budget(tmp_path):
    h = np.zeros(5, HIT)
    h["seq_id"], h["i"], h["power_db"], h["freq_hz"] = np.arange(5), 7, 12.5, 3000000000
    arrs = dict(bench.hit_arrays(h), power_db=np.ones((2, 8), np.float32), flags=np.array([0, 1], np.uint8))
    bench.write_outputs(str(tmp_path / "out"), arrs)
    got = {f[:-4]: np.load(tmp_path / "out" / f) for f in os.listdir(tmp_path / "out")}
    assert set(got) == {"hits_seq_id", "hits_bin", "hits_power_db", "hits_freq_hz", "power_db", "flags"}
    assert got["power_db"].dtype == np.float32 and got["hits_power_db"].dtype == np.float32
    assert got["flags"].dtype == np.float64 and got["hits_freq_hz"][0] == 3e9 and list(got["hits_seq_id"]) == [0, 1, 2, 3, 4]
    big = bench.hit_arrays(np.zeros(1 << 20, HIT), budget=1 << 20)          # more records than the budget: a seeded sample
    assert len(big["hits_rows"]) == len(big["hits_bin"]) == (1 << 20) // 28
    try:
        bench.write_outputs(str(tmp_path / "no"), {"x": np.zeros(bench.DUMP_BUDGET // 8 + 1)})
        raise AssertionError("over the budget")
    except ValueError:
        assert not os.path.exists(tmp_path / "no")
