"""bench.py's command line: --dump-outputs writes the last timed tick's
output exactly and reproducibly, --steps sets the number of timed ticks, and
a plain run carries none of the --full legs."""
import json
import sys
from pathlib import Path

import numpy as np
import pytest

from dbsp_amd import ROW_DT, gen, oracle

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
import bench  # noqa: E402


def _load(d):
    return {p.stem: np.load(p) for p in Path(d).glob("*.npy")}


def test_dump_outputs_is_exact_and_canonical(tmp_path):
    rows = np.array([(7, 2, -1), (3, (1 << 60) + 5, 4), (3, 1, 9),
                     (7, 2, -3)], dtype=ROW_DT)
    bench.dump_outputs(tmp_path, rows)
    got = _load(tmp_path)
    assert set(got) == {"k", "v_hi", "v_lo", "w"}
    assert all(a.dtype == np.float64 for a in got.values())
    # rows ordered by (k, v, w); v is past 2^53 and is split losslessly
    assert got["k"].tolist() == [3, 3, 7, 7]
    assert got["w"].tolist() == [9, 4, -3, -1]
    v = (got["v_hi"].astype(np.uint64) << np.uint64(32)) | \
        got["v_lo"].astype(np.uint64)
    assert v.tolist() == [1, (1 << 60) + 5, 2, 2]
    # any input order gives the same files
    other = tmp_path / "shuffled"
    bench.dump_outputs(other, rows[[2, 0, 3, 1]])
    for name, a in _load(other).items():
        assert np.array_equal(a, got[name])


def test_dump_outputs_f64_column_and_empty(tmp_path):
    rows = np.zeros(3, dtype=ROW_DT)
    rows["k"] = [5, 1, 3]
    rows["v"] = np.array([0.25, -1e300, 3.5]).view(np.uint64)
    rows["w"] = [1, 1, -1]
    bench.dump_outputs(tmp_path, rows, f64_cols=("v",))
    got = _load(tmp_path)
    assert got["k"].tolist() == [1, 3, 5]
    assert got["v"].tolist() == [-1e300, 3.5, 0.25]
    bench.dump_outputs(tmp_path / "empty", np.empty(0, dtype=ROW_DT))
    assert {n: len(a) for n, a in _load(tmp_path / "empty").items()} == \
        {"k": 0, "v": 0, "w": 0}


def test_dump_outputs_samples_past_the_byte_budget(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_MAX_BYTES", 4096)
    rows = np.zeros(1000, dtype=ROW_DT)
    rows["k"] = np.arange(1000)[::-1]
    rows["w"] = 1
    bench.dump_outputs(tmp_path / "a", rows)
    bench.dump_outputs(tmp_path / "b", rows)
    a, b = _load(tmp_path / "a"), _load(tmp_path / "b")
    assert sum(x.nbytes for x in a.values()) <= 4096
    idx = a["sample_index"].astype(np.int64)
    assert len(idx) == 4096 // 32 and (np.diff(idx) > 0).all()
    assert np.array_equal(a["k"], idx.astype(np.float64))  # sorted rows: k == i
    for name in a:
        assert np.array_equal(a[name], b[name])


@pytest.mark.gpu
def test_plain_run_steps_and_dump_match_oracle(tmp_path, monkeypatch, capsys):
    steps, warmup, tick = 3, 2, 5000
    monkeypatch.setattr(sys, "argv", [
        "bench.py", "--gpus", "1", "--steps", str(steps), "--warmup",
        str(warmup), "--tick", str(tick), "--dump-outputs", str(tmp_path)])
    bench.main()
    line = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert line["steps"] == steps and line["warmup"] == warmup
    assert line["config"]["events_timed"] == steps * tick
    assert line["ms_per_step"] > 0
    assert line["value"] == pytest.approx(
        tick / (line["ms_per_step"] * 1e-3), rel=1e-2)
    assert "cpu_baseline" not in line and "roofline" not in line
    # the dump is the output delta of tick warmup+steps of the seeded stream
    evs = gen.generate((warmup + steps) * tick, seed=1)
    q = oracle.Query(3)
    for lo in range(0, len(evs), tick):
        exp = q.step(evs[lo:lo + tick], cap=1 << 22)
    q.close()
    exp = np.sort(exp, order=["k", "v", "w"])
    got = _load(tmp_path)
    assert set(got) == {"k", "v", "w"} and len(exp) > 0
    for name in ("k", "v", "w"):
        assert got[name].dtype == np.float64
        assert np.array_equal(got[name], exp[name].astype(np.float64)), name
