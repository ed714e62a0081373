"""bench.py's command line and --dump-outputs files (no GPU: the plans are host stand-ins)."""
import sys
from types import SimpleNamespace

import numpy as np
import pytest

import bench


def parse(monkeypatch, *argv):
    monkeypatch.setattr(sys, "argv", ["bench.py"] + list(argv))
    return bench.parse()


def test_plain_run_has_no_legs(monkeypatch):
    a = parse(monkeypatch, "--gpus", "1", "--steps", "7", "--warmup", "3")
    assert (a.steps, a.warmup, a.full, a.dump_outputs) == (7, 3, False, None)
    assert all(getattr(a, leg) <= 0 for leg in bench.LEGS)
    a = parse(monkeypatch, "--full", "--sp-beams", "2", "--dump-outputs", "d")
    assert a.full and a.sp_beams == 2 and a.dump_outputs == "d"
    # the scripts' "no legs" arguments stay valid without --full
    parse(monkeypatch, "--no-cpu", "--e2e-beams", "0", "--sp-beams", "0", "--fft-beams", "0", "--rfi-beams", "0",
          "--stream-beams", "0")


@pytest.mark.parametrize("leg", sorted(bench.LEGS))
def test_leg_without_full_is_an_error(monkeypatch, leg):
    with pytest.raises(SystemExit):
        parse(monkeypatch, "--" + leg.replace("_", "-"), "1")


class HostPlan:
    """get_series / series_sum of a Plan over a host array [numdms][numout]."""

    def __init__(self, series):
        self.series = series
        self.numout = series.shape[1]
        self.pp = SimpleNamespace(numdms=series.shape[0])

    def get_series(self, dm0, ndm, t0, count):
        return self.series[dm0:dm0 + ndm, t0:t0 + count].copy()

    def series_sum(self, dm, t0, count):
        return float(self.series[dm, t0:t0 + count].astype(np.float64).sum())


def test_dump_outputs_files(tmp_path):
    rng = np.random.default_rng(1)
    shapes = [(5, 3 * bench.DUMP_WINDOW + 17), (3, bench.DUMP_WINDOW - 24), (4, bench.DUMP_WINDOW)]
    plans = [HostPlan(rng.integers(0, 1000, s).astype(np.float32)) for s in shapes]
    bench.dump_outputs(str(tmp_path / "a"), plans, 0, 1)
    bench.dump_outputs(str(tmp_path / "b"), plans, 0, 1)
    names = sorted(p.name for p in (tmp_path / "a").iterdir())
    assert names == ["series_index.npy", "series_sums.npy", "series_windows.npy"]
    for n in names:
        assert np.array_equal(np.load(tmp_path / "a" / n), np.load(tmp_path / "b" / n))
    idx = np.load(tmp_path / "a" / "series_index.npy")
    sums = np.load(tmp_path / "a" / "series_sums.npy")
    wins = np.load(tmp_path / "a" / "series_windows.npy")
    assert idx.dtype == np.float64 and sums.dtype == np.float64 and wins.dtype == np.float32
    assert np.array_equal(sums, np.concatenate([p.series.astype(np.float64).sum(axis=1) for p in plans]))
    at = 0
    for p, row in zip(plans, idx.astype(np.int64)):
        nd, n, w, s0, s1, s2 = row
        assert (nd, n, w) == (p.pp.numdms, p.numout, min(bench.DUMP_WINDOW, p.numout))
        assert s0 == 0 and s2 == n - w and 0 <= s1 <= n - w
        got = wins[at:at + nd * 3 * w].reshape(nd, 3, w)
        for k, s in enumerate((s0, s1, s2)):
            assert np.array_equal(got[:, k], p.series[:, s:s + w])
        at += nd * 3 * w
    assert at == wins.size
    bench.dump_outputs(str(tmp_path / "c"), plans[:1], 2, 4)
    assert sorted(p.name for p in (tmp_path / "c").iterdir()) == [
        "series_index_rank2.npy", "series_sums_rank2.npy", "series_windows_rank2.npy"]
