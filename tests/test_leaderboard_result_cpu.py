"""What reality_check.py, overfit.py and diversify.py share (strategy_records.py, and `_selected` of
`StrategyPeriodStats`), with torch on the CPU: no env, no library."""
import numpy as np
import pytest
import torch

from gym_trading_env_amd.period_stats import StrategyPeriodStats
from gym_trading_env_amd.strategy_records import LeaderboardResult, f64_on, is_int_in

CPU = torch.device("cpu")


def test_is_int_in_refuses_bools_fractions_and_the_outside():
    lo, hi = 1, 256
    for bad in (True, False, 2.5, lo - 1, hi + 1, np.int64(hi + 1), float(hi + 1)):
        assert not is_int_in(bad, lo, hi), bad
    for good in (np.int64(3), 3, lo, hi, 3.0, np.int32(hi)):
        assert is_int_in(good, lo, hi), good
    assert not is_int_in(3.0, lo, hi, floats=False) and is_int_in(np.int64(3), lo, hi, floats=False)
    assert not is_int_in(True, lo, hi, floats=False)
    assert is_int_in(-2 ** 70, -float("inf"), float("inf"), floats=False)      # no range: a seed


def test_f64_on_converts_numpy_and_strided_torch():
    a = np.arange(12, dtype=np.float32).reshape(3, 4) / 3
    t = f64_on(torch, CPU, a, lambda s: s == (3, 4), "a must have shape (3, 4)")
    assert t.dtype == torch.float64 and t.is_contiguous() and tuple(t.shape) == (3, 4) and t.device == CPU
    assert t.numpy().tobytes() == a.astype(np.float64).tobytes()
    strided = torch.arange(24, dtype=torch.float32).reshape(4, 6)[:, ::2].t()       # [3, 4], not contiguous
    assert not strided.is_contiguous()
    t = f64_on(torch, CPU, strided, lambda s: s == (3, 4), "a must have shape (3, 4)")
    assert t.dtype == torch.float64 and t.is_contiguous() and tuple(t.shape) == (3, 4)
    assert torch.equal(t, strided.to(torch.float64))
    ints = f64_on(torch, CPU, [1, 2, 3], lambda s: s == (3,), "a must have shape (3,)")
    assert ints.dtype == torch.float64 and ints.tolist() == [1.0, 2.0, 3.0]


def test_f64_on_refuses_a_wrong_shape_in_the_words_of_each_caller():
    n, most, B, S = 4, 65536, 6, 16
    callers = (
        (np.ones((5, 3)), lambda s: len(s) == 2 and s[1] == n and 1 <= s[0] <= most,
         f"weights must have shape [R, {n}] with 1 <= R <= {most}", "weights must have shape [R, 4] with 1 <= R <= 65536, not (5, 3)"),
        (np.ones(5), lambda s: s == (B,), f"benchmark must have shape ({B},)", "benchmark must have shape (6,), not (5,)"),
        (torch.ones(S, 1), lambda s: s == (S,), f"scores must have shape ({S},)", "scores must have shape (16,), not (16, 1)"))
    for values, fits, expected, text in callers:
        with pytest.raises(ValueError) as e:
            f64_on(torch, CPU, values, fits, expected)
        assert str(e.value) == text
    # the weights' other refusals: one dimension, no row
    for bad in (np.ones(n), np.ones((0, n))):
        with pytest.raises(ValueError, match="weights must have shape"):
            f64_on(torch, CPU, bad, callers[0][1], callers[0][2])
    assert tuple(f64_on(torch, CPU, np.ones((7, n)), callers[0][1], callers[0][2]).shape) == (7, n)


SUMMARY = [("picked", "<i4"), ("share", "<f8")]


class CountedSummary:
    """stands in for the summary tensor on the device: counts its transfers to the host"""

    def __init__(self, record):
        self.record, self.reads = record, 0

    def cpu(self):
        self.reads += 1
        return torch.from_numpy(self.record.view(np.uint8).copy())


class Minimal(LeaderboardResult):
    SUMMARY_DTYPE = SUMMARY
    ARRAYS = ("first", "second")

    def __init__(self, out, keep):
        super().__init__(None, out, keep)
        self.first, self.second = out["first"], out["first"].to(torch.float64) * 0.5

    @property
    def picked(self):
        return int(self._read()["picked"])

    @property
    def share(self):
        return float(self._read()["share"])

    def _scalars(self):
        return dict(picked=self.picked, share=self.share, label="minimal")


def _minimal():
    record = np.zeros(1, np.dtype(SUMMARY))
    record["picked"], record["share"] = 7, 0.375
    summary = CountedSummary(record)
    kept = (object(), None)
    return Minimal(dict(first=torch.arange(5, dtype=torch.int32), summary=summary), kept), summary, kept


def test_the_summary_is_read_once_and_only_when_asked_for():
    result, summary, kept = _minimal()
    assert summary.reads == 0 and result._keep is kept and result._env is None
    assert result.picked == 7 and summary.reads == 1
    assert result.share == 0.375 and result.picked == 7 and summary.reads == 1
    result.numpy()
    assert summary.reads == 1


def test_numpy_gives_the_declared_arrays_and_scalars():
    result, summary, _ = _minimal()
    host = result.numpy()
    assert list(host) == ["first", "second", "picked", "share", "label"]
    assert isinstance(host["first"], np.ndarray) and host["first"].dtype == np.int32
    assert host["first"].tolist() == [0, 1, 2, 3, 4] and host["second"].tolist() == [0.0, 0.5, 1.0, 1.5, 2.0]
    assert (host["picked"], host["share"], host["label"]) == (7, 0.375, "minimal") and summary.reads == 1


def test_selected_periods_ascend_and_too_few_are_refused():
    board = object.__new__(StrategyPeriodStats)      # `_mask` and `_selected` read the period count alone
    board.num_periods = 9
    mask, ids = board._selected([7, 2, 5, 2], 3, "three, please")
    assert ids == [2, 5, 7] and mask.dtype == bool and np.flatnonzero(mask).tolist() == ids
    with pytest.raises(ValueError, match="^four, please$"):
        board._selected([7, 2, 5], 4, "four, please")
    assert board._selected(None)[1] == list(range(9)) and board._selected([], 0, "never")[1] == []
    assert board._selected(np.arange(9) % 4 == 1, 2, "two")[1] == [1, 5]
    with pytest.raises(ValueError, match="^two$"):
        board._selected(torch.arange(9) == 3, 2, "two")
