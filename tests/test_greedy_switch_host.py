"""CPU: the host side of the greedy MLP selection -- the MODEGPT_MLP_GREEDY switch, the round partition and the decoder
(modegpt_amd/reports.py); no torch device, no library call."""
import math

import pytest

from modegpt_amd import reports
from tests import greedy_model as G


def test_switch_unset_and_zero_are_off(monkeypatch):
    monkeypatch.delenv("MODEGPT_MLP_GREEDY", raising=False)
    assert reports.mlp_greedy_rounds() == 0
    monkeypatch.setenv("MODEGPT_MLP_GREEDY", "0")
    assert reports.mlp_greedy_rounds() == 0


@pytest.mark.parametrize("raw,want", [("1", 1), ("8", 8), ("128", 128), (" 32 ", 32)])
def test_switch_positive_integer_is_the_round_count(monkeypatch, raw, want):
    monkeypatch.setenv("MODEGPT_MLP_GREEDY", raw)
    assert reports.mlp_greedy_rounds() == want


@pytest.mark.parametrize("raw", ["", "on", "true", "-1", "1.5", "8 rounds", "0x10", "+4"])
def test_switch_anything_else_raises_and_names_the_variable(monkeypatch, raw):
    monkeypatch.setenv("MODEGPT_MLP_GREEDY", raw)
    with pytest.raises(ValueError, match="MODEGPT_MLP_GREEDY"):
        reports.mlp_greedy_rounds()


def test_switch_is_read_at_call_time(monkeypatch):
    monkeypatch.setenv("MODEGPT_MLP_GREEDY", "4")
    assert reports.mlp_greedy_rounds() == 4
    monkeypatch.setenv("MODEGPT_MLP_GREEDY", "9")
    assert reports.mlp_greedy_rounds() == 9
    monkeypatch.delenv("MODEGPT_MLP_GREEDY")
    assert reports.mlp_greedy_rounds() == 0


def test_partition_is_the_models():
    for r in (0, 1, 7, 91, 10035):
        for rounds in (1, 3, 8, 32, 128, r + 3):
            assert reports.greedy_partition(r, rounds) == G.partition(r, rounds)
    with pytest.raises(ValueError):
        reports.greedy_partition(5, 0)
    with pytest.raises(ValueError):
        reports.greedy_partition(-1, 2)


def test_decoder():
    nan = float("nan")
    m = reports.decode_mlp_greedy([8.0, 4.0, 1.0, 0.5], [[3.0, 1.5], [2.0, 1.9], [0.4, nan]], 2, 17)
    assert m == {"rounds": 3, "rank": 17, "objective": [8.0, 4.0, 1.0, 0.5], "objective_over_total": 0.0625, "dead_picks": 2,
                 "min_cut_gap": pytest.approx(0.05)}
    assert "ridge_at_rank" not in m and "greedy_over_ridge" not in m
    m = reports.decode_mlp_greedy([8.0, 0.5], [[nan, nan]], 0, 3, ridge_at_rank=1.0, greedy_at_rank=0.5)
    assert m["min_cut_gap"] is None and m["ridge_at_rank"] == 1.0 and m["greedy_at_rank"] == 0.5 and m["greedy_over_ridge"] == 0.5
    # non-finite figures become None: nothing json.dump would write as NaN
    m = reports.decode_mlp_greedy([8.0, nan], None, 0, 3, ridge_at_rank=nan, greedy_at_rank=0.5)
    assert m["objective"] == [8.0, None] and m["objective_over_total"] is None and m["min_cut_gap"] is None
    assert m["ridge_at_rank"] is None and m["greedy_over_ridge"] is None
    flat = [m["objective_over_total"], m["min_cut_gap"], m["ridge_at_rank"], m["greedy_over_ridge"], *m["objective"]]
    assert not any(isinstance(x, float) and not math.isfinite(x) for x in flat)
    with pytest.raises(ValueError):
        reports.decode_mlp_greedy([1.0], None, 0, 0)


def test_ops_re_exports_the_host_side():
    from modegpt_amd import ops
    assert ops.mlp_greedy_rounds is reports.mlp_greedy_rounds and ops.decode_mlp_greedy is reports.decode_mlp_greedy
    assert ops.greedy_partition is reports.greedy_partition and callable(ops.nystrom_greedy_select)
