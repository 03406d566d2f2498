"""modegpt_amd/reports.py, the host side of the opt-in reports, on its own: it imports without torch, reproduces every dict that
scripts/record_report_decoders.py recorded in tests/golden/report_decoders.json with the decoders as they stood in ops.py (ordinary
inputs; zero, NaN and Inf energies; a NaN inside a curve; rank 0 and rank n; an empty head list; a non-monotone Q/K curve; missing
optional arguments; MHA rows with a NaN bound; the inputs that raise), ops re-exports every moved name, and every switch reads its
variable when it is called."""
import json
import math
import os
import subprocess
import sys

import pytest

from modegpt_amd import reports

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "report_decoders.json")
DECODERS = ("decode_margin", "decode_rank_curve", "decode_output_error", "decode_qk_margin", "decode_qk_logit_error",
            "decode_vo_spectrum", "decode_vo_output_error")
SWITCHES = {"rank_curve_enabled": "MODEGPT_RANK_CURVE", "output_error_enabled": "MODEGPT_OUTPUT_ERROR",
            "qk_error_enabled": "MODEGPT_QK_ERROR", "vo_error_enabled": "MODEGPT_VO_ERROR",
            "mlp_intercept_enabled": "MODEGPT_MLP_INTERCEPT", "keep_bias_enabled": "MODEGPT_KEEP_BIAS"}
CONSTANTS = ("RANK_CURVE_KEEP", "RANK_CURVE_TARGETS", "QK_ERROR_TARGETS", "VO_ERROR_TARGETS", "OUTPUT_ERROR_LEVELS", "MARGIN_FIELDS",
             "QK_MARGIN_FIELDS", "VO_SPECTRUM_FIELDS")

with open(GOLDEN) as _f:
    CASES = json.load(_f)


def same(a, b):
    """Equality of two decoded values through json: same types (a bool is no int, an int no float; a tuple reads back as a list),
    floats equal as numbers, NaN equal to NaN."""
    if isinstance(a, (list, tuple)) and isinstance(b, (list, tuple)):
        return len(a) == len(b) and all(same(x, y) for x, y in zip(a, b))
    if isinstance(a, dict) and isinstance(b, dict):
        return list(a) == list(b) and all(same(a[k], b[k]) for k in a)
    if type(a) is not type(b):
        return False
    if isinstance(a, float) and math.isnan(a):
        return math.isnan(b)
    return a == b


def test_same_is_strict():
    nan = float("nan")
    assert same({"a": [1.0, nan, None, True]}, {"a": [1.0, nan, None, True]})
    assert not same(1, 1.0) and not same(True, 1) and not same(nan, 1.0) and not same([1.0], [1.0, 2.0]) and not same(0.0, None)
    assert not same({"a": 1, "b": 2}, {"b": 2, "a": 1})


def test_imports_without_torch():
    code = ("import sys; import modegpt_amd.reports as r; "
            "assert 'torch' not in sys.modules, 'torch'; assert 'modegpt_amd.ops' not in sys.modules, 'ops'; "
            "assert 'modegpt_amd._lib' not in sys.modules, '_lib'; print(sorted(set(vars(r)) & {'math', 'os', 'torch'}))")
    out = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    assert out.stdout.strip() == "['math', 'os']"


def test_fixture_covers_every_decoder():
    assert {c["fn"] for c in CASES} == set(DECODERS)
    assert all(("result" in c) != ("raises" in c) for c in CASES)
    for fn in DECODERS:
        assert sum(c["fn"] == fn and "result" in c for c in CASES) >= 6


@pytest.mark.parametrize("i", range(len(CASES)), ids=["%s-%d" % (c["fn"], i) for i, c in enumerate(CASES)])
def test_decoder_reproduces_the_recording(i):
    c = CASES[i]
    fn = getattr(reports, c["fn"])
    if "raises" in c:
        with pytest.raises(Exception) as err:
            fn(*c["args"], **c["kwargs"])
        assert type(err.value).__name__ == c["raises"]
        return
    got = fn(*c["args"], **c["kwargs"])
    assert same(json.loads(json.dumps(got)), c["result"]), "%s%r %r\n got  %r\n want %r" % (c["fn"], c["args"], c["kwargs"], got, c["result"])


def test_ops_reexports_every_moved_name():
    from modegpt_amd import ops
    for name in DECODERS + CONSTANTS + tuple(SWITCHES):
        assert getattr(ops, name) is getattr(reports, name), name
    assert reports.RANK_CURVE_TARGETS == reports.QK_ERROR_TARGETS == reports.VO_ERROR_TARGETS == (1e-1, 1e-2, 1e-3)
    assert reports.OUTPUT_ERROR_LEVELS == (1e-1, 1e-2, 1e-3)
    assert reports.RANK_CURVE_KEEP == tuple(k / 100 for k in range(5, 101, 5))


@pytest.mark.parametrize("name", sorted(SWITCHES))
def test_switch_reads_its_variable_at_call_time(name, monkeypatch):
    fn, var = getattr(reports, name), SWITCHES[name]
    for other in SWITCHES.values():
        monkeypatch.delenv(other, raising=False)
    assert fn() is False
    for value in ("1", "on", "true", "ON", "On", "TRUE", "True", "tRuE"):
        monkeypatch.setenv(var, value)
        assert fn() is True, value
    for value in ("0", "", "off", "false", "yes", "2", "11", " 1", "1 ", "enable", "t", "y"):
        monkeypatch.setenv(var, value)
        assert fn() is False, value
    monkeypatch.setenv(var, "1")
    for other_name, other in SWITCHES.items():          # nobody else's variable is read
        if other_name != name:
            assert getattr(reports, other_name)() is False, other_name
    monkeypatch.delenv(var)
    assert fn() is False
    assert var in fn.__doc__


def test_keep_bias_keeps_its_architecture_rule(monkeypatch):
    monkeypatch.delenv("MODEGPT_KEEP_BIAS", raising=False)
    assert reports.keep_bias_enabled("qwen2") is True and reports.keep_bias_enabled("llama") is False
    assert reports.keep_bias_enabled(None) is False
    monkeypatch.setenv("MODEGPT_KEEP_BIAS", "on")
    assert reports.keep_bias_enabled("llama") is True and reports.keep_bias_enabled() is True
