"""The decode GEMV's whole host plan (csrc/kq_gemv_host.hip plan_rows, read through
mi355x_debug_rows_plan: no launch, no device access) stays what tests/golden/rows_plans.json
records, field by field: the wave split, the trim of its floors, rows per wave, the chain batch,
LDS, grid, the prologue's and the stream's form, the claimed-rows unit and the kernel
instantiation. Without a device the plan counts 256 compute units, as the MI355X has, so the
file holds on both machines.

The golden file was recorded with this module's recorder (`python -m tests.test_rows_plan [path]`,
from the repository root) BEFORE plan_rows() was restructured into named steps and moved out of
kq_api.hip; a planner change regenerates it on purpose, never as a side effect.
"""
import json
import os
import sys
from contextlib import contextmanager

import pytest

from tests.test_rows_stream_plan import LAUNCHES

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "rows_plans.json")
Q4, Q5, Q6 = 12, 13, 14
PROLOGUES = (("none", 0), ("rms_norm", 1), ("swiglu", 2))


@contextmanager
def _default():
    yield


@contextmanager
def _knob(name, value):
    import ggml_mi355x as g
    g.debug_knob(name, value)
    try:
        yield
    finally:
        g.debug_knob(name)  # (NaN: back to the product default)


@contextmanager
def _waves(n):
    import ggml_mi355x as g
    prev = g.gemv_waves(n)
    try:
        yield
    finally:
        g.gemv_waves(prev)


@contextmanager
def _impl(impl):
    import ggml_mi355x as g
    prev = g.gemv_impl(impl)
    try:
        yield
    finally:
        g.gemv_impl(prev)


# launches planned under every selector / knob that plan_rows reads: between them the short form,
# the long one, claimed rows, a mixed launch and a small one
SETTING_LAUNCHES = [("tl-qkv", 2048, [(Q4, 2048), (Q4, 256), (Q6, 256)]),
                    ("tl-o", 2048, [(Q4, 2048)]),
                    ("8b-gate-up", 4096, [(Q4, 14336), (Q4, 14336)]),
                    ("8b-head", 4096, [(Q6, 128256)]),
                    ("70b-gate-up", 8192, [(Q4, 28672), (Q4, 28672)])]
SETTINGS = {
    "gemv_waves=2": lambda: _waves(2),
    "gemv_impl=DYN": lambda: _impl(3),
    "GEMV_DYN=0": lambda: _knob("GEMV_DYN", 0),
    "GEMV_SHORT=0": lambda: _knob("GEMV_SHORT", 0),
    "GEMV_WPC=4": lambda: _knob("GEMV_WPC", 4),
    "GEMV_SMALL_WG=64": lambda: _knob("GEMV_SMALL_WG", 64),
    "GEMV_SMALL_MB=0": lambda: _knob("GEMV_SMALL_MB", 0),
    "GEMV_PRE0=3": lambda: _knob("GEMV_PRE0", 3),
    "GEMV_DYN_P=2": lambda: _knob("GEMV_DYN_P", 2),
}


def _cases():
    """name -> (setting, mats, K, fusedq, prologue)"""
    c = {}
    for model, name, K, mats, _ in LAUNCHES:
        for pname, pro in PROLOGUES:
            c[f"{model}:{name}:{pname}"] = (_default, mats, K, True, pro)
    c["q8l:K14336"] = (_default, [(Q6, 4096)], 14336, False, 0)
    c["q8l:K40960-above-fused-limit"] = (_default, [(Q4, 64)], 256 * 160, False, 0)
    c["fused:K37120-unsupported"] = (_default, [(Q4, 16)], 256 * 145, True, 0)
    c["q5-only"] = (_default, [(Q5, 4096)], 4096, True, 0)
    c["four-mixed-trim"] = (_default, [(Q4, 4096), (Q5, 8), (Q6, 8), (Q4, 8)], 2048, True, 0)
    # (the shares above truncate to 1525 + 3 + 4 + 2 of 1536 waves: no floor applies. With one row each
    # the three small shares truncate to 0 and are floored to 1 beside 1534: one wave is trimmed)
    c["four-mixed-trim-one-row"] = (_default, [(Q4, 4096), (Q5, 1), (Q6, 1), (Q4, 1)], 2048, True, 0)
    c["zero-rows-in-the-middle"] = (_default, [(Q4, 2048), (Q4, 0), (Q6, 256)], 2048, True, 0)
    c["fewer-rows-than-waves:K256"] = (_default, [(Q4, 3)], 256, True, 0)
    c["fewer-rows-than-waves:K2048"] = (_default, [(Q6, 5)], 2048, True, 0)
    c["K256-300-rows"] = (_default, [(Q4, 300)], 256, True, 0)
    c["equal-rows-claimed"] = (_default, [(Q4, 28672), (Q4, 28672)], 8192, True, 0)
    c["unequal-rows-static"] = (_default, [(Q4, 28672), (Q4, 14336)], 8192, True, 0)
    # which error wins where several checks fail (check_descs and the planner's own conditions)
    c["err:bad-type-and-K-above-fused-limit"] = (_default, [(0, 16)], 256 * 145, True, 0)
    c["err:bad-type-and-K-above-4096-blocks"] = (_default, [(0, 16)], 256 * 4097, False, 0)
    c["err:negative-rows-after-bad-type"] = (_default, [(0, 16), (Q4, -1)], 2048, True, 0)
    c["err:bad-type-after-negative-rows"] = (_default, [(Q4, -1), (0, 16)], 2048, True, 0)
    c["err:negative-rows-and-K-above-fused-limit"] = (_default, [(Q4, -1)], 256 * 145, True, 0)
    c["err:rows-above-int32"] = (_default, [(Q4, 1 << 31)], 2048, True, 0)
    c["err:K-not-a-multiple-of-256"] = (_default, [(0, 16)], 2000, True, 0)
    for sname, setting in SETTINGS.items():
        for lname, K, mats in SETTING_LAUNCHES:
            c[f"{sname}:{lname}"] = (setting, mats, K, True, 1 if lname == "tl-qkv" else 0)
    return c


CASES = _cases()


def _plan(case):
    import ggml_mi355x as g
    setting, mats, K, fusedq, pro = CASES[case]
    with setting():
        return g.rows_plan(mats, K, fusedq=fusedq, prologue=pro)


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


def test_golden_has_every_case(golden):
    assert sorted(golden) == sorted(CASES)


@pytest.mark.parametrize("case", sorted(CASES))
def test_rows_plan_unchanged(golden, case):
    import ggml_mi355x as g
    got, want = _plan(case), golden[case]
    if isinstance(want, int):
        assert got == want, (got, want)
        return
    assert isinstance(got, dict), got
    assert sorted(got) == sorted(g.ROWS_PLAN_FIELDS) == sorted(want)
    diff = {f: (got[f], want[f]) for f in g.ROWS_PLAN_FIELDS if got[f] != want[f]}
    assert not diff, diff


def test_expected_outcomes(golden):
    """What the recorded cases were chosen to exercise (so a regenerated file cannot lose it)."""
    import ggml_mi355x as g
    assert golden["fused:K37120-unsupported"] == g.E_UNSUPPORTED
    assert golden["q8l:K40960-above-fused-limit"]["kernel"] >= 0
    assert golden["q5-only"]["tmask"] == 2
    assert golden["four-mixed-trim"]["tmask"] == 7
    t = golden["four-mixed-trim-one-row"]  # 1534 + 1 + 1 + 1 waves trimmed to the cap of 6 x 256
    assert [t[f"wave_prefix{i}"] for i in range(5)] == [0, 1533, 1534, 1535, 1536]
    assert golden["equal-rows-claimed"]["dyn"] == 1 and golden["unequal-rows-static"]["dyn"] == 0
    z = golden["zero-rows-in-the-middle"]
    assert z["wave_prefix1"] == z["wave_prefix2"]  # the empty matrix owns no wave
    assert all(p["kernel"] >= 0 for p in golden.values() if isinstance(p, dict))


def test_argument_checks():
    import ggml_mi355x as g
    assert g.rows_plan([(Q4, 1)] * 5, 2048) == g.E_INVAL
    assert g.rows_plan([(Q4, 2048)], 2048, prologue=3) == g.E_INVAL
    assert g.rows_plan([(Q4, 2048)], 2048, fusedq=False, prologue=1) == g.E_INVAL


if __name__ == "__main__":  # record the golden file (run from the repository root: python -m tests.test_rows_plan)
    sys.path.insert(0, os.path.join(os.path.dirname(GOLDEN), "..", "..", "ggml-neon-opt_amd"))
    out = sys.argv[1] if len(sys.argv) > 1 else GOLDEN
    plans = {name: _plan(name) for name in sorted(CASES)}
    with open(out, "w") as f:
        json.dump(plans, f, indent=0, sort_keys=True)
        f.write("\n")
    print("recorded", len(plans), "plans ->", out)
