"""CPU: mi355x_attn_prompt_precision, the selector of the f16 matrix-core prompt attention
(include/ggml_mi355x.h): its values and errors, the default, the query, that it gives the previous
value back, the ABI symbol, and the tools' MI355X_ATTN_PROMPT translation. No launch, no device."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "ggml-neon-opt_amd")]


@pytest.fixture
def g():
    """The package, with the selector put back to EXACT after the test."""
    import ggml_mi355x as g
    g.lib()
    yield g
    g.lib().mi355x_attn_prompt_precision(0)


def test_constants_match_the_header(g):
    txt = open(os.path.join(ROOT, "include", "ggml_mi355x.h")).read()
    assert "#define MI355X_ATTN_PROMPT_EXACT 0" in txt and "#define MI355X_ATTN_PROMPT_F16 1" in txt
    assert (g.ATTN_PROMPT_EXACT, g.ATTN_PROMPT_F16) == (0, 1)


def test_default_is_exact(g):
    assert g.attn_prompt_precision() == g.ATTN_PROMPT_EXACT  # no argument: the query
    assert g.attn_prompt_precision(-1) == g.ATTN_PROMPT_EXACT
    # a fresh process, before any call, with the tools' switch in the environment: the library reads none
    code = ("import sys; sys.path[:0] = [%r, %r]; import ggml_mi355x as g; print(g.attn_prompt_precision(-1))"
            % (ROOT, os.path.join(ROOT, "ggml-neon-opt_amd")))
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True,
                         env=dict(os.environ, MI355X_ATTN_PROMPT="f16"))
    assert out.returncode == 0 and out.stdout.strip() == "0", (out.stdout, out.stderr)


def test_returns_the_previous_value_and_restores(g):
    assert g.attn_prompt_precision(g.ATTN_PROMPT_F16) == g.ATTN_PROMPT_EXACT
    assert g.attn_prompt_precision(-1) == g.ATTN_PROMPT_F16  # the query changes nothing
    assert g.attn_prompt_precision(-1) == g.ATTN_PROMPT_F16
    assert g.attn_prompt_precision(g.ATTN_PROMPT_F16) == g.ATTN_PROMPT_F16
    prev = g.attn_prompt_precision(g.ATTN_PROMPT_EXACT)
    assert prev == g.ATTN_PROMPT_F16
    assert g.attn_prompt_precision(prev) == g.ATTN_PROMPT_EXACT  # put back from the returned value
    assert g.attn_prompt_precision(g.ATTN_PROMPT_EXACT) == g.ATTN_PROMPT_F16
    assert g.attn_prompt_precision() == g.ATTN_PROMPT_EXACT


@pytest.mark.parametrize("bad", [2, 3, -2, 100, -100])
def test_any_other_value_is_invalid_and_changes_nothing(g, bad):
    for cur in (g.ATTN_PROMPT_EXACT, g.ATTN_PROMPT_F16):
        g.attn_prompt_precision(cur)
        assert g.attn_prompt_precision(bad) == g.E_INVAL
        assert g.attn_prompt_precision(-1) == cur


def test_other_selectors_are_independent(g):
    """The prompt form, the streamed mode and the GEMMs' precision keep their values."""
    before = (g.attn_prompt_impl(g.ATTN_GROUP), g.attn_stream(0), g.prefill_precision(-1))
    try:
        g.attn_prompt_precision(g.ATTN_PROMPT_F16)
        assert (g.attn_prompt_impl(g.ATTN_GROUP), g.attn_stream(0), g.prefill_precision(-1)) == \
            (g.ATTN_GROUP, 0, before[2])
        assert g.attn_prompt_precision(-1) == g.ATTN_PROMPT_F16
    finally:
        g.attn_prompt_impl(before[0])
        g.attn_stream(before[1])


def test_abi_symbol(g):
    assert "mi355x_attn_prompt_precision" in g.EXPORTED_SYMBOLS
    out = subprocess.run(["nm", "-D", "--defined-only", g.LIB_PATH], capture_output=True, text=True).stdout
    assert any(l.split()[-1] == "mi355x_attn_prompt_precision" for l in out.splitlines() if l.strip())
    sym = subprocess.run(["nm", "-D", "--defined-only", "-C", g.LIB_PATH], capture_output=True, text=True).stdout
    assert "kq_attn_prompt_f16<64>" in sym and "kq_attn_prompt_f16<128>" in sym  # both instantiations are in the library


def test_tools_switch(g):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import knobs
    finally:
        sys.path.pop(0)
    assert knobs.apply_env({"MI355X_ATTN_PROMPT": "f16"}) == {"MI355X_ATTN_PROMPT": "f16"}
    assert g.attn_prompt_precision(-1) == g.ATTN_PROMPT_F16
    knobs.apply_env({"MI355X_ATTN_PROMPT": "exact"})
    assert g.attn_prompt_precision(-1) == g.ATTN_PROMPT_EXACT
    knobs.apply_env({})
    assert g.attn_prompt_precision(-1) == g.ATTN_PROMPT_EXACT
