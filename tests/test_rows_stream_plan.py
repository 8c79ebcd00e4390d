"""The host's choice of the decode GEMV's stream form (mi355x_rows_stream_plan: no launch, no
device access; without a device the plan counts 256 compute units, as the MI355X has).

A launch takes the short-stream form where every matrix's longest wave streams no more steps
than the ring of its type holds (steps <= depth: 3 steps of 16 superblocks for Q4_K / Q5_K, 2
for Q6_K) and one chain batch covers a wave's rows; else the generic loop. The plan reports the
steps and depth of the matrix with the least room.
"""
import pytest

Q4, Q5, Q6 = 12, 13, 14
DEPTH = {Q4: 3, Q5: 3, Q6: 2}

# the decode launches of the three models: (name, K, [(type, rows)], form is short)
TINYLLAMA = [("q/k/v", 2048, [(Q4, 2048), (Q4, 256), (Q6, 256)], True),
             ("o-proj", 2048, [(Q4, 2048)], True),
             ("gate + up", 2048, [(Q4, 5632), (Q4, 5632)], True),
             ("down", 5632, [(Q6, 2048)], True),
             ("down Q4_K", 5632, [(Q4, 2048)], True),
             ("head", 2048, [(Q6, 32000)], False)]
LLAMA3_8B = [("q/k/v", 4096, [(Q4, 4096), (Q4, 1024), (Q6, 1024)], True),
             ("o-proj", 4096, [(Q4, 4096)], True),
             ("gate + up", 4096, [(Q4, 14336), (Q4, 14336)], False),
             ("down", 14336, [(Q6, 4096)], False),
             ("head", 4096, [(Q6, 128256)], False)]
LLAMA3_70B = [("q/k/v", 8192, [(Q4, 8192), (Q4, 1024), (Q6, 1024)], False),
              ("o-proj", 8192, [(Q4, 8192)], False),
              ("gate + up", 8192, [(Q4, 28672), (Q4, 28672)], False),
              ("head", 8192, [(Q6, 128256)], False)]
LAUNCHES = [(m, *l) for m, ls in (("tinyllama", TINYLLAMA), ("llama3-8b", LLAMA3_8B), ("llama3-70b", LLAMA3_70B))
            for l in ls]


@pytest.mark.parametrize("model,name,K,mats,short", LAUNCHES, ids=[f"{l[0]}:{l[1]}" for l in LAUNCHES])
def test_model_launch_forms(model, name, K, mats, short):
    import ggml_mi355x as g
    steps, depth, form = g.rows_stream_plan(mats, K)
    assert depth in {DEPTH[t] for t, _ in mats}
    assert steps >= 1
    if short:
        assert form == g.ROWS_SHORT and steps <= depth, (steps, depth, form)
    else:
        assert form in (g.ROWS_LONG, g.ROWS_CLAIMED) and steps > depth, (steps, depth, form)


@pytest.fixture
def waves2():
    """Two waves per workgroup: 512 waves on 256 compute units, so the rows that fill them to
    a given depth stay small."""
    import ggml_mi355x as g
    prev = g.gemv_waves(2)
    yield 2 * 256
    g.gemv_waves(prev)


@pytest.mark.parametrize("ty", [Q4, Q5, Q6])
def test_ring_boundary(waves2, ty):
    """K = 4096 is one row per step: with rows = D x waves every wave streams exactly D steps
    (short); one more row gives one wave D + 1 (long)."""
    import ggml_mi355x as g
    D = DEPTH[ty]
    assert g.rows_stream_plan([(ty, D * waves2)], 4096) == (D, D, g.ROWS_SHORT)
    assert g.rows_stream_plan([(ty, D * waves2 + 1)], 4096) == (D + 1, D, g.ROWS_LONG)
    assert g.rows_stream_plan([(ty, (D - 1) * waves2 + 1)], 4096) == (D, D, g.ROWS_SHORT)


def test_mixed_launch_goes_by_each_type(waves2):
    """Each matrix against the ring of its own type: three steps on the Q4_K waves are short
    beside a Q6_K matrix of one step, and a Q6_K matrix of three steps makes the launch long."""
    import ggml_mi355x as g
    # waves go by bytes: 1380 Q4_K rows take 489 of the 512 waves (3 rows), 44 Q6_K rows 22 (2 rows)
    assert g.rows_stream_plan([(Q4, 1380), (Q6, 44)], 4096) == (3, 3, g.ROWS_SHORT)
    steps, depth, form = g.rows_stream_plan([(Q4, 100), (Q6, 1100)], 4096)  # Q6_K waves: 3 rows
    assert steps > depth and form == g.ROWS_LONG


def test_small_batch_is_long():
    """One chain batch must cover a wave's rows: K = 256 at 300 rows gives the waves 16 rows
    in one step; a batch of 8 rows would need two replays, which the short form does not do."""
    import ggml_mi355x as g
    assert g.rows_stream_plan([(Q4, 300)], 256) == (1, 3, g.ROWS_SHORT)
    assert g.rows_stream_plan([(Q4, 300)], 256, batch_rows=16) == (1, 3, g.ROWS_SHORT)
    assert g.rows_stream_plan([(Q4, 300)], 256, batch_rows=15) == (1, 3, g.ROWS_LONG)
    assert g.rows_stream_plan([(Q4, 300)], 256, batch_rows=8) == (1, 3, g.ROWS_LONG)


def test_knob_forces_the_generic_form():
    import ggml_mi355x as g
    assert g.debug_knob("GEMV_SHORT", 0) == 1  # the product default
    try:
        assert g.rows_stream_plan([(Q4, 2048)], 2048) == (1, 3, g.ROWS_LONG)
    finally:
        g.debug_knob("GEMV_SHORT")  # (NaN: back to the default)
    assert g.rows_stream_plan([(Q4, 2048)], 2048) == (1, 3, g.ROWS_SHORT)


def test_argument_checks():
    import ggml_mi355x as g
    assert g.rows_stream_plan([(Q4, 2048)], 2000) == g.E_INVAL
    assert g.rows_stream_plan([(Q4, 2048)], 0) == g.E_INVAL
    assert g.rows_stream_plan([(Q4, 2048)], 2048, batch_rows=-1) == g.E_INVAL
    assert g.rows_stream_plan([(Q4, 1)] * 5, 2048) == g.E_INVAL
    assert g.rows_stream_plan([(0, 2048)], 2048) == g.E_UNSUPPORTED
    assert g.rows_stream_plan([(Q4, 16)], 256 * 145) == g.E_UNSUPPORTED
